/*
 * encode_plan.c -- hap_encode_plan.h walked by a plain program (built with -fsanitize=address,undefined by
 * tests/test_host_sanitizers.py; links hap_frame.c and nothing else).
 *
 * 1. A recorded table: what hapb_encode decided for these calls BEFORE the plan became a header of its own -- the rows
 *    were printed by the planning lines of that hap_batch.c, lifted into a throw-away program, with its layout codes
 *    (4 / 10 / 2 / 12) and launcher bits written as the file format's layout values and sets of them.  Every field of
 *    every plan must equal its row.
 * 2. Invariants that hold whatever the recording says, over the recorded calls and over a product of formats, sizes,
 *    chunk counts, flags, switches and sources: the control word reads back field by field, and layout, half-tiles,
 *    fused and placed are set only where the kernels can honour them.
 */
#include "hap_encode_plan.h"
#include <stdio.h>
#include <string.h>

#define IDX HAPGPU_ENCODE_FRAGMENT_INDEX
#define COARSE HAPGPU_ENCODE_COARSE_MATCHES
#define SMALLER HAPGPU_ENCODE_SMALLER_FILES
#define FINE HAPGPU_ENCODE_FINE_CHUNKS
#define REFINE HAPGPU_ENCODE_REFINE_ENDPOINTS
#define DXT1 HapTextureFormat_RGB_DXT1
#define DXT5 HapTextureFormat_RGBA_DXT5
#define YCOCG HapTextureFormat_YCoCg_DXT5
#define RGTC1 HapTextureFormat_A_RGTC1
#define BC7 HapTextureFormat_RGBA_BPTC_UNORM
#define BC6U HapTextureFormat_RGB_BPTC_UNSIGNED_FLOAT
#define BC6S HapTextureFormat_RGB_BPTC_SIGNED_FLOAT

enum { SRC_NONE, SRC_RGBA8, SRC_TENSOR, SRC_NV12, SRC_RGBA16F, SRC_A8, SRC_KINDS };

typedef struct recorded_tex {
    unsigned nibble, compressor, chunk_count, chunk_bytes, header_len, fpc, gran_log2, layout, half_tiles, fused, windowed;
    unsigned long long bound;
} recorded_tex;

typedef struct recorded_plan {
    /* the call */
    const char *name;
    unsigned knobs[7];      /* frag_log2, byte_granular, position_lanes, rgtc1_fields, no_half_tiles, no_fusion, placing_allowed */
    unsigned flags, count;
    unsigned long bytes[2];
    unsigned formats[2], compressors[2], chunks[2];
    int source;
    unsigned width, height;
    unsigned long row_bytes;
    /* what was decided */
    unsigned rc;
    int planned;            /* 0: refused (rc), nothing else recorded */
    unsigned flags_out, chunks_out[2], frag_log2, refine, outer_header, frags_per_frame, chunks_per_frame, max_frags_per_tex,
             max_chunks_per_tex, slot_stride, placed;
    unsigned long long placed_extent, frame_raw_bound, stage_in_bytes;
    unsigned kinds[4];      /* granularities, layouts, fused, textures */
    int any_snappy, any_half_tiles;
    recorded_tex tex[2];
} recorded_plan;

static const recorded_plan recorded[] = {
    {"YCoCg 64x64, pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x0u, 0x8u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 3u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, textures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, textures, no index", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x0u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x0u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4446ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"DXT5 64x64, pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x0u, 0x4u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 2u, 0u, 4835ull}, {0}}},
    {"DXT5 64x64, pictures, refine", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x21u, 1u, {4096ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x21u, {1u, 0u}, 13u, 0x2u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"DXT1 64x64, 3 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {3u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {3u, 0u}, 13u, 0x0u, 0u, 2u, 2u, 2u, 2u, 8784u, 1u, 3136ull, 2052ull, 2048ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 2u, 1024u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 2482ull}, {0}}},
    {"RGTC1 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 2052ull, 2048ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 2048u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2446ull}, {0}}},
    {"RGTC1 2048x2048", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2097152ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 256u, 1u, 256u, 1u, 8784u, 1u, 2230310ull, 2097156ull, 2097152ull, {0x0u, 0x40u, 0x0u, 1u}, 1, 1,
     {{0x1u, 1u, 1u, 2097152u, 4u, 256u, 1u, 6u, 1u, 0u, 0u, 2446734ull}, {0}}},
    {"RGTC1 2048x2048, rgtc1_fields 44", {13u, 0u, 0u, 44u, 0u, 0u, 1u}, 0x1u, 1u, {2097152ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 256u, 1u, 256u, 1u, 8784u, 1u, 2230310ull, 2097156ull, 2097152ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0x1u, 1u, 1u, 2097152u, 4u, 256u, 2u, 2u, 1u, 0u, 0u, 2446734ull}, {0}}},
    {"RGTC1 2048x2048, rgtc1_fields 0", {13u, 0u, 0u, 0u, 0u, 0u, 1u}, 0x1u, 1u, {2097152ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 256u, 1u, 256u, 1u, 8784u, 0u, 0ull, 2097156ull, 2097152ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 2097152u, 4u, 256u, 1u, 0u, 0u, 0u, 1u, 2446734ull}, {0}}},
    {"BC7 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {BC7, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xcu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"BC7 64x64, coarse", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x3u, 1u, {4096ul, 0ul}, {BC7, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x3u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x100u, 0x0u, 1u}, 1, 1,
     {{0xcu, 1u, 1u, 4096u, 4u, 1u, 2u, 8u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, smaller files", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x5u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x4u, {1u, 0u}, 16u, 0x0u, 0u, 1u, 1u, 1u, 1u, 67920u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 1080p, fine chunks, 0 asked", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x9u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {0u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x9u, {270u, 0u}, 13u, 0x0u, 0u, 270u, 270u, 270u, 270u, 8784u, 0u, 0ull, 2073604ull, 2073600ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 270u, 7680u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 2429210ull}, {0}}},
    {"YCoCg 1040x64, 65 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {66560ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {65u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {65u, 0u}, 13u, 0x0u, 0u, 65u, 65u, 65u, 65u, 8784u, 0u, 0ull, 66564ull, 66560ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 65u, 1024u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 80035ull}, {0}}},
    {"YCoCg + RGTC1 64x64, pictures, chunks 1, 2", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {4096ul, 2048ul}, {YCOCG, RGTC1}, {1u, 1u}, {1u, 2u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 2u}, 13u, 0x0u, 4u, 3u, 3u, 2u, 2u, 8784u, 0u, 0ull, 6156ull, 6144ull, {0x2u, 0x10u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0x1u, 1u, 2u, 1024u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2482ull}}},
    {"YCoCg + RGTC1 64x64, pictures, second stored", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {4096ul, 2048ul}, {YCOCG, RGTC1}, {1u, 0u}, {1u, 2u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 2u}, 13u, 0x0u, 4u, 2u, 2u, 1u, 1u, 8784u, 0u, 0ull, 6156ull, 6144ull, {0x0u, 0x10u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0x1u, 0u, 1u, 2048u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 2078ull}}},
    {"YCoCg 64x64, position_lanes", {13u, 0u, 1u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, byte_granular", {13u, 1u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x1u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, frag_log2 12", {12u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 12u, 0x0u, 0u, 1u, 1u, 1u, 1u, 4560u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, no_half_tiles", {13u, 0u, 0u, 26u, 1u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4458ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"DXT5 100001 bytes, 3 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {100001ul, 0ul}, {DXT5, 0}, {1u, 0u}, {3u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {3u, 0u}, 13u, 0x0u, 0u, 14u, 2u, 14u, 2u, 8784u, 1u, 107329ull, 100005ull, 100096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 2u, 50000u, 4u, 7u, 1u, 4u, 1u, 0u, 0u, 116760ull}, {0}}},
    {"DXT1 8 bytes, 2 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {8ul, 0ul}, {DXT1, 0}, {1u, 0u}, {2u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {2u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 566ull, 12ull, 256ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 1u, 8u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 66ull}, {0}}},
    {"DXT5 16 MiB", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16777216ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 2048u, 1u, 2048u, 1u, 8784u, 1u, 17842214ull, 16777224ull, 16777216ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 16777216u, 8u, 2048u, 1u, 4u, 1u, 0u, 0u, 19573475ull}, {0}}},
    {"DXT1 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 2606ull, 2052ull, 2048ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 1u, 2048u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 2446ull}, {0}}},
    {"DXT5 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"BC6H unsigned 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {BC6U, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x2u, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"BC6H signed 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {BC6S, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x3u, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"DXT1 one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {8ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 566ull, 12ull, 256ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 1u, 8u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 66ull}, {0}}},
    {"DXT5 one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 574ull, 20ull, 256ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 16u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 75ull}, {0}}},
    {"YCoCg one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 574ull, 20ull, 256ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 16u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 75ull}, {0}}},
    {"RGTC1 one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {8ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 12ull, 256ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 8u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 66ull}, {0}}},
    {"BC7 one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16ul, 0ul}, {BC7, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 20ull, 256ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xcu, 1u, 1u, 16u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 75ull}, {0}}},
    {"BC6H unsigned one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16ul, 0ul}, {BC6U, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 20ull, 256ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x2u, 1u, 1u, 16u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 75ull}, {0}}},
    {"BC6H signed one block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16ul, 0ul}, {BC6S, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 20ull, 256ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x3u, 1u, 1u, 16u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 75ull}, {0}}},
    {"DXT5 100001 bytes, 1 chunk (odd: bytes)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {100001ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 13u, 1u, 13u, 1u, 8784u, 0u, 0ull, 100005ull, 100096ull, {0x1u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xeu, 1u, 1u, 100001u, 4u, 13u, 0u, 0u, 0u, 0u, 0u, 116724ull}, {0}}},
    {"DXT1 100001 bytes, 65 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {100001ul, 0ul}, {DXT1, 0}, {1u, 0u}, {65u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {65u, 0u}, 13u, 0x0u, 0u, 50u, 50u, 50u, 50u, 8784u, 1u, 126529ull, 100005ull, 100096ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 50u, 2000u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 118520ull}, {0}}},
    {"DXT5 8 bytes, 16 chunks (no block per chunk: stored)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {8ul, 0ul}, {DXT5, 0}, {1u, 0u}, {16u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {16u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 12ull, 256ull, {0x0u, 0x0u, 0x0u, 1u}, 0, 0,
     {{0xeu, 0u, 1u, 8u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 612ull}, {0}}},
    {"RGTC1 2 MiB less a block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2097144ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 256u, 1u, 256u, 1u, 8784u, 0u, 0ull, 2097148ull, 2097152ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 2097144u, 4u, 256u, 1u, 0u, 0u, 0u, 0u, 2446725ull}, {0}}},
    {"RGTC1 2 MiB, no index (windowed)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x0u, 1u, {2097152ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x0u, {1u, 0u}, 13u, 0x0u, 0u, 256u, 1u, 256u, 1u, 8784u, 1u, 2179102ull, 2097156ull, 2097152ull, {0x0u, 0x40u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 2097152u, 4u, 256u, 1u, 6u, 0u, 0u, 1u, 2446734ull}, {0}}},
    {"YCoCg 1 MiB, no index (windowed)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x0u, 1u, {1048576ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x0u, {1u, 0u}, 13u, 0x0u, 0u, 128u, 1u, 128u, 1u, 8784u, 1u, 1089566ull, 1048580ull, 1048576ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 1048576u, 4u, 128u, 1u, 4u, 0u, 0u, 1u, 1223395ull}, {0}}},
    {"DXT1 1 MiB, no index (not windowed)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x0u, 1u, {1048576ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x0u, {1u, 0u}, 13u, 0x0u, 0u, 128u, 1u, 128u, 1u, 8784u, 1u, 1089566ull, 1048580ull, 1048576ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 0,
     {{0xbu, 1u, 1u, 1048576u, 4u, 128u, 2u, 2u, 0u, 0u, 0u, 1223395ull}, {0}}},
    {"BC7 1 MiB (windowed)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {1048576ul, 0ul}, {BC7, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 128u, 1u, 128u, 1u, 8784u, 0u, 0ull, 1048580ull, 1048576ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xcu, 1u, 1u, 1048576u, 4u, 128u, 1u, 0u, 0u, 0u, 1u, 1223395ull}, {0}}},
    {"YCoCg 16 MiB, stored", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16777216ul, 0ul}, {YCOCG, 0}, {0u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 2048u, 1u, 2048u, 1u, 8784u, 0u, 0ull, 16777224ull, 16777216ull, {0x0u, 0x0u, 0x0u, 1u}, 0, 0,
     {{0xfu, 0u, 1u, 16777216u, 8u, 2048u, 0u, 0u, 0u, 0u, 1u, 16777241ull}, {0}}},
    {"YCoCg 16 MiB less the tables (8-byte header by them)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {16773120ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 2048u, 1u, 2048u, 1u, 8784u, 1u, 17838118ull, 16773128ull, 16773120ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 16773120u, 8u, 2048u, 1u, 4u, 1u, 0u, 0u, 19568697ull}, {0}}},
    {"YCoCg + RGTC1 16 MiB + 8 MiB (8-byte outer header)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {16777216ul, 8388608ul}, {YCOCG, RGTC1}, {1u, 1u}, {16u, 16u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {16u, 16u}, 13u, 0x0u, 8u, 3072u, 32u, 2048u, 16u, 8784u, 0u, 0ull, 25165844ull, 25165824ull, {0x0u, 0x50u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 16u, 1048576u, 8u, 128u, 1u, 4u, 1u, 0u, 0u, 19574020ull}, {0x1u, 1u, 16u, 524288u, 4u, 64u, 1u, 6u, 1u, 0u, 0u, 9787316ull}}},
    {"DXT5 1 GiB, 1 chunk (tables beyond 24 bits)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {1073741824ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     1u, 0},
    {"DXT5 4 GiB less a block, no index (extent beyond 32 bits)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x0u, 1u, {4294967280ul, 0ul}, {DXT5, 0}, {1u, 0u}, {64u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x0u, {64u, 0u}, 13u, 0x0u, 0u, 524299u, 43u, 524299u, 43u, 8784u, 0u, 0ull, 4294967288ull, 4294967296ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 0,
     {{0xeu, 1u, 43u, 99882960u, 8u, 12193u, 1u, 4u, 0u, 0u, 1u, 5010796771ull}, {0}}},
    {"YCoCg 64x64, 3 chunks (limited to 2)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {3u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {3u, 0u}, 13u, 0x0u, 0u, 2u, 2u, 2u, 2u, 8784u, 1u, 5184ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 2u, 2048u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4872ull}, {0}}},
    {"YCoCg 64x64, 65 chunks (limited to 64)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {65u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {65u, 0u}, 13u, 0x0u, 0u, 64u, 64u, 64u, 64u, 8784u, 1u, 38044ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 64u, 64u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 7124ull}, {0}}},
    {"YCoCg 1080p, 3 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {3u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {3u, 0u}, 13u, 0x0u, 0u, 255u, 3u, 255u, 3u, 8784u, 1u, 2206258ull, 2073604ull, 2073600ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 3u, 691200u, 4u, 85u, 1u, 4u, 1u, 0u, 0u, 2419331ull}, {0}}},
    {"YCoCg 64x64, coarse (no layout for it)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x3u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x3u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x4u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 2u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"DXT1 64x64, coarse", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x3u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x3u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 2606ull, 2052ull, 2048ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 1u, 2048u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 2446ull}, {0}}},
    {"BC6H unsigned 64x64, coarse", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x3u, 1u, {4096ul, 0ul}, {BC6U, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x3u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x100u, 0x0u, 1u}, 1, 1,
     {{0x2u, 1u, 1u, 4096u, 4u, 1u, 2u, 8u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"BC6H signed 64x64, coarse, no index", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x2u, 1u, {4096ul, 0ul}, {BC6S, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x2u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4446ull, 4100ull, 4096ull, {0x0u, 0x100u, 0x0u, 1u}, 1, 0,
     {{0x3u, 1u, 1u, 4096u, 4u, 1u, 2u, 8u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"BC7 100001 bytes, coarse, 1 chunk", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x3u, 1u, {100001ul, 0ul}, {BC7, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x3u, {1u, 0u}, 13u, 0x0u, 0u, 13u, 1u, 13u, 1u, 8784u, 0u, 0ull, 100005ull, 100096ull, {0x1u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xcu, 1u, 1u, 100001u, 4u, 13u, 0u, 0u, 0u, 0u, 0u, 116724ull}, {0}}},
    {"YCoCg 1080p, smaller files + fine chunks (fine ignored)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0xdu, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {4u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0xcu, {4u, 0u}, 16u, 0x0u, 0u, 32u, 4u, 32u, 4u, 67920u, 0u, 0ull, 2073604ull, 2073600ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 4u, 518400u, 4u, 8u, 1u, 0u, 0u, 0u, 0u, 2419368ull}, {0}}},
    {"YCoCg 1080p, smaller files, pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x5u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {4u, 0u}, SRC_RGBA8, 1920u, 1080u, 7680ul,
     0u, 1, 0x4u, {4u, 0u}, 16u, 0x0u, 0u, 32u, 4u, 32u, 4u, 67920u, 0u, 0ull, 2073604ull, 2073600ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 4u, 518400u, 4u, 8u, 1u, 0u, 0u, 0u, 0u, 2419368ull}, {0}}},
    {"YCoCg 1080p, fine chunks, pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x9u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 1920u, 1080u, 7680ul,
     0u, 1, 0x9u, {270u, 0u}, 13u, 0x0u, 0u, 270u, 270u, 270u, 270u, 8784u, 0u, 0ull, 2073604ull, 2073600ull, {0x0u, 0x0u, 0x8u, 1u}, 1, 1,
     {{0xfu, 1u, 270u, 7680u, 4u, 1u, 1u, 4u, 1u, 3u, 0u, 2429210ull}, {0}}},
    {"DXT1 64x64, fine chunks, stored (count kept)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x9u, 1u, {2048ul, 0ul}, {DXT1, 0}, {0u, 0u}, {2u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x9u, {2u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 2052ull, 2048ull, {0x0u, 0x0u, 0x0u, 1u}, 0, 0,
     {{0xbu, 0u, 1u, 2048u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 2078ull}, {0}}},
    {"YCoCg + RGTC1 1080p, fine chunks, second stored", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x9u, 2u, {2073600ul, 1036800ul}, {YCOCG, RGTC1}, {1u, 0u}, {0u, 5u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x9u, {270u, 5u}, 13u, 0x0u, 4u, 397u, 271u, 270u, 270u, 8784u, 0u, 0ull, 3110412ull, 3110400ull, {0x0u, 0x10u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 270u, 7680u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 2429210ull}, {0x1u, 0u, 1u, 1036800u, 4u, 127u, 0u, 0u, 0u, 0u, 0u, 1036845ull}}},
    {"YCoCg 64x64, refine, textures (no job: not looked at)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x21u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x21u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, refine, pictures (still fused)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x21u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x21u, {1u, 0u}, 13u, 0x2u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x0u, 0x8u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 3u, 0u, 4835ull}, {0}}},
    {"YCoCg + RGTC1 64x64, refine, pictures (two textures: not looked at)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x21u, 2u, {4096ul, 2048ul}, {YCOCG, RGTC1}, {1u, 1u}, {1u, 1u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x21u, {1u, 1u}, 13u, 0x0u, 4u, 2u, 2u, 1u, 1u, 8784u, 0u, 0ull, 6156ull, 6144ull, {0x2u, 0x10u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0x1u, 1u, 1u, 2048u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2446ull}}},
    {"YCoCg + RGTC1 64x64, first stored", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {4096ul, 2048ul}, {YCOCG, RGTC1}, {0u, 1u}, {1u, 2u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 2u}, 13u, 0x0u, 4u, 3u, 3u, 2u, 2u, 8784u, 0u, 0ull, 6156ull, 6144ull, {0x2u, 0x0u, 0x0u, 2u}, 1, 0,
     {{0xfu, 0u, 1u, 4096u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 4121ull}, {0x1u, 1u, 2u, 1024u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2482ull}}},
    {"YCoCg + RGTC1 64x64, both stored", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {4096ul, 2048ul}, {YCOCG, RGTC1}, {0u, 0u}, {1u, 1u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 1u}, 13u, 0x0u, 4u, 2u, 2u, 1u, 1u, 8784u, 0u, 0ull, 6156ull, 6144ull, {0x0u, 0x0u, 0x0u, 2u}, 0, 0,
     {{0xfu, 0u, 1u, 4096u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 4121ull}, {0x1u, 0u, 1u, 2048u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 2073ull}}},
    {"YCoCg + RGTC1 2048x2048", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {4194304ul, 2097152ul}, {YCOCG, RGTC1}, {1u, 1u}, {16u, 16u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {16u, 16u}, 13u, 0x0u, 4u, 768u, 32u, 512u, 16u, 8784u, 0u, 0ull, 6291468ull, 6291456ull, {0x0u, 0x50u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 16u, 262144u, 4u, 32u, 1u, 4u, 1u, 0u, 0u, 4893956ull}, {0x1u, 1u, 16u, 131072u, 4u, 16u, 1u, 6u, 1u, 0u, 0u, 2447284ull}}},
    {"RGTC1 + DXT5 64x64", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 2u, {2048ul, 4096ul}, {RGTC1, DXT5}, {1u, 1u}, {1u, 1u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 1u}, 13u, 0x0u, 4u, 2u, 2u, 1u, 1u, 8784u, 0u, 0ull, 6156ull, 6144ull, {0x2u, 0x10u, 0x0u, 2u}, 1, 1,
     {{0x1u, 1u, 1u, 2048u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2446ull}, {0xeu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}}},
    {"YCoCg 64x64, pictures whose rows are no multiple of 4", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 258ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, pictures of 4 GiB", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 4096u, 1048576ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg, pictures narrower than a block", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 2u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, tensors", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_TENSOR, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"DXT5 64x64, tensors, refine", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x21u, 1u, {4096ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_TENSOR, 64u, 64u, 256ul,
     0u, 1, 0x21u, {1u, 0u}, 13u, 0x2u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, NV12", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NV12, 64u, 64u, 64ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"DXT1 64x64, NV12", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NV12, 64u, 64u, 64ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 2606ull, 2052ull, 2048ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 1u, 2048u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 2446ull}, {0}}},
    {"BC6H unsigned 64x64, RGBA16F pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {BC6U, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA16F, 64u, 64u, 512ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x2u, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"RGTC1 64x64, A8 pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_A8, 64u, 64u, 64ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 2052ull, 2048ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 2048u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2446ull}, {0}}},
    {"DXT1 64x64, pictures (never fused)", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 2606ull, 2052ull, 2048ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0xbu, 1u, 1u, 2048u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 2446ull}, {0}}},
    {"BC7 64x64, pictures", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {BC7, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xcu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, pictures, stored", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {0u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x0u, 0x0u, 0x0u, 1u}, 0, 0,
     {{0xfu, 0u, 1u, 4096u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 4121ull}, {0}}},
    {"YCoCg 1080p, pictures, 65 chunks", {13u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {65u, 0u}, SRC_RGBA8, 1920u, 1080u, 7680ul,
     0u, 1, 0x1u, {65u, 0u}, 13u, 0x0u, 0u, 256u, 64u, 256u, 64u, 8784u, 1u, 2207388ull, 2073604ull, 2073600ull, {0x0u, 0x0u, 0x8u, 1u}, 1, 1,
     {{0xfu, 1u, 64u, 32400u, 4u, 4u, 1u, 4u, 1u, 3u, 0u, 2421588ull}, {0}}},
    {"YCoCg 64x64, frag_log2 16", {16u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 16u, 0x0u, 0u, 1u, 1u, 1u, 1u, 67920u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 1080p, frag_log2 12, pictures", {12u, 0u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {4u, 0u}, SRC_RGBA8, 1920u, 1080u, 7680ul,
     0u, 1, 0x1u, {4u, 0u}, 12u, 0x0u, 0u, 508u, 4u, 508u, 4u, 4560u, 0u, 0ull, 2073604ull, 2073600ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 4u, 518400u, 4u, 127u, 1u, 0u, 0u, 0u, 0u, 2419368ull}, {0}}},
    {"DXT1 64x64, byte_granular", {13u, 1u, 0u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 2052ull, 2048ull, {0x1u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xbu, 1u, 1u, 2048u, 4u, 1u, 0u, 0u, 0u, 0u, 0u, 2446ull}, {0}}},
    {"DXT1 64x64, position_lanes", {13u, 0u, 1u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {DXT1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 2052ull, 2048ull, {0x4u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xbu, 1u, 1u, 2048u, 4u, 1u, 2u, 0u, 0u, 0u, 0u, 2446ull}, {0}}},
    {"YCoCg 64x64, position_lanes, pictures", {13u, 0u, 1u, 26u, 0u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 4835ull}, {0}}},
    {"RGTC1 64x64, rgtc1_fields 44", {13u, 0u, 0u, 44u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 2606ull, 2052ull, 2048ull, {0x0u, 0x4u, 0x0u, 1u}, 1, 1,
     {{0x1u, 1u, 1u, 2048u, 4u, 1u, 2u, 2u, 1u, 0u, 0u, 2446ull}, {0}}},
    {"RGTC1 64x64, rgtc1_fields 0", {13u, 0u, 0u, 0u, 0u, 0u, 1u}, 0x1u, 1u, {2048ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 2052ull, 2048ull, {0x2u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 2048u, 4u, 1u, 1u, 0u, 0u, 0u, 0u, 2446ull}, {0}}},
    {"RGTC1 100004 bytes, rgtc1_fields 44 (chunks of 4 mod 8)", {13u, 0u, 0u, 44u, 0u, 0u, 1u}, 0x1u, 1u, {100004ul, 0ul}, {RGTC1, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 13u, 1u, 13u, 1u, 8784u, 0u, 0ull, 100008ull, 100096ull, {0x4u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0x1u, 1u, 1u, 100004u, 4u, 13u, 2u, 0u, 0u, 0u, 0u, 116728ull}, {0}}},
    {"YCoCg + RGTC1 2048x2048, rgtc1_fields 44", {13u, 0u, 0u, 44u, 0u, 0u, 1u}, 0x1u, 2u, {4194304ul, 2097152ul}, {YCOCG, RGTC1}, {1u, 1u}, {16u, 16u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {16u, 16u}, 13u, 0x0u, 4u, 768u, 32u, 512u, 16u, 8784u, 0u, 0ull, 6291468ull, 6291456ull, {0x0u, 0x14u, 0x0u, 2u}, 1, 1,
     {{0xfu, 1u, 16u, 262144u, 4u, 32u, 1u, 4u, 1u, 0u, 0u, 4893956ull}, {0x1u, 1u, 16u, 131072u, 4u, 16u, 2u, 2u, 1u, 0u, 0u, 2447284ull}}},
    {"YCoCg 64x64, no_half_tiles, pictures", {13u, 0u, 0u, 26u, 1u, 0u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4458ull, 4100ull, 4096ull, {0x0u, 0x0u, 0x8u, 1u}, 1, 0,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 0u, 3u, 0u, 4835ull}, {0}}},
    {"YCoCg 1080p, no_half_tiles (windowed)", {13u, 0u, 0u, 26u, 1u, 0u, 1u}, 0x1u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {4u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {4u, 0u}, 13u, 0x0u, 0u, 256u, 4u, 256u, 4u, 8784u, 1u, 2156612ull, 2073604ull, 2073600ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 4u, 518400u, 4u, 64u, 1u, 4u, 0u, 0u, 1u, 2419368ull}, {0}}},
    {"YCoCg 64x64, no_fusion, pictures", {13u, 0u, 0u, 26u, 0u, 1u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"DXT5 64x64, no_fusion, pictures", {13u, 0u, 0u, 26u, 0u, 1u, 1u}, 0x1u, 1u, {4096ul, 0ul}, {DXT5, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 1u, 4654ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xeu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, placing refused", {13u, 0u, 0u, 26u, 0u, 0u, 0u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_NONE, 0u, 0u, 0ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x0u, 0x10u, 0x0u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 0u, 0u, 4835ull}, {0}}},
    {"YCoCg 64x64, placing refused, pictures", {13u, 0u, 0u, 26u, 0u, 0u, 0u}, 0x1u, 1u, {4096ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {1u, 0u}, SRC_RGBA8, 64u, 64u, 256ul,
     0u, 1, 0x1u, {1u, 0u}, 13u, 0x0u, 0u, 1u, 1u, 1u, 1u, 8784u, 0u, 0ull, 4100ull, 4096ull, {0x0u, 0x0u, 0x8u, 1u}, 1, 1,
     {{0xfu, 1u, 1u, 4096u, 4u, 1u, 1u, 4u, 1u, 3u, 0u, 4835ull}, {0}}},
    {"everything off, YCoCg 1080p, pictures", {13u, 1u, 1u, 0u, 1u, 1u, 0u}, 0x1u, 1u, {2073600ul, 0ul}, {YCOCG, 0}, {1u, 0u}, {4u, 0u}, SRC_RGBA8, 1920u, 1080u, 7680ul,
     0u, 1, 0x1u, {4u, 0u}, 13u, 0x0u, 0u, 256u, 4u, 256u, 4u, 8784u, 0u, 0ull, 2073604ull, 2073600ull, {0x1u, 0x0u, 0x0u, 1u}, 1, 0,
     {{0xfu, 1u, 4u, 518400u, 4u, 64u, 0u, 0u, 0u, 0u, 1u, 2419368ull}, {0}}},
};

static unsigned long failures, checks;
static const char *what = "";
#define CHECK(cond) do { checks++; if (!(cond)) { failures++; fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, what); } } while (0)

static const hap_encode_source *source_of(hap_encode_source *s, int kind, unsigned width, unsigned height, unsigned long row_bytes)
{
    if (kind == SRC_NONE)
        return NULL;
    s->picture_kind = kind == SRC_RGBA16F ? HAPGPU_PICTURE_RGBA16F : kind == SRC_A8 ? HAPGPU_PICTURE_A8 : HAPGPU_PICTURE_RGBA8;
    s->planes = kind == SRC_TENSOR;
    s->video = kind == SRC_NV12;
    s->width = width;
    s->height = height;
    s->row_bytes = row_bytes;
    return s;
}

static hap_encode_knobs knobs_of(const unsigned *k)
{
    hap_encode_knobs knobs;
    knobs.frag_log2 = k[0];
    knobs.byte_granular = k[1];
    knobs.position_lanes = k[2];
    knobs.rgtc1_fields = k[3];
    knobs.no_half_tiles = k[4];
    knobs.no_fusion = k[5];
    knobs.placing_allowed = k[6];
    return knobs;
}

static void equals_recording(const hap_encode_plan *p, unsigned rc, const recorded_plan *r)
{
    unsigned i;
    CHECK(rc == r->rc);
    if (rc != HapResult_No_Error || !r->planned) {
        CHECK(rc != HapResult_No_Error && !r->planned);
        return;
    }
    CHECK(p->flags == r->flags_out && p->frag_log2 == r->frag_log2 && p->refine == r->refine);
    CHECK(p->outer_header == r->outer_header && p->frags_per_frame == r->frags_per_frame && p->chunks_per_frame == r->chunks_per_frame);
    CHECK(p->max_frags_per_tex == r->max_frags_per_tex && p->max_chunks_per_tex == r->max_chunks_per_tex);
    CHECK(p->slot_stride == r->slot_stride);
    CHECK(p->placed == r->placed && p->placed_extent == r->placed_extent);
    CHECK(p->frame_raw_bound == r->frame_raw_bound && p->stage_in_bytes == r->stage_in_bytes);
    CHECK(p->kinds.granularities == r->kinds[0] && p->kinds.layouts == r->kinds[1] && p->kinds.fused == r->kinds[2] &&
          p->kinds.textures == r->kinds[3]);
    CHECK(p->any_snappy == r->any_snappy && p->any_half_tiles == r->any_half_tiles);
    for (i = 0; i < r->count; i++) {
        const hap_encode_tex *t = &p->tex[i];
        const recorded_tex *e = &r->tex[i];
        CHECK(p->chunk_counts[i] == r->chunks_out[i]);
        CHECK(t->format == r->formats[i] && t->bytes == r->bytes[i] && t->nibble == e->nibble && t->compressor == e->compressor);
        CHECK(t->chunk_count == e->chunk_count && t->chunk_bytes == e->chunk_bytes && t->header_len == e->header_len && t->fpc == e->fpc);
        CHECK(t->gran_log2 == e->gran_log2 && t->layout == e->layout && t->half_tiles == e->half_tiles && t->fused == e->fused);
        CHECK(t->windowed == e->windowed && t->bound == e->bound);
    }
}

/* what holds of every plan, whatever the recording says */
static void invariants(const hap_encode_plan *p, const hap_encode_knobs *k, unsigned count, const hap_encode_source *source)
{
    unsigned i, placed, kinds_g = 0, kinds_l = 0, kinds_f = 0, frags = 0, chunks = 0;
    for (i = 0; i < count; i++) {
        const hap_encode_tex *t = &p->tex[i];
        const unsigned unit = t->layout == HAPGPU_LAYOUT_2_6_4_4 || t->layout == HAPGPU_LAYOUT_4_4_4_4 ? 16u : 8u;
        for (placed = 0; placed < 2u; placed++) {
            /* the control word reads back field by field */
            const uint32_t w = hap_encode_plan_control(p, i, placed);
            CHECK(hapgpu_control_granularity_log2(w) == t->gran_log2 && t->gran_log2 <= 2u);
            CHECK(hapgpu_control_window_256(w) == (t->windowed ? HAP_FRAGMENT_WINDOW_256 : 0u));
            CHECK(hapgpu_control_layout(w) == t->layout);
            CHECK(hapgpu_control_half_tiles(w) == t->half_tiles);
            CHECK(hapgpu_control_fused(w) == t->fused);
            CHECK(hapgpu_control_placed(w) == (i == 0u ? placed : 0u));
            CHECK(w == hapgpu_control(hapgpu_control_granularity_log2(w), hapgpu_control_window_256(w), hapgpu_control_layout(w),
                                      hapgpu_control_half_tiles(w), hapgpu_control_fused(w), hapgpu_control_placed(w)));
        }
        CHECK(t->layout == HAPGPU_LAYOUT_NONE || t->layout == HAPGPU_LAYOUT_4_4 || t->layout == HAPGPU_LAYOUT_2_6_4_4 ||
              t->layout == HAPGPU_LAYOUT_2_6 || t->layout == HAPGPU_LAYOUT_4_4_4_4);
        /* a layout: default fragments, whole units per chunk, a Snappy texture */
        if (t->layout != HAPGPU_LAYOUT_NONE)
            CHECK(p->frag_log2 == 13u && t->chunk_bytes % unit == 0 && t->compressor == HapCompressorSnappy && t->gran_log2 != 0u);
        if (t->half_tiles)
            CHECK(t->layout != HAPGPU_LAYOUT_NONE && (p->flags & HAPGPU_ENCODE_FRAGMENT_INDEX) && !k->no_half_tiles);
        /* (a table of group tables is decoded over a whole-fragment ring) */
        if (t->windowed)
            CHECK(!t->half_tiles && p->frag_log2 == 13u);
        if (t->fused)
            CHECK(count == 1u && source && source->picture_kind == HAPGPU_PICTURE_RGBA8 && !source->planes && !source->video &&
                  source->row_bytes % 4u == 0 && t->layout == HAPGPU_LAYOUT_2_6_4_4 && !k->no_fusion &&
                  (t->fused == HAPGPU_FUSED_YCOCG ? t->format == HapTextureFormat_YCoCg_DXT5
                                                  : t->fused == HAPGPU_FUSED_DXT5 && t->format == HapTextureFormat_RGBA_DXT5 && !p->refine));
        CHECK(t->chunk_count >= 1u && (size_t)t->chunk_count * t->chunk_bytes <= t->bytes);
        CHECK((size_t)t->fpc << p->frag_log2 >= t->chunk_bytes && (t->fpc == 0u || ((size_t)t->fpc - 1u) << p->frag_log2 < t->chunk_bytes));
        CHECK(t->header_len == 4u || t->header_len == 8u);
        if (t->compressor == HapCompressorSnappy) {
            if (t->fused) kinds_f |= 1u << t->fused;
            else if (t->layout) kinds_l |= 1u << t->layout;
            else kinds_g |= 1u << t->gran_log2;
        }
        frags += t->chunk_count * t->fpc;
        chunks += t->chunk_count;
    }
    /* every Snappy texture is some kernel's, and no kernel is started for nothing */
    CHECK(p->kinds.granularities == kinds_g && p->kinds.layouts == kinds_l && p->kinds.fused == kinds_f && p->kinds.textures == count);
    CHECK((p->any_snappy != 0) == ((kinds_g | kinds_l | kinds_f) != 0u));
    CHECK(p->frags_per_frame == frags && p->chunks_per_frame == chunks);
    CHECK(p->slot_stride % 16u == 0 && p->slot_stride >= (1u << p->frag_log2) + (1u << p->frag_log2) / 32u + 64u + HAPGPU_SLOT_SCRATCH_BYTES);
    CHECK((count == 2u) == (p->outer_header != 0u));
    if (p->placed) {
        CHECK(k->placing_allowed && count == 1u && p->tex[0].compressor == HapCompressorSnappy &&
              p->tex[0].layout != HAPGPU_LAYOUT_NONE && p->tex[0].chunk_count <= 64u);
        CHECK(p->placed_extent >= p->frame_raw_bound && p->placed_extent <= 0xFFFFFFFFul);
    } else {
        CHECK(p->placed_extent == 0);
    }
    if (p->flags & HAPGPU_ENCODE_SMALLER_FILES)
        CHECK(!(p->flags & HAPGPU_ENCODE_FRAGMENT_INDEX) && p->frag_log2 == 16u);
}

int main(void)
{
    static const unsigned formats[] = {DXT1, DXT5, YCOCG, RGTC1, BC7, BC6U, BC6S};
    static const unsigned long blocks[] = {1ul, 256ul, 6250ul, 8100ul, 1ul << 17, 1ul << 20};
    static const unsigned chunk_counts[] = {1u, 3u, 65u};
    static const unsigned flag_sets[] = {0u, IDX, IDX | COARSE, IDX | SMALLER, IDX | FINE, IDX | REFINE, COARSE | FINE, IDX | SMALLER | FINE};
    static const unsigned knob_sets[][7] = {{13u, 0u, 0u, 26u, 0u, 0u, 1u}, {12u, 0u, 0u, 26u, 0u, 0u, 1u}, {16u, 0u, 0u, 26u, 0u, 0u, 1u},
                                            {13u, 1u, 0u, 26u, 0u, 0u, 1u}, {13u, 0u, 1u, 26u, 0u, 0u, 1u}, {13u, 0u, 0u, 44u, 0u, 0u, 1u},
                                            {13u, 0u, 0u, 0u, 0u, 0u, 1u},  {13u, 0u, 0u, 26u, 1u, 0u, 1u}, {13u, 0u, 0u, 26u, 0u, 1u, 1u},
                                            {13u, 0u, 0u, 26u, 0u, 0u, 0u}, {13u, 1u, 1u, 44u, 1u, 1u, 0u}};
    unsigned long walked = 0;
    unsigned i, fi, bi, ci, gi, ki, two;
    int si;
    char label[160];

    /* 1. the recording */
    for (i = 0; i < sizeof(recorded) / sizeof(recorded[0]); i++) {
        const recorded_plan *r = &recorded[i];
        const hap_encode_knobs knobs = knobs_of(r->knobs);
        hap_encode_source s;
        const hap_encode_source *source = source_of(&s, r->source, r->width, r->height, r->row_bytes);
        hap_encode_plan p;
        const unsigned rc = hap_encode_plan_of(&p, &knobs, r->flags, r->count, r->bytes, r->formats, r->compressors, r->chunks, source);
        what = r->name;
        equals_recording(&p, rc, r);
        if (rc == HapResult_No_Error)
            invariants(&p, &knobs, r->count, source);
    }
    /* 2. the invariants over a product of the same axes: one texture, and with an RGTC1 plane of half its blocks' bytes
       behind a 16-byte colour texture */
    what = label;
    for (fi = 0; fi < sizeof(formats) / sizeof(formats[0]); fi++)
        for (bi = 0; bi < sizeof(blocks) / sizeof(blocks[0]); bi++)
            for (ci = 0; ci < sizeof(chunk_counts) / sizeof(chunk_counts[0]); ci++)
                for (gi = 0; gi < sizeof(flag_sets) / sizeof(flag_sets[0]); gi++)
                    for (ki = 0; ki < sizeof(knob_sets) / sizeof(knob_sets[0]); ki++)
                        for (si = 0; si < SRC_KINDS; si++)
                            for (two = 0; two < 2u; two++) {
                                const hap_encode_knobs knobs = knobs_of(knob_sets[ki]);
                                const unsigned long block = (unsigned long)hapf_block_bytes(formats[fi]);
                                const unsigned long bytes[2] = {blocks[bi] * block + (bi == 2u ? 1ul : 0ul), blocks[bi] * 8ul};
                                const unsigned fmts[2] = {formats[fi], RGTC1};
                                const unsigned comps[2] = {HapCompressorSnappy, two == 1u && (ci & 1u) ? HapCompressorNone : HapCompressorSnappy};
                                const unsigned counts[2] = {chunk_counts[ci], chunk_counts[(ci + 1u) % 3u]};
                                const unsigned count = 1u + two;
                                hap_encode_source s;
                                const hap_encode_source *source = source_of(&s, si, 64u, 64u, (gi & 1u) ? 256ul : 258ul);
                                hap_encode_plan p;
                                unsigned rc;
                                if (two && formats[fi] != YCOCG)
                                    continue;
                                snprintf(label, sizeof(label), "format 0x%x, %lu bytes, %u chunks, flags 0x%x, switches %u, source %d, %u textures",
                                         formats[fi], bytes[0], counts[0], flag_sets[gi], ki, si, count);
                                rc = hap_encode_plan_of(&p, &knobs, flag_sets[gi], count, bytes, fmts, comps, counts, source);
                                CHECK(rc == HapResult_No_Error || rc == HapResult_Bad_Arguments);
                                if (rc == HapResult_No_Error)
                                    invariants(&p, &knobs, count, source);
                                walked++;
                            }
    if (failures) {
        fprintf(stderr, "%lu of %lu checks failed\n", failures, checks);
        return 1;
    }
    printf("%u recorded plans equal, %lu plans walked, %lu checks: ok\n", (unsigned)(sizeof(recorded) / sizeof(recorded[0])), walked, checks);
    return 0;
}
