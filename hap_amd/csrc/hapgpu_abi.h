/*
 * hapgpu_abi.h -- the thin C ABI between the host-side C code (hap_api.c,
 * hap_batch.c, hap_frame.c: pure C99, no HIP headers) and the HIP translation
 * unit (hapgpu_runtime.hip + kernels).  Plain pointers, integers and PODs
 * only.  Structures marked [device] are laid out identically for gcc/clang
 * host code and hipcc device code (fixed-width members, natural alignment).
 */
#ifndef HAPGPU_ABI_H
#define HAPGPU_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Environment switches that exist for A/B measurements only (copy kernels against hipMemcpyAsync, ring sizes, compressor
   layouts ...) are read by measurement builds (tools/build_variants.sh, -DHAP_MEASUREMENT_BUILD); the product library does
   not look at them: every switch it does read is listed in INTEGRATION.md and exercised by a test
   (tests/test_cabi_cpu.py::test_every_environment_switch_is_documented_and_tested). */
#ifdef HAP_MEASUREMENT_BUILD
#define HAP_AB_ENV(name) getenv(name)
#else
#define HAP_AB_ENV(name) ((const char *)0)
#endif

/* ---- container constants (reference hap.c:41-51, 84-88) ---- */
#define HAP_NIBBLE_NONE 0xAu
#define HAP_NIBBLE_SNAPPY 0xBu
#define HAP_NIBBLE_COMPLEX 0xCu
#define HAP_SECTION_MULTI 0x0Du
#define HAP_SECTION_INSTRUCTIONS 0x01u
#define HAP_SECTION_COMPRESSORS 0x02u
#define HAP_SECTION_SIZES 0x03u
#define HAP_SECTION_OFFSETS 0x04u
#define HAP_SECTION_FRAGMENTS 0x46u   /* private: hap_gpu.h */
#define HAP_FRAGMENT_TABLE_VERSION 1u       /* fragment sizes only */
#define HAP_FRAGMENT_TABLE_VERSION_FIELDS 4u /* + a group table per fragment: "field streams".  (Version 2, one byte per
                                                half-tile, and version 3, 96-byte group tables without the groups' output
                                                bytes, were written by earlier builds: version 2 tables are ignored, of
                                                version 3 the fragment sizes are used.) */
#define HAP_FRAGMENT_TABLE_VERSION_FIELDS_R4 3u
#define HAP_GROUP_TABLE_BYTES_R4 96u
#define HAP_GROUP_TABLE_BYTES 196u           /* 64 groups of equally many elements, 24 bits each -- compressed bytes |
                                                output bytes << 12 -- then LE16 element count, LE16 zero */
#define HAP_HALF_TILE_BYTES 128u
#define HAP_HALF_TILES_PER_FRAGMENT 64u      /* 8 KiB fragments */

/* A fragment's slot in the compressor's scratch: at most 130 bytes per half-tile of elements, then a few bytes per
   lane that stores with nothing to write are pointed at (snappy_compress_blocks.hip) */
#define HAPGPU_SLOT_DATA_BYTES (HAP_HALF_TILES_PER_FRAGMENT * 130u)
#define HAPGPU_SLOT_SCRATCH_BYTES 272u

/* internal status codes beyond HapResult (never returned to API callers) */
#define HAPGPU_STATUS_INDEX_MISMATCH 100u /* fragment index inconsistent: redo without it */

/* ------------------------------------------------------------------ */
/* encode side                                                          */
/* ------------------------------------------------------------------ */

/* [device] one texture of one frame */
typedef struct HapGpuTexEnc {
    uint64_t src;            /* device address of the block-compressed texture */
    uint32_t bytes;          /* texture bytes */
    uint32_t format_nibble;  /* low nibble of the section type (hap.c:45-51) */
    uint32_t compressor;     /* 0 none, 1 snappy (hap.h:50-53) */
    uint32_t chunk_count;    /* already limited (hap.c:277-300) */
    uint32_t chunk_bytes;    /* bytes / chunk_count */
    uint32_t header_len;     /* 4 or 8 (hap.c:398-405, 425-428) */
    uint32_t frags_per_chunk;
    uint32_t frag_first;     /* global index of this texture's first fragment */
    uint32_t emit_index;     /* write the fragment-size section */
    uint32_t control;        /* what the host has decided for the compressor and the pack kernel: HAPGPU_CONTROL_* below */
    uint32_t frags_per_chunk_inv; /* HAPGPU_DIV_INV(frags_per_chunk) */
} HapGpuTexEnc;

/* The field layouts of the block compressor, by the value the file format gives them (the fragment table's byte 6,
   high nibble; hapf_texture_plan.frag_fields; HapGpuDecodeJob.fields_period; the kernels' LAYOUT): the one numbering. */
enum {
    HAPGPU_LAYOUT_NONE = 0,        /* a position per lane (snappy_compress.hip) */
    HAPGPU_LAYOUT_4_4 = 2,         /* DXT1: 8-byte blocks of [4, 4] */
    HAPGPU_LAYOUT_2_6_4_4 = 4,     /* DXT5 / YCoCg-DXT5: 16-byte blocks of [2, 6, 4, 4] */
    HAPGPU_LAYOUT_2_6 = 6,         /* RGTC1: 8-byte blocks of [2, 6] */
    HAPGPU_LAYOUT_4_4_4_4 = 8      /* opaque 16-byte blocks (BC7, BC6H) as four dwords */
};
/* What the block compressor makes from the frame's RGBA8 picture itself instead of reading it at src (and writes to src
   on the way): bc_encode_core.hpp's kFmt* + 1 (snappy_compress_blocks.hip asserts it). */
enum {
    HAPGPU_FUSED_NONE = 0,         /* the texture is at src */
    HAPGPU_FUSED_DXT1 = 1,
    HAPGPU_FUSED_DXT5 = 2,
    HAPGPU_FUSED_YCOCG = 3,        /* scaled YCoCg-DXT5 */
    HAPGPU_FUSED_RGTC1 = 4         /* from alpha */
};

/* HapGpuTexEnc.control, field by field.  Nobody shifts or masks the word but the functions below. */
#define HAPGPU_CONTROL_GRANULARITY_SHIFT 0u   /* granularity_log2 of the element stream: 0 = bytes, 1 = every position, offset
                                                 and length even (lets the decoder move 16 bits per lane), 2 = multiples of 4 */
#define HAPGPU_CONTROL_GRANULARITY_MASK 0xFFu
#define HAPGPU_CONTROL_WINDOW_SHIFT 8u        /* match window in 256-byte units (0 = whole fragment) */
#define HAPGPU_CONTROL_WINDOW_MASK 0xFFu
#define HAPGPU_CONTROL_LAYOUT_SHIFT 16u       /* HAPGPU_LAYOUT_* */
#define HAPGPU_CONTROL_LAYOUT_MASK 0xFu
#define HAPGPU_CONTROL_HALF_TILES_SHIFT 20u   /* "field stream": no element crosses a 128-byte half-tile and the compressor
                                                 writes every fragment's group table (fragment table version 4) */
#define HAPGPU_CONTROL_HALF_TILES_MASK 1u
#define HAPGPU_CONTROL_FUSED_SHIFT 24u        /* HAPGPU_FUSED_* */
#define HAPGPU_CONTROL_FUSED_MASK 7u
#define HAPGPU_CONTROL_PLACED_SHIFT 27u       /* "placed": the block-per-lane compressor writes every fragment's stream at its
                                                 final place in the frame (the sizes of everything before it: frag_sizes entries
                                                 with HAPGPU_FRAG_PUBLISHED set, chunk_acc words of the chunks before) instead of
                                                 a slot, on the assumption that every chunk shrinks; the pack kernel reports
                                                 HAPGPU_STATUS_NOT_PLACED for a frame where one did not (or a wavefront gave up
                                                 waiting), and the host encodes that frame again through slots.  First texture
                                                 of a frame only. */
#define HAPGPU_CONTROL_PLACED_MASK 1u
/* (const: values of their arguments alone -- a kernel's single combined test may hold them) */
#ifdef __HIP__
#define HAPGPU_ABI_INLINE static inline __attribute__((const)) __attribute__((host)) __attribute__((device))
#else
#define HAPGPU_ABI_INLINE static inline __attribute__((const))
#endif
#define HAPGPU_CONTROL_FIELD(control, NAME) (((control) >> HAPGPU_CONTROL_##NAME##_SHIFT) & HAPGPU_CONTROL_##NAME##_MASK)
HAPGPU_ABI_INLINE uint32_t hapgpu_control(unsigned granularity_log2, unsigned window_256, unsigned layout, unsigned half_tiles,
                                          unsigned fused, unsigned placed)
{
    return (uint32_t)(granularity_log2 << HAPGPU_CONTROL_GRANULARITY_SHIFT | window_256 << HAPGPU_CONTROL_WINDOW_SHIFT |
                      layout << HAPGPU_CONTROL_LAYOUT_SHIFT | half_tiles << HAPGPU_CONTROL_HALF_TILES_SHIFT |
                      fused << HAPGPU_CONTROL_FUSED_SHIFT | placed << HAPGPU_CONTROL_PLACED_SHIFT);
}
HAPGPU_ABI_INLINE unsigned hapgpu_control_granularity_log2(uint32_t control) { return HAPGPU_CONTROL_FIELD(control, GRANULARITY); }
HAPGPU_ABI_INLINE unsigned hapgpu_control_window_256(uint32_t control) { return HAPGPU_CONTROL_FIELD(control, WINDOW); }
HAPGPU_ABI_INLINE unsigned hapgpu_control_layout(uint32_t control) { return HAPGPU_CONTROL_FIELD(control, LAYOUT); }
HAPGPU_ABI_INLINE unsigned hapgpu_control_half_tiles(uint32_t control) { return HAPGPU_CONTROL_FIELD(control, HALF_TILES); }
HAPGPU_ABI_INLINE unsigned hapgpu_control_fused(uint32_t control) { return HAPGPU_CONTROL_FIELD(control, FUSED); }
HAPGPU_ABI_INLINE unsigned hapgpu_control_placed(uint32_t control) { return HAPGPU_CONTROL_FIELD(control, PLACED); }
/* 1: a texture of the position-per-lane compressor's kernel for granularity_log2 (no layout, that granularity): both
   fields in one comparison, which is that kernel's test */
HAPGPU_ABI_INLINE int hapgpu_control_is_positions(uint32_t control, unsigned granularity_log2)
{
    return (control & (HAPGPU_CONTROL_GRANULARITY_MASK << HAPGPU_CONTROL_GRANULARITY_SHIFT |
                       HAPGPU_CONTROL_LAYOUT_MASK << HAPGPU_CONTROL_LAYOUT_SHIFT)) ==
           (granularity_log2 << HAPGPU_CONTROL_GRANULARITY_SHIFT | (unsigned)HAPGPU_LAYOUT_NONE << HAPGPU_CONTROL_LAYOUT_SHIFT);
}

/* what the compressor's wavefronts divide by without dividing: floor(x inv / 2^32) is x / d or one short of it for
   every 32-bit x (d >= 1) */
#define HAPGPU_DIV_INV(d) (0xFFFFFFFFu / (uint32_t)(d))
#define HAPGPU_FRAG_PUBLISHED 0x80000000u
#define HAPGPU_STATUS_NOT_PLACED 0x7E50u

/* [device] one frame */
typedef struct HapGpuFrameEnc {
    uint64_t dst;            /* device address of the frame buffer */
    uint64_t dst_cap;
    uint32_t tex_count;      /* 1 or 2 */
    uint32_t outer_header_len; /* 0 (single texture), 4 or 8 (hap.c:562-576) */
    HapGpuTexEnc tex[2];
    /* results */
    uint64_t bytes_used;
    uint32_t status;
    uint32_t notes;          /* HAPGPU_FRAME_NOTE_*: what the kernels tell the host beside the status (zero before the launch) */
    /* textures whose control word names a HAPGPU_FUSED_* kind are made from this RGBA8 picture by the second stage itself */
    uint64_t rgba;
    uint32_t rgba_row_bytes; /* (the picture is smaller than 4 GiB) */
    uint32_t rgba_blocks_x;  /* width / 4 */
    uint32_t rgba_blocks_x_inv; /* HAPGPU_DIV_INV(rgba_blocks_x) */
    uint32_t reserved2;
    /* placed textures: one 64-bit word per chunk of the frame (zero before the launch), in which the compressor's
       wavefronts add up fragments << 32 | bytes as they learn their sizes */
    uint64_t chunk_acc;
} HapGpuFrameEnc;
/* a wavefront of a placed texture gave up waiting for its predecessors' sizes (snappy_compress_blocks.hip): the frame
   comes back HAPGPU_STATUS_NOT_PLACED for that reason, not for a chunk that did not shrink */
#define HAPGPU_FRAME_NOTE_WAVE_TIMED_OUT 1u

/* the layouts that hapgpu_abi.h promises the device: pinned (C99 has no static assertion: an array of negative size) */
typedef char hapgpu_abi_tex_enc_is_56_bytes[sizeof(HapGpuTexEnc) == 56 ? 1 : -1];
typedef char hapgpu_abi_frame_enc_is_184_bytes[sizeof(HapGpuFrameEnc) == 184 ? 1 : -1];
typedef char hapgpu_abi_control_is_at_44[offsetof(HapGpuTexEnc, control) == 44 ? 1 : -1];

/* [device] one byte-range move of the gather pass (one per fragment) */
typedef struct HapGpuCopyEntry {
    uint64_t src;
    uint64_t dst;
    uint32_t len;
    uint32_t reserved;
} HapGpuCopyEntry;

/* ------------------------------------------------------------------ */
/* decode side                                                          */
/* ------------------------------------------------------------------ */

/* [device] one chunk as listed by the frame's tables (hap.c:794-809) */
typedef struct HapGpuChunkIn {
    uint32_t src_off;        /* from the start of the payload ("frame_data") */
    uint32_t src_len;
    uint32_t codec;          /* compressor table byte; bit 31 set = not requested by the client */
    uint32_t unit_first;     /* first unit slot of this chunk (relative to the job) */
    uint32_t unit_count;     /* slots reserved for it */
    uint32_t frag_first;     /* first fragment-table entry of this chunk, if the frame has one */
    /* written by the plan kernel for the expansion kernel (one wavefront per chunk turns the chunk's
       fragment-table entries into units) */
    uint32_t plan_expand;    /* 1: expand with the fragment table */
    uint32_t plan_hdr;       /* bytes of the chunk's varint length prefix */
    uint32_t plan_out_len;   /* decoded bytes of the chunk */
    uint32_t reserved;
    uint64_t plan_out_off;   /* where they go, relative to the job's dst */
} HapGpuChunkIn;

#define HAPGPU_JOB_COMPLEX 0u
#define HAPGPU_JOB_SNAPPY 1u  /* 0xB_: one Snappy stream (hap.c:885-904) */
#define HAPGPU_JOB_RAW 2u     /* 0xA_ (hap.c:905-916) */

/* [device] one texture to decode */
typedef struct HapGpuDecodeJob {
    uint64_t payload;        /* device address of the first chunk's bytes */
    uint64_t payload_len;    /* bytes from payload to the end of the texture section */
    uint64_t dst;
    uint64_t dst_cap;
    uint64_t chunks;         /* device address of HapGpuChunkIn[chunk_count] */
    uint64_t frag_sizes;     /* device address of the u32 fragment-size entries inside the frame, or 0 */
    uint64_t units;          /* device address of this job's HapGpuDecodeUnit[unit_count] */
    uint32_t chunk_count;
    uint32_t mode;           /* HAPGPU_JOB_* */
    uint32_t frag_log2;
    uint32_t frag_entries;   /* number of fragment-size entries */
    uint32_t unit_count;
    uint32_t reserved;       /* bits 0..7: granularity_log2 announced by the fragment table (0 bytes, 1 16-bit,
                                2 32-bit); bits 8..15: its match window in 256-byte units (0 = none announced);
                                bit 16: no table, but every chunk is as short as a fragment: group_tables is scratch
                                (HAP_GROUP_TABLE_BYTES per unit of the CALL) that hapgpu_k_guess_group_tables fills,
                                fields_period the layout the texture format implies */
    /* results */
    uint64_t bytes_used;
    uint32_t status;         /* HapResult or HAPGPU_STATUS_* */
    uint32_t fields_period;  /* HAPGPU_LAYOUT_*: the table is version 3 and promises field streams of that layout; NONE otherwise */
    uint64_t group_tables;     /* device address of the group tables inside the frame (96 bytes per fragment entry), or 0 */
} HapGpuDecodeJob;

#define HAPGPU_UNIT_SKIP 0u
#define HAPGPU_UNIT_SNAPPY_STREAM 1u   /* varint header + elements */
#define HAPGPU_UNIT_SNAPPY_FRAGMENT 2u /* bare elements producing exactly dst_len bytes */
#define HAPGPU_UNIT_COPY 3u
#define HAPGPU_UNIT_SNAPPY_FRAGMENT16 4u /* fragment whose elements are all 16-bit granular */
#define HAPGPU_UNIT_SNAPPY_FRAGMENT32 5u /* ... all 32-bit granular */
#define HAPGPU_UNIT_SNAPPY_FIELDS4 6u   /* fragment of a field stream, 16-byte blocks of 2 + 6 + 4 + 4 bytes; aux = its group table */
#define HAPGPU_UNIT_SNAPPY_FIELDS2 7u   /* ... 8-byte blocks of 4 + 4 bytes */
#define HAPGPU_UNIT_SNAPPY_FIELDS26 8u  /* ... 8-byte blocks of 2 + 6 bytes */
#define HAPGPU_UNIT_SNAPPY_FIELDS44 10u /* ... 16-byte blocks of 4 + 4 + 4 + 4 bytes (opaque formats) */
#define HAPGPU_UNIT_SNAPPY_BLOCK 9u     /* one 64 KiB block of another encoder's stream (or one 8 KiB block of a table-less
                                           stream of this library), found by the block scan: bare elements, copies stay
                                           inside the block; decoded by the whole-stream kernel.  aux = its
                                           HapGpuScanChunk, reserved = block number (| HAPGPU_BLOCK_FINE), src = the stream */
#define HAPGPU_BLOCK_FINE (1ull << 32)  /* flag in reserved: the unit is an 8 KiB block */
#define HAPGPU_SCAN_FINE 8192u          /* the block scan's fine granularity (one fragment of this library's streams) */
#define HAPGPU_UNIT_WINDOWED 0x10u       /* flag on the three fragment kinds: every copy offset is <= 3 KiB, so an 8 KiB
                                            fragment decodes through a 4 KiB LDS ring (twice the waves per CU) */
#define HAP_FRAGMENT_WINDOW_256 12u      /* that window in 256-byte units, as written to the fragment table */

/* Block scan of another encoder's Snappy stream (snappy_decode.hip): the stream's compressed bytes are looked at in
   segments of HAPGPU_SCAN_SEGMENT bytes (of the 16-byte aligned address range that holds them). */
#ifndef HAPGPU_SCAN_SEGMENT
#define HAPGPU_SCAN_SEGMENT 4096u
#endif
typedef struct HapGpuScanChunk {
    /* filled by the host */
    uint32_t unit;           /* index of the stream's whole-stream unit in the call's unit array */
    uint32_t seg_first;      /* first of its seg_count segment records */
    uint32_t seg_count;      /* >= segments the stream can touch: (src_len + 15 + 4095) / 4096 */
    uint32_t slots;          /* unit slots for 64 KiB blocks, directly behind the stream unit */
    uint64_t bpos;           /* device address of fine_slots + 1 words: compressed position where each 8 KiB of output
                                begins (a 64 KiB block begins at every eighth) */
    /* written by the device (the host sends zeros) */
    uint32_t ok;             /* the element chain was followed to the stream's end and the lengths agree */
    uint32_t expected;       /* 64 KiB blocks */
    uint32_t found;          /* 64 KiB block starts that fall on an element boundary: all of them = BLOCK units run */
    /* host */
    uint32_t fine_slots;     /* unit slots for 8 KiB blocks, at fine_unit_first of the call's unit array (behind all the
                                ordinary units): streams written by this library without a fragment table have an
                                element boundary at every 8 KiB (its fragments) -- eight times the units of
                                libsnappy's 64 KiB blocks */
    /* device */
    uint32_t expected_fine;  /* 8 KiB blocks */
    uint32_t found_fine;     /* 8 KiB marks on element boundaries: all of them = the fine BLOCK units run first */
    uint32_t fine_failed;    /* ... and one of them met a copy that reaches before its block (marks on element boundaries
                                do not make a stream's 8 KiB pieces independent): the 64 KiB blocks / the stream unit
                                of the launch's second phase decode the stream instead */
    uint32_t fine_unit_first; /* device: index of the stream's first fine unit slot in the call's unit array (from the pool) */
    uint32_t seg_bytes;      /* host: the call's segment size, HAPGPU_SCAN_SEGMENT or half of it (0: HAPGPU_SCAN_SEGMENT) */
    uint32_t probe_found;    /* of the first two 8 KiB marks (output positions 8192 and 16384): the rest of the fine
                                marks are only looked for when both fall on element boundaries -- in a libsnappy
                                stream they hardly ever do, and its scan then costs what it did with 64 KiB marks only */
    /* device: the workgroup-per-block kernel */
    uint32_t dependent;      /* a 64 KiB block whose element chain it had verified copies from before the block: the
                                stream's blocks are not independent, and the stream unit decodes it */
    uint32_t resolved;       /* 64 KiB blocks of the stream it decoded; they count (HapGpuResolvedBlockCount) unless
                                the stream turned out dependent, where the stream unit writes them again */
} HapGpuScanChunk;

typedef struct HapGpuScanSegment {   /* device only */
    uint32_t exit_coord;     /* where the segment's (guessed) chain left the segment */
    uint32_t cum_total;      /* output bytes that chain produced from its start to there */
    uint32_t flags;          /* 1: the chain met something that is not an element; 2: it reached the end of the input */
    uint32_t elements;       /* elements of that chain from its start to there */
} HapGpuScanSegment;
/* (per segment, in an array of its own, 4 x uint32: the window in which the true chain joined the recorded one --
   0xFFFFFFFF: never --, the absolute output position and the absolute element number of the recorded chain's zero, and
   1 where the true chain may have entered the segment in front of that window.  A window's record, 64 bits: byte of the
   window at which the chain entered it | output bytes of the chain so far << 8 | its elements so far << 40) */

/* [device] one wavefront's worth of decode work */
typedef struct HapGpuDecodeUnit {
    uint64_t src;
    uint64_t dst;
    uint32_t src_len;
    uint32_t dst_len;
    uint32_t kind;           /* HAPGPU_UNIT_* */
    uint32_t job;            /* index of the owning job (status word) */
    uint64_t aux;            /* FIELDS units: device address of the fragment's group table (HAP_GROUP_TABLE_BYTES);
                                STREAM units: number of SKIP slots that follow for the block scan's BLOCK units */
    /* reserved: fragment units: readable bytes after the fragment (<= 15); STREAM units: 0 or the HapGpuScanChunk
       that decides whether the stream unit or its BLOCK units run */
    uint64_t reserved;
} HapGpuDecodeUnit;

/* [device] the rectangle a region call wants of a texture, in texels of a `width`-wide texture (hap_region.h) */
typedef struct HapGpuRegion {
    uint32_t width, x, y, w, h;
} HapGpuRegion;

/* ------------------------------------------------------------------ */
/* runtime (hapgpu_runtime.hip) + launchers (each in its kernels' file) */
/* ------------------------------------------------------------------ */
typedef struct hapgpu_rt hapgpu_rt;

int hapgpu_rt_create(int device, hapgpu_rt **rt);
void hapgpu_rt_destroy(hapgpu_rt *rt);
/* 1: HIP device memory (usable by kernels in place), 0: host memory */
int hapgpu_rt_is_device_ptr(hapgpu_rt *rt, const void *p);
/* grow-only scratch arenas, slot 0..15; contents undefined after growth */
void *hapgpu_rt_device_scratch(hapgpu_rt *rt, int slot, size_t bytes);
void *hapgpu_rt_pinned_scratch(hapgpu_rt *rt, int slot, size_t bytes);
int hapgpu_rt_h2d(hapgpu_rt *rt, void *dst, const void *src, size_t bytes);
int hapgpu_rt_d2h(hapgpu_rt *rt, void *dst, const void *src, size_t bytes);
int hapgpu_rt_d2h_rows(hapgpu_rt *rt, void *dst, size_t dpitch, const void *src, size_t spitch, size_t row, size_t rows);
int hapgpu_rt_d2d(hapgpu_rt *rt, void *dst, const void *src, size_t bytes);
int hapgpu_rt_zero(hapgpu_rt *rt, void *dst, size_t bytes);
/* 1: kernels may be handed pinned-scratch addresses directly (no copy in front of or behind them) */
int hapgpu_rt_pinned_is_mapped(hapgpu_rt *rt);
int hapgpu_rt_sync(hapgpu_rt *rt);
/* 64 KiB blocks of other encoders' streams decoded by a workgroup each since the runtime was made (waits for the stream) */
unsigned hapgpu_rt_resolved_blocks(hapgpu_rt *rt);
void hapgpu_rt_lock(hapgpu_rt *rt);
void hapgpu_rt_unlock(hapgpu_rt *rt);
/* 0: the lock was free and is now held by the caller */
int hapgpu_rt_trylock(hapgpu_rt *rt);
int hapgpu_rt_device(hapgpu_rt *rt);
/* Launch sequences recorded as HIP graphs (hapgpu_runtime.hip).  key: everything the sequence's kernel arguments and
 * copy sizes depend on.  _begin: 1 = a recorded sequence was launched (skip the launches), 0 = recording (issue the
 * launches, then _end), 2 = launch as usual.  _end(failed): 0 = instantiated, remembered and launched. */
int hapgpu_rt_graph_begin(hapgpu_rt *rt, uint64_t key);
int hapgpu_rt_graph_end(hapgpu_rt *rt, uint64_t key, int failed);
/* no more recordings for this runtime (its recorded sequences stay usable): after a capture / instantiate / launch failure */
void hapgpu_rt_graphs_disable(hapgpu_rt *rt);

/* kernels: all asynchronous on the runtime's stream; 0 = launched */

/* [device] Addresses of a block-codec launch: three columns of `pictures` device addresses, each either a DEVICE array
   (column[c]) or, for one picture, the address itself (one[c], read where column[c] is NULL).  Encode: sources, outputs,
   second outputs (Hap Q Alpha's RGTC1 plane; video pictures: their CbCr planes, a 0 skipping the picture); decode: textures, alpha planes, pictures
   (to video pictures: textures, CbCr planes, Y planes, a 0 in any column skipping the picture).  A source or texture address of
   0 skips the picture, and so does an encode output of 0. */
typedef struct HapGpuPictureTable {
    const uint64_t *column[3];
    uint64_t one[3];
} HapGpuPictureTable;

/* The layout of the pictures a block-codec launch reads or writes */
enum {
    HAPGPU_PICTURE_RGBA8 = 0,      /* 4 bytes a texel */
    HAPGPU_PICTURE_RGBA16F = 1,    /* 8 bytes a texel: four half floats; BC6H textures only, and those from nothing else */
    HAPGPU_PICTURE_A8 = 2          /* 1 byte a texel: RGTC1 textures only */
};
#define HAPGPU_PICTURE_TEXEL_BYTES(kind) ((kind) == HAPGPU_PICTURE_RGBA16F ? 8u : (kind) == HAPGPU_PICTURE_A8 ? 1u : 4u)

/* pictures of layout `picture_kind` -> blocks of `hap_texture_format`.  RGBA8 -> RGB_DXT1, RGBA_DXT5, YCoCg_DXT5,
   A_RGTC1 (the alpha channel) or RGBA_BPTC_UNORM (BC7); RGBA16F -> RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT
   (BC6H: sources and row_bytes 16-byte aligned); A8 -> A_RGTC1, at most 65535 block rows.
   YCoCg_DXT5 with_alpha: Hap Q Alpha, the RGTC1 alpha plane to the second outputs from the same read of every picture.
   Sources and row_bytes 4-byte aligned, outputs 8- (DXT1, RGTC1) or 16-byte aligned; wide != 0 promises 16-byte aligned
   sources and row pitch.
   flags (the word that was with_alpha: 0 and 1 mean what they meant): HAPGPU_BLOCK_ENCODE_WITH_ALPHA as above;
   HAPGPU_BLOCK_ENCODE_REFINE makes the colour blocks of RGB_DXT1 and RGBA_DXT5 with refined end points
   (HAPGPU_ENCODE_REFINE_ENDPOINTS, hap_gpu.h; bc_refine_core.hpp) and is ignored for every other format. */
#define HAPGPU_BLOCK_ENCODE_WITH_ALPHA 1u
#define HAPGPU_BLOCK_ENCODE_REFINE 2u
int hapgpu_k_block_encode(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, unsigned width,
                          unsigned height, size_t row_bytes, unsigned hap_texture_format, unsigned flags, int wide,
                          unsigned picture_kind);
/* blocks of `hap_texture_format` -> pictures of layout `picture_kind`: RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 (with_alpha: the
   RGTC1 plane supplies A) and RGBA_BPTC_UNORM to RGBA8; RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT (BC6H) to
   RGBA16F; A_RGTC1 to A8 (at most 65535 block rows).  Textures 8- (DXT1, RGTC1) or 16-byte aligned, alpha planes 8-byte
   aligned.  RGBA8 and RGBA16F pictures and their row_bytes 16-byte aligned; A8 pictures and their row_bytes 4-byte
   aligned, and wide != 0 promises 16 bytes for them too (ignored for the other layouts). */
int hapgpu_k_block_decode(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                          unsigned width, unsigned height, unsigned hap_texture_format, size_t row_bytes, int wide,
                          unsigned picture_kind);
/* ... to RGBA8 pictures of (width >> scale_log2) x (height >> scale_log2), scale_log2 1 or 2: every output texel the box
   mean of the 2^scale_log2 x 2^scale_log2 texels hapgpu_k_block_decode makes there, per channel, halves rounded up
   ((sum + (1 << (2 * scale_log2 - 1))) >> (2 * scale_log2)).  RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 (with_alpha: the RGTC1
   plane supplies A) and RGBA_BPTC_UNORM; width and height are the texture's.  Textures and alpha planes aligned as
   there; pictures and their row_bytes (at least (width >> scale_log2) * 4) to the 16 >> scale_log2 bytes a lane stores
   per row.  The same table, profile class and return codes. */
int hapgpu_k_block_decode_scaled(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                 unsigned width, unsigned height, unsigned hap_texture_format, unsigned scale_log2,
                                 size_t row_bytes);
/* ... the rectangle (x, y, region_width, region_height; multiples of 4 inside width x height) of every texture to an RGBA8
   picture of region_width x region_height, byte for byte the crop of what hapgpu_k_block_decode writes: lane id is block
   (id % (region_width / 4), id / (region_width / 4)) of the rectangle and reads texture (and alpha plane) block
   (id / (region_width / 4) + y / 4) * (width / 4) + id % (region_width / 4) + x / 4 -- no block outside the rectangle is
   read.  RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 (with_alpha) and RGBA_BPTC_UNORM.  Pictures and row_bytes (at least
   region_width * 4) 16-byte aligned.  The same table, profile class and return codes. */
int hapgpu_k_block_decode_region(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                 unsigned width, unsigned height, unsigned hap_texture_format, unsigned x, unsigned y,
                                 unsigned region_width, unsigned region_height, size_t row_bytes);
/* ... to planar tensors of (width >> scale_log2) x (height >> scale_log2), scale_log2 0 to 2, without an RGBA8 picture in
   between (bc_decode_planes.hip): `channels` (3 or 4: R, G, B[, A]) planes plane_bytes apart, rows row_bytes apart,
   elements of element_kind (0 half, 1 bfloat16, 2 float: e = 2, 2, 4 bytes).  For the byte v that
   hapgpu_k_block_decode (scale_log2 0) or hapgpu_k_block_decode_scaled writes for a texel and channel c, the element is
   (float)v * scale[c] (one binary32 multiply) + bias[c] (one binary32 add, not fused), rounded to nearest even to the
   element kind, subnormal halves kept.  scale and bias: `channels` floats each, in host memory, copied by the call.
   RGB_DXT1, RGBA_DXT5 and YCoCg_DXT5 (with_alpha: the RGTC1 plane supplies A).  Tensors (the third column of the table),
   plane_bytes and row_bytes aligned to the (4 >> scale_log2) * e bytes a lane stores per row; row_bytes at least
   (width >> scale_log2) * e, plane_bytes at least row_bytes * ((height >> scale_log2) - 1) + (width >> scale_log2) * e.
   The same table, profile class and return codes. */
int hapgpu_k_block_decode_planes(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                 unsigned width, unsigned height, unsigned hap_texture_format, unsigned scale_log2,
                                 unsigned channels, unsigned element_kind, size_t plane_bytes, size_t row_bytes,
                                 const float *scale, const float *bias);
/* ... the rectangle of region_width x region_height (multiples of 4, inside width x height) of every texture to planar
   tensors of (region_width >> scale_log2) x (region_height >> scale_log2), a different rectangle per picture: bit for bit
   rows [y >> scale_log2, (y + region_height) >> scale_log2) and columns [x >> scale_log2, (x + region_width) >> scale_log2)
   of every plane hapgpu_k_block_decode_planes writes (a box mean never spans two blocks).  Where a picture's rectangle
   begins is a texture block index, (y / 4) * (width / 4) + x / 4: origins[z] for picture z (a DEVICE array; the caller's
   promise that every rectangle lies inside its texture, as the table's addresses are), or, where origins is NULL, `origin`
   for all of them (checked).  Lane id is block (bx, by) = (id % (region_width / 4), id / (region_width / 4)) of the
   rectangle and of its tensor and reads texture (and alpha plane) block origin + by * (width / 4) + bx: no block outside
   a picture's rectangle is read.  Formats, tensors, scale and bias as for hapgpu_k_block_decode_planes, the layout rules
   at the rectangle's size.  The same table, profile class and return codes. */
int hapgpu_k_block_decode_planes_region(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                        unsigned width, unsigned height, unsigned hap_texture_format,
                                        const uint32_t *origins, unsigned origin, unsigned region_width,
                                        unsigned region_height, unsigned scale_log2, unsigned channels,
                                        unsigned element_kind, size_t plane_bytes, size_t row_bytes, const float *scale,
                                        const float *bias);
/* ... a crop per picture, at any texel position and size, resized to planar tensors of out_width x out_height (1 to 16384
   each), bc_resample_planes.hip.  With s = scale_log2 and P the (width >> s) x (height >> s) RGBA8 picture
   hapgpu_k_block_decode (s 0) or hapgpu_k_block_decode_scaled writes, picture z's crop is (x, y, w, h) in texels of P:
   crops[4 * z ..] (a DEVICE array), or, where crops is NULL, the four words at `crop` (host) for all of them.  w, h >= 1,
   x + w <= width >> s, y + h <= height >> s, w <= 4 * out_width, h <= 4 * out_height: checked for `crop`; a picture of
   `crops` that breaks them is left unwritten.  Every output byte is resample_taps.hpp's blend of four texels of P inside
   the crop -- include/hap_gpu.h: HapGpuDecodeFramesPlanesResized has the definition -- and the element is
   hapgpu_k_block_decode_planes' conversion of it.  Only the blocks that hold texels of the crop are read.  Formats,
   scale and bias as for hapgpu_k_block_decode_planes.  A lane stores single elements: tensors, plane_bytes and row_bytes
   multiples of e, row_bytes at least out_width * e, plane_bytes at least row_bytes * (out_height - 1) + out_width * e.
   The same table, profile class and return codes. */
int hapgpu_k_block_decode_planes_resized(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                         unsigned width, unsigned height, unsigned hap_texture_format,
                                         const uint32_t *crops, const unsigned *crop, unsigned out_width,
                                         unsigned out_height, unsigned scale_log2, unsigned channels,
                                         unsigned element_kind, size_t plane_bytes, size_t row_bytes, const float *scale,
                                         const float *bias);
/* blocks of `hap_texture_format` against RGBA8 reference pictures (the third column of the table: read, not written),
   without a decoded picture in between (bc_measure.hip): for every picture whose texture address is not 0,
   totals[picture][0..3] = the sum over all width x height texels of (d - p)^2 for R, G, B, A and totals[picture][4..7] the
   sum of |d - p|, d the byte hapgpu_k_block_decode writes for the texel and channel and p the reference picture's --
   exact integers.  RGB_DXT1, RGBA_DXT5 and YCoCg_DXT5 (with_alpha: the RGTC1 plane supplies A; without one A is 255,
   DXT5's own apart).  Two launches: a workgroup per 1024 blocks stores eight 32-bit partial sums to
   partials[picture][workgroup][8] (device, 16-byte aligned, pictures * hapgpu_block_measure_partial_bytes(width, height)
   bytes), then a workgroup per picture adds them in 64 bits to totals (device, 8-byte aligned); the totals of a picture
   with texture address 0 are left as they are.  Textures and alpha planes aligned as for hapgpu_k_block_decode; reference
   pictures and row_bytes (at least width * 4) 16-byte aligned, and only width * 4 bytes of each row are read.  The same
   table, profile class and return codes. */
int hapgpu_k_block_measure(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                           unsigned width, unsigned height, unsigned hap_texture_format, size_t row_bytes,
                           uint32_t *partials, unsigned long long *totals);
size_t hapgpu_block_measure_partial_bytes(unsigned width, unsigned height);
/* [device] One layer of one output picture of a composite launch: its texture (device address; 0 skips the whole
   picture, as a texture address of 0 does in HapGpuPictureTable), its RGTC1 alpha plane or 0, the texture's format
   (HapTextureFormat: RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5) and the layer's opacity byte.  24 bytes. */
typedef struct HapGpuCompositeLayer {
    uint64_t texture;
    uint64_t alpha;
    uint32_t format;
    uint32_t opacity;        /* 0 .. 255 */
} HapGpuCompositeLayer;
#define HAPGPU_COMPOSITE_LAYERS_MAX 16u     /* include/hap_gpu.h: HAPGPU_COMPOSITE_MAX_LAYERS */
/* layers of blocks "over" a background colour -> RGBA8 pictures, without the layers' pictures in between
   (bc_composite.hip).  layers: [pictures][layer_count] descriptors (device), layer 0 at the bottom; outputs: `pictures`
   device addresses (a device array; 0 skips the picture); background: 4 bytes R, G, B, A in host memory, copied by the
   call.  Every texel of picture z starts as the background and takes, for l = 0 .. layer_count - 1, with (Rs, Gs, Bs, As)
   the bytes hapgpu_k_block_decode writes there for layers[z][l]'s texture (and plane) and o its opacity,
       a = rdiv255(As * o);  Cd = rdiv255(Cs * a + Cd * (255 - a)) for R, G, B;  Ad = a + rdiv255(Ad * (255 - a))
   (composite_blend.hpp; rdiv255(x) = the integer nearest to x / 255); the picture is the canvas after the last layer.
   All layers have the pictures' width x height; layers of one picture may differ in format.  Textures 8- (DXT1) or
   16-byte aligned, alpha planes 8-byte aligned, pictures and row_bytes (at least width * 4) 16-byte aligned; only
   width * 4 bytes of each row are written.  The profile class of hapgpu_k_block_decode.  Returns 0 launched, 1 bad
   arguments, 4 launch failure. */
int hapgpu_k_block_composite(hapgpu_rt *rt, const HapGpuCompositeLayer *layers, unsigned layer_count,
                             const uint64_t *outputs, unsigned pictures, const unsigned char *background, unsigned width,
                             unsigned height, size_t row_bytes);
/* [device] One layer of one output picture of a placed composite launch: HapGpuCompositeLayer's four members, then
   what of the layer is visible on the canvas, in blocks (hap_place.h: hap_place_clip) -- canvas blocks
   cx0 <= bx < cx0 + cw, cy0 <= by < cy0 + ch have the layer's block first + (by - cy0) * layer_blocks_x + (bx - cx0)
   under them, every other canvas block none of this layer; cw == 0: nothing visible.  48 bytes. */
typedef struct HapGpuPlacedLayer {
    uint64_t texture;
    uint64_t alpha;
    uint32_t format;
    uint32_t opacity;        /* 0 .. 255 */
    uint32_t cx0, cy0, cw, ch;
    uint32_t first, layer_blocks_x;
} HapGpuPlacedLayer;
/* hapgpu_k_block_composite for layers of sizes of their own, placed and clipped on the canvas (bc_composite.hip): a
   texel of a canvas block inside a layer's clip takes that layer's texel by the same three formulas, every other texel
   is left as the canvas has it.  Every block index first + (ch - 1) * layer_blocks_x + cw - 1 and below must lie inside
   the layer's texture (and plane): the launch does not know the layers' sizes.  Everything else -- outputs, background,
   alignment, the profile class, the return codes -- as hapgpu_k_block_composite. */
int hapgpu_k_block_composite_placed(hapgpu_rt *rt, const HapGpuPlacedLayer *layers, unsigned layer_count,
                                    const uint64_t *outputs, unsigned pictures, const unsigned char *background,
                                    unsigned width, unsigned height, size_t row_bytes);
/* hapgpu_k_block_composite_placed with the canvases going to the block encoder in registers, not to memory as pictures
   (bc_composite_encode.hip): blocks of `dst_format` (RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; dst_with_alpha, YCoCg_DXT5 only:
   + the RGTC1 plane of A) of textures of width x height, byte for byte what hapgpu_k_block_encode makes of the RGBA8
   pictures hapgpu_k_block_composite_placed writes for the same layers and background -- the canvas bytes as they are,
   premultiplied.  outputs: `pictures` device addresses of the destination textures (a device array; 0 skips the
   picture), outputs2: of the destination planes (dst_with_alpha only; else not read and may be NULL).  At most 65535
   block rows.  Layers, their alignment and the background as hapgpu_k_block_composite_placed has them, destinations
   aligned to their blocks.  Timed as HapGpuKernel_BlockEncode.  Returns 0 launched, 1 bad arguments, 4 launch failure. */
int hapgpu_k_block_composite_encode(hapgpu_rt *rt, const HapGpuPlacedLayer *layers, unsigned layer_count,
                                    const uint64_t *outputs, const uint64_t *outputs2, unsigned pictures,
                                    const unsigned char *background, unsigned width, unsigned height, unsigned dst_format,
                                    int dst_with_alpha);
/* planar tensors -> blocks of `hap_texture_format`, without an RGBA8 picture in between (bc_encode_planes.hip): the way
   back of hapgpu_k_block_decode_planes.  Tensors (the first column of the table) of `channels` (3 or 4: R, G, B[, A])
   planes plane_bytes apart, rows row_bytes apart, elements of element_kind (0 half, 1 bfloat16, 2 float: e = 2, 2, 4
   bytes).  An element x of plane c becomes the texel byte of x * scale[c] (one binary32 multiply) + bias[c] (one binary32
   add, not fused): 0 for a NaN and anything not above 0, 255 from 255 up, else rounded to nearest, halves to even
   (plane_quantise.hpp); with three planes A is 255.  The blocks are byte for byte what hapgpu_k_block_encode makes of
   the RGBA8 pictures of those bytes: RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 (with_alpha: + the RGTC1 plane of A to the second
   outputs) or A_RGTC1.  scale and bias: `channels` floats each, in host memory, copied by the call.  Tensors, plane_bytes
   and row_bytes aligned to the 4 * e bytes a lane loads per row; row_bytes at least width * e, plane_bytes at least
   row_bytes * (height - 1) + width * e; at most 65535 block rows.  Outputs aligned to their blocks.  flags:
   hapgpu_k_block_encode's (HAPGPU_BLOCK_ENCODE_WITH_ALPHA, HAPGPU_BLOCK_ENCODE_REFINE).  Timed as
   HapGpuKernel_BlockEncode.  Returns 0 launched, 1 bad arguments, 4 launch failure. */
int hapgpu_k_block_encode_planes(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, unsigned width,
                                 unsigned height, unsigned hap_texture_format, unsigned flags, unsigned channels,
                                 unsigned element_kind, size_t plane_bytes, size_t row_bytes, const float *scale,
                                 const float *bias);
/* NV12 video pictures -> blocks of `hap_texture_format`, without an RGBA8 picture in between (bc_encode_video.hip).  The
   table's columns are [Y planes][outputs][CbCr planes]: a Y plane of width x height bytes, rows luma_row_bytes apart, and
   a plane of (width / 2) x (height / 2) interleaved Cb, Cr pairs, rows chroma_row_bytes apart; a 0 in any column skips
   the picture.  Texel (x, y) is ycbcr_rgb.hpp's RGBA of Y[y][x] and the pair at [y >> 1][x >> 1] under `matrix`
   (HapGpuYCbCrMatrix) and `range` (HapGpuYCbCrRange), A 255; the blocks are byte for byte what hapgpu_k_block_encode
   makes of the RGBA8 pictures of those texels: RGB_DXT1 or YCoCg_DXT5.  Planes and both pitches 4-byte aligned, both
   pitches at least width, at most 65535 block rows.  Outputs aligned to their blocks.  flags:
   HAPGPU_BLOCK_ENCODE_REFINE (RGB_DXT1; ignored for YCoCg_DXT5); HAPGPU_BLOCK_ENCODE_WITH_ALPHA is refused.  Timed as
   HapGpuKernel_BlockEncode.  Returns 0 launched, 1 bad arguments, 4 launch failure. */
int hapgpu_k_block_encode_video(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, unsigned width,
                                unsigned height, unsigned hap_texture_format, unsigned flags, size_t luma_row_bytes,
                                size_t chroma_row_bytes, unsigned matrix, unsigned range);
/* blocks of `hap_texture_format` (RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; alpha is never read) -> NV12 video pictures of
   (width >> scale_log2) x (height >> scale_log2), scale_log2 0 to 2, without an RGBA8 picture in between
   (bc_decode_video.hip).  The table's columns are [textures][CbCr planes][Y planes]: a Y plane of W x H bytes, rows
   luma_row_bytes apart, and a plane of (W / 2) x (H / 2) interleaved Cb, Cr pairs, rows chroma_row_bytes apart; a 0 in any
   column skips the picture.  With d the RGBA8 picture hapgpu_k_block_decode (scale_log2 0) or
   hapgpu_k_block_decode_scaled writes for the texture, Y[y][x] is rgb_ycbcr.hpp's luma of d(x, y) and pair [j][i] its pair
   of the sums over d(2i..2i+1, 2j..2j+1), under `matrix` (HapGpuYCbCrMatrix) and `range` (HapGpuYCbCrRange).  width and
   height are the textures', multiples of 4 << scale_log2; at most 65535 destination block rows.  Textures aligned to what
   a lane reads of a block row (their block << scale_log2, at most 16 bytes); planes and both pitches 4-byte aligned, both
   pitches at least W.  Only the samples are written.  Timed as HapGpuKernel_BlockDecode.  Returns 0 launched, 1 bad
   arguments, 4 launch failure. */
int hapgpu_k_block_decode_video(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, unsigned width,
                                unsigned height, unsigned hap_texture_format, unsigned scale_log2, size_t luma_row_bytes,
                                size_t chroma_row_bytes, unsigned matrix, unsigned range);
/* [device] Addresses of a transcode launch, as HapGpuPictureTable's: source textures, source alpha planes, destination
   textures, destination alpha planes (Hap Q Alpha's second texture). */
typedef struct HapGpuTranscodeTable {
    const uint64_t *column[4];
    uint64_t one[4];
} HapGpuTranscodeTable;
/* blocks of `src_format` (RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; with_alpha: an RGTC1 plane supplies A) -> blocks of
   `dst_format` (RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; dst_with_alpha, YCoCg_DXT5 only: + the RGTC1 plane of A) of textures of
   (width >> scale_log2) x (height >> scale_log2), scale_log2 0 to 2, without a picture in between: byte for byte what
   hapgpu_k_block_encode makes of the RGBA8 pictures hapgpu_k_block_decode (scale_log2 0) or hapgpu_k_block_decode_scaled
   writes for the sources.  width and height are the sources', multiples of 4 << scale_log2; at most 65535 destination
   block rows.  Sources and their planes aligned to what a lane reads of a block row (their block << scale_log2, at
   most 16 bytes), destinations to their blocks.  A source without alpha gives A = 255; a destination without alpha
   does not read the plane.  Timed as HapGpuKernel_BlockEncode.  Returns 0 launched, 1 bad arguments, 4 launch failure. */
int hapgpu_k_block_transcode(hapgpu_rt *rt, const HapGpuTranscodeTable *table, unsigned pictures, unsigned src_format,
                             int with_alpha, unsigned width, unsigned height, unsigned scale_log2, unsigned dst_format,
                             int dst_with_alpha);
/* Which compressor kernels a call's textures need: sets over the values their control words hold, bit v for value v.  A
   texture is in exactly one set: fused (it is made on the way), else layouts (a layout other than NONE), else
   granularities (a position per lane). */
typedef struct HapGpuCompressKinds {
    unsigned granularities;  /* bit g: some position-per-lane texture has granularity_log2 g (0..2) */
    unsigned layouts;        /* bit HAPGPU_LAYOUT_*: some texture that exists has that field layout */
    unsigned fused;          /* bit HAPGPU_FUSED_*: some texture is made from its frame's picture by the block compressor */
    unsigned textures;       /* textures per frame */
} HapGpuCompressKinds;
/* group_tables: HAP_GROUP_TABLE_BYTES bytes per fragment (same indexing as frag_sizes), written for textures with half-tiles */
int hapgpu_k_snappy_compress(hapgpu_rt *rt, const HapGpuFrameEnc *frames, unsigned frame_count,
                             unsigned max_frags_per_texture, unsigned frag_log2,
                             void *slots, unsigned slot_stride, uint32_t *frag_sizes, uint8_t *group_tables,
                             const HapGpuCompressKinds *kinds);
/* copies: one entry per fragment, then (from index extra_first) chunks_per_frame entries per frame for the
 * group tables of field streams */
int hapgpu_k_frame_pack(hapgpu_rt *rt, HapGpuFrameEnc *frames, unsigned frame_count,
                        unsigned frag_log2, const void *slots, unsigned slot_stride,
                        const uint32_t *frag_sizes, const uint8_t *group_tables, HapGpuCopyEntry *copies,
                        unsigned extra_first, unsigned chunks_per_frame, unsigned max_chunks_per_texture,
                        unsigned textures, void *pack_scratch);
/* bytes of pack_scratch needed per chunk (frame_count * chunks_per_frame of them) */
unsigned hapgpu_pack_scratch_bytes_per_chunk(void);
int hapgpu_k_frame_gather(hapgpu_rt *rt, const HapGpuCopyEntry *copies, unsigned count);
/* first `prefix` bytes of every device-resident frame (0 pointer = skip) -> out_dev + i * prefix */
int hapgpu_k_gather_prefixes(hapgpu_rt *rt, const uint64_t *frames_dev, const uint64_t *lengths_dev,
                             unsigned count, unsigned prefix, void *out_dev);
/* ... and, for entries with far_dev[f] != 0, the bytes at the second texture's section when it starts beyond the first
   prefix (far_at_dev[f] = its offset, 0 = none / inside the first prefix) */
int hapgpu_k_gather_prefixes_far(hapgpu_rt *rt, const uint64_t *frames_dev, const uint64_t *lengths_dev,
                                 unsigned count, unsigned prefix, void *out_dev, const uint8_t *far_dev,
                                 void *out2_dev, uint64_t *far_at_dev);
/* clears `units` (all SKIP) then plans every job; max_chunks: largest chunk_count among the jobs */
int hapgpu_k_decode_plan(hapgpu_rt *rt, HapGpuDecodeJob *jobs, unsigned job_count,
                         HapGpuDecodeUnit *units, unsigned unit_count, unsigned max_chunks);
/* A region call: every unit of units[0 .. unit_count) that holds no byte of a block of `region` -- its place in its
   texture: dst - the job's dst, dst_len; the texture's block size: job_block_bytes[unit.job] (device; 0: leave the job's
   units alone) -- becomes HAPGPU_UNIT_SKIP, and with `count` its dst_len is added to the runtime's skipped-bytes counter
   (hapgpu_rt_skipped_bytes; count 0: a frame's second pass, which the first has counted).  Of a scanned stream's 64 KiB and
   8 KiB blocks, both blanked, the set the decoder is about to run is counted; a stream whose 8 KiB pieces fail later and
   fall back stays counted by those.  To be run when the unit list is final: after hapgpu_k_decode_plan and, where it adds
   units, after hapgpu_k_scan_blocks (running it in front of the scan as well keeps chunks nobody needs from being
   scanned; in front of hapgpu_k_guess_group_tables, no table is made for a blanked piece). */
int hapgpu_k_skip_units(hapgpu_rt *rt, HapGpuDecodeUnit *units, unsigned unit_count, const HapGpuDecodeJob *jobs,
                        const uint32_t *job_block_bytes, const HapGpuRegion *region, int count);
/* ... with a rectangle per job: job_regions[unit.job] (device, next to job_block_bytes) in place of the one `region`.  A
   job that skips nothing carries a rectangle that needs everything -- the whole of its texture --, or a block size of 0. */
int hapgpu_k_skip_units_per_job(hapgpu_rt *rt, HapGpuDecodeUnit *units, unsigned unit_count, const HapGpuDecodeJob *jobs,
                                const uint32_t *job_block_bytes, const HapGpuRegion *job_regions, int count);
/* decoded bytes of the units hapgpu_k_skip_units blanked since the runtime was made (waits for the stream) */
unsigned long long hapgpu_rt_skipped_bytes(hapgpu_rt *rt);
/* splits whole-stream units that consist of independent 64 KiB blocks (what libsnappy writes) into BLOCK units,
 * using the slots reserved behind them; streams that do not qualify stay as they are.  chunks: one entry per stream
 * (host-filled part copied to the device by the caller); segs / recs / joins: device scratch of seg_total entries /
 * seg_total * 64 words of 8 bytes / seg_total * 8 bytes */
int hapgpu_k_scan_blocks(hapgpu_rt *rt, HapGpuDecodeUnit *units, const HapGpuDecodeJob *jobs, HapGpuScanChunk *chunks,
                         unsigned chunk_count, HapGpuScanSegment *segs, void *recs, void *joins, unsigned seg_total,
                         uint32_t *fine_work /* [0]: count (zero on entry), then the unit indices of the 8 KiB blocks to decode
                                                (room for fine_pool of them), then the pool's cursor (zero on entry) */,
                         unsigned fine_first, unsigned fine_pool /* the 8 KiB blocks' unit slots: units[fine_first .. + fine_pool),
                                                                    handed out to the streams on the device */);
/* The block scan's records of one call, for the launches behind it (hapgpu_k_guess_group_tables, hapgpu_k_snappy_decode;
 * a NULL pointer: no scan in this call).  recs / joins / chunks / chunk_count: as given to hapgpu_k_scan_blocks;
 * blocks_hint: about how many 64 KiB blocks the scanned streams hold */
typedef struct HapGpuScanRecords {
    const void *recs;
    const void *joins;
    const HapGpuScanChunk *chunks;
    unsigned chunk_count;
    unsigned blocks_hint;
} HapGpuScanRecords;
/* frag_log2: fragment size of the batch's FRAGMENT units (0: none present);
 * fragment_kinds: bit g set = fragments of granularity_log2 g present */
/* fragment_kinds bits 8 / 9 / 10: field-stream units of [2,6,4,4] / [4,4] / [2,6] blocks present */
/* any_stream_or_copy_units: 0 none, 1 whole streams / raw copies, 2 the same with block-scanned streams among them */
int hapgpu_k_snappy_decode(hapgpu_rt *rt, const HapGpuDecodeUnit *units, unsigned unit_count,
                           HapGpuDecodeJob *jobs, unsigned frag_log2, unsigned fragment_kinds,
                           int any_stream_or_copy_units,
                           const uint32_t *fine_work, unsigned fine_slots /* the block scan's list and its capacity (0: none) */,
                           const HapGpuScanRecords *scan);

/* measurement */
void hapgpu_rt_set_profiling(hapgpu_rt *rt, int enable);
int hapgpu_rt_collect_profile(hapgpu_rt *rt, unsigned long *launches, double *ms, unsigned classes);
/* group tables for the STREAM units of jobs whose reserved bit 16 is set (fragments that came as chunks of their own,
   without a private table): units that turn out to be field streams become FIELDS units (snappy_decode_fields.hip) */
/* (work != NULL: only the units the block scan listed there -- the 8 KiB pieces of table-less streams of this library;
   unit_count then spans the fine region behind the ordinary units as well; with the scan's records their tables come
   from those) */
int hapgpu_k_guess_group_tables(hapgpu_rt *rt, HapGpuDecodeUnit *units, unsigned unit_count, const HapGpuDecodeJob *jobs,
                                const uint32_t *work, unsigned work_slots, const HapGpuScanRecords *scan);
int hapgpu_rt_timer_start(hapgpu_rt *rt);
int hapgpu_rt_timer_stop(hapgpu_rt *rt, double *ms);

#ifdef __cplusplus
}
#endif
#endif
