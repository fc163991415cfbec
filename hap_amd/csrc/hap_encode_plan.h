/*
 * hap_encode_plan.h -- what hapb_encode (hap_batch.c) decides about a call before it looks at a frame: the geometry of
 * every texture, which compressor kernel takes it, and what the call's scratch holds per frame.  Plain C arithmetic
 * over hap_frame.c's size functions, no runtime and no allocation: one definition for the call and for the stand-alone
 * program that walks it (tests/c/encode_plan.c).
 */
#ifndef HAP_ENCODE_PLAN_H
#define HAP_ENCODE_PLAN_H

#include "../../include/hap_gpu.h"
#include "hap_frame.h"

/* the context's switches that the plan reads (hap_batch.h: HapGpuContext) */
typedef struct hap_encode_knobs {
    unsigned frag_log2, byte_granular, position_lanes, rgtc1_fields, no_half_tiles, no_fusion;
    unsigned placing_allowed;   /* 0: the context or the call gathers whatever the geometry allows */
} hap_encode_knobs;

/* what the fusion rule asks of the pictures a call's textures are made from (hap_batch.h: HapbSource) */
typedef struct hap_encode_source {
    unsigned picture_kind;      /* HAPGPU_PICTURE_* */
    int planes, video;          /* planar tensors / NV12 pictures, not interleaved pictures */
    unsigned width, height;
    unsigned long row_bytes;
} hap_encode_source;

typedef struct hap_encode_tex {
    unsigned format, nibble, compressor, chunk_count, chunk_bytes, header_len, fpc;
    unsigned gran_log2, layout, half_tiles, fused;    /* the control word's fields (hapgpu_abi.h) */
    unsigned windowed;          /* its fragments announce the 3 KiB match window (HAP_FRAGMENT_WINDOW_256) */
    unsigned long bytes;
    size_t bound;               /* hap_max_encoded_length for the requested compressor (hap.c:386) */
} hap_encode_tex;

typedef struct hap_encode_plan {
    unsigned flags;             /* the call's, as they take effect: SMALLER_FILES clears the index */
    unsigned chunk_counts[2];   /* ... and its chunk counts: FINE_CHUNKS replaces those of Snappy textures */
    unsigned frag_log2;
    unsigned refine;            /* HAPGPU_BLOCK_ENCODE_REFINE or 0: what the call's block kernels are told */
    hap_encode_tex tex[2];
    unsigned outer_header;      /* 0 (single texture), 4 or 8 (hap.c:562-576) */
    unsigned frags_per_frame, chunks_per_frame, max_frags_per_tex, max_chunks_per_tex;
    size_t frame_raw_bound;     /* a frame with every texture stored as it is */
    size_t stage_in_bytes;      /* a frame's textures in staging, 256-byte aligned each */
    unsigned slot_stride;
    int any_snappy, any_half_tiles;
    HapGpuCompressKinds kinds;
    unsigned placed;            /* texture 0's fragments go where they belong in the frame -- as far as the frames
                                   themselves, their number and the context's history have no say */
    size_t placed_extent;       /* how far they can reach into a frame's buffer (0: not placed) */
} hap_encode_plan;

/* the control word of texture i of a frame of the call (placed: what the call has made of plan->placed) */
static inline uint32_t hap_encode_plan_control(const hap_encode_plan *p, unsigned i, unsigned placed)
{
    const hap_encode_tex *t = &p->tex[i];
    return hapgpu_control(t->gran_log2, t->windowed ? HAP_FRAGMENT_WINDOW_256 : 0u, t->layout, t->half_tiles, t->fused,
                          i == 0u ? placed : 0u);
}

/* bytes of a Snappy texture's instructions: the tables every Hap parser reads + the private fragment section */
static inline size_t hap_encode_plan_instructions(const hap_encode_tex *t, unsigned flags)
{
    size_t ilen = hapf_instructions_length(t->chunk_count);
    if (flags & HAPGPU_ENCODE_FRAGMENT_INDEX)
        ilen += 8u + (t->half_tiles ? 4u + HAP_GROUP_TABLE_BYTES : 4u) * (size_t)t->chunk_count * t->fpc;
    return ilen;
}

/* count 1 or 2 textures that encode_textures_valid has passed (hap_batch.c); source: NULL where the client made the
   textures.  Returns HapResult_No_Error, or HapResult_Bad_Arguments where a texture's instruction container would not
   fit its 24-bit length: *p then holds nothing. */
static inline unsigned hap_encode_plan_of(hap_encode_plan *p, const hap_encode_knobs *k, unsigned flags, unsigned count,
                                          const unsigned long *input_bytes, const unsigned *formats, const unsigned *compressors,
                                          const unsigned *chunk_counts, const hap_encode_source *source)
{
    static const hap_encode_plan none;
    /* HAPGPU_ENCODE_SMALLER_FILES: 64 KiB fragments (a match may lie 64 KiB back, like libsnappy's), elements on
       16-bit positions anywhere instead of whole block fields, and no fragment table */
    const int smaller = (flags & HAPGPU_ENCODE_SMALLER_FILES) != 0;
    const unsigned frag_log2 = smaller ? 16u : k->frag_log2, frag_bytes = 1u << frag_log2;
    /* a call that starts from RGBA8 pictures (hapb_source_frames): the block compressor makes the blocks of its
       fragment itself, one pass less over the texture and the pixel loads of one wave under the matching of the
       others (snappy_compress_blocks.hip).  One texture per frame. */
    const int fusable = source && !k->no_fusion && count == 1u && source->picture_kind == HAPGPU_PICTURE_RGBA8 && !source->planes &&
                        !source->video && (source->row_bytes & 3u) == 0 &&
                        (unsigned long long)source->row_bytes * source->height < 0xFFFFFFFFull && source->width / 4u >= 1u;
    unsigned i;
    *p = none;
    p->flags = smaller ? flags & ~HAPGPU_ENCODE_FRAGMENT_INDEX : flags;
    flags = p->flags;
    p->frag_log2 = frag_log2;
    /* HAPGPU_ENCODE_REFINE_ENDPOINTS: looked at where this call makes the blocks itself, of one texture a frame (the
       kernels look at it for RGB_DXT1 and RGBA_DXT5 alone) */
    p->refine = (source && count == 1u && (flags & HAPGPU_ENCODE_REFINE_ENDPOINTS)) ? HAPGPU_BLOCK_ENCODE_REFINE : 0u;
    /* HAPGPU_ENCODE_FINE_CHUNKS: one chunk per Snappy fragment (8 KiB of texture) -- the chunk size table every Hap parser
       reads (hap.c:265-300) then says where each independently compressed piece begins.  (Whatever the call's counts
       say for those textures is not looked at.) */
    for (i = 0; i < count; i++)
        p->chunk_counts[i] = ((flags & HAPGPU_ENCODE_FINE_CHUNKS) && !smaller && compressors[i] == HapCompressorSnappy)
                                 ? hapf_fine_chunk_count(input_bytes[i], formats[i]) : chunk_counts[i];
    chunk_counts = p->chunk_counts;
    if (count == 2) {
        size_t worst = 0;                                             /* hap.c:563-576 */
        for (i = 0; i < count; i++)
            worst += input_bytes[i] + hapf_instructions_length(chunk_counts[i]) + 4u;
        p->outer_header = worst > 0xFFFFFFu ? 8u : 4u;
    }
    p->kinds.textures = count;
    for (i = 0; i < count; i++) {
        hap_encode_tex *t = &p->tex[i];
        t->format = formats[i];
        t->nibble = hapf_nibble_from_format(formats[i]);
        t->compressor = compressors[i];
        t->bytes = input_bytes[i];
        t->bound = hapf_texture_bound(t->bytes, t->format, t->compressor, chunk_counts[i]);
        t->header_len = t->bytes > 0xFFFFFFu ? 8u : 4u;              /* hap.c:398-405 */
        if (t->compressor == HapCompressorSnappy) {
            t->chunk_count = hapf_limit_chunk_count(t->bytes, t->format, chunk_counts[i]);
            t->chunk_bytes = (unsigned)(t->bytes / t->chunk_count);
        }
        if (t->compressor == HapCompressorSnappy && t->chunk_bytes == 0) {
            /* less than one block per chunk (not a real texture): the reference compresses
               zero-length chunks, finds no gain and stores the section as-is (hap.c:478-495) */
            t->compressor = HapCompressorNone;
        }
        if (t->compressor == HapCompressorSnappy) {
            p->any_snappy = 1;
        } else {
            t->chunk_count = 1;
            t->chunk_bytes = (unsigned)t->bytes;
        }
        t->fpc = (t->chunk_bytes + frag_bytes - 1) / frag_bytes;
        /* 16-bit granular element streams need even chunk sizes (always true for block textures) */
        if (t->compressor == HapCompressorSnappy && !k->byte_granular) {
            /* DXT1 blocks are two 4-byte fields (endpoints, indices): everything repeats on 4-byte
               boundaries.  The alpha-style blocks of RGTC1 / DXT5 / YCoCg start their index bytes at
               byte 2, so those streams are 2-byte granular. */
            if ((t->format == HapTextureFormat_RGB_DXT1 || (flags & HAPGPU_ENCODE_COARSE_MATCHES) ||
                 (t->format == HapTextureFormat_A_RGTC1 && k->rgtc1_fields && k->rgtc1_fields != 26u)) && (t->chunk_bytes & 3u) == 0)
                t->gran_log2 = 2u;
            else if ((t->chunk_bytes & 1u) == 0)
                t->gran_log2 = 1u;
        }
        /* alpha-style blocks (2 endpoint + 6 index bytes [+ 4 + 4 of the colour half]) go to the field-per-lane
           compressor when everything lines up: default fragment size, whole blocks per chunk, 16-bit streams */
        t->layout = HAPGPU_LAYOUT_NONE;
        if (t->compressor == HapCompressorSnappy && frag_log2 == 13u && !k->position_lanes && !smaller) {
            if (t->gran_log2 == 1u && (t->format == HapTextureFormat_RGBA_DXT5 || t->format == HapTextureFormat_YCoCg_DXT5) &&
                (t->chunk_bytes & 15u) == 0)
                t->layout = HAPGPU_LAYOUT_2_6_4_4;
            else if (t->gran_log2 == 2u && (t->format == HapTextureFormat_RGB_DXT1 ||
                                            (t->format == HapTextureFormat_A_RGTC1 && k->rgtc1_fields)) && (t->chunk_bytes & 7u) == 0)
                t->layout = HAPGPU_LAYOUT_4_4;
            else if (t->gran_log2 == 1u && t->format == HapTextureFormat_A_RGTC1 && k->rgtc1_fields == 26u &&
                     (t->chunk_bytes & 7u) == 0 && t->bytes >= ((size_t)2u << 20))
                t->layout = HAPGPU_LAYOUT_2_6;
            else if ((flags & HAPGPU_ENCODE_COARSE_MATCHES) && t->gran_log2 == 2u && (t->chunk_bytes & 15u) == 0 &&
                     (t->format == HapTextureFormat_RGBA_BPTC_UNORM || t->format == HapTextureFormat_RGB_BPTC_UNSIGNED_FLOAT ||
                      t->format == HapTextureFormat_RGB_BPTC_SIGNED_FLOAT))
                t->layout = HAPGPU_LAYOUT_4_4_4_4;  /* the size-for-speed option: the block kernels instead of the
                                                       position-per-lane ones */
            /* (RGTC1 planes of 2 MiB and more -- block rows longer than a fragment -- take their natural [2, 6] layout:
               same size as the position-per-lane kernel there (0.171 against 0.169 of an 8K alpha plane).  Smaller
               ones stay with positions per lane: their matches start inside the index bytes of the row above, which
               lies inside the fragment -- 0.25 against 0.45 of a 2048 x 512 plane) */
        }
        /* field streams (fragment table version 4): with the table requested, the block compressor's streams come with
           a group table per fragment (where each of the decoder's 64 lanes starts reading) */
        t->half_tiles = (t->layout != HAPGPU_LAYOUT_NONE && (flags & HAPGPU_ENCODE_FRAGMENT_INDEX) && !k->no_half_tiles) ? 1u : 0u;
        if (t->half_tiles)
            p->any_half_tiles = 1;
        t->fused = HAPGPU_FUSED_NONE;
        if (fusable && t->layout == HAPGPU_LAYOUT_2_6_4_4) {
            if (t->format == HapTextureFormat_YCoCg_DXT5)
                t->fused = HAPGPU_FUSED_YCOCG;
            else if (t->format == HapTextureFormat_RGBA_DXT5 && !p->refine)
                /* (refined end points: the fused block compressor keeps its one definition of a block, and the
                   texture comes from the block kernel like a DXT1 one) */
                t->fused = HAPGPU_FUSED_DXT5;
            /* (DXT1, two blocks to a lane: built and measured -- 115 registers once the match stage's units are read
               back from the texture instead of kept; 60 4K frames 0.663 against 0.658 ms, 60 1080p frames 0.241
               against 0.233: its block encoder is further from its instruction-issue limit than the 16-byte ones',
               nothing to win.  The kernel keeps the two-pass form; the launcher does not start it.) */
        }
        if (t->compressor == HapCompressorSnappy) {
            /* which kernel the launcher starts for it */
            if (t->fused)
                p->kinds.fused |= 1u << t->fused;
            else if (t->layout != HAPGPU_LAYOUT_NONE)
                p->kinds.layouts |= 1u << t->layout;
            else
                p->kinds.granularities |= 1u << t->gran_log2;
        }
        if (t->compressor == HapCompressorSnappy) {
            /* header choice uses the layout that will actually be written (hap.c:425-428) */
            const size_t ilen = hap_encode_plan_instructions(t, flags);
            if (ilen + 4u > 0xFFFFFFu)            /* instruction container must fit a 24-bit length */
                return HapResult_Bad_Arguments;
            if (t->bytes + ilen + 4u > 0xFFFFFFu)
                t->header_len = 8u;
        }
        /* 8 KiB fragments keep hash matches within 3 KiB so that the decoder can halve its ring -- except for
           small textures, whose block rows are short enough for the row above to lie inside the fragment
           (rows of up to ~5 KiB: below 1080p for 16-byte blocks, below 4K for 8-byte blocks) */
        /* (field streams with their group table are decoded over a whole-fragment ring: no window) */
        t->windowed = frag_log2 == 13u && !t->half_tiles &&
                      t->bytes >= (hapf_block_bytes(t->format) == 8u ? ((size_t)2u << 20) : ((size_t)1u << 20));
        if ((size_t)t->chunk_count * t->fpc > p->max_frags_per_tex)
            p->max_frags_per_tex = t->chunk_count * t->fpc;
        p->frags_per_frame += t->chunk_count * t->fpc;
        p->chunks_per_frame += t->chunk_count;
        if (t->chunk_count > p->max_chunks_per_tex)
            p->max_chunks_per_tex = t->chunk_count;
        p->stage_in_bytes += (t->bytes + 255u) / 256u * 256u;
        p->frame_raw_bound += t->header_len + t->bytes;
    }
    p->frame_raw_bound += p->outer_header;
    /* the block compressor can put the first texture's fragments straight into the frame (no gather pass over them):
       its wavefronts learn the sizes of what lies before them from each other (snappy_compress_blocks.hip) */
    /* (up to 64 chunks: their totals are one load per wavefront.  16 8K frames of 400 chunks: 0.966 ms placed against 0.880
       gathered; of 1 chunk -- 4050 fragments to look back over -- 1.110 against 1.111) */
    /* (frames of two textures -- Hap Q Alpha -- with their FIRST texture placed and the second one gathered behind it:
       measured in round 5 and slower at every chunk count, because such calls run the compressor that reads finished
       textures, whose wavefronts are short: what a placed one waits for -- every fragment before it compressed -- is a
       larger share of its life than in the kernel that makes its blocks itself.  16 8K Hap Q Alpha frames, 24 + 24
       chunks: compress 0.493 -> 0.722 ms for a gather of 0.106 -> 0.036; 4 16K frames, 64 + 64: 0.922 -> 1.537 for
       0.219 -> 0.082.  One texture per frame.) */
    p->placed = (k->placing_allowed && count == 1u && p->tex[0].compressor == HapCompressorSnappy &&
                 p->tex[0].layout != HAPGPU_LAYOUT_NONE && frag_log2 == 13u && p->tex[0].chunk_count <= 64u) ? 1u : 0u;
    p->slot_stride = (frag_bytes + frag_bytes / 32u + 64u + HAPGPU_SLOT_SCRATCH_BYTES + 15u) / 16u * 16u;
    /* how far placed fragments can reach into the frame buffer if nothing shrinks (the frame is then encoded again, but
       the bytes have been written): the chunked layout's headers and tables + every fragment at its largest (what a slot
       holds).  The bound hap.h asks of the client's buffer covers it except for chunks of a few hundred bytes with the
       private table requested; buffers that do not are served through slots. */
    if (p->placed) {
        const hap_encode_tex *t = &p->tex[0];
        p->placed_extent = p->outer_header + 8u + 4u + hap_encode_plan_instructions(t, flags) + 5u * (size_t)t->chunk_count + t->bytes +
                           (size_t)t->chunk_count * t->fpc * (frag_bytes / 32u + 64u);
        /* the compressor's wavefronts add up what lies before them in the frame in 32 bits: every such sum is a
           position below this extent (a texture is below 4 GiB, but its fragments at their largest need not be).
           Beyond it the frame goes through slots. */
        if (p->placed_extent > 0xFFFFFFFFul) {
            p->placed = 0u;
            p->placed_extent = 0;
        }
    }
    return HapResult_No_Error;
}

#endif
