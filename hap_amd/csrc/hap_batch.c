/*
 * hap_batch.c -- host-side orchestration of the GPU hot path (pure C99).
 *
 * Implements the batched entry points of include/hap_gpu.h; the six hap.h
 * functions in hap_api.c are thin wrappers around the batch-of-one case.
 * The host does only container arithmetic (header lengths, chunk-count
 * limiting, section location, table parsing -- see hap_frame.c) and fills the
 * descriptor arrays of hapgpu_abi.h; every byte of texture payload is moved,
 * compressed or decompressed by HIP kernels.  There is no CPU fallback: when
 * no HIP device is present the functions fail with HapResult_Internal_Error.
 * Here: frames from textures, pictures and tensors (hapb_encode and the block
 * encoders before it), textures from frames (hapb_decode), the join on the
 * device.  What goes on from block textures is hap_pictures.c's.
 *
 * Reference behaviour mirrored here: argument checks and result codes of
 * HapEncode (hap.c:506-604, 355-504) and HapDecode (hap.c:993-1040, 732-930).
 */
#include "hap_batch_private.h"
#include "measurement_guard.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef HAPB_TRACE
#include <stdio.h>
#include <time.h>
static double hapb_now_us(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
#define HAPB_MARK(name) do { double t_ = hapb_now_us(); fprintf(stderr, "  [decode %u] %-10s +%.1f us\n", frame_count, name, t_ - hapb_t0); hapb_t0 = t_; } while (0)
#else
#define HAPB_MARK(name) do { } while (0)
#endif
#define PREFIX_BYTES 2048u   /* headers + tables of a frame with up to ~400 chunks; larger ones are fetched on demand */
#define PREFIX_BATCH_MAX_BYTES ((size_t)32u << 20)   /* the longer second prefix, all frames of a call together (x2: a far window each) */
#define COPY_PIECE 65536u

int context_busy(HapGpuContext *c, unsigned *results, unsigned frame_count)
{
    unsigned f;
    if (!c->pending_encode)
        return 0;
    fprintf(stderr, "hap_amd: the context has an encode call in flight (HapGpuEncodeFramesFinish first)\n");
    for (f = 0; results && f < frame_count; f++)
        results[f] = HapResult_Internal_Error;
    return 1;
}

/* ================================================================== encode */

typedef struct tex_geom {
    unsigned format, compressor, chunk_count, chunk_bytes, header_len, fpc, nibble, gran_log2, field_period, half_tiles;
    unsigned long bytes;
    size_t bound;        /* hap_max_encoded_length for the requested compressor (hap.c:386) */
} tex_geom;

unsigned encode_textures_valid(unsigned count, const unsigned long *input_bytes, const unsigned *formats,
                               const unsigned *compressors, const unsigned *chunk_counts, unsigned flags)
{
    const int smaller = (flags & HAPGPU_ENCODE_SMALLER_FILES) != 0;
    unsigned i;
    /* (with HAPGPU_ENCODE_FINE_CHUNKS the call's chunk counts are replaced: whatever they say is not looked at) */
    for (i = 0; i < count; i++)
        if (chunk_counts[i] == 0 && !((flags & HAPGPU_ENCODE_FINE_CHUNKS) && !smaller && compressors[i] == HapCompressorSnappy))
            return HapResult_Bad_Arguments;
    if (count == 2 &&
        formats[0] != HapTextureFormat_YCoCg_DXT5 && formats[1] != HapTextureFormat_YCoCg_DXT5 &&
        formats[0] != HapTextureFormat_A_RGTC1 && formats[1] != HapTextureFormat_A_RGTC1)
        return HapResult_Bad_Arguments;
    for (i = 0; i < count; i++)
        if (input_bytes[i] == 0 || input_bytes[i] > 0xFFFFFFFFul || hapf_nibble_from_format(formats[i]) == 0 ||
            (compressors[i] != HapCompressorNone && compressors[i] != HapCompressorSnappy))
            return HapResult_Bad_Arguments;
    return HapResult_No_Error;
}

/* the columns of a block-encode job's address table, frame_count entries each: the sources and an output per texture;
   video pictures: Y planes, outputs, CbCr planes */
static unsigned job_table_columns(const HapbBlockEncodeJob *job)
{
    return job->source.video ? 3u : 1u + job->count;
}

unsigned hapb_encode(HapGpuContext *ctx, unsigned frame_count, unsigned count,
                     const void *const *inputs, const unsigned long *input_bytes,
                     const unsigned *formats, const unsigned *compressors, const unsigned *chunk_counts,
                     void *const *outputs, const unsigned long *output_bytes,
                     unsigned long *output_used, unsigned *results, unsigned flags,
                     const HapbEncodeArgs *args)
{
    static const HapbEncodeArgs no_args;
    const HapbEncodeArgs *const a = args ? args : &no_args;
    const int inputs_are_device = a->inputs_are_device;
    const HapbBlockEncodeJob *const job = a->job;
    /* HAPGPU_ENCODE_REFINE_ENDPOINTS: looked at where this call makes the blocks itself, of one texture a frame (the
       kernels look at it for RGB_DXT1 and RGBA_DXT5 alone) */
    const unsigned refine = (job && count == 1u && (flags & HAPGPU_ENCODE_REFINE_ENDPOINTS)) ? HAPGPU_BLOCK_ENCODE_REFINE : 0u;
    tex_geom g[2];
    unsigned fine_counts[2] = {0u, 0u};
    unsigned i, f, first_error = HapResult_No_Error;
    unsigned outer_header = 0, frags_per_frame = 0, max_frags_per_tex = 0, live = 0, chunks_per_frame = 0;
    int any_half_tiles = 0;
    uint8_t *dgrouptables = NULL;
    void *dpack = NULL;
    unsigned max_chunks_per_tex = 0;
    /* HAPGPU_ENCODE_SMALLER_FILES: 64 KiB fragments (a match may lie 64 KiB back, like libsnappy's), elements on
       16-bit positions anywhere instead of whole block fields, and no fragment table */
    const int smaller = (flags & HAPGPU_ENCODE_SMALLER_FILES) != 0;
    unsigned frag_log2 = smaller ? 16u : ctx->frag_log2, frag_bytes = 1u << frag_log2;
    unsigned slot_stride;
    int any_snappy = 0;
    unsigned gran_mask = 0;
    size_t placed_extent = 0;
    unsigned placed = 0u;                            /* texture 0's fragments are written where they belong in the frame (bit 27) */
    uint64_t *dacc = NULL;
    unsigned fused[2] = {0u, 0u}, fused_mask = 0u;   /* textures the second stage makes from the RGBA itself (code: reserved bits 24..26) */
    size_t stage_in_bytes = 0, stage_out_bytes = 0, frame_raw_bound = 0;
    hapgpu_rt *rt = ctx->rt;
    HapGpuFrameEnc *hframes, *dframes;
    uint8_t *dslots, *tex_stage = NULL, *out_stage = NULL;
    uint32_t *dfragsizes;
    HapGpuCopyEntry *dcopies;
    size_t *stage_off_in = NULL, *stage_off_out = NULL;
    unsigned *live_index = NULL;

    if (frame_count == 0)
        return HapResult_No_Error;
    if (!results)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, results, frame_count))
        return HapResult_Internal_Error;
    /* frame-independent argument checks, reference hap.c:518-559 */
    {
        unsigned rc = HapResult_No_Error;
        if (count == 0 || count > 2 || !inputs || !input_bytes || !formats || !compressors || !chunk_counts ||
            !outputs || !output_bytes || !output_used)
            rc = HapResult_Bad_Arguments;
        if (rc == HapResult_No_Error)
            rc = encode_textures_valid(count, input_bytes, formats, compressors, chunk_counts, flags);
        if (rc != HapResult_No_Error) {
            for (f = 0; f < frame_count; f++)
                results[f] = rc;
            return rc;
        }
    }
    if (smaller)
        flags &= ~HAPGPU_ENCODE_FRAGMENT_INDEX;
    /* HAPGPU_ENCODE_FINE_CHUNKS: one chunk per Snappy fragment (8 KiB of texture) -- the chunk size table every Hap parser
       reads (hap.c:265-300) then says where each independently compressed piece begins */
    if ((flags & HAPGPU_ENCODE_FINE_CHUNKS) && !smaller) {
        for (i = 0; i < count; i++)
            fine_counts[i] = compressors[i] == HapCompressorSnappy ? HapGpuFineChunkCount(input_bytes[i], formats[i]) : chunk_counts[i];
        chunk_counts = fine_counts;
    }
    /* geometry shared by every frame of the batch */
    if (count == 2) {
        size_t worst = 0;                                             /* hap.c:563-576 */
        for (i = 0; i < count; i++)
            worst += input_bytes[i] + hapf_instructions_length(chunk_counts[i]) + 4u;
        outer_header = worst > 0xFFFFFFu ? 8u : 4u;
    }
    for (i = 0; i < count; i++) {
        tex_geom *t = &g[i];
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
            any_snappy = 1;
        } else {
            t->chunk_count = 1;
            t->chunk_bytes = (unsigned)t->bytes;
        }
        t->fpc = (t->chunk_bytes + frag_bytes - 1) / frag_bytes;
        /* 16-bit granular element streams need even chunk sizes (always true for block textures) */
        t->gran_log2 = 0u;
        if (t->compressor == HapCompressorSnappy && !ctx->byte_granular) {
            /* DXT1 blocks are two 4-byte fields (endpoints, indices): everything repeats on 4-byte
               boundaries.  The alpha-style blocks of RGTC1 / DXT5 / YCoCg start their index bytes at
               byte 2, so those streams are 2-byte granular. */
            if ((t->format == HapTextureFormat_RGB_DXT1 || (flags & HAPGPU_ENCODE_COARSE_MATCHES) ||
                 (t->format == HapTextureFormat_A_RGTC1 && ctx->rgtc1_fields && ctx->rgtc1_fields != 26u)) && (t->chunk_bytes & 3u) == 0)
                t->gran_log2 = 2u;
            else if ((t->chunk_bytes & 1u) == 0)
                t->gran_log2 = 1u;
        }
        /* alpha-style blocks (2 endpoint + 6 index bytes [+ 4 + 4 of the colour half]) go to the field-per-lane
           compressor when everything lines up: default fragment size, whole blocks per chunk, 16-bit streams */
        t->field_period = 0u;
        if (t->compressor == HapCompressorSnappy && frag_log2 == 13u && !ctx->position_lanes && !smaller) {
            if (t->gran_log2 == 1u && (t->format == HapTextureFormat_RGBA_DXT5 || t->format == HapTextureFormat_YCoCg_DXT5) &&
                (t->chunk_bytes & 15u) == 0)
                t->field_period = 4u;
            else if (t->gran_log2 == 2u && (t->format == HapTextureFormat_RGB_DXT1 ||
                                            (t->format == HapTextureFormat_A_RGTC1 && ctx->rgtc1_fields)) && (t->chunk_bytes & 7u) == 0)
                t->field_period = 10u;      /* 2 fields per block, the [4, 4] layout (code 2 | 8) */
            else if (t->gran_log2 == 1u && t->format == HapTextureFormat_A_RGTC1 && ctx->rgtc1_fields == 26u &&
                     (t->chunk_bytes & 7u) == 0 && t->bytes >= ((size_t)2u << 20))
                t->field_period = 2u;       /* [2, 6]: endpoints, indices */
            else if ((flags & HAPGPU_ENCODE_COARSE_MATCHES) && t->gran_log2 == 2u && (t->chunk_bytes & 15u) == 0 &&
                     (t->format == HapTextureFormat_RGBA_BPTC_UNORM || t->format == HapTextureFormat_RGB_BPTC_UNSIGNED_FLOAT ||
                      t->format == HapTextureFormat_RGB_BPTC_SIGNED_FLOAT))
                t->field_period = 12u;      /* opaque 16-byte blocks as four dwords (the size-for-speed option): the block
                                               kernels instead of the position-per-lane ones */
            /* (RGTC1 planes of 2 MiB and more -- block rows longer than a fragment -- take their natural [2, 6] layout:
               same size as the position-per-lane kernel there (0.171 against 0.169 of an 8K alpha plane).  Smaller
               ones stay with positions per lane: their matches start inside the index bytes of the row above, which
               lies inside the fragment -- 0.25 against 0.45 of a 2048 x 512 plane) */
        }
        /* field streams (fragment table version 3): with the table requested, the block compressor's streams come with
           a group table per fragment (96 bytes: where each of the decoder's 64 lanes starts reading) */
        t->half_tiles = ((t->field_period == 4u || t->field_period == 10u || t->field_period == 2u || t->field_period == 12u) && (flags & HAPGPU_ENCODE_FRAGMENT_INDEX) &&
                         !ctx->no_half_tiles) ? 1u : 0u;
        if (t->half_tiles)
            any_half_tiles = 1;
        /* a call that starts from RGBA8 pictures (hapb_source_frames): the block compressor makes the blocks of its
           fragment itself, one pass less over the texture and the pixel loads of one wave under the matching of the
           others (snappy_compress_blocks.hip).  One texture per frame. */
        {
            if (job && !ctx->no_fusion && count == 1u && job->source.picture_kind == HAPGPU_PICTURE_RGBA8 && !job->source.planes &&
                !job->source.video && (job->source.row_bytes & 3u) == 0 && (unsigned long long)job->source.row_bytes * job->source.height < 0xFFFFFFFFull &&
                job->source.width / 4u >= 1u) {
                /* (code: HapGpuTexEnc.reserved bits 24..26; mask bit: which kernel the launcher starts) */
                if (t->field_period == 4u && t->format == HapTextureFormat_YCoCg_DXT5) {
                    fused[i] = 3u; fused_mask |= 1u;
                } else if (t->field_period == 4u && t->format == HapTextureFormat_RGBA_DXT5 && !refine) {
                    /* (refined end points: the fused block compressor keeps its one definition of a block, and the
                       texture comes from the block kernel like a DXT1 one) */
                    fused[i] = 2u; fused_mask |= 2u;
                }
                /* (DXT1, two blocks to a lane: built and measured -- 115 registers once the match stage's units are read
                   back from the texture instead of kept; 60 4K frames 0.663 against 0.658 ms, 60 1080p frames 0.241
                   against 0.233: its block encoder is further from its instruction-issue limit than the 16-byte ones',
                   nothing to win.  The kernel keeps the two-pass form; the launcher does not start it.) */
            }
        }
        if (t->compressor == HapCompressorSnappy && !fused[i])
            gran_mask |= t->field_period == 4u ? 32u : t->field_period == 10u ? 64u : t->field_period == 2u ? 16u
                         : t->field_period == 12u ? 128u : 1u << t->gran_log2;
        if (t->compressor == HapCompressorSnappy) {
            /* header choice uses the layout that will actually be written (hap.c:425-428) */
            size_t ilen = hapf_instructions_length(t->chunk_count);
            if (flags & HAPGPU_ENCODE_FRAGMENT_INDEX)
                ilen += 8u + (t->half_tiles ? 4u + HAP_GROUP_TABLE_BYTES : 4u) * (size_t)t->chunk_count * t->fpc;
            if (ilen + 4u > 0xFFFFFFu) {          /* instruction container must fit a 24-bit length */
                for (f = 0; f < frame_count; f++) {
                    results[f] = HapResult_Bad_Arguments;
                    output_used[f] = 0;
                }
                return HapResult_Bad_Arguments;
            }
            if (t->bytes + ilen + 4u > 0xFFFFFFu)
                t->header_len = 8u;
        }
        if ((size_t)t->chunk_count * t->fpc > max_frags_per_tex)
            max_frags_per_tex = t->chunk_count * t->fpc;
        frags_per_frame += t->chunk_count * t->fpc;
        chunks_per_frame += t->chunk_count;
        if (t->chunk_count > max_chunks_per_tex)
            max_chunks_per_tex = t->chunk_count;
        stage_in_bytes += align_up(t->bytes, 256);
        frame_raw_bound += t->header_len + t->bytes;
    }
    frame_raw_bound += outer_header;
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
    placed = (!ctx->no_placing && !a->never_place && !ctx->placing_off && count == 1u && g[0].compressor == HapCompressorSnappy && g[0].field_period != 0u && frag_log2 == 13u &&
              g[0].chunk_count <= 64u) ? 1u : 0u;
    slot_stride = (unsigned)align_up(frag_bytes + frag_bytes / 32u + 64u + HAPGPU_SLOT_SCRATCH_BYTES, 16);
    /* how far placed fragments can reach into the frame buffer if nothing shrinks (the frame is then encoded again, but
       the bytes have been written): the chunked layout's headers and tables + every fragment at its largest (what a slot
       holds).  The bound hap.h asks of the client's buffer covers it except for chunks of a few hundred bytes with the
       private table requested; buffers that do not are served through slots. */
    if (placed) {
        const size_t frags = (size_t)g[0].chunk_count * g[0].fpc;
        size_t ilen = hapf_instructions_length(g[0].chunk_count);
        if (flags & HAPGPU_ENCODE_FRAGMENT_INDEX)
            ilen += 8u + (g[0].half_tiles ? 4u + HAP_GROUP_TABLE_BYTES : 4u) * frags;
        placed_extent = outer_header + 8u + 4u + ilen + 5u * (size_t)g[0].chunk_count + g[0].bytes + frags * (frag_bytes / 32u + 64u);
        /* the compressor's wavefronts add up what lies before them in the frame in 32 bits: every such sum is a
           position below this extent (a texture is below 4 GiB, but its fragments at their largest need not be).
           Beyond it the frame goes through slots. */
        if (placed_extent > 0xFFFFFFFFul) {
            placed = 0u;
            placed_extent = 0;
        }
    }

    /* per-frame checks; frames that fail are left out of the launch */
    live_index = (unsigned *)malloc(sizeof(unsigned) * frame_count);
    stage_off_in = (size_t *)calloc(frame_count, sizeof(size_t));
    stage_off_out = (size_t *)calloc(frame_count, sizeof(size_t));
    if (!live_index || !stage_off_in || !stage_off_out) {
        free(live_index); free(stage_off_in); free(stage_off_out);
        return HapResult_Internal_Error;
    }
    {
        size_t in_total = 0, out_total = 0;
        for (f = 0; f < frame_count; f++) {
            unsigned rc = HapResult_No_Error;
            if (!outputs[f] || output_bytes[f] == 0)
                rc = HapResult_Bad_Arguments;
            for (i = 0; rc == HapResult_No_Error && i < count; i++)
                if (!inputs[(size_t)f * count + i])
                    rc = HapResult_Bad_Arguments;
            if (rc == HapResult_No_Error) {
                /* hap.c:386-389 for the first texture; later textures are re-checked against
                   the space actually left once the sizes are known */
                size_t avail = output_bytes[f] > outer_header ? output_bytes[f] - outer_header : 0;
                if (avail < g[0].bound || output_bytes[f] < frame_raw_bound)
                    rc = HapResult_Buffer_Too_Small;
                /* second texture: the reference compares its bound with what is left after the
                   first section's ACTUAL size (hap.c:589); that size is not known before the
                   launch, so the first section's maximum (raw storage) is assumed */
                else if (count == 2 && avail - (g[0].header_len + g[0].bytes) < g[1].bound)
                    rc = HapResult_Buffer_Too_Small;
            }
            results[f] = rc;
            output_used[f] = 0;
            if (rc != HapResult_No_Error) {
                if (first_error == HapResult_No_Error)
                    first_error = rc;
                continue;
            }
            live_index[live++] = f;
            if (output_bytes[f] < placed_extent)
                placed = 0u;
            if (!inputs_are_device) {
                int staged = 0;
                for (i = 0; i < count; i++)
                    if (!is_dev(ctx, inputs[(size_t)f * count + i]))
                        staged = 1;
                if (staged) {
                    stage_off_in[f] = in_total + 1;         /* +1: 0 means "not staged" */
                    in_total += stage_in_bytes;
                }
            }
            if (!is_dev(ctx, outputs[f])) {
                stage_off_out[f] = out_total + 1;
                /* (+8 per texture: a section written in the chunked form may exceed header + bytes by up to
                   header_len - 1 bytes, see the comparison in frame_pack_kernel / hap.c:478) */
                out_total += align_up(frame_raw_bound + 8u * count > placed_extent ? frame_raw_bound + 8u * count : placed_extent, 256);
            }
        }
        stage_in_bytes = in_total;
        stage_out_bytes = out_total;
    }
    if (live == 0) {
        free(live_index); free(stage_off_in); free(stage_off_out);
        return first_error;
    }
    /* (frames are interleaved over the workgroups: with a dozen of them, few fragments of the same frame are in flight
       together and the waiting costs less than the gather pass; measured on 8K frames: 1 frame 0.130 against 0.114 ms,
       8 the same, 16 0.885 against 0.914, 60 2.90 against 3.08) */
    if (live < ctx->placing_min_frames)
        placed = 0u;
    if (placed && ctx->placing_holdoff) {
        ctx->placing_holdoff -= 1u;
        placed = 0u;
    }
    if (ctx->placing_off)                            /* (after a timeout: counted down call by call, then placing is back) */
        ctx->placing_off -= 1u;

    /* scratch */
    hframes = (HapGpuFrameEnc *)hapgpu_rt_pinned_scratch(rt, P_FRAMES, sizeof(HapGpuFrameEnc) * live);
    dframes = (HapGpuFrameEnc *)hapgpu_rt_device_scratch(rt, D_FRAMES, sizeof(HapGpuFrameEnc) * live);
    dslots = any_snappy ? (uint8_t *)hapgpu_rt_device_scratch(rt, D_SLOTS, (size_t)slot_stride * frags_per_frame * live) : NULL;
    dfragsizes = (uint32_t *)hapgpu_rt_device_scratch(rt, D_FRAGSIZES, sizeof(uint32_t) * (size_t)frags_per_frame * live);
    dcopies = (HapGpuCopyEntry *)hapgpu_rt_device_scratch(rt, D_COPIES, sizeof(HapGpuCopyEntry) * ((size_t)frags_per_frame + chunks_per_frame) * live);
    dpack = hapgpu_rt_device_scratch(rt, D_PACK, (size_t)hapgpu_pack_scratch_bytes_per_chunk() * chunks_per_frame * live);
    if (placed)
        dacc = (uint64_t *)hapgpu_rt_device_scratch(rt, D_CHUNK_ACC, sizeof(uint64_t) * (size_t)chunks_per_frame * live);
    if (any_half_tiles)
        dgrouptables = (uint8_t *)hapgpu_rt_device_scratch(rt, D_GROUPTABLES, (size_t)HAP_GROUP_TABLE_BYTES * frags_per_frame * live);
    if (stage_in_bytes)
        tex_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TEX_STAGE, stage_in_bytes);
    if (stage_out_bytes)
        out_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_FRAME_STAGE, stage_out_bytes);
    if (!hframes || !dframes || (placed && !dacc) || (any_snappy && !dslots) || !dfragsizes || !dcopies || !dpack || (any_half_tiles && !dgrouptables) ||
        (stage_in_bytes && !tex_stage) || (stage_out_bytes && !out_stage)) {
        free(live_index); free(stage_off_in); free(stage_off_out);
        for (f = 0; f < frame_count; f++)
            if (results[f] == HapResult_No_Error)
                results[f] = HapResult_Internal_Error;
        return HapResult_Internal_Error;
    }

    /* descriptors (+ host->device staging of textures) */
    {
        unsigned k, rc = 0;
        for (k = 0; k < live; k++) {
            HapGpuFrameEnc *fe = &hframes[k];
            size_t in_cursor = 0;
            f = live_index[k];
            memset(fe, 0, sizeof(*fe));
            fe->dst = (uint64_t)(uintptr_t)(stage_off_out[f] ? out_stage + (stage_off_out[f] - 1) : (uint8_t *)outputs[f]);
            fe->dst_cap = output_bytes[f];
            fe->tex_count = count;
            fe->outer_header_len = outer_header;
            fe->status = HapResult_Internal_Error;   /* overwritten by the pack kernel */
            if (placed)
                fe->chunk_acc = (uint64_t)(uintptr_t)(dacc + (size_t)k * chunks_per_frame);
            if (fused_mask) {
                fe->rgba = job->host_table[f];
                fe->rgba_row_bytes = (uint32_t)job->source.row_bytes;
                fe->rgba_blocks_x = job->source.width / 4u;
                fe->rgba_blocks_x_inv = HAPGPU_DIV_INV(job->source.width / 4u);
            }
            for (i = 0; i < count; i++) {
                HapGpuTexEnc *te = &fe->tex[i];
                const void *src = inputs[(size_t)f * count + i];
                if (stage_off_in[f] && !is_dev(ctx, src)) {
                    uint8_t *d = tex_stage + (stage_off_in[f] - 1) + in_cursor;
                    rc |= (unsigned)hapgpu_rt_h2d(rt, d, src, g[i].bytes);
                    src = d;
                }
                in_cursor += align_up(g[i].bytes, 256);
                te->src = (uint64_t)(uintptr_t)src;
                te->bytes = (uint32_t)g[i].bytes;
                te->format_nibble = g[i].nibble;
                te->compressor = g[i].compressor;
                te->chunk_count = g[i].chunk_count;
                te->chunk_bytes = g[i].chunk_bytes;
                te->header_len = g[i].header_len;
                te->frags_per_chunk = g[i].fpc;
                te->frags_per_chunk_inv = HAPGPU_DIV_INV(g[i].fpc ? g[i].fpc : 1u);
                te->frag_first = k * frags_per_frame + (i ? g[0].chunk_count * g[0].fpc : 0u);
                te->emit_index = (flags & HAPGPU_ENCODE_FRAGMENT_INDEX) ? 1u : 0u;
                /* 8 KiB fragments keep hash matches within 3 KiB so that the decoder can halve its ring -- except for
                   small textures, whose block rows are short enough for the row above to lie inside the fragment
                   (rows of up to ~5 KiB: below 1080p for 16-byte blocks, below 4K for 8-byte blocks) */
                {
                    const int small_blocks = hapf_block_bytes(g[i].format) == 8u;
                    /* (field streams with their group table are decoded over a whole-fragment ring: no window) */
                    const int windowed = frag_log2 == 13u && !g[i].half_tiles &&
                                         g[i].bytes >= (small_blocks ? ((size_t)2u << 20) : ((size_t)1u << 20));
                    te->reserved = g[i].gran_log2 | (windowed ? (HAP_FRAGMENT_WINDOW_256 << 8) : 0u) | (g[i].field_period << 16) |
                                   (g[i].half_tiles << 20) | (fused[i] << 24) | ((i == 0u ? placed : 0u) << 27);
                }
            }
        }
        {
            /* The launches of this call as one sequence.  With every buffer in device memory (nothing staged) nothing
               in it depends on the buffers themselves -- their addresses are in the tables copied from pinned memory --
               so the sequence is recorded once per geometry as a HIP graph and replayed with one launch. */
            uint64_t key = 0xCBF29CE484222325ull;
            int graph = 2;
            unsigned launch_rc = 0;
#define HAPB_MIX(v) (key = (key ^ (uint64_t)(v)) * 0x100000001B3ull)
            if (stage_in_bytes == 0 && stage_out_bytes == 0 && inputs_are_device != 2 && !smaller && frag_log2 == 13u) {
                HAPB_MIX(live); HAPB_MIX(count); HAPB_MIX(flags); HAPB_MIX(frag_log2); HAPB_MIX(ctx->byte_granular);
                HAPB_MIX(ctx->position_lanes); HAPB_MIX(ctx->rgtc1_fields); HAPB_MIX(ctx->no_half_tiles); HAPB_MIX(fused_mask); HAPB_MIX(placed);
                for (i = 0; i < count; i++) {
                    HAPB_MIX(g[i].format); HAPB_MIX(g[i].compressor); HAPB_MIX(g[i].chunk_count); HAPB_MIX(g[i].bytes);
                }
                if (job) {
                    const HapbSource *const src = &job->source;
                    HAPB_MIX(job->frame_count); HAPB_MIX(src->width); HAPB_MIX(src->height); HAPB_MIX(src->row_bytes);
                    HAPB_MIX(job->wide + 2); HAPB_MIX(src->picture_kind);
                    if (src->planes) {
                        /* (scale and bias are kernel arguments: part of what a recording holds) */
                        HAPB_MIX(src->planes->channels + 8u); HAPB_MIX(src->planes->element); HAPB_MIX(src->planes->plane_bytes);
                        for (i = 0; i < src->planes->channels; i++) {
                            uint32_t bits[2];
                            memcpy(&bits[0], &job->plane_scale[i], 4);
                            memcpy(&bits[1], &job->plane_bias[i], 4);
                            HAPB_MIX(bits[0]); HAPB_MIX(bits[1]);
                        }
                    }
                    if (src->video) {
                        /* (the pitch, the matrix and the range are kernel arguments too) */
                        HAPB_MIX(16u); HAPB_MIX(src->video->chroma_row_bytes); HAPB_MIX(src->video->matrix); HAPB_MIX(src->video->range);
                    }
                }
                graph = hapgpu_rt_graph_begin(rt, key);
            }
#undef HAPB_MIX
            /* (a recording that cannot be ended, instantiated or launched has run nothing: graphs are switched off for
               this context and the same launches are issued once more, plainly) */
            while (graph != 1) {
                if (job) {
                    const HapbSource *const src = &job->source;
                    launch_rc |= (unsigned)hapgpu_rt_h2d(rt, job->device_table, job->host_table,
                                                         sizeof(uint64_t) * (size_t)job_table_columns(job) * job->frame_count);
                    /* Hap Q Alpha: both textures from one pass over the RGBA (64 + 16 + 8 bytes per block);
                       else one launch per texture that the second stage does not make itself.  (A batch takes at most
                       65535 block rows.) */
                    const int pair = job->count == 2 && job->formats[0] == HapTextureFormat_YCoCg_DXT5 &&
                                     job->formats[1] == HapTextureFormat_A_RGTC1;
                    for (i = 0; i < (pair ? 1u : job->count); i++)
                        if (pair || !fused[i]) {
                            const uint64_t *dt = job->device_table;
                            /* (video pictures: one texture a frame, and the third column holds their CbCr planes) */
                            const HapGpuPictureTable t = {{dt, dt + (size_t)(1u + i) * job->frame_count,
                                                           pair || src->video ? dt + 2u * (size_t)job->frame_count : NULL}, {0u, 0u, 0u}};
                            launch_rc |= src->height / 4u > 65535u ? 1u :
                                         src->video ?
                                         (unsigned)hapgpu_k_block_encode_video(rt, &t, job->frame_count, src->width, src->height,
                                                                               job->formats[i], refine, src->row_bytes,
                                                                               src->video->chroma_row_bytes, src->video->matrix,
                                                                               src->video->range) :
                                         src->planes ?
                                         (unsigned)hapgpu_k_block_encode_planes(rt, &t, job->frame_count, src->width, src->height,
                                                                                job->formats[i], (unsigned)pair | refine, src->planes->channels,
                                                                                src->planes->element, src->planes->plane_bytes,
                                                                                src->row_bytes, job->plane_scale, job->plane_bias) :
                                         (unsigned)hapgpu_k_block_encode(rt, &t, job->frame_count, src->width, src->height,
                                                                         src->row_bytes, job->formats[i], (unsigned)pair | refine, job->wide,
                                                                         src->picture_kind);
                        }
                }
                launch_rc |= (unsigned)hapgpu_rt_h2d(rt, dframes, hframes, sizeof(HapGpuFrameEnc) * live);
                if (placed) {
                    launch_rc |= (unsigned)hapgpu_rt_zero(rt, dacc, sizeof(uint64_t) * (size_t)chunks_per_frame * live);
                    launch_rc |= (unsigned)hapgpu_rt_zero(rt, dfragsizes, sizeof(uint32_t) * (size_t)frags_per_frame * live);
                }
                if (any_snappy)
                    launch_rc |= (unsigned)hapgpu_k_snappy_compress(rt, dframes, live, max_frags_per_tex, frag_log2, dslots, slot_stride,
                                                                    dfragsizes, dgrouptables, gran_mask | (count << 8) | (fused_mask << 16));   /* bits 8..15: textures per frame */
                launch_rc |= (unsigned)hapgpu_k_frame_pack(rt, dframes, live, frag_log2, dslots, slot_stride, dfragsizes, dgrouptables,
                                                           dcopies, frags_per_frame * live, chunks_per_frame, max_chunks_per_tex, count, dpack);
                /* (placed fragments -- single-texture frames -- and their group tables are where they belong: nothing to
                   gather.  A frame reported as not placed is encoded again as a whole.) */
                if (!(placed && count == 1u))
                    launch_rc |= (unsigned)hapgpu_k_frame_gather(rt, dcopies, (frags_per_frame + chunks_per_frame) * live);
                launch_rc |= (unsigned)hapgpu_rt_d2h(rt, hframes, dframes, sizeof(HapGpuFrameEnc) * live);
                if (graph == 0) {
                    /* (a recording can also be invalidated from outside -- another thread of the process synchronising the
                       device while it runs: then the launches themselves report errors.  Either way nothing has run.) */
                    const int ended = hapgpu_rt_graph_end(rt, key, launch_rc != 0);
                    if (ended != 0 || launch_rc != 0) {
                        hapgpu_rt_graphs_disable(rt);
                        graph = 2;
                        launch_rc = 0;
                        continue;
                    }
                }
                break;
            }
            rc |= launch_rc;
        }
        /* everything the call launches is on the stream: the rest -- waiting, reading the results, the second pass over
           frames that were not placed -- is hapb_encode_complete's, at once or (HapGpuEncodeFramesRGBABegin / ...Finish)
           when the client asks for the results */
        {
            HapbEncodePending *pd = (HapbEncodePending *)calloc(1, sizeof(*pd));
            const size_t n_in = (size_t)frame_count * count;
            if (pd) {
                pd->inputs = (const void **)malloc(sizeof(void *) * n_in);
                pd->outputs = (void **)malloc(sizeof(void *) * frame_count);
                pd->output_bytes = (unsigned long *)malloc(sizeof(unsigned long) * frame_count);
            }
            if (!pd || !pd->inputs || !pd->outputs || !pd->output_bytes) {
                if (pd) { free(pd->inputs); free(pd->outputs); free(pd->output_bytes); }
                free(pd);
                hapgpu_rt_sync(rt);
                for (k = 0; k < live; k++)
                    results[live_index[k]] = HapResult_Internal_Error;
                free(live_index); free(stage_off_in); free(stage_off_out);
                return HapResult_Internal_Error;
            }
            memcpy(pd->inputs, inputs, sizeof(void *) * n_in);
            memcpy(pd->outputs, outputs, sizeof(void *) * frame_count);
            memcpy(pd->output_bytes, output_bytes, sizeof(unsigned long) * frame_count);
            for (i = 0; i < count; i++) {
                pd->input_bytes[i] = input_bytes[i];
                pd->formats[i] = formats[i];
                pd->compressors[i] = compressors[i];
                pd->chunk_counts[i] = chunk_counts[i];
            }
            pd->frame_count = frame_count;
            pd->count = count;
            pd->flags = flags;
            pd->inputs_are_device = inputs_are_device;
            pd->output_used = output_used;
            pd->results = results;
            pd->live = live;
            pd->placed = placed;
            pd->first_error = first_error;
            pd->launch_rc = rc;
            pd->live_index = live_index;
            pd->stage_off_out = stage_off_out;
            pd->hframes = hframes;
            pd->out_stage = out_stage;
            if (job) {
                pd->job = *job;
                pd->has_job = 1;
                if (job->source.planes) {
                    /* (the caller's description need not outlive the first half either) */
                    pd->planes = *job->source.planes;
                    pd->planes.scale = pd->planes.bias = NULL;
                    pd->job.source.planes = &pd->planes;
                }
                if (job->source.video) {
                    /* (... nor need its array of CbCr planes: their addresses are in the job's table) */
                    pd->video = *job->source.video;
                    pd->video.chroma = NULL;
                    pd->job.source.video = &pd->video;
                }
            }
            free(stage_off_in);
            if (a->defer) {
                ctx->pending_encode = pd;
                return first_error;
            }
            return hapb_encode_complete(ctx, pd);
        }
    }
}

/* The second half of hapb_encode: waits for the launches, reads the per-frame results back, copies staged frames to the
   client's host buffers, and encodes the frames that were not placed once more.  Frees `pd`. */
unsigned hapb_encode_complete(HapGpuContext *ctx, HapbEncodePending *pd)
{
    hapgpu_rt *rt = ctx->rt;
    const unsigned frame_count = pd->frame_count, count = pd->count, live = pd->live, flags = pd->flags;
    unsigned *const results = pd->results;
    unsigned long *const output_used = pd->output_used;
    unsigned first_error = pd->first_error, rc = pd->launch_rc, f, i, k;
    rc |= (unsigned)hapgpu_rt_sync(rt);
    if (rc) {
        for (k = 0; k < live; k++)
            results[pd->live_index[k]] = HapResult_Internal_Error;
        first_error = HapResult_Internal_Error;
        goto done;
    }
    /* results (+ device->host copy of staged frames) */
    {
        int copied = 0;
        for (k = 0; k < live; k++) {
            HapGpuFrameEnc *fe = &pd->hframes[k];
            f = pd->live_index[k];
            results[f] = fe->status;
            if (fe->status == HAPGPU_STATUS_NOT_PLACED && (fe->reserved & 1u)) {
                /* a wavefront gave up waiting for its predecessors (snappy_compress_blocks.hip): something keeps the
                   grid from advancing in order -- this context gathers from now on */
                ctx->placement_timeouts += 1u;
                if (!ctx->placing_off)
                    fprintf(stderr, "hap_amd: a placed encode waited too long for its predecessors (another kernel, a profiler, CU "
                                    "masking?): this context gathers for its next 64 encode calls\n");
                ctx->placing_off = 64u;              /* calls that gather before placing is tried again */
            }
            if (fe->status == HapResult_No_Error) {
                output_used[f] = (unsigned long)fe->bytes_used;
                if (pd->stage_off_out[f]) {
                    if (hapgpu_rt_d2h(rt, pd->outputs[f], pd->out_stage + (pd->stage_off_out[f] - 1), (size_t)fe->bytes_used))
                        results[f] = HapResult_Internal_Error;
                    copied = 1;
                }
            }
            if (results[f] != HapResult_No_Error && results[f] != HAPGPU_STATUS_NOT_PLACED && first_error == HapResult_No_Error)
                first_error = results[f];
        }
        if (copied && hapgpu_rt_sync(rt))
            first_error = HapResult_Internal_Error;
    }
    /* frames with a chunk that Snappy did not shrink (stored raw, hap.c:460-466: everything behind it lies elsewhere
       than the wavefronts assumed): once more, through slots.  The textures are where they were -- the client's --
       or, in a call that started from pictures, are made again from the pictures: the fused kernel of a placed call
       does not keep them (snappy_compress_blocks.hip). */
    if (pd->placed) {
        unsigned again = 0;
        for (f = 0; f < frame_count; f++)
            again += results[f] == HAPGPU_STATUS_NOT_PLACED;
        if (again) {
            /* all of them in one batch */
            /* (results before it returns, and through slots: such a call cannot report a frame as not placed) */
            HapbEncodeArgs again_args = {pd->inputs_are_device, NULL, 0, 1};
            HapbBlockEncodeJob rjob;
            uint64_t *rtable = NULL;
            const void **rin = (const void **)malloc(sizeof(void *) * (size_t)again * count);
            void **rout = (void **)malloc(sizeof(void *) * again);
            unsigned long *rcap = (unsigned long *)malloc(sizeof(unsigned long) * again * 2u);
            unsigned *rres = (unsigned *)malloc(sizeof(unsigned) * again * 2u);
            if (pd->has_job)
                rtable = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)job_table_columns(&pd->job) * again);
            if (rin && rout && rcap && rres && (!pd->has_job || rtable)) {
                unsigned long *rused = rcap + again;
                unsigned *rmap = rres + again, m = 0;
                for (f = 0; f < frame_count; f++)
                    if (results[f] == HAPGPU_STATUS_NOT_PLACED) {
                        for (i = 0; i < count; i++)
                            rin[(size_t)m * count + i] = pd->inputs[(size_t)f * count + i];
                        rout[m] = pd->outputs[f];
                        rcap[m] = pd->output_bytes[f];
                        rres[m] = HapResult_Internal_Error;
                        rused[m] = 0;
                        if (pd->has_job) {
                            /* the pictures and texture places of these frames, as a table of its own */
                            unsigned t;
                            for (t = 0; t < job_table_columns(&pd->job); t++)
                                rtable[(size_t)t * again + m] = pd->job.host_table[(size_t)t * pd->job.frame_count + f];
                        }
                        rmap[m++] = f;
                    }
                if (pd->has_job) {
                    /* the table goes where the first pass's was: pinned memory at an address that stays -- a recorded
                       launch sequence (HAP_AMD_GRAPHS) copies from THAT address again when it is replayed (found by
                       tools/stress.py: a table in malloc'd memory was gone by then) */
                    uint64_t *pinned = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, sizeof(uint64_t) * (size_t)job_table_columns(&pd->job) * again);
                    rjob = pd->job;
                    rjob.frame_count = again;
                    if (pinned) {
                        memcpy(pinned, rtable, sizeof(uint64_t) * (size_t)job_table_columns(&pd->job) * again);
                        rjob.host_table = pinned;
                    } else {
                        rjob.host_table = rtable;
                    }
                    again_args.job = &rjob;
                }
                hapb_encode(ctx, again, count, rin, pd->input_bytes, pd->formats, pd->compressors, pd->chunk_counts, rout, rcap, rused, rres,
                            flags, &again_args);
                for (m = 0; m < again; m++) {
                    results[rmap[m]] = rres[m] == HAPGPU_STATUS_NOT_PLACED ? HapResult_Internal_Error : rres[m];
                    output_used[rmap[m]] = rused[m];
                }
            } else {
                for (f = 0; f < frame_count; f++)
                    if (results[f] == HAPGPU_STATUS_NOT_PLACED)
                        results[f] = HapResult_Internal_Error;
            }
            free(rin); free(rout); free(rcap); free(rres); free(rtable);
            ctx->placement_retries += again;
            for (f = 0; f < frame_count; f++)
                if (results[f] != HapResult_No_Error && first_error == HapResult_No_Error)
                    first_error = results[f];
            /* content that does not shrink tends to stay: a call that had to encode most of its frames twice
               keeps the next calls from trying (and then tries again) */
            if (2u * again > live)
                ctx->placing_holdoff = ctx->placing_holdoff_calls;
        }
    }
done:
    free(pd->live_index); free(pd->stage_off_out);
    free(pd->inputs); free(pd->outputs); free(pd->output_bytes);
    free(pd);
    return first_error;
}

void hapb_encode_abandon(HapGpuContext *ctx, HapbEncodePending *pd)
{
    (void)hapgpu_rt_sync(ctx->rt);
    free(pd->live_index); free(pd->stage_off_out);
    free(pd->inputs); free(pd->outputs); free(pd->output_bytes);
    free(pd);
}

/* The size of a texel belongs to the pictures (HAPGPU_PICTURE_TEXEL_BYTES of their kind), not to the texture format:
   RGTC1 is made from RGBA8 pictures and from A8 ones.  What a format does fix is which pictures may hold it. */
static int is_bc6h(unsigned format)
{
    return format == HapTextureFormat_RGB_BPTC_UNSIGNED_FLOAT || format == HapTextureFormat_RGB_BPTC_SIGNED_FLOAT;
}

/* pictures of `kind` make `format` (bptc: the caller asked for BC7 from RGBA8): RGBA16F makes BC6H and nothing else
   does, A8 makes RGTC1 */
static int kind_makes_format(unsigned kind, unsigned format, int bptc)
{
    if (kind == HAPGPU_PICTURE_RGBA16F)
        return is_bc6h(format);
    if (kind == HAPGPU_PICTURE_A8)
        return format == HapTextureFormat_A_RGTC1;
    return format == HapTextureFormat_RGB_DXT1 || format == HapTextureFormat_RGBA_DXT5 ||
           format == HapTextureFormat_YCoCg_DXT5 || format == HapTextureFormat_A_RGTC1 || bptc;
}

/* the size of an element of a planar tensor */
static size_t plane_element_bytes(unsigned element)
{
    return element == HapGpuPlaneElement_F32 ? 4u : 2u;
}

int hapb_planes_encode_valid(unsigned width, unsigned height, unsigned long row_bytes, const HapbPlanes *planes,
                             unsigned count, const unsigned *formats)
{
    size_t e, unit;
    if (!planes->scale || !planes->bias || planes->channels < 3u || planes->channels > 4u ||
        planes->element > HapGpuPlaneElement_F32 || width == 0 || height == 0 || (width & 3u) || (height & 3u) ||
        height / 4u > 65535u || !formats)
        return 0;
    /* what a lane loads per row: the tensors' pitches are multiples of it */
    e = plane_element_bytes(planes->element);
    unit = 4u * e;
    if (row_bytes < (unsigned long)width * e || row_bytes % unit || planes->plane_bytes % unit ||
        planes->plane_bytes / row_bytes < height - 1u ||
        planes->plane_bytes < row_bytes * (unsigned long)(height - 1u) + (unsigned long)width * e)
        return 0;
    if (count == 2u)
        return formats[0] == HapTextureFormat_YCoCg_DXT5 && formats[1] == HapTextureFormat_A_RGTC1;
    return count == 1u && kind_makes_format(HAPGPU_PICTURE_RGBA8, formats[0], 0);
}

int hapb_video_encode_valid(unsigned width, unsigned height, unsigned long row_bytes, const HapbVideo *video,
                            unsigned count, const unsigned *formats)
{
    if (video->matrix > HapGpuYCbCrMatrix_BT709 || video->range > HapGpuYCbCrRange_Full || width == 0 || height == 0 ||
        (width & 3u) || (height & 3u) || height / 4u > 65535u || !formats)
        return 0;
    /* a lane loads a dword per row of either plane; width / 2 pairs are width bytes */
    if (row_bytes < width || (row_bytes & 3u) || video->chroma_row_bytes < width || (video->chroma_row_bytes & 3u))
        return 0;
    /* opaque pictures: Hap and Hap Q */
    return count == 1u && (formats[0] == HapTextureFormat_RGB_DXT1 || formats[0] == HapTextureFormat_YCoCg_DXT5);
}

/* the size of a source's texel: of a tensor, one element of one plane; of a video picture, one Y sample */
static size_t source_texel_bytes(const HapbSource *source)
{
    if (source->video)
        return 1u;
    return source->planes ? plane_element_bytes(source->planes->element) : HAPGPU_PICTURE_TEXEL_BYTES(source->picture_kind);
}

/* what the kernels ask of a source's address (in device memory) and row pitch when they read it: tensors four
   elements, RGBA16F pictures 16 bytes, else 4 (video pictures: of both planes) */
static unsigned source_align_mask(const HapbSource *source)
{
    if (source->video)
        return 3u;
    if (source->planes)
        return 4u * (unsigned)plane_element_bytes(source->planes->element) - 1u;
    return source->picture_kind == HAPGPU_PICTURE_RGBA16F ? 15u : 3u;
}

/* the whole-call answer: every result set (a NULL results: none), `code` returned */
static unsigned answer_all(unsigned *results, unsigned frame_count, unsigned code)
{
    unsigned f;
    for (f = 0; results && f < frame_count; f++)
        results[f] = code;
    return code;
}

unsigned hapb_source_texture(HapGpuContext *ctx, const HapbSource *source, const void *picture, unsigned format,
                             void *output, unsigned long output_bytes, unsigned long *used, unsigned flags)
{
    const HapbPlanes *const planes = source->planes;
    const HapbVideo *const video = source->video;
    const void *const chroma = video && video->chroma ? video->chroma[0] : NULL;
    const unsigned kind = source->picture_kind, width = source->width, height = source->height;
    const unsigned long row_bytes = source->row_bytes;
    /* BC7 only when asked (HAPGPU_ENCODE_BPTC_BLOCKS); BC6H only from half pictures, and nothing else from those; A8
       pictures make RGTC1 */
    const int bptc = !planes && !video && (flags & HAPGPU_ENCODE_BPTC_BLOCKS) && format == HapTextureFormat_RGBA_BPTC_UNORM;
    const int grid_rows = bptc || kind != HAPGPU_PICTURE_RGBA8;    /* a block row per grid row */
    const size_t texel = source_texel_bytes(source), block = hapf_block_bytes(format);
    const unsigned align = source_align_mask(source);
    hapgpu_rt *rt = ctx->rt;
    HapGpuPictureTable t = {{NULL, NULL, NULL}, {0u, 0u, 0u}};
    size_t need;
    const void *src = picture;
    void *dst = output;
    int rc;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    if (!picture || !output || (video && !chroma) ||
        (video  ? !hapb_video_encode_valid(width, height, row_bytes, video, 1u, &format) :
         planes ? !hapb_planes_encode_valid(width, height, row_bytes, planes, 1u, &format)
                : width == 0 || height == 0 || (width & 3u) || (height & 3u) || row_bytes < (unsigned long)width * texel ||
                  !kind_makes_format(kind, format, bptc)))
        return HapResult_Bad_Arguments;
    need = (size_t)(width / 4u) * (height / 4u) * block;
    if (output_bytes < need)
        return HapResult_Buffer_Too_Small;
    /* tensors and both planes of a video picture in device memory, aligned to what a lane loads; device pictures 4-byte
       aligned with rows a multiple of 4 (half pictures: 16 and 16), at most 65535 block rows for BC7, BC6H and A8
       pictures, 2^32 * 255/256 blocks for the others; device outputs aligned to their blocks */
    if ((video  ? !is_dev(ctx, picture) || !is_dev(ctx, chroma) || (((uintptr_t)picture | (uintptr_t)chroma) & align) :
         planes ? !is_dev(ctx, picture) || ((uintptr_t)picture & align)
                : (row_bytes & align) || (is_dev(ctx, picture) && ((uintptr_t)picture & align)) ||
                  (grid_rows ? height / 4u > 65535u : (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)) ||
        (is_dev(ctx, output) && ((uintptr_t)output & (block - 1u))))
        return HapResult_Bad_Arguments;
    if (!is_dev(ctx, picture)) {
        const size_t picture_bytes = (size_t)row_bytes * (height - 1u) + (size_t)width * texel;
        void *s = hapgpu_rt_device_scratch(rt, D_RGBA_STAGE, picture_bytes);
        if (!s || hapgpu_rt_h2d(rt, s, picture, picture_bytes))
            return HapResult_Internal_Error;
        src = s;
    }
    if (!is_dev(ctx, output)) {
        dst = hapgpu_rt_device_scratch(rt, D_BC_TEX, need);
        if (!dst)
            return HapResult_Internal_Error;
    }
    t.one[0] = (uint64_t)(uintptr_t)src;
    t.one[1] = (uint64_t)(uintptr_t)dst;
    t.one[2] = (uint64_t)(uintptr_t)chroma;
    rc = video  ? hapgpu_k_block_encode_video(rt, &t, 1u, width, height, format, 0u, row_bytes, video->chroma_row_bytes,
                                              video->matrix, video->range) :
         planes ? hapgpu_k_block_encode_planes(rt, &t, 1u, width, height, format, 0u, planes->channels, planes->element,
                                               planes->plane_bytes, row_bytes, planes->scale, planes->bias)
                : hapgpu_k_block_encode(rt, &t, 1u, width, height, row_bytes, format,
                                        (flags & HAPGPU_ENCODE_REFINE_ENDPOINTS) ? HAPGPU_BLOCK_ENCODE_REFINE : 0u,
                                        (((uintptr_t)src | row_bytes) & 15u) == 0 && !(kind == HAPGPU_PICTURE_A8 && ctx->no_wide_planes),
                                        kind);
    if (rc == 1)
        return HapResult_Bad_Arguments;
    if (rc || (dst != output && hapgpu_rt_d2h(rt, output, dst, need)) || hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    if (used)
        *used = (unsigned long)need;
    return HapResult_No_Error;
}

/* one slice of hapb_source_frames: at most HAP_SLICE_ENTRIES frames, or a call that is refused as a whole.  A planar
   source has passed hapb_planes_encode_valid, a video source hapb_video_encode_valid, and its array of CbCr planes is
   there */
static unsigned source_slice(HapGpuContext *ctx, const HapbSource *source, unsigned frame_count,
                             const void *const *pictures, unsigned count, const unsigned *formats,
                             const unsigned *compressors, const unsigned *chunk_counts, void *const *outputs,
                             const unsigned long *output_bytes, unsigned long *output_used, unsigned *results,
                             unsigned flags, int defer)
{
    hapgpu_rt *rt = ctx->rt;
    const HapbPlanes *const planes = source->planes;
    const HapbVideo *const video = source->video;
    const unsigned picture_kind = source->picture_kind, width = source->width, height = source->height;
    const unsigned long row_bytes = source->row_bytes;
    const size_t texel = source_texel_bytes(source);
    const unsigned align = source_align_mask(source);
    unsigned long tex_bytes[2] = {0, 0};
    size_t per_frame = 0, rgba_bytes, tex_off[2] = {0, 0};
    unsigned i, f, rc;
    uint8_t *textures, *rgba_stage = NULL;
    const void **tex_ptrs;
    uint64_t *hsrc, *dsrc;
    int wide = !(picture_kind == HAPGPU_PICTURE_A8 && ctx->no_wide_planes);
    if (context_busy(ctx, results, frame_count))
        return HapResult_Internal_Error;
    if (!results || !pictures || count == 0 || count > 2 || !formats || width == 0 || height == 0 ||
        (width & 3u) || (height & 3u) || row_bytes < (unsigned long)width * texel ||
        (picture_kind != HAPGPU_PICTURE_RGBA8 && (row_bytes & align)) ||
        (picture_kind == HAPGPU_PICTURE_A8 && height / 4u > 65535u))
        return answer_all(results, frame_count, HapResult_Bad_Arguments);
    for (i = 0; i < count; i++) {
        /* (BC7 only when asked, and alone: no Hap variant pairs it with a second texture) */
        const int bptc = !planes && !video && (flags & HAPGPU_ENCODE_BPTC_BLOCKS) && count == 1u && formats[i] == HapTextureFormat_RGBA_BPTC_UNORM;
        /* (half pictures make BC6H, alone, and nothing else; RGBA8 pictures never make it; A8 pictures make RGTC1, alone) */
        if ((picture_kind != HAPGPU_PICTURE_RGBA8 && count != 1u) || !kind_makes_format(picture_kind, formats[i], bptc))
            return answer_all(results, frame_count, HapResult_Bad_Arguments);
        tex_bytes[i] = (unsigned long)((size_t)(width / 4u) * (height / 4u) * hapf_block_bytes(formats[i]));
        tex_off[i] = per_frame;
        per_frame += align_up(tex_bytes[i], 256);
    }
    rgba_bytes = (size_t)row_bytes * (height - 1u) + (size_t)width * texel;
    textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, per_frame * frame_count);
    tex_ptrs = (const void **)malloc(sizeof(void *) * (size_t)frame_count * count);
    /* address table of the batched block-encode launches: [sources][outputs of texture 0][of texture 1]; video pictures,
       one texture a frame: [Y planes][outputs][CbCr planes] */
    hsrc = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, sizeof(uint64_t) * 3u * frame_count);
    dsrc = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, sizeof(uint64_t) * 3u * frame_count);
    if (!textures || !tex_ptrs || !hsrc || !dsrc) {
        free(tex_ptrs);
        return answer_all(results, frame_count, HapResult_Internal_Error);
    }
    memset(hsrc, 0, sizeof(uint64_t) * 3u * frame_count);       /* address 0: the kernel skips the picture */
    for (f = 0; f < frame_count; f++) {
        const void *src = pictures[f];
        for (i = 0; i < count; i++)
            tex_ptrs[(size_t)f * count + i] = NULL;     /* NULL input => Bad_Arguments for that frame */
        if (!src)
            continue;
        /* (a tensor in host memory, or one the lanes' loads would be misaligned in: its frame is Bad_Arguments) */
        if (planes && (!is_dev(ctx, src) || ((uintptr_t)src & align)))
            continue;
        /* (... and so is a video picture either of whose planes is missing, in host memory or misaligned) */
        if (video) {
            const void *const chroma = video->chroma[f];
            if (!chroma || !is_dev(ctx, src) || !is_dev(ctx, chroma) || (((uintptr_t)src | (uintptr_t)chroma) & align))
                continue;
            hsrc[2u * (size_t)frame_count + f] = (uint64_t)(uintptr_t)chroma;
        }
        if (!is_dev(ctx, src)) {
            /* one staging buffer per frame so that uploads and kernels can overlap on the stream */
            if (!rgba_stage) {
                rgba_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_RGBA_STAGE, align_up(rgba_bytes, 256) * frame_count);
                if (!rgba_stage)
                    break;
            }
            if (hapgpu_rt_h2d(rt, rgba_stage + align_up(rgba_bytes, 256) * f, src, rgba_bytes))
                break;
            src = rgba_stage + align_up(rgba_bytes, 256) * f;
        }
        /* (a half picture in device memory is read 16 bytes at a time, an A8 one 4: misaligned, its frame is
           Bad_Arguments) */
        if (picture_kind != HAPGPU_PICTURE_RGBA8 && ((uintptr_t)src & align))
            continue;
        hsrc[f] = (uint64_t)(uintptr_t)src;
        if (((uintptr_t)src | row_bytes) & 15u)
            wide = 0;
        for (i = 0; i < count; i++) {
            uint8_t *t = textures + per_frame * f + tex_off[i];
            hsrc[(size_t)(1u + i) * frame_count + f] = (uint64_t)(uintptr_t)t;
            tex_ptrs[(size_t)f * count + i] = t;
        }
    }
    /* the block encode (one launch per texture format over the whole batch, addresses in a small device table) is
       issued by hapb_encode at the head of its own launches: one sequence per call */
    {
        HapbBlockEncodeJob job;
        const HapbEncodeArgs args = {rgba_stage ? 2 : 1, &job, defer, 0};
        memset(&job, 0, sizeof(job));
        job.host_table = hsrc;
        job.device_table = dsrc;
        job.frame_count = frame_count;
        job.count = count;
        job.source = *source;
        job.wide = wide;
        for (i = 0; i < count; i++)
            job.formats[i] = formats[i];
        for (i = 0; planes && i < planes->channels; i++) {
            job.plane_scale[i] = planes->scale[i];
            job.plane_bias[i] = planes->bias[i];
        }
        rc = hapb_encode(ctx, frame_count, count, tex_ptrs, tex_bytes, formats, compressors, chunk_counts, outputs,
                         output_bytes, output_used, results, flags, &args);
    }
    free(tex_ptrs);
    return rc;
}

unsigned hapb_source_frames(HapGpuContext *ctx, const HapbSource *source, unsigned frame_count,
                            const void *const *pictures, unsigned count, const unsigned *formats,
                            const unsigned *compressors, const unsigned *chunk_counts, void *const *outputs,
                            const unsigned long *output_bytes, unsigned long *output_used, unsigned *results,
                            unsigned flags, int defer)
{
    unsigned r = HapResult_No_Error, done;
    if (defer && frame_count > HAP_SLICE_ENTRIES)
        return HapResult_Bad_Arguments;
    if (frame_count == 0)
        return HapResult_No_Error;
    /* tensors: everything that does not depend on a frame, before any device is touched */
    if (source->planes &&
        (!results || !pictures || !compressors || !chunk_counts || !outputs || !output_bytes || !output_used ||
         !hapb_planes_encode_valid(source->width, source->height, source->row_bytes, source->planes, count, formats)))
        return answer_all(results, frame_count, HapResult_Bad_Arguments);
    /* video pictures: the same */
    if (source->video &&
        (!results || !pictures || !source->video->chroma || !compressors || !chunk_counts || !outputs || !output_bytes ||
         !output_used ||
         !hapb_video_encode_valid(source->width, source->height, source->row_bytes, source->video, count, formats)))
        return answer_all(results, frame_count, HapResult_Bad_Arguments);
    /* (the kernels index frames with a grid dimension that holds 65535: larger batches go in slices; a call without the
       arrays the slices would be cut from is refused in one piece) */
    if (frame_count <= HAP_SLICE_ENTRIES || !pictures || !outputs || !output_bytes || !output_used || !results)
        return source_slice(ctx, source, frame_count, pictures, count, formats, compressors, chunk_counts, outputs,
                            output_bytes, output_used, results, flags, defer);
    for (done = 0; done < frame_count; done += HAP_SLICE_ENTRIES) {
        const unsigned n = frame_count - done < HAP_SLICE_ENTRIES ? frame_count - done : HAP_SLICE_ENTRIES;
        /* (a slice's CbCr planes are cut from the call's like its pictures) */
        HapbVideo video;
        HapbSource cut = *source;
        unsigned rc;
        if (source->video) {
            video = *source->video;
            video.chroma += done;
            cut.video = &video;
        }
        rc = source_slice(ctx, &cut, n, pictures + done, count, formats, compressors, chunk_counts, outputs + done,
                          output_bytes + done, output_used + done, results + done, flags, 0);
        if (r == HapResult_No_Error)
            r = rc;
    }
    return r;
}

/* ================================================================== decode */

/* the block layout ("fields per block" code of the fragment table) a texture format's field streams have; 0: none */
static unsigned field_layout_of_format(unsigned format)
{
    switch (format) {
    case HapTextureFormat_RGBA_DXT5:
    case HapTextureFormat_YCoCg_DXT5: return 4u;
    case HapTextureFormat_RGB_DXT1: return 2u;
    case HapTextureFormat_A_RGTC1: return 6u;
    default: return 0u;
    }
}

typedef struct fetch_ctx {
    HapGpuContext *ctx;
    const uint8_t *device_frame;
} fetch_ctx;

static int fetch_from_device(void *user, uint64_t offset, uint64_t length, uint8_t *dst)
{
    fetch_ctx *fc = (fetch_ctx *)user;
    if (hapgpu_rt_d2h(fc->ctx->rt, dst, fc->device_frame + offset, (size_t)length))
        return 1;
    return hapgpu_rt_sync(fc->ctx->rt);
}

/* work function handed to the client's HapDecodeCallback: marks chunk `index` as requested */
typedef struct request_marks {
    unsigned count;
    volatile unsigned char *requested;
} request_marks;

static void mark_chunk(void *p, unsigned index)
{
    request_marks *m = (request_marks *)p;
    if (m && index < m->count)
        m->requested[index] = 1;
}

/* Unit slots to reserve behind a whole-stream unit for the block scan (snappy_decode.hip): one per 64 KiB of output.
   The output length is on the device (the stream's varint); bound it by the client's buffer and by the format's
   largest expansion (a 3-byte copy element produces 64 bytes).  Streams of one block need none. */
static void scan_entry(HapGpuScanChunk *e, unsigned unit, unsigned long src_len, unsigned long dst_cap, uint32_t *dbpos,
                       unsigned *seg_cursor, unsigned *word_cursor, unsigned seg_bytes, unsigned *fine_cursor);

static unsigned stream_scan_segments(unsigned long src_len, unsigned seg_bytes)
{
    return (unsigned)(((unsigned long long)src_len + 15u + seg_bytes - 1u) / seg_bytes);
}

static unsigned long long stream_output_bound(unsigned long src_len, unsigned long dst_cap)
{
    unsigned long long bound = (unsigned long long)src_len * 22u;
    return bound > dst_cap ? dst_cap : bound;
}

/* 64 KiB blocks (libsnappy's) */
static unsigned stream_coarse_slots(unsigned long src_len, unsigned long dst_cap)
{
    unsigned long long bound = stream_output_bound(src_len, dst_cap);
    if (bound <= 65536u)
        return 0u;
    bound = (bound + 65535u) / 65536u;
    return bound > 4096u ? 4096u : (unsigned)bound;
}

/* 8 KiB blocks (the fragments of this library's own table-less streams): none for streams that are not scanned, or
   too long to give every 8 KiB a slot */
static unsigned stream_fine_slots(unsigned long src_len, unsigned long dst_cap)
{
    unsigned long long bound = stream_output_bound(src_len, dst_cap);
    if (bound <= 65536u)
        return 0u;
    bound = (bound + HAPGPU_SCAN_FINE - 1u) / HAPGPU_SCAN_FINE;
    return bound > 32768u ? 0u : (unsigned)bound;
}

/* unit slots directly behind a whole-stream unit: one per 64 KiB block (the 8 KiB blocks' slots lie behind all the
   ordinary units of the call) */
static unsigned stream_block_slots(unsigned long src_len, unsigned long dst_cap)
{
    return stream_coarse_slots(src_len, dst_cap);
}

/* words of block positions a scanned stream needs: one per mark + the end */
static unsigned stream_mark_words(unsigned long src_len, unsigned long dst_cap)
{
    const unsigned coarse = stream_coarse_slots(src_len, dst_cap), fine = stream_fine_slots(src_len, dst_cap);
    return (fine > coarse ? fine : coarse) + 1u;
}

static void scan_entry(HapGpuScanChunk *e, unsigned unit, unsigned long src_len, unsigned long dst_cap, uint32_t *dbpos,
                       unsigned *seg_cursor, unsigned *word_cursor, unsigned seg_bytes, unsigned *fine_cursor)
{
    const unsigned coarse = stream_coarse_slots(src_len, dst_cap), fine = coarse ? stream_fine_slots(src_len, dst_cap) : 0u;
    memset(e, 0, sizeof(*e));
    e->unit = unit;
    e->seg_first = *seg_cursor;
    e->seg_count = stream_scan_segments(src_len, seg_bytes);
    e->seg_bytes = seg_bytes;
    e->slots = coarse;
    e->fine_slots = fine;              /* (its words of block positions; the unit slots come from the call's pool, on the device) */
    e->fine_unit_first = 0;
    e->bpos = (uint64_t)(uintptr_t)(dbpos + *word_cursor);
    *seg_cursor += e->seg_count;
    *word_cursor += stream_mark_words(src_len, dst_cap);
    *fine_cursor += fine;
}

unsigned hapb_decode(HapGpuContext *ctx, unsigned frame_count, const void *const *inputs,
                     const unsigned long *input_bytes, unsigned index, void *const *outputs,
                     const unsigned long *output_bytes, unsigned long *output_used,
                     unsigned *output_formats, unsigned *results, unsigned flags, const HapbDecodeArgs *args)
{
    static const HapbDecodeArgs no_args;
    const HapbDecodeArgs *const a = args ? args : &no_args;
    hapgpu_rt *rt = ctx->rt;
    hapf_texture_plan *plans;
    hapf_reader *readers;
    fetch_ctx *fetchers;
    unsigned f, live = 0, first_error = HapResult_No_Error, total_units = 0, total_chunks = 0;
    unsigned frag_log2_seen = 0, frag_kinds = 0, max_chunks = 0, max_stream_src = 0, guess_units = 0;
    unsigned char *guess_frame = NULL;                         /* frames whose chunks may be field-stream fragments without a table */
    int use_guess = 0, use_scan_guess = 0;
    uint8_t *dguess = NULL;
    int any_stream = 0, need_retry = 0;
    unsigned scan_chunks = 0, scan_segs = 0, scan_words = 0;   /* streams with BLOCK slots; their segments; bpos words */
    /* (r06 measured shorter segments for calls of few streams -- a wavefront of the scan's first kernel walks a segment's
       windows one after the other -- and found nothing: one reference-made 8K frame, walk + merge 56 + 80 us at 2 KiB,
       60 + 122 at 1 KiB, the whole scan 0.088 ms at 2 KiB and at 4 KiB) */
    const unsigned scan_seg_bytes = HAPGPU_SCAN_SEGMENT;
    unsigned fine_total = 0;                                   /* unit slots for the 8 KiB blocks of scanned streams */
    uint32_t *dwork = NULL;                                    /* [0]: count, then the fine units the scan listed */
    unsigned far_seen = 0;
    /* (a call for several textures of the same frames: HapGpuDecodeFrameTextures hands the per-entry indices over) */
    const unsigned *const entry_index = a->indices;
    /* (a region call: the rectangle the textures are wanted for -- units that hold none of its blocks are blanked on the
       device, hapgpu_k_skip_units; a texture's block size is its format's, known once the frame is planned) */
    const HapGpuRegion *const region = a->region;
    /* (... or a rectangle per entry, HapGpuDecodeFramesPlanesRegion: they travel behind the job table, a rectangle per
       job, and the skip looks up the one of a unit's job) */
    const HapGpuRegion *const entry_regions = a->regions;
    const int skipping = region || entry_regions;
    const int region_counted = !a->region_uncounted;
    uint32_t *hblock = NULL, *dblock = NULL;                   /* per job, behind the job tables: the texture's block size */
    HapGpuRegion *hregion = NULL, *dregion = NULL;             /* ... and behind those, per job: its rectangle (entry_regions) */
    const size_t job_bytes = sizeof(HapGpuDecodeJob) + sizeof(uint32_t) + sizeof(HapGpuRegion);
#define TEXTURE_INDEX(f) (entry_index ? entry_index[f] : index)
    const int block_scan = !(flags & HAPGPU_DECODE_NO_BLOCK_SCAN) && !ctx->no_block_scan;
    uint8_t *prefix = NULL, *in_stage = NULL, *out_stage = NULL;
    size_t in_stage_bytes = 0, out_stage_bytes = 0, prefix_bytes = PREFIX_BYTES;
    unsigned prefix_pass;
    size_t *in_off, *out_off;
    HapGpuDecodeJob *hjobs, *djobs;
    HapGpuChunkIn *hchunks, *dchunks;
    HapGpuDecodeUnit *dunits;
    HapGpuScanChunk *hscan = NULL, *dscan = NULL;
    HapGpuScanSegment *dsegs = NULL;
    uint32_t *dbpos = NULL;
    uint8_t *drecs = NULL, *djoins = NULL;
    unsigned *job_of_frame;
    unsigned char *in_dev = NULL, *out_dev = NULL;     /* pointer classification, done once per buffer */
    unsigned char *client_marks = NULL;                /* what the client's callback asked for (single-frame path) */
    unsigned client_marks_count = 0;
    int rc = 0;

#ifdef HAPB_TRACE
    double hapb_t0 = hapb_now_us();
#endif
    if (frame_count == 0)
        return HapResult_No_Error;
    if (!results)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, results, frame_count))
        return HapResult_Internal_Error;
    if (!inputs || !input_bytes || !outputs || !output_bytes || index > 1) {
        for (f = 0; f < frame_count; f++)
            results[f] = HapResult_Bad_Arguments;
        return HapResult_Bad_Arguments;
    }
    plans = (hapf_texture_plan *)calloc(frame_count, sizeof(*plans));
    readers = (hapf_reader *)calloc(frame_count, sizeof(*readers));
    fetchers = (fetch_ctx *)calloc(frame_count, sizeof(*fetchers));
    in_off = (size_t *)calloc(frame_count, sizeof(size_t));
    out_off = (size_t *)calloc(frame_count, sizeof(size_t));
    job_of_frame = (unsigned *)calloc(frame_count, sizeof(unsigned));
    in_dev = (unsigned char *)calloc(frame_count, 1);
    out_dev = (unsigned char *)calloc(frame_count, 1);
    guess_frame = (unsigned char *)calloc(frame_count, 1);
    if (!plans || !readers || !fetchers || !in_off || !out_off || !job_of_frame || !in_dev || !out_dev || !guess_frame) {
        rc = 1;
        goto fail_alloc;
    }

    /* 1. make the container headers host-visible: device frames get a prefix copied back */
    {
        unsigned device_frames = 0;
        for (f = 0; f < frame_count; f++) {
            results[f] = HapResult_No_Error;
            if (!inputs[f] || !outputs[f]) {
                results[f] = HapResult_Bad_Arguments;
                continue;
            }
            in_dev[f] = (unsigned char)is_dev(ctx, inputs[f]);
            out_dev[f] = (unsigned char)is_dev(ctx, outputs[f]);
            if (in_dev[f])
                device_frames++;
        }
        /* (a second pass with a longer prefix when the tables of some frame do not fit the first one -- frames of
           thousands of chunks, HAPGPU_ENCODE_FINE_CHUNKS: one more round trip for the whole batch instead of a fetch
           on demand per frame and table) */
        for (prefix_pass = 0; prefix_pass < 2u; prefix_pass++) {
            size_t need_max = 0;
            if (device_frames && prefix_pass == 1u) {
                /* the longer prefix is a convenience, never a reason to fail the batch: if its scratch cannot
                   be had, the call goes on with the short prefixes it already holds the sizes for, and tables beyond them
                   are fetched on demand, frame by frame */
                const size_t block = (size_t)prefix_bytes * frame_count;
                if (!hapgpu_rt_device_scratch(rt, D_PREFIX, 2u * block + sizeof(uint64_t) * frame_count) ||
                    !hapgpu_rt_pinned_scratch(rt, P_PREFIX, 2u * block + sizeof(uint64_t) * frame_count))
                    prefix_bytes = PREFIX_BYTES;
            }
            if (device_frames) {
                /* one gather kernel + one copy bring every device frame's header prefix to the host -- and, for a later
                   texture of a multi-texture frame (which begins where the first one ends, far beyond the prefix), the
                   bytes at its section too: the kernel reads the two section headers in front of it itself.
                   Device block: prefixes | second prefixes | their offsets;  upload: pointers | lengths | wanted flags */
                const size_t up_bytes = sizeof(uint64_t) * 2u * frame_count + frame_count;
                const size_t block = (size_t)prefix_bytes * frame_count;
                uint64_t *hptr = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_PTRS, up_bytes);
                uint64_t *dptr = (uint64_t *)hapgpu_rt_device_scratch(rt, D_PTRS, up_bytes);
                uint8_t *dprefix = (uint8_t *)hapgpu_rt_device_scratch(rt, D_PREFIX, 2u * block + sizeof(uint64_t) * frame_count);
                unsigned far = 0;
                prefix = (uint8_t *)hapgpu_rt_pinned_scratch(rt, P_PREFIX, 2u * block + sizeof(uint64_t) * frame_count);
                if (!prefix || !hptr || !dptr || !dprefix) {
                    rc = 1;
                    goto fail_alloc;
                }
                for (f = 0; f < frame_count; f++) {
                    const int dev_frame = results[f] == HapResult_No_Error && in_dev[f];
                    hptr[f] = dev_frame ? (uint64_t)(uintptr_t)inputs[f] : 0u;
                    hptr[frame_count + f] = input_bytes[f];
                    ((uint8_t *)(hptr + 2u * frame_count))[f] = (uint8_t)(dev_frame && TEXTURE_INDEX(f) > 0);
                    far += dev_frame && TEXTURE_INDEX(f) > 0;
                }
                if (hapgpu_rt_pinned_is_mapped(rt)) {
                    /* the kernel reads the pointers from, and writes the prefixes to, the pinned buffers themselves: one
                       launch instead of a copy up, a launch and a copy back */
                    if (far)
                        rc |= hapgpu_k_gather_prefixes_far(rt, hptr, hptr + frame_count, frame_count, prefix_bytes, prefix,
                                                           (const uint8_t *)(hptr + 2u * frame_count), prefix + block,
                                                           (uint64_t *)(prefix + 2u * block));
                    else
                        rc |= hapgpu_k_gather_prefixes(rt, hptr, hptr + frame_count, frame_count, prefix_bytes, prefix);
                } else {
                    rc |= hapgpu_rt_h2d(rt, dptr, hptr, up_bytes);
                    if (far) {
                        rc |= hapgpu_k_gather_prefixes_far(rt, dptr, dptr + frame_count, frame_count, prefix_bytes, dprefix,
                                                           (const uint8_t *)(dptr + 2u * frame_count), dprefix + block,
                                                           (uint64_t *)(dprefix + 2u * block));
                        rc |= hapgpu_rt_d2h(rt, prefix, dprefix, 2u * block + sizeof(uint64_t) * frame_count);
                    } else {
                        rc |= hapgpu_k_gather_prefixes(rt, dptr, dptr + frame_count, frame_count, prefix_bytes, dprefix);
                        rc |= hapgpu_rt_d2h(rt, prefix, dprefix, block);
                    }
                }
                far_seen = far;
            }
            for (f = 0; f < frame_count; f++) {
                if (results[f] != HapResult_No_Error)
                    continue;
                if (in_dev[f]) {
                    size_t n = input_bytes[f] < prefix_bytes ? input_bytes[f] : prefix_bytes;
                    hapf_reader_init_host(&readers[f], prefix + (size_t)prefix_bytes * f, n);
                    fetchers[f].ctx = ctx;
                    fetchers[f].device_frame = (const uint8_t *)inputs[f];
                    readers[f].fetch = fetch_from_device;
                    readers[f].user = &fetchers[f];
                    readers[f].total_len = input_bytes[f];
                } else {
                    hapf_reader_init_host(&readers[f], inputs[f], input_bytes[f]);
                    in_off[f] = in_stage_bytes + 1;
                    in_stage_bytes += align_up(input_bytes[f], 256);
                }
            }
            if (device_frames)
                rc |= hapgpu_rt_sync(rt);
            if (rc)
                goto fail_alloc;
            if (far_seen) {
                /* the second prefix is a second window of the reader -- taken only where the host, reading the same two
                   section headers, arrives at the offset the kernel reported (anything else: the reader fetches on demand) */
                const size_t block = (size_t)prefix_bytes * frame_count;
                const uint64_t *far_at = (const uint64_t *)(prefix + 2u * block);
                for (f = 0; f < frame_count; f++) {
                    hapf_section top, first;
                    uint64_t at;
                    if (results[f] != HapResult_No_Error || !in_dev[f] || TEXTURE_INDEX(f) == 0 || readers[f].view_len < 16u)
                        continue;
                    if (hapf_read_section(readers[f].view, (uint32_t)input_bytes[f], &top) != HapResult_No_Error ||
                        top.type != 0x0Du || top.header_len + 8u > readers[f].view_len ||
                        hapf_read_section(readers[f].view + top.header_len, top.length, &first) != HapResult_No_Error)
                        continue;                                  /* (the planner reports what is wrong with it) */
                    at = (uint64_t)top.header_len + first.header_len + first.length;
                    if (at + 16u <= readers[f].view_len || at >= input_bytes[f] || far_at[f] != at)
                        continue;
                    readers[f].view2_off = at;
                    readers[f].view2 = prefix + block + (size_t)prefix_bytes * f;
                    readers[f].view2_len = input_bytes[f] - at < prefix_bytes ? input_bytes[f] - at : prefix_bytes;
                }
            }

            if (!device_frames || prefix_pass == 1u)
                break;
            for (f = 0; f < frame_count; f++) {
                /* how far the tables of the texture asked for reach: [outer header] section header, instructions header +
                   length (sections: hap.c:137-212) */
                const uint8_t *v;
                size_t have, at = 0;
                hapf_section sec, ins;
                if (results[f] != HapResult_No_Error || !in_dev[f])
                    continue;
                v = readers[f].view;
                have = readers[f].view_len;
                if (TEXTURE_INDEX(f) > 0) {
                    if (!readers[f].view2)
                        continue;
                    v = readers[f].view2;
                    have = readers[f].view2_len;
                } else if (have >= 8u && v[3] == HAP_SECTION_MULTI) {
                    at = (v[0] | v[1] | v[2]) ? 4u : 8u;
                }
                if (have < at + 16u || hapf_read_section(v + at, 0xFFFFFFFFu, &sec) != HapResult_No_Error || (sec.type >> 4) != HAP_NIBBLE_COMPLEX ||
                    hapf_read_section(v + at + sec.header_len, 0xFFFFFFFFu, &ins) != HapResult_No_Error || ins.type != HAP_SECTION_INSTRUCTIONS)
                    continue;
                /* the tables the HOST reads: compressors, sizes, offsets (hap.c:84-88).  The private section's contents
                   are the kernels' business -- an 8K frame's is 800 KB -- only its header is looked at */
                {
                    const size_t ins_at = at + sec.header_len + ins.header_len, ins_end = ins_at + ins.length;
                    size_t q = ins_at, need = 0;
                    unsigned chunks_seen = 0;
                    while (q + 8u <= ins_end) {
                        hapf_section in;
                        if (q + 8u > have) {
                            /* a table header beyond the prefix: behind a compressor table of n entries come 4 n bytes of sizes
                               and perhaps 4 n of offsets */
                            need = q + 16u + 8u * (size_t)chunks_seen + 16u;
                            break;
                        }
                        if (hapf_read_section(v + q, 0xFFFFFFFFu, &in) != HapResult_No_Error)
                            break;
                        if (in.type == HAP_SECTION_COMPRESSORS || in.type == HAP_SECTION_SIZES || in.type == HAP_SECTION_OFFSETS) {
                            if (in.type == HAP_SECTION_COMPRESSORS)
                                chunks_seen = in.length;
                            if (q + in.header_len + in.length > need)
                                need = q + in.header_len + in.length;
                        }
                        q += (size_t)in.header_len + in.length;
                    }
                    if (need > ins_end)
                        need = ins_end;
                    /* (a table that claims to run past the end of its frame is a Bad_Frame for the planner; it does not
                       get to size anybody's scratch) */
                    if (need > input_bytes[f])
                        need = input_bytes[f];
                    if (need > have && need > need_max)
                        need_max = need;
                }
            }
            /* (bounded per frame AND for the batch: one frame's claim decides the prefix of all of them) */
            if (need_max <= prefix_bytes || need_max > ((size_t)4u << 20) ||
                align_up(need_max, 256) * (size_t)frame_count > PREFIX_BATCH_MAX_BYTES)
                break;
            prefix_bytes = align_up(need_max, 256);
            for (f = 0; f < frame_count; f++)
                hapf_reader_free(&readers[f]);
            memset(readers, 0, sizeof(*readers) * frame_count);
            in_stage_bytes = 0;
            memset(in_off, 0, sizeof(size_t) * frame_count);
        }
    }

    HAPB_MARK("prefixes");
    /* 2. plan on the host: sections and tables only (hap_frame.c) */
    for (f = 0; f < frame_count; f++) {
        hapf_texture_plan *p = &plans[f];
        int c;
        if (results[f] != HapResult_No_Error)
            continue;
        hapf_plan_texture(&readers[f], (uint32_t)input_bytes[f], TEXTURE_INDEX(f), 1, p);
        if (output_formats && p->format)
            output_formats[f] = p->format;
        if (p->result != HapResult_No_Error) {
            results[f] = p->result;
            continue;
        }
        if (flags & HAPGPU_DECODE_IGNORE_FRAGMENT_INDEX)
            p->frag_table_offset = 0;
        if (p->mode == HAPGPU_JOB_COMPLEX &&
            !(p->frag_table_offset && p->chunk_count > 0 && p->frag_entries >= (unsigned)p->chunk_count &&
              p->frag_entries % (unsigned)p->chunk_count == 0))
            p->frag_table_offset = 0;
        /* no table, but every chunk as short as one fragment (HAPGPU_ENCODE_FINE_CHUNKS): candidates for the
           block-per-lane decoder, whose starting points a pre-pass can find (snappy_decode_fields.hip) */
        if (p->mode == HAPGPU_JOB_COMPLEX && !p->frag_table_offset && !(flags & HAPGPU_DECODE_NO_FIELD_GUESS) &&
            field_layout_of_format(p->format) && p->chunk_count > 1) {
            unsigned snappy_chunks = 0;
            int fits = 1;
            for (c = 0; c < p->chunk_count; c++) {
                const HapGpuChunkIn *ch = &p->chunks[c];
                if ((ch->codec & 0xFFu) != HAP_NIBBLE_SNAPPY)
                    continue;
                snappy_chunks++;
                if (ch->src_len > HAPGPU_SLOT_DATA_BYTES + 64u + 5u)
                    fits = 0;
            }
            if (fits && snappy_chunks) {
                guess_frame[f] = 1;
                guess_units += snappy_chunks;
            }
        }
    }
    /* (a lane per fragment finds the starting points: worth it from a few thousand fragments on -- one frame's are
       decoded sooner by the generic kernel, a wavefront each) */
    use_guess = guess_units && (guess_units >= 4096u || (flags & HAPGPU_DECODE_GUESS_FIELDS));
    for (f = 0; f < frame_count; f++) {
        hapf_texture_plan *p = &plans[f];
        unsigned units = 0;
        int c;
        /* (the chunks of a frame on that road are not looked over for 64 KiB blocks: one unit each) */
        const int frame_scan = block_scan && !(use_guess && (guess_frame[f] & 1));
        if (results[f] != HapResult_No_Error)
            continue;
        if (p->mode == HAPGPU_JOB_COMPLEX) {
            unsigned per_chunk = 0;
            if (p->frag_table_offset)
                per_chunk = p->frag_entries / (unsigned)p->chunk_count;
            for (c = 0; c < p->chunk_count; c++) {
                HapGpuChunkIn *ch = &p->chunks[c];
                unsigned codec = ch->codec & 0xFFu;
                ch->unit_first = units;
                ch->frag_first = per_chunk * (unsigned)c;
                if (codec == HAP_NIBBLE_SNAPPY)
                    ch->unit_count = per_chunk ? per_chunk
                                               : 1u + (frame_scan ? stream_block_slots(ch->src_len, output_bytes[f]) : 0u);
                else if (codec == HAP_NIBBLE_NONE)
                    ch->unit_count = ch->src_len ? (ch->src_len + COPY_PIECE - 1) / COPY_PIECE : 1u;
                else
                    ch->unit_count = 1u;
                units += ch->unit_count;
                if (codec == HAP_NIBBLE_SNAPPY && !per_chunk) {
                    any_stream = 1;
                    if (ch->src_len > max_stream_src)
                        max_stream_src = ch->src_len;
                }
                if (codec == HAP_NIBBLE_NONE)
                    any_stream = 1;
            }
            if (per_chunk) {
                if (frag_log2_seen && frag_log2_seen != p->frag_log2) {
                    /* one fragment size per launch: later frames fall back to whole-stream units */
                    p->frag_table_offset = 0;
                    units = 0;
                    for (c = 0; c < p->chunk_count; c++) {
                        HapGpuChunkIn *ch = &p->chunks[c];
                        if ((ch->codec & 0xFFu) == HAP_NIBBLE_SNAPPY)
                            ch->unit_count = 1u + (frame_scan ? stream_block_slots(ch->src_len, output_bytes[f]) : 0u);
                        ch->unit_first = units;
                        units += ch->unit_count;
                    }
                    any_stream = 1;
                    max_stream_src = 0xFFFFFFFFu;
                } else {
                    frag_log2_seen = p->frag_log2;
                }
            }
            if (!p->frag_table_offset) {
                /* the 8 KiB blocks of all the frame's streams together: what each could expand to, but no more than the
                   texture holds (+ a ragged last block per stream) -- the slots are handed out on the device */
                unsigned long long fine_sum = 0, streams = 0;
                for (c = 0; c < p->chunk_count; c++)
                    if ((p->chunks[c].codec & 0xFFu) == HAP_NIBBLE_SNAPPY && p->chunks[c].unit_count > 1u) {
                        guess_frame[f] |= 2;
                        scan_chunks += 1u;
                        scan_segs += stream_scan_segments(p->chunks[c].src_len, scan_seg_bytes);
                        scan_words += stream_mark_words(p->chunks[c].src_len, output_bytes[f]);
                        fine_sum += stream_fine_slots(p->chunks[c].src_len, output_bytes[f]);
                        streams += 1u;
                    }
                if (fine_sum > output_bytes[f] / HAPGPU_SCAN_FINE + streams)
                    fine_sum = output_bytes[f] / HAPGPU_SCAN_FINE + streams;
                fine_total += (unsigned)fine_sum;
            }
            total_chunks += (unsigned)p->chunk_count;
            if ((unsigned)p->chunk_count > max_chunks)
                max_chunks = (unsigned)p->chunk_count;
        } else if (p->mode == HAPGPU_JOB_RAW) {
            units = p->section_length ? (p->section_length + COPY_PIECE - 1) / COPY_PIECE : 1u;
            any_stream = 1;
        } else {
            if (p->section_length > max_stream_src)
                max_stream_src = p->section_length;
            units = 1u + (block_scan ? stream_block_slots(p->section_length, output_bytes[f]) : 0u);
            if (units > 1u) {
                guess_frame[f] |= 2;
                scan_chunks += 1u;
                scan_segs += stream_scan_segments(p->section_length, scan_seg_bytes);
                scan_words += stream_mark_words(p->section_length, output_bytes[f]);
                fine_total += stream_fine_slots(p->section_length, output_bytes[f]);
            }
            any_stream = 1;
        }
        job_of_frame[f] = live++;
        total_units += units;
        p->frag_entries = p->frag_table_offset ? p->frag_entries : 0;
        p->unit_count = units;
        if (!out_dev[f]) {
            out_off[f] = out_stage_bytes + 1;
            out_stage_bytes += align_up(output_bytes[f], 256);
        }
    }
    if (live == 0)
        goto finish;
    /* streams without a table that the block scan cuts into 8 KiB pieces (plain hap.h frames of this library: one or a
       few chunks of many fragments): the starting points inside every piece the scan lists can be had from the scan's own
       records (r06: a wavefront per piece looks up the windows that hold every ceil(N / 64)-th element and walks a dozen
       elements each; until r05 a lane per piece walked its ~400 elements twice: 1.95 ms per 60 8K frames, 0.87 now), and
       the block-per-lane decoder then takes the pieces that are field-stream fragments; the others (another encoder's)
       stay with the generic kernel.  Calls, plain 8K frames: 1 frame 0.435 ms against 0.412 through the generic kernel
       alone, 8 frames 0.84 against 1.09, 60 frames 4.03 against 6.30 (r05, lane per piece: 4.98): from two frames' pieces on. */
    use_scan_guess = fine_total && !(flags & HAPGPU_DECODE_NO_FIELD_GUESS);

    /* 3. device descriptors */
    hjobs = (HapGpuDecodeJob *)hapgpu_rt_pinned_scratch(rt, P_JOBS, job_bytes * live);
    hchunks = (HapGpuChunkIn *)hapgpu_rt_pinned_scratch(rt, P_CHUNKS, sizeof(HapGpuChunkIn) * (total_chunks + 1u));
    djobs = (HapGpuDecodeJob *)hapgpu_rt_device_scratch(rt, D_JOBS, job_bytes * live);
    dchunks = (HapGpuChunkIn *)hapgpu_rt_device_scratch(rt, D_CHUNKS, sizeof(HapGpuChunkIn) * (total_chunks + 1u));
    /* (the fine block units of the block scan live behind the ordinary ones: [total_units, total_units + fine_total)) */
    dunits = (HapGpuDecodeUnit *)hapgpu_rt_device_scratch(rt, D_UNITS, sizeof(HapGpuDecodeUnit) * ((size_t)total_units + fine_total + 1u));
    if (in_stage_bytes)
        in_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_IN_STAGE, in_stage_bytes);
    if (out_stage_bytes)
        out_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_OUT_STAGE, out_stage_bytes);
    if (!hjobs || !hchunks || !djobs || !dchunks || !dunits || (in_stage_bytes && !in_stage) ||
        (out_stage_bytes && !out_stage)) {
        rc = 1;
        goto fail_alloc;
    }
    hblock = (uint32_t *)(hjobs + live);
    dblock = (uint32_t *)(djobs + live);
    hregion = (HapGpuRegion *)(hblock + live);
    dregion = (HapGpuRegion *)(dblock + live);
    if (scan_chunks) {
        /* one arena: chunk table | segment summaries | block positions | fine work list | joins | window records */
        const size_t o_segs = align_up(sizeof(HapGpuScanChunk) * scan_chunks, 64);
        const size_t o_bpos = o_segs + sizeof(HapGpuScanSegment) * scan_segs;
        const size_t o_work = align_up(o_bpos + sizeof(uint32_t) * scan_words, 64);
        const size_t o_joins = align_up(o_work + sizeof(uint32_t) * ((size_t)fine_total + 2u), 64);   /* count | list | pool cursor */
        const size_t o_recs = align_up(o_joins + (size_t)16u * scan_segs, 64);
        uint8_t *arena = (uint8_t *)hapgpu_rt_device_scratch(rt, D_SCAN, o_recs + (size_t)512u * scan_segs);
        hscan = (HapGpuScanChunk *)hapgpu_rt_pinned_scratch(rt, P_SCAN, sizeof(HapGpuScanChunk) * scan_chunks);
        if (!arena || !hscan) {
            rc = 1;
            goto fail_alloc;
        }
        dscan = (HapGpuScanChunk *)arena;
        dsegs = (HapGpuScanSegment *)(arena + o_segs);
        dbpos = (uint32_t *)(arena + o_bpos);
        dwork = (uint32_t *)(arena + o_work);
        djoins = arena + o_joins;
        drecs = arena + o_recs;
    }
    if (use_guess || use_scan_guess) {
        /* (a table per unit slot; the scan's pieces are the slots behind the ordinary ones) */
        dguess = (uint8_t *)hapgpu_rt_device_scratch(rt, D_GUESS, (size_t)HAP_GROUP_TABLE_BYTES *
                                                     ((size_t)total_units + (use_scan_guess ? fine_total : 0u) + 1u));
        if (!dguess) {
            rc = 1;
            goto fail_alloc;
        }
    }
    {
        unsigned chunk_cursor = 0, unit_cursor = 0, scan_cursor = 0, seg_cursor = 0, word_cursor = 0, fine_cursor = 0;
        request_marks marks;
        HapGpuScanRecords scan;      /* the block scan's records, once it has run */
        const void *staged_src = NULL;
        unsigned long staged_len = 0;
        const uint8_t *staged_dev = NULL;
        marks.count = 0;
        marks.requested = NULL;
        memset(&scan, 0, sizeof(scan));
        for (f = 0; f < frame_count; f++) {
            hapf_texture_plan *p = &plans[f];
            HapGpuDecodeJob *job;
            const uint8_t *frame_dev;
            unsigned units;
            if (results[f] != HapResult_No_Error)
                continue;
            units = p->unit_count;
            job = &hjobs[job_of_frame[f]];
            memset(job, 0, sizeof(*job));
            if (in_off[f] && inputs[f] == staged_src && input_bytes[f] == staged_len) {
                /* (the entry before this one was the same host frame -- HapGpuDecodeFramesRGBA asks for both textures of a
                   frame in one call: one upload serves both) */
                frame_dev = staged_dev;
            } else if (in_off[f]) {
                uint8_t *d = in_stage + (in_off[f] - 1);
                rc |= hapgpu_rt_h2d(rt, d, inputs[f], input_bytes[f]);
                frame_dev = d;
                staged_src = inputs[f];
                staged_len = input_bytes[f];
                staged_dev = d;
            } else {
                frame_dev = (const uint8_t *)inputs[f];
            }
            job->dst = (uint64_t)(uintptr_t)(out_off[f] ? out_stage + (out_off[f] - 1) : (uint8_t *)outputs[f]);
            job->dst_cap = output_bytes[f];
            job->mode = p->mode;
            job->unit_count = units;
            job->units = (uint64_t)(uintptr_t)(dunits + unit_cursor);
            job->status = HapResult_Internal_Error;
            hblock[job_of_frame[f]] = skipping ? (uint32_t)hapf_block_bytes(p->format) : 0u;
            if (entry_regions)
                hregion[job_of_frame[f]] = entry_regions[f];
            if (p->mode == HAPGPU_JOB_COMPLEX) {
                job->payload = (uint64_t)(uintptr_t)(frame_dev + p->payload_offset);
                job->payload_len = p->payload_length;
                job->chunk_count = (uint32_t)p->chunk_count;
                job->chunks = (uint64_t)(uintptr_t)(dchunks + chunk_cursor);
                if (p->frag_table_offset) {
                    job->frag_sizes = (uint64_t)(uintptr_t)(frame_dev + p->frag_table_offset);
                    job->frag_log2 = p->frag_log2;
                    job->frag_entries = p->frag_entries;
                    job->reserved = p->frag_gran_log2 | (p->frag_window256 << 8);
                    /* bits 0..2: plain fragment kernels needed, bits 4..6: windowed ones (8 KiB fragments whose
                       table promises offsets of at most 3 KiB), bits 8 / 9: field streams (table version 3) */
                    if (p->frag_tiles_offset && p->frag_fields && !(flags & HAPGPU_DECODE_IGNORE_HALF_TILES)) {
                        job->fields_period = p->frag_fields;
                        job->group_tables = (uint64_t)(uintptr_t)(frame_dev + p->frag_tiles_offset);
                        frag_kinds |= p->frag_fields == 4u ? 0x100u : p->frag_fields == 2u ? 0x200u : p->frag_fields == 8u ? 0x800u : 0x400u;
                    } else if (p->frag_log2 == 13u && p->frag_window256 != 0 && p->frag_window256 <= HAP_FRAGMENT_WINDOW_256)
                        frag_kinds |= 16u << p->frag_gran_log2;
                    else
                        frag_kinds |= 1u << p->frag_gran_log2;
                }
                if (dguess && use_guess && (guess_frame[f] & 1)) {
                    const unsigned layout = field_layout_of_format(p->format);
                    job->fields_period = layout;
                    job->group_tables = (uint64_t)(uintptr_t)dguess;
                    job->reserved |= 1u << 16;
                    frag_kinds |= layout == 4u ? 0x100u : layout == 2u ? 0x200u : layout == 8u ? 0x800u : 0x400u;
                }
                if (p->chunk_count > 0)
                    memcpy(hchunks + chunk_cursor, p->chunks, sizeof(HapGpuChunkIn) * (size_t)p->chunk_count);
                chunk_cursor += (unsigned)p->chunk_count;
                if (scan_chunks && !p->frag_table_offset) {
                    int c;
                    for (c = 0; c < p->chunk_count; c++) {
                        const HapGpuChunkIn *ch = &p->chunks[c];
                        if ((ch->codec & 0xFFu) != HAP_NIBBLE_SNAPPY || ch->unit_count <= 1u)
                            continue;
                        scan_entry(&hscan[scan_cursor++], unit_cursor + ch->unit_first, ch->src_len, output_bytes[f],
                                   dbpos, &seg_cursor, &word_cursor, scan_seg_bytes, &fine_cursor);
                    }
                }
            } else {
                job->payload = (uint64_t)(uintptr_t)(frame_dev + p->section_offset);
                job->payload_len = p->section_length;
                if (scan_chunks && p->mode == HAPGPU_JOB_SNAPPY && units > 1u)
                    scan_entry(&hscan[scan_cursor++], unit_cursor, p->section_length, output_bytes[f], dbpos, &seg_cursor,
                               &word_cursor, scan_seg_bytes, &fine_cursor);
            }
            if (dguess && use_scan_guess && (guess_frame[f] & 2) && field_layout_of_format(p->format) && !job->fields_period) {
                const unsigned layout = field_layout_of_format(p->format);
                job->fields_period = layout;
                job->group_tables = (uint64_t)(uintptr_t)dguess;
                job->reserved |= 1u << 16;
                /* 0x1000: units for the block-per-lane decoder may appear among the scan's pieces as well */
                frag_kinds |= (layout == 4u ? 0x100u : layout == 2u ? 0x200u : 0x400u) | 0x1000u;
            }
            unit_cursor += units;
        }
        HAPB_MARK("host plan");
        rc |= hapgpu_rt_h2d(rt, djobs, hjobs, (entry_regions ? job_bytes : sizeof(HapGpuDecodeJob) + (region ? sizeof(uint32_t) : 0u)) * live);
        if (total_chunks)
            rc |= hapgpu_rt_h2d(rt, dchunks, hchunks, sizeof(HapGpuChunkIn) * total_chunks);
        rc |= hapgpu_k_decode_plan(rt, djobs, live, dunits, total_units, frag_log2_seen ? max_chunks : 0u);
        /* a region call: the chunks, table fragments and raw pieces that hold none of the rectangle's blocks go here --
           in front of the block scan, so that a chunk nobody needs is not scanned either (the scan looks at STREAM units) */
        if (entry_regions)
            rc |= hapgpu_k_skip_units_per_job(rt, dunits, total_units, djobs, dblock, dregion, region_counted);
        else if (region)
            rc |= hapgpu_k_skip_units(rt, dunits, total_units, djobs, dblock, region, region_counted);

        /* hap.h callback contract (single-frame HapDecode only): the client is asked to "run" the
           chunks once planning succeeded and there is more than one (reference hap.c:852-862) */
        if (a->callback && frame_count == 1 && !rc && results[0] == HapResult_No_Error &&
            plans[0].mode == HAPGPU_JOB_COMPLEX && plans[0].chunk_count > 1) {
            unsigned char *req;
            int c, all = 1;
            rc |= hapgpu_rt_d2h(rt, hjobs, djobs, sizeof(HapGpuDecodeJob));
            rc |= hapgpu_rt_sync(rt);
            if (!rc && hjobs[0].status == HapResult_No_Error) {
                req = (unsigned char *)calloc((size_t)plans[0].chunk_count, 1);
                if (!req) {
                    rc = 1;
                } else {
                    marks.count = (unsigned)plans[0].chunk_count;
                    marks.requested = req;
                    if (a->marks && a->mark_count == marks.count)
                        memcpy(req, a->marks, marks.count);      /* a second pass: the client was asked already */
                    else
                        a->callback(mark_chunk, &marks, marks.count, a->callback_info);
                    free(client_marks);
                    client_marks = (unsigned char *)malloc(marks.count);
                    if (client_marks) {
                        memcpy(client_marks, req, marks.count);
                        client_marks_count = marks.count;
                    }
                    for (c = 0; c < plans[0].chunk_count; c++)
                        if (!req[c])
                            all = 0;
                    if (!all) {
                        /* chunks the client never asked for stay undecoded: blank their units
                           (HAPGPU_UNIT_SKIP is 0; unit slots of consecutive chunks are contiguous) */
                        /* a staged (host) output must come back unchanged where nothing is decoded */
                        if (out_off[0])
                            rc |= hapgpu_rt_h2d(rt, out_stage + (out_off[0] - 1), outputs[0],
                                                output_bytes[0] < hjobs[0].bytes_used ? output_bytes[0] : (size_t)hjobs[0].bytes_used);
                        for (c = 0; c < plans[0].chunk_count;) {
                            unsigned first, units = 0;
                            if (req[c]) {
                                c++;
                                continue;
                            }
                            first = plans[0].chunks[c].unit_first;
                            while (c < plans[0].chunk_count && !req[c] &&
                                   plans[0].chunks[c].unit_first == first + units) {
                                units += plans[0].chunks[c].unit_count;
                                c++;
                            }
                            rc |= hapgpu_rt_zero(rt, dunits + first, sizeof(HapGpuDecodeUnit) * (size_t)units);
                        }
                    }
                    free(req);
                }
            }
        }
        /* streams of other encoders (no fragment table): find their independent 64 KiB blocks first */
        if (scan_chunks && scan_cursor == scan_chunks) {
            scan.recs = drecs;
            scan.joins = djoins;
            scan.chunks = dscan;
            scan.chunk_count = scan_chunks;
            /* (about how many 64 KiB blocks the scanned streams hold: an eighth of the 8 KiB pieces the host made room for --
               what the frames' textures hold -- or, without those, what the compressed bytes would be at three to one) */
            scan.blocks_hint = fine_total ? fine_total / 8u + 1u : scan_segs / 5u + 1u;
            rc |= hapgpu_rt_h2d(rt, dscan, hscan, sizeof(HapGpuScanChunk) * scan_chunks);
            rc |= hapgpu_rt_zero(rt, dwork, sizeof(uint32_t));
            if (fine_total)
                rc |= hapgpu_rt_zero(rt, dwork + 1u + fine_total, sizeof(uint32_t));
            if ((frag_kinds & 0x1000u) || (skipping && fine_total))       /* (the decoder below walks all the pieces' slots, not only the listed ones) */
                rc |= hapgpu_rt_zero(rt, dunits + total_units, sizeof(HapGpuDecodeUnit) * (size_t)fine_total);
            rc |= hapgpu_k_scan_blocks(rt, dunits, djobs, dscan, scan_chunks, dsegs, drecs, djoins, scan_segs,
                                       fine_total ? dwork : NULL, total_units, fine_total);
            /* ... and the 64 KiB and 8 KiB blocks the scan found: in front of the table maker below, which makes no
               table for a piece that is blanked */
            if (entry_regions)
                rc |= hapgpu_k_skip_units_per_job(rt, dunits, total_units + fine_total, djobs, dblock, dregion, region_counted);
            else if (region)
                rc |= hapgpu_k_skip_units(rt, dunits, total_units + fine_total, djobs, dblock, region, region_counted);
        }
        if (dguess && use_guess)
            rc |= hapgpu_k_guess_group_tables(rt, dunits, total_units, djobs, NULL, 0u, NULL);
        if (dguess && (frag_kinds & 0x1000u)) {
            if (scan_chunks && scan_cursor == scan_chunks)
                rc |= hapgpu_k_guess_group_tables(rt, dunits, total_units + fine_total, djobs, dwork, fine_total, &scan);
            else
                frag_kinds &= ~0x1000u;
        }
        rc |= hapgpu_k_snappy_decode(rt, dunits, total_units, djobs, frag_log2_seen, frag_kinds,
                                     /* 3: every stream is as short as one 8 KiB fragment (frames written with
                                        HAPGPU_ENCODE_FINE_CHUNKS): the 2 KiB ring of the block-scan launches instead of the 32 KiB one, 30 wavefronts per CU instead of 4 */
                                     any_stream ? (scan_chunks ? 2 : (max_stream_src <= HAPGPU_SLOT_DATA_BYTES + 64u ? 3 : 1)) : 0,
                                     (scan_chunks && scan_cursor == scan_chunks && fine_total) ? dwork : NULL, fine_total,
                                     any_stream && scan.recs ? &scan : NULL);
        rc |= hapgpu_rt_d2h(rt, hjobs, djobs, sizeof(HapGpuDecodeJob) * live);
        HAPB_MARK("launched");
        rc |= hapgpu_rt_sync(rt);
        HAPB_MARK("completed");
        if (rc)
            goto fail_alloc;
    }

    /* 4. results */
    {
        int copied = 0;
        for (f = 0; f < frame_count; f++) {
            HapGpuDecodeJob *job;
            if (results[f] != HapResult_No_Error)
                continue;
            job = &hjobs[job_of_frame[f]];
            if (job->status == HAPGPU_STATUS_INDEX_MISMATCH) {
                need_retry = 1;
                results[f] = HAPGPU_STATUS_INDEX_MISMATCH;
                continue;
            }
            results[f] = job->status;
            if (job->status == HapResult_No_Error) {
                if (output_used)
                    output_used[f] = (unsigned long)job->bytes_used;
                if (out_off[f]) {
                    rc |= hapgpu_rt_d2h(rt, outputs[f], out_stage + (out_off[f] - 1), (size_t)job->bytes_used);
                    copied = 1;
                }
            }
        }
        if (copied)
            rc |= hapgpu_rt_sync(rt);
        if (rc)
            goto fail_alloc;
    }

    /* 5. frames whose fragment table did not describe their streams: decode them the generic way */
    if (need_retry) {
        for (f = 0; f < frame_count; f++) {
            if (results[f] != HAPGPU_STATUS_INDEX_MISMATCH)
                continue;
            /* (a region call skips again on this road: whole chunks and raw pieces, all it has without table and scan --
               no more than the first pass skipped of this frame, and counted there: the frame's own rectangle, uncounted.
               The client of a single frame has given its marks: they go along, and the callback with them) */
            const HapbDecodeArgs again = {NULL, region, entry_regions ? &entry_regions[f] : NULL, 1,
                                          frame_count == 1 ? client_marks : NULL, client_marks_count,
                                          frame_count == 1 ? a->callback : NULL, a->callback_info};
            results[f] = HapResult_No_Error;
            ctx->table_fallbacks += 1;
            hapb_decode(ctx, 1, &inputs[f], &input_bytes[f], TEXTURE_INDEX(f), &outputs[f], &output_bytes[f],
                        output_used ? &output_used[f] : NULL, output_formats ? &output_formats[f] : NULL,
                        &results[f], (flags | HAPGPU_DECODE_IGNORE_FRAGMENT_INDEX | HAPGPU_DECODE_NO_BLOCK_SCAN | HAPGPU_DECODE_NO_FIELD_GUESS) &
                                     ~HAPGPU_DECODE_GUESS_FIELDS, &again);
        }
    }

finish:
    HAPB_MARK("results");
    for (f = 0; f < frame_count; f++) {
        if (results[f] != HapResult_No_Error && first_error == HapResult_No_Error)
            first_error = results[f];
        hapf_plan_free(&plans[f]);
        hapf_reader_free(&readers[f]);
    }
    free(plans); free(readers); free(fetchers); free(in_off); free(out_off); free(job_of_frame);
    free(in_dev); free(out_dev); free(client_marks); free(guess_frame);
    return first_error;

fail_alloc:
    for (f = 0; f < frame_count; f++) {
        if (results[f] == HapResult_No_Error || results[f] == HAPGPU_STATUS_INDEX_MISMATCH)
            results[f] = HapResult_Internal_Error;
        if (plans) hapf_plan_free(&plans[f]);
        if (readers) hapf_reader_free(&readers[f]);
    }
    free(plans); free(readers); free(fetchers); free(in_off); free(out_off); free(job_of_frame);
    free(in_dev); free(out_dev); free(client_marks); free(guess_frame);
    return HapResult_Internal_Error;
}

/* ============================================================= join on the device */
/* Sink of hapj_join for frames in device memory: header bytes are collected on the host and uploaded in one copy, the
   groups' tables and payloads become device-to-device moves of the gather kernel (pieces of at most 64 KiB, one
   wavefront each).  Two launches: what the host made first, then the moves (table contents land on top of the zeros
   of their header region). */
#define JOIN_PIECE 65536u
typedef struct move_list {
    HapGpuCopyEntry *e;
    size_t count, cap;
} move_list;

typedef struct device_sink {
    uint8_t *bytes;               /* host-made bytes, 16-byte aligned pieces */
    size_t bytes_used, bytes_cap;
    move_list puts, moves;        /* puts: src = offset into `bytes` until the upload address is known */
    const void *const *frames;
    uint8_t *out;
} device_sink;

static int move_append(move_list *l, uint64_t src, uint64_t dst, size_t len)
{
    while (len) {
        const size_t n = len < JOIN_PIECE ? len : JOIN_PIECE;
        if (l->count == l->cap) {
            const size_t cap = l->cap ? 2u * l->cap : 256u;
            HapGpuCopyEntry *e = (HapGpuCopyEntry *)realloc(l->e, cap * sizeof(*e));
            if (!e)
                return 1;
            l->e = e;
            l->cap = cap;
        }
        l->e[l->count].src = src;
        l->e[l->count].dst = dst;
        l->e[l->count].len = (uint32_t)n;
        l->e[l->count].reserved = 0;
        l->count++;
        src += n; dst += n; len -= n;
    }
    return 0;
}

static int device_put(void *user, uint64_t dst_off, const void *src, size_t len)
{
    device_sink *d = (device_sink *)user;
    const size_t padded = (len + 15u) & ~(size_t)15u;
    if (len == 0)
        return 0;
    if (d->bytes_used + padded > d->bytes_cap) {
        const size_t cap = 2u * (d->bytes_used + padded) + 4096u;
        uint8_t *b = (uint8_t *)realloc(d->bytes, cap);
        if (!b)
            return 1;
        d->bytes = b;
        d->bytes_cap = cap;
    }
    memcpy(d->bytes + d->bytes_used, src, len);
    memset(d->bytes + d->bytes_used + len, 0, padded - len);
    if (move_append(&d->puts, (uint64_t)d->bytes_used, (uint64_t)(uintptr_t)(d->out + dst_off), len))
        return 1;
    d->bytes_used += padded;
    return 0;
}

static int device_move(void *user, unsigned group, uint64_t src_off, uint64_t dst_off, size_t len)
{
    device_sink *d = (device_sink *)user;
    return move_append(&d->moves, (uint64_t)(uintptr_t)((const uint8_t *)d->frames[group] + src_off),
                       (uint64_t)(uintptr_t)(d->out + dst_off), len);
}

unsigned hapb_join_device(HapGpuContext *ctx, unsigned group_count, const void *const *frames,
                          const unsigned long *frame_bytes, void *output, unsigned long output_bytes,
                          unsigned long *output_used)
{
    hapgpu_rt *rt = ctx->rt;
    hapf_reader *readers;
    fetch_ctx *fetchers;
    uint8_t *prefix, *dprefix;
    uint64_t *hptr, *dptr;
    device_sink ds;
    hapj_sink sink;
    unsigned g, result, rc = 0;

    if (group_count == 0 || !frames || !frame_bytes || !output || !output_used)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    for (g = 0; g < group_count; g++)
        if (!frames[g] || frame_bytes[g] > 0xFFFFFFFFul || !is_dev(ctx, frames[g]))
            return HapResult_Bad_Arguments;
    if (!is_dev(ctx, output))
        return HapResult_Bad_Arguments;
    readers = (hapf_reader *)calloc(group_count, sizeof(*readers));
    fetchers = (fetch_ctx *)calloc(group_count, sizeof(*fetchers));
    hptr = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_PTRS, sizeof(uint64_t) * 2u * group_count);
    dptr = (uint64_t *)hapgpu_rt_device_scratch(rt, D_PTRS, sizeof(uint64_t) * 2u * group_count);
    dprefix = (uint8_t *)hapgpu_rt_device_scratch(rt, D_PREFIX, (size_t)PREFIX_BYTES * group_count);
    prefix = (uint8_t *)hapgpu_rt_pinned_scratch(rt, P_PREFIX, (size_t)PREFIX_BYTES * group_count);
    if (!readers || !fetchers || !hptr || !dptr || !dprefix || !prefix) {
        free(readers); free(fetchers);
        return HapResult_Internal_Error;
    }
    /* the groups' headers come to the host (one gather + one copy); what the planner needs beyond the prefix -- the
       tables of frames with many chunks -- it fetches on demand */
    for (g = 0; g < group_count; g++) {
        hptr[g] = (uint64_t)(uintptr_t)frames[g];
        hptr[group_count + g] = frame_bytes[g];
    }
    rc |= (unsigned)hapgpu_rt_h2d(rt, dptr, hptr, sizeof(uint64_t) * 2u * group_count);
    rc |= (unsigned)hapgpu_k_gather_prefixes(rt, dptr, dptr + group_count, group_count, PREFIX_BYTES, dprefix);
    rc |= (unsigned)hapgpu_rt_d2h(rt, prefix, dprefix, (size_t)PREFIX_BYTES * group_count);
    rc |= (unsigned)hapgpu_rt_sync(rt);
    if (rc) {
        free(readers); free(fetchers);
        return HapResult_Internal_Error;
    }
    for (g = 0; g < group_count; g++) {
        const size_t n = frame_bytes[g] < PREFIX_BYTES ? frame_bytes[g] : PREFIX_BYTES;
        hapf_reader_init_host(&readers[g], prefix + (size_t)PREFIX_BYTES * g, n);
        fetchers[g].ctx = ctx;
        fetchers[g].device_frame = (const uint8_t *)frames[g];
        readers[g].fetch = fetch_from_device;
        readers[g].user = &fetchers[g];
        readers[g].total_len = frame_bytes[g];
    }
    memset(&ds, 0, sizeof(ds));
    ds.frames = frames;
    ds.out = (uint8_t *)output;
    sink.user = &ds;
    sink.put = device_put;
    sink.move = device_move;
    result = hapj_join(group_count, readers, frame_bytes, &sink, output_bytes, output_used);
    if (result == HapResult_No_Error) {
        const size_t entries = ds.puts.count + ds.moves.count;
        uint8_t *dbytes = (uint8_t *)hapgpu_rt_device_scratch(rt, D_JOBS, ds.bytes_used + 16u);
        HapGpuCopyEntry *dmoves = (HapGpuCopyEntry *)hapgpu_rt_device_scratch(rt, D_COPIES, sizeof(HapGpuCopyEntry) * (entries + 1u));
        size_t i;
        if (!dbytes || !dmoves) {
            result = HapResult_Internal_Error;
        } else {
            for (i = 0; i < ds.puts.count; i++)
                ds.puts.e[i].src += (uint64_t)(uintptr_t)dbytes;
            if (ds.bytes_used)
                rc |= (unsigned)hapgpu_rt_h2d(rt, dbytes, ds.bytes, ds.bytes_used);
            if (ds.puts.count)
                rc |= (unsigned)hapgpu_rt_h2d(rt, dmoves, ds.puts.e, sizeof(HapGpuCopyEntry) * ds.puts.count);
            if (ds.moves.count)
                rc |= (unsigned)hapgpu_rt_h2d(rt, dmoves + ds.puts.count, ds.moves.e, sizeof(HapGpuCopyEntry) * ds.moves.count);
            if (ds.puts.count)
                rc |= (unsigned)hapgpu_k_frame_gather(rt, dmoves, (unsigned)ds.puts.count);
            if (ds.moves.count)
                rc |= (unsigned)hapgpu_k_frame_gather(rt, dmoves + ds.puts.count, (unsigned)ds.moves.count);
            rc |= (unsigned)hapgpu_rt_sync(rt);     /* (the lists live in pageable memory: nothing may still read them) */
            if (rc)
                result = HapResult_Internal_Error;
        }
    }
    free(ds.bytes); free(ds.puts.e); free(ds.moves.e);
    for (g = 0; g < group_count; g++)
        hapf_reader_free(&readers[g]);
    free(readers); free(fetchers);
    return result;
}
