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
#include "hap_encode_plan.h"
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

/* the whole-call answer: every result set (a NULL results: none), `code` returned */
static unsigned answer_all(unsigned *results, unsigned frame_count, unsigned code)
{
    unsigned f;
    for (f = 0; results && f < frame_count; f++)
        results[f] = code;
    return code;
}

/* ================================================================== encode */

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

/* What one hapb_encode call holds from step to step: its arguments, the plan (hap_encode_plan.h), which frames it
   launches, and its scratch. */
typedef struct encode_call {
    HapGpuContext *ctx;
    const HapbBlockEncodeJob *job;
    int inputs_are_device;
    unsigned frame_count, count;
    const void *const *inputs;
    void *const *outputs;
    const unsigned long *output_bytes;
    unsigned long *output_used;
    unsigned *results;
    hap_encode_plan plan;
    unsigned placed;                  /* plan.placed, after the frames, their number and the context have had their say */
    /* admission: the frames that are launched, and where in staging those with host buffers lie (+ 1; 0: not staged) */
    unsigned live, first_error;
    unsigned *live_index;
    size_t *stage_off_in, *stage_off_out;
    size_t stage_in_bytes, stage_out_bytes;
    /* scratch */
    HapGpuFrameEnc *hframes, *dframes;
    uint8_t *dslots, *tex_stage, *out_stage, *dgrouptables;
    uint32_t *dfragsizes;
    HapGpuCopyEntry *dcopies;
    void *dpack;
    uint64_t *dacc;
} encode_call;

/* the one owner of a call's admission arrays (what a HapbEncodePending has taken over is NULL here) */
static void encode_call_free(encode_call *c)
{
    free(c->live_index); free(c->stage_off_in); free(c->stage_off_out);
    c->live_index = NULL;
    c->stage_off_in = c->stage_off_out = NULL;
}

/* ... and of a HapbEncodePending and its arrays */
static void encode_pending_free(HapbEncodePending *pd)
{
    free(pd->live_index); free(pd->stage_off_out);
    free(pd->inputs); free(pd->outputs); free(pd->output_bytes);
    free(pd);
}

/* every frame the call would have launched: Internal_Error */
static unsigned encode_fail_live(const encode_call *c)
{
    unsigned k;
    for (k = 0; k < c->live; k++)
        c->results[c->live_index[k]] = HapResult_Internal_Error;
    return HapResult_Internal_Error;
}

/* 1. per-frame checks: result codes, live_index, staging offsets, and a frame's veto against placing.  Frames that fail
   are left out of the launch.  0: out of memory */
static int encode_admit_frames(encode_call *c)
{
    const hap_encode_plan *const p = &c->plan;
    const unsigned count = c->count;
    size_t in_total = 0, out_total = 0;
    unsigned f, i;
    c->live_index = (unsigned *)malloc(sizeof(unsigned) * c->frame_count);
    c->stage_off_in = (size_t *)calloc(c->frame_count, sizeof(size_t));
    c->stage_off_out = (size_t *)calloc(c->frame_count, sizeof(size_t));
    if (!c->live_index || !c->stage_off_in || !c->stage_off_out)
        return 0;
    for (f = 0; f < c->frame_count; f++) {
        unsigned rc = HapResult_No_Error;
        if (!c->outputs[f] || c->output_bytes[f] == 0)
            rc = HapResult_Bad_Arguments;
        for (i = 0; rc == HapResult_No_Error && i < count; i++)
            if (!c->inputs[(size_t)f * count + i])
                rc = HapResult_Bad_Arguments;
        if (rc == HapResult_No_Error) {
            /* hap.c:386-389 for the first texture; later textures are re-checked against
               the space actually left once the sizes are known */
            size_t avail = c->output_bytes[f] > p->outer_header ? c->output_bytes[f] - p->outer_header : 0;
            if (avail < p->tex[0].bound || c->output_bytes[f] < p->frame_raw_bound)
                rc = HapResult_Buffer_Too_Small;
            /* second texture: the reference compares its bound with what is left after the
               first section's ACTUAL size (hap.c:589); that size is not known before the
               launch, so the first section's maximum (raw storage) is assumed */
            else if (count == 2 && avail - (p->tex[0].header_len + p->tex[0].bytes) < p->tex[1].bound)
                rc = HapResult_Buffer_Too_Small;
        }
        c->results[f] = rc;
        c->output_used[f] = 0;
        if (rc != HapResult_No_Error) {
            if (c->first_error == HapResult_No_Error)
                c->first_error = rc;
            continue;
        }
        c->live_index[c->live++] = f;
        if (c->output_bytes[f] < p->placed_extent)
            c->placed = 0u;
        if (!c->inputs_are_device) {
            int staged = 0;
            for (i = 0; i < count; i++)
                if (!is_dev(c->ctx, c->inputs[(size_t)f * count + i]))
                    staged = 1;
            if (staged) {
                c->stage_off_in[f] = in_total + 1;         /* +1: 0 means "not staged" */
                in_total += p->stage_in_bytes;
            }
        }
        if (!is_dev(c->ctx, c->outputs[f])) {
            c->stage_off_out[f] = out_total + 1;
            /* (+8 per texture: a section written in the chunked form may exceed header + bytes by up to
               header_len - 1 bytes, see the comparison in frame_pack_kernel / hap.c:478) */
            out_total += align_up(p->frame_raw_bound + 8u * count > p->placed_extent ? p->frame_raw_bound + 8u * count : p->placed_extent, 256);
        }
    }
    c->stage_in_bytes = in_total;
    c->stage_out_bytes = out_total;
    return 1;
}

/* 2. what the call's size and the context's history say about placing */
static void encode_placing_policy(encode_call *c)
{
    HapGpuContext *const ctx = c->ctx;
    /* (frames are interleaved over the workgroups: with a dozen of them, few fragments of the same frame are in flight
       together and the waiting costs less than the gather pass; measured on 8K frames: 1 frame 0.130 against 0.114 ms,
       8 the same, 16 0.885 against 0.914, 60 2.90 against 3.08) */
    if (c->live < ctx->placing_min_frames)
        c->placed = 0u;
    if (c->placed && ctx->placing_holdoff) {
        ctx->placing_holdoff -= 1u;
        c->placed = 0u;
    }
    if (ctx->placing_off)                            /* (after a timeout: counted down call by call, then placing is back) */
        ctx->placing_off -= 1u;
}

/* 3. scratch for the live frames.  0: out of memory */
static int encode_scratch(encode_call *c)
{
    const hap_encode_plan *const p = &c->plan;
    hapgpu_rt *const rt = c->ctx->rt;
    const size_t live = c->live, frags = (size_t)p->frags_per_frame * live, chunks = (size_t)p->chunks_per_frame * live;
    c->hframes = (HapGpuFrameEnc *)hapgpu_rt_pinned_scratch(rt, P_FRAMES, sizeof(HapGpuFrameEnc) * live);
    c->dframes = (HapGpuFrameEnc *)hapgpu_rt_device_scratch(rt, D_FRAMES, sizeof(HapGpuFrameEnc) * live);
    c->dslots = p->any_snappy ? (uint8_t *)hapgpu_rt_device_scratch(rt, D_SLOTS, (size_t)p->slot_stride * frags) : NULL;
    c->dfragsizes = (uint32_t *)hapgpu_rt_device_scratch(rt, D_FRAGSIZES, sizeof(uint32_t) * frags);
    c->dcopies = (HapGpuCopyEntry *)hapgpu_rt_device_scratch(rt, D_COPIES, sizeof(HapGpuCopyEntry) * (frags + chunks));
    c->dpack = hapgpu_rt_device_scratch(rt, D_PACK, (size_t)hapgpu_pack_scratch_bytes_per_chunk() * chunks);
    if (c->placed)
        c->dacc = (uint64_t *)hapgpu_rt_device_scratch(rt, D_CHUNK_ACC, sizeof(uint64_t) * chunks);
    if (p->any_half_tiles)
        c->dgrouptables = (uint8_t *)hapgpu_rt_device_scratch(rt, D_GROUPTABLES, (size_t)HAP_GROUP_TABLE_BYTES * frags);
    if (c->stage_in_bytes)
        c->tex_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TEX_STAGE, c->stage_in_bytes);
    if (c->stage_out_bytes)
        c->out_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_FRAME_STAGE, c->stage_out_bytes);
    return c->hframes && c->dframes && (!c->placed || c->dacc) && (!p->any_snappy || c->dslots) && c->dfragsizes && c->dcopies &&
           c->dpack && (!p->any_half_tiles || c->dgrouptables) && (!c->stage_in_bytes || c->tex_stage) &&
           (!c->stage_out_bytes || c->out_stage);
}

/* 4. the frames' descriptors in pinned memory, and host textures on their way to staging.  != 0: a copy failed */
static unsigned encode_fill_descriptors(const encode_call *c)
{
    const hap_encode_plan *const p = &c->plan;
    const unsigned count = c->count;
    unsigned i, k, rc = 0;
    for (k = 0; k < c->live; k++) {
        HapGpuFrameEnc *fe = &c->hframes[k];
        const unsigned f = c->live_index[k];
        size_t in_cursor = 0;
        memset(fe, 0, sizeof(*fe));
        fe->dst = (uint64_t)(uintptr_t)(c->stage_off_out[f] ? c->out_stage + (c->stage_off_out[f] - 1) : (uint8_t *)c->outputs[f]);
        fe->dst_cap = c->output_bytes[f];
        fe->tex_count = count;
        fe->outer_header_len = p->outer_header;
        fe->status = HapResult_Internal_Error;   /* overwritten by the pack kernel */
        if (c->placed)
            fe->chunk_acc = (uint64_t)(uintptr_t)(c->dacc + (size_t)k * p->chunks_per_frame);
        if (p->kinds.fused) {
            fe->rgba = c->job->host_table[f];
            fe->rgba_row_bytes = (uint32_t)c->job->source.row_bytes;
            fe->rgba_blocks_x = c->job->source.width / 4u;
            fe->rgba_blocks_x_inv = HAPGPU_DIV_INV(c->job->source.width / 4u);
        }
        for (i = 0; i < count; i++) {
            const hap_encode_tex *t = &p->tex[i];
            HapGpuTexEnc *te = &fe->tex[i];
            const void *src = c->inputs[(size_t)f * count + i];
            if (c->stage_off_in[f] && !is_dev(c->ctx, src)) {
                uint8_t *d = c->tex_stage + (c->stage_off_in[f] - 1) + in_cursor;
                rc |= (unsigned)hapgpu_rt_h2d(c->ctx->rt, d, src, t->bytes);
                src = d;
            }
            in_cursor += align_up(t->bytes, 256);
            te->src = (uint64_t)(uintptr_t)src;
            te->bytes = (uint32_t)t->bytes;
            te->format_nibble = t->nibble;
            te->compressor = t->compressor;
            te->chunk_count = t->chunk_count;
            te->chunk_bytes = t->chunk_bytes;
            te->header_len = t->header_len;
            te->frags_per_chunk = t->fpc;
            te->frags_per_chunk_inv = HAPGPU_DIV_INV(t->fpc ? t->fpc : 1u);
            te->frag_first = k * p->frags_per_frame + (i ? p->tex[0].chunk_count * p->tex[0].fpc : 0u);
            te->emit_index = (p->flags & HAPGPU_ENCODE_FRAGMENT_INDEX) ? 1u : 0u;
            te->control = hap_encode_plan_control(p, i, c->placed);
        }
    }
    return rc;
}

/* 5. With every buffer in device memory (nothing staged) nothing in the call's launches depends on the buffers
   themselves -- their addresses are in the tables copied from pinned memory -- so the sequence is recorded once per
   geometry as a HIP graph and replayed with one launch.  1: such a call, *key_out everything its kernel arguments and
   copy sizes depend on */
static int encode_graph_key(const encode_call *c, uint64_t *key_out)
{
    const hap_encode_plan *const p = &c->plan;
    const HapGpuContext *const ctx = c->ctx;
    const HapbBlockEncodeJob *const job = c->job;
    uint64_t key = 0xCBF29CE484222325ull;
    unsigned i;
    if (c->stage_in_bytes != 0 || c->stage_out_bytes != 0 || c->inputs_are_device == 2 ||
        (p->flags & HAPGPU_ENCODE_SMALLER_FILES) || p->frag_log2 != 13u)
        return 0;
#define HAPB_MIX(v) (key = (key ^ (uint64_t)(v)) * 0x100000001B3ull)
    HAPB_MIX(c->live); HAPB_MIX(c->count); HAPB_MIX(p->flags); HAPB_MIX(p->frag_log2); HAPB_MIX(ctx->byte_granular);
    HAPB_MIX(ctx->position_lanes); HAPB_MIX(ctx->rgtc1_fields); HAPB_MIX(ctx->no_half_tiles); HAPB_MIX(p->kinds.fused); HAPB_MIX(c->placed);
    for (i = 0; i < c->count; i++) {
        HAPB_MIX(p->tex[i].format); HAPB_MIX(p->tex[i].compressor); HAPB_MIX(p->tex[i].chunk_count); HAPB_MIX(p->tex[i].bytes);
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
#undef HAPB_MIX
    *key_out = key;
    return 1;
}

/* 6. the launches of the call as one sequence.  != 0: one of them failed */
static unsigned encode_launches(const encode_call *c)
{
    const hap_encode_plan *const p = &c->plan;
    const HapbBlockEncodeJob *const job = c->job;
    hapgpu_rt *const rt = c->ctx->rt;
    const unsigned live = c->live, count = c->count;
    unsigned i, rc = 0;
    if (job) {
        const HapbSource *const src = &job->source;
        /* Hap Q Alpha: both textures from one pass over the RGBA (64 + 16 + 8 bytes per block);
           else one launch per texture that the second stage does not make itself.  (A batch takes at most
           65535 block rows.) */
        const int pair = job->count == 2 && job->formats[0] == HapTextureFormat_YCoCg_DXT5 &&
                         job->formats[1] == HapTextureFormat_A_RGTC1;
        rc |= (unsigned)hapgpu_rt_h2d(rt, job->device_table, job->host_table,
                                      sizeof(uint64_t) * (size_t)job_table_columns(job) * job->frame_count);
        for (i = 0; i < (pair ? 1u : job->count); i++)
            if (pair || !p->tex[i].fused) {
                const uint64_t *dt = job->device_table;
                /* (video pictures: one texture a frame, and the third column holds their CbCr planes) */
                const HapGpuPictureTable t = {{dt, dt + (size_t)(1u + i) * job->frame_count,
                                               pair || src->video ? dt + 2u * (size_t)job->frame_count : NULL}, {0u, 0u, 0u}};
                rc |= src->height / 4u > 65535u ? 1u :
                      src->video ?
                      (unsigned)hapgpu_k_block_encode_video(rt, &t, job->frame_count, src->width, src->height,
                                                            job->formats[i], p->refine, src->row_bytes,
                                                            src->video->chroma_row_bytes, src->video->matrix,
                                                            src->video->range) :
                      src->planes ?
                      (unsigned)hapgpu_k_block_encode_planes(rt, &t, job->frame_count, src->width, src->height,
                                                             job->formats[i], (unsigned)pair | p->refine, src->planes->channels,
                                                             src->planes->element, src->planes->plane_bytes,
                                                             src->row_bytes, job->plane_scale, job->plane_bias) :
                      (unsigned)hapgpu_k_block_encode(rt, &t, job->frame_count, src->width, src->height,
                                                      src->row_bytes, job->formats[i], (unsigned)pair | p->refine, job->wide,
                                                      src->picture_kind);
            }
    }
    rc |= (unsigned)hapgpu_rt_h2d(rt, c->dframes, c->hframes, sizeof(HapGpuFrameEnc) * live);
    if (c->placed) {
        rc |= (unsigned)hapgpu_rt_zero(rt, c->dacc, sizeof(uint64_t) * (size_t)p->chunks_per_frame * live);
        rc |= (unsigned)hapgpu_rt_zero(rt, c->dfragsizes, sizeof(uint32_t) * (size_t)p->frags_per_frame * live);
    }
    if (p->any_snappy)
        rc |= (unsigned)hapgpu_k_snappy_compress(rt, c->dframes, live, p->max_frags_per_tex, p->frag_log2, c->dslots, p->slot_stride,
                                                 c->dfragsizes, c->dgrouptables, &p->kinds);
    rc |= (unsigned)hapgpu_k_frame_pack(rt, c->dframes, live, p->frag_log2, c->dslots, p->slot_stride, c->dfragsizes, c->dgrouptables,
                                        c->dcopies, p->frags_per_frame * live, p->chunks_per_frame, p->max_chunks_per_tex, count, c->dpack);
    /* (placed fragments -- single-texture frames -- and their group tables are where they belong: nothing to
       gather.  A frame reported as not placed is encoded again as a whole.) */
    if (!(c->placed && count == 1u))
        rc |= (unsigned)hapgpu_k_frame_gather(rt, c->dcopies, (p->frags_per_frame + p->chunks_per_frame) * live);
    rc |= (unsigned)hapgpu_rt_d2h(rt, c->hframes, c->dframes, sizeof(HapGpuFrameEnc) * live);
    return rc;
}

/* ... replayed where the runtime holds a recording of them, recorded where it wants one, else issued plainly */
static unsigned encode_launch(const encode_call *c)
{
    hapgpu_rt *const rt = c->ctx->rt;
    uint64_t key = 0;
    const int graph = encode_graph_key(c, &key) ? hapgpu_rt_graph_begin(rt, key) : 2;
    unsigned rc;
    if (graph == 1)
        return 0;
    rc = encode_launches(c);
    /* (a recording that cannot be ended, instantiated or launched has run nothing: graphs are switched off for
       this context and the same launches are issued once more, plainly.  A recording can also be invalidated from
       outside -- another thread of the process synchronising the device while it runs: then the launches themselves
       report errors.  Either way nothing has run.) */
    if (graph == 0 && (hapgpu_rt_graph_end(rt, key, rc != 0) != 0 || rc != 0)) {
        hapgpu_rt_graphs_disable(rt);
        rc = encode_launches(c);
    }
    return rc;
}

/* 7. what hapb_encode_complete needs of the call: copies of the client's arrays, and the call's admission arrays, which
   are the pending call's from here.  NULL: out of memory */
static HapbEncodePending *encode_pending(encode_call *c, const unsigned long *input_bytes, const unsigned *formats,
                                         const unsigned *compressors, unsigned launch_rc)
{
    const HapbBlockEncodeJob *const job = c->job;
    const size_t n_in = (size_t)c->frame_count * c->count;
    HapbEncodePending *pd = (HapbEncodePending *)calloc(1, sizeof(*pd));
    unsigned i;
    if (!pd)
        return NULL;
    pd->inputs = (const void **)malloc(sizeof(void *) * n_in);
    pd->outputs = (void **)malloc(sizeof(void *) * c->frame_count);
    pd->output_bytes = (unsigned long *)malloc(sizeof(unsigned long) * c->frame_count);
    if (!pd->inputs || !pd->outputs || !pd->output_bytes) {
        encode_pending_free(pd);
        return NULL;
    }
    memcpy(pd->inputs, c->inputs, sizeof(void *) * n_in);
    memcpy(pd->outputs, c->outputs, sizeof(void *) * c->frame_count);
    memcpy(pd->output_bytes, c->output_bytes, sizeof(unsigned long) * c->frame_count);
    for (i = 0; i < c->count; i++) {
        pd->input_bytes[i] = input_bytes[i];
        pd->formats[i] = formats[i];
        pd->compressors[i] = compressors[i];
        pd->chunk_counts[i] = c->plan.chunk_counts[i];
    }
    pd->frame_count = c->frame_count;
    pd->count = c->count;
    pd->flags = c->plan.flags;
    pd->inputs_are_device = c->inputs_are_device;
    pd->output_used = c->output_used;
    pd->results = c->results;
    pd->live = c->live;
    pd->placed = c->placed;
    pd->first_error = c->first_error;
    pd->launch_rc = launch_rc;
    pd->live_index = c->live_index;
    pd->stage_off_out = c->stage_off_out;
    c->live_index = NULL;
    c->stage_off_out = NULL;
    pd->hframes = c->hframes;
    pd->out_stage = c->out_stage;
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
    return pd;
}

unsigned hapb_encode(HapGpuContext *ctx, unsigned frame_count, unsigned count,
                     const void *const *inputs, const unsigned long *input_bytes,
                     const unsigned *formats, const unsigned *compressors, const unsigned *chunk_counts,
                     void *const *outputs, const unsigned long *output_bytes,
                     unsigned long *output_used, unsigned *results, unsigned flags,
                     const HapbEncodeArgs *args)
{
    static const HapbEncodeArgs no_args;
    static const encode_call no_call;
    const HapbEncodeArgs *const a = args ? args : &no_args;
    encode_call c = no_call;
    HapbEncodePending *pd = NULL;
    unsigned f, rc = HapResult_No_Error;

    if (frame_count == 0)
        return HapResult_No_Error;
    if (!results)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, results, frame_count))
        return HapResult_Internal_Error;
    /* frame-independent argument checks, reference hap.c:518-559 */
    if (count == 0 || count > 2 || !inputs || !input_bytes || !formats || !compressors || !chunk_counts ||
        !outputs || !output_bytes || !output_used)
        rc = HapResult_Bad_Arguments;
    if (rc == HapResult_No_Error)
        rc = encode_textures_valid(count, input_bytes, formats, compressors, chunk_counts, flags);
    if (rc != HapResult_No_Error)
        return answer_all(results, frame_count, rc);
    /* geometry and policy shared by every frame of the batch */
    {
        const hap_encode_knobs knobs = {ctx->frag_log2, ctx->byte_granular, ctx->position_lanes, ctx->rgtc1_fields,
                                        ctx->no_half_tiles, ctx->no_fusion,
                                        !ctx->no_placing && !a->never_place && !ctx->placing_off};
        hap_encode_source source = {0u, 0, 0, 0u, 0u, 0ul};
        if (a->job) {
            const HapbSource *const s = &a->job->source;
            source.picture_kind = s->picture_kind;
            source.planes = s->planes != NULL;
            source.video = s->video != NULL;
            source.width = s->width;
            source.height = s->height;
            source.row_bytes = s->row_bytes;
        }
        rc = hap_encode_plan_of(&c.plan, &knobs, flags, count, input_bytes, formats, compressors, chunk_counts,
                                a->job ? &source : NULL);
        if (rc != HapResult_No_Error) {
            for (f = 0; f < frame_count; f++)
                output_used[f] = 0;
            return answer_all(results, frame_count, rc);
        }
    }
    c.ctx = ctx;
    c.job = a->job;
    c.inputs_are_device = a->inputs_are_device;
    c.frame_count = frame_count;
    c.count = count;
    c.inputs = inputs;
    c.outputs = outputs;
    c.output_bytes = output_bytes;
    c.output_used = output_used;
    c.results = results;
    c.placed = c.plan.placed;

    if (!encode_admit_frames(&c)) {
        rc = HapResult_Internal_Error;
    } else if (c.live == 0) {
        rc = c.first_error;
    } else {
        encode_placing_policy(&c);
        if (!encode_scratch(&c)) {
            rc = encode_fail_live(&c);
        } else {
            unsigned launch_rc = encode_fill_descriptors(&c);
            launch_rc |= encode_launch(&c);
            /* everything the call launches is on the stream: the rest -- waiting, reading the results, the second pass
               over frames that were not placed -- is hapb_encode_complete's, at once or (HapGpuEncodeFramesRGBABegin /
               ...Finish) when the client asks for the results */
            pd = encode_pending(&c, input_bytes, formats, compressors, launch_rc);
            if (!pd) {
                hapgpu_rt_sync(ctx->rt);
                rc = encode_fail_live(&c);
            }
        }
    }
    encode_call_free(&c);
    if (!pd)
        return rc;
    if (a->defer) {
        ctx->pending_encode = pd;
        return c.first_error;
    }
    return hapb_encode_complete(ctx, pd);
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
            if (fe->status == HAPGPU_STATUS_NOT_PLACED && (fe->notes & HAPGPU_FRAME_NOTE_WAVE_TIMED_OUT)) {
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
    encode_pending_free(pd);
    return first_error;
}

void hapb_encode_abandon(HapGpuContext *ctx, HapbEncodePending *pd)
{
    (void)hapgpu_rt_sync(ctx->rt);
    encode_pending_free(pd);
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
    case HapTextureFormat_YCoCg_DXT5: return HAPGPU_LAYOUT_2_6_4_4;
    case HapTextureFormat_RGB_DXT1: return HAPGPU_LAYOUT_4_4;
    case HapTextureFormat_A_RGTC1: return HAPGPU_LAYOUT_2_6;
    default: return HAPGPU_LAYOUT_NONE;
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
                        frag_kinds |= p->frag_fields == HAPGPU_LAYOUT_2_6_4_4 ? 0x100u : p->frag_fields == HAPGPU_LAYOUT_4_4 ? 0x200u : p->frag_fields == HAPGPU_LAYOUT_4_4_4_4 ? 0x800u : 0x400u;
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
                    frag_kinds |= layout == HAPGPU_LAYOUT_2_6_4_4 ? 0x100u : layout == HAPGPU_LAYOUT_4_4 ? 0x200u : layout == HAPGPU_LAYOUT_4_4_4_4 ? 0x800u : 0x400u;
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
                frag_kinds |= (layout == HAPGPU_LAYOUT_2_6_4_4 ? 0x100u : layout == HAPGPU_LAYOUT_4_4 ? 0x200u : 0x400u) | 0x1000u;
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
