/*
 * hap_api.c -- the exported symbols: the six functions of include/hap.h (same
 * names and signatures as the reference, /root/reference/source/hap.h:76-152)
 * and the context / batch functions of include/hap_gpu.h.  Pure C99.
 */
#include "hap_batch.h"
#include "hap_region.h"
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------ contexts -- */

unsigned int HapGpuCreate(int device, HapGpuContext **context)
{
    HapGpuContext *c;
    int rc;
    if (!context)
        return HapResult_Bad_Arguments;
    *context = NULL;
    c = (HapGpuContext *)calloc(1, sizeof(*c));
    if (!c)
        return HapResult_Internal_Error;
    rc = hapgpu_rt_create(device, &c->rt);
    if (rc) {
        free(c);
        return rc == 1 ? HapResult_Bad_Arguments : HapResult_Internal_Error;
    }
    c->frag_log2 = 13;   /* 8 KiB: best decode occupancy for ~1 % more bytes than 16 KiB */
    {
        const char *e = getenv("HAP_AMD_FRAGMENT_LOG2");
        if (e && atoi(e) >= 10 && atoi(e) <= 16)
            c->frag_log2 = (unsigned)atoi(e);
    }
    {
        const char *e = getenv("HAP_AMD_BYTE_GRANULAR");
        c->byte_granular = (e && atoi(e) != 0) ? 1u : 0u;
        c->position_lanes = HAP_AB_ENV("HAP_AMD_POSITION_LANES") ? 1u : 0u;
        c->no_half_tiles = HAP_AB_ENV("HAP_AMD_NO_HALF_TILES") ? 1u : 0u;
        c->no_block_scan = getenv("HAP_AMD_NO_BLOCK_SCAN") ? 1u : 0u;
        c->no_fusion = getenv("HAP_AMD_NO_FUSION") ? 1u : 0u;
        c->no_wide_planes = HAP_AB_ENV("HAP_AMD_NO_WIDE_PLANES") ? 1u : 0u;
        c->no_placing = getenv("HAP_AMD_NO_PLACING") ? 1u : 0u;
        c->placing_holdoff_calls = getenv("HAP_AMD_PLACING_HOLDOFF") ? (unsigned)atoi(getenv("HAP_AMD_PLACING_HOLDOFF")) : 8u;
        c->placing_min_frames = getenv("HAP_AMD_PLACING_MIN_FRAMES") ? (unsigned)atoi(getenv("HAP_AMD_PLACING_MIN_FRAMES")) : 8u;
        /* RGTC1 planes of large textures go through the [2, 6] field kernel (block-per-lane decodable: 2.9x the decode
           rate at the same size); HAP_AMD_RGTC1_LAYOUT overrides: 0 = position-per-lane compressor, 44 = [4, 4] */
        c->rgtc1_fields = 26u;
        if (HAP_AB_ENV("HAP_AMD_RGTC1_LAYOUT")) {
            const char *layout = HAP_AB_ENV("HAP_AMD_RGTC1_LAYOUT");
            const int v = layout ? atoi(layout) : 26;
            if (v == 0 || v == 26 || v == 44)
                c->rgtc1_fields = (unsigned)v;
        }
    }
    *context = c;
    return HapResult_No_Error;
}

void HapGpuDestroy(HapGpuContext *context)
{
    if (!context)
        return;
    /* an encode call begun and never finished: its launches are waited for (hapgpu_rt_destroy synchronises), its results
       are NOT written -- the client's arrays may be gone by now */
    if (context->pending_encode) {
        hapb_encode_abandon(context, context->pending_encode);
        context->pending_encode = NULL;
    }
    hapgpu_rt_destroy(context->rt);
    free(context);
}

static pthread_once_t g_default_once = PTHREAD_ONCE_INIT;
static HapGpuContext *g_default;

static void make_default(void)
{
    const char *e = getenv("HAP_AMD_DEVICE");
    if (HapGpuCreate(e ? atoi(e) : -1, &g_default) != HapResult_No_Error) {
        g_default = NULL;
        fprintf(stderr, "hap_amd: cannot create a GPU context; HapEncode/HapDecode will fail "
                        "(this library has no CPU path)\n");
    }
}

HapGpuContext *HapGpuDefaultContext(void)
{
    pthread_once(&g_default_once, make_default);
    return g_default;
}

/* hap.h has no context argument, and the reference is re-entrant (no globals in hap.c): a client may call
 * HapDecode from several threads at once, or again from inside its HapDecodeCallback (hap.h:113-130) while the
 * outer call is still waiting for it.  A context serves one call at a time, so the hap.h entry points take
 * whichever default context is free and add one (same device, own stream and scratch) when all are busy. */
#define HAP_DEFAULT_POOL 8
static HapGpuContext *g_pool[HAP_DEFAULT_POOL];
static pthread_t g_pool_owner[HAP_DEFAULT_POOL];     /* the thread inside a hap.h call on that member, if g_pool_busy */
static unsigned char g_pool_busy[HAP_DEFAULT_POOL];
static unsigned g_pool_count;
static pthread_mutex_t g_pool_lock = PTHREAD_MUTEX_INITIALIZER;

/* returns a default context with its lock HELD, or NULL when there is no GPU -- or when every member of the pool is
   in use by calls of THIS thread (HapDecode nested HAP_DEFAULT_POOL deep through callbacks): waiting would never end */
static HapGpuContext *acquire_default_context(void)
{
    HapGpuContext *first = HapGpuDefaultContext(), *c = NULL;
    const pthread_t self = pthread_self();
    unsigned i;
    int wait_for = -1;
    if (!first)
        return NULL;
    pthread_mutex_lock(&g_pool_lock);
    if (g_pool_count == 0)
        g_pool[g_pool_count++] = first;
    for (i = 0; i < g_pool_count && !c; i++)
        if (hapgpu_rt_trylock(g_pool[i]->rt) == 0) {
            c = g_pool[i];
            g_pool_owner[i] = self;
            g_pool_busy[i] = 1;
        }
    if (c)
        c->frag_log2 = first->frag_log2;       /* (HapGpuSetFragmentLog2 on the default context reaches every member) */
    if (!c && g_pool_count < HAP_DEFAULT_POOL &&
        HapGpuCreate(hapgpu_rt_device(first->rt), &c) == HapResult_No_Error) {
        c->frag_log2 = first->frag_log2;
        g_pool_owner[g_pool_count] = self;
        g_pool_busy[g_pool_count] = 1;
        g_pool[g_pool_count++] = c;
        hapgpu_rt_lock(c->rt);
    }
    if (!c) {
        /* pool exhausted: wait for a member that some other thread (or a client holding the default context's handle)
           is using */
        for (i = 0; i < g_pool_count; i++) {
            if (!(g_pool_busy[i] && pthread_equal(g_pool_owner[i], self)) && wait_for < 0)
                wait_for = (int)i;
        }
    }
    pthread_mutex_unlock(&g_pool_lock);
    if (!c && wait_for >= 0) {
        c = g_pool[wait_for];
        hapgpu_rt_lock(c->rt);
        pthread_mutex_lock(&g_pool_lock);
        g_pool_owner[wait_for] = self;
        g_pool_busy[wait_for] = 1;
        c->frag_log2 = first->frag_log2;
        pthread_mutex_unlock(&g_pool_lock);
    }
    return c;
}

static void release_default_context(HapGpuContext *c)
{
    unsigned i;
    pthread_mutex_lock(&g_pool_lock);
    for (i = 0; i < g_pool_count; i++)
        if (g_pool[i] == c)
            g_pool_busy[i] = 0;
    pthread_mutex_unlock(&g_pool_lock);
    hapgpu_rt_unlock(c->rt);
}

unsigned int HapGpuSetFragmentLog2(HapGpuContext *context, unsigned int log2_bytes)
{
    if (!context || log2_bytes < 10 || log2_bytes > 16)
        return HapResult_Bad_Arguments;
    context->frag_log2 = log2_bytes;
    return HapResult_No_Error;
}

unsigned long HapGpuTableFallbackCount(HapGpuContext *context)
{
    unsigned long n;
    if (!context)
        return 0;
    hapgpu_rt_lock(context->rt);
    n = context->table_fallbacks;
    hapgpu_rt_unlock(context->rt);
    if (context == g_default) {                /* the hap.h entry points may have run on any member of the pool */
        unsigned i;
        pthread_mutex_lock(&g_pool_lock);
        for (i = 0; i < g_pool_count; i++)
            if (g_pool[i] != context)
                n += g_pool[i]->table_fallbacks;
        pthread_mutex_unlock(&g_pool_lock);
    }
    return n;
}

unsigned long HapGpuResolvedBlockCount(HapGpuContext *context)
{
    unsigned long n;
    if (!context)
        return 0;
    hapgpu_rt_lock(context->rt);
    n = hapgpu_rt_resolved_blocks(context->rt);
    hapgpu_rt_unlock(context->rt);
    return n;
}

unsigned long HapGpuSkippedTextureBytes(HapGpuContext *context)
{
    unsigned long n;
    if (!context)
        return 0;
    hapgpu_rt_lock(context->rt);
    n = (unsigned long)hapgpu_rt_skipped_bytes(context->rt);
    hapgpu_rt_unlock(context->rt);
    return n;
}

unsigned int HapGpuRegionNeedsBytes(unsigned int width, unsigned int blockBytes, unsigned int regionX, unsigned int regionY,
                                    unsigned int regionWidth, unsigned int regionHeight, unsigned long firstByte,
                                    unsigned long byteCount)
{
    return (unsigned)hap_region_needs_bytes(width, blockBytes, regionX, regionY, regionWidth, regionHeight, firstByte, byteCount);
}

unsigned long HapGpuPlacementRetryCount(HapGpuContext *context)
{
    unsigned long n;
    if (!context)
        return 0;
    hapgpu_rt_lock(context->rt);
    n = context->placement_retries;
    hapgpu_rt_unlock(context->rt);
    return n;
}

unsigned int HapGpuFineChunkCount(unsigned long textureBytes, unsigned int textureFormat)
{
    return hapf_fine_chunk_count(textureBytes, textureFormat);
}

unsigned long HapGpuPlacementTimeoutCount(HapGpuContext *context)
{
    unsigned long n;
    if (!context)
        return 0;
    hapgpu_rt_lock(context->rt);
    n = context->placement_timeouts;
    hapgpu_rt_unlock(context->rt);
    return n;
}

unsigned int HapGpuSynchronize(HapGpuContext *context)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapgpu_rt_sync(context->rt) ? HapResult_Internal_Error : HapResult_No_Error;
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* --------------------------------------------------------------- hap.h -- */

/* reference hap.c:324-353 */
unsigned long HapMaxEncodedLength(unsigned int count, unsigned long *lengths,
                                  unsigned int *textureFormats, unsigned int *chunkCounts)
{
    unsigned long total = 8;
    unsigned i;
    if (count == 0 || count > 2 || !lengths || !textureFormats || !chunkCounts)
        return 0;
    for (i = 0; i < count; i++) {
        if (chunkCounts[i] == 0)
            return 0;
        total += (unsigned long)hapf_texture_bound(lengths[i], textureFormats[i], HapCompressorSnappy, chunkCounts[i]);
    }
    return total;
}

static unsigned env_encode_flags(void)
{
    const char *e = getenv("HAP_AMD_FRAGMENT_INDEX"), *c = getenv("HAP_AMD_COARSE_MATCHES"), *s = getenv("HAP_AMD_SMALLER_FILES");
    /* Frames from plain hap.h HapEncode carry nothing the Hap specification does not name: the private fragment table
       (section 0x46 inside the Decode Instructions Container) is written on request only, HAP_AMD_FRAGMENT_INDEX=1 --
       the reference skips unknown sections there (hap.c:701-703), but a drop-in library cannot know that every other
       parser of its frames does.  The batched HapGpu* calls take it as a flag. */
    return ((e && atoi(e) != 0) ? HAPGPU_ENCODE_FRAGMENT_INDEX : 0u) |
           ((c && atoi(c) != 0) ? HAPGPU_ENCODE_COARSE_MATCHES : 0u) |
           ((s && atoi(s) != 0) ? HAPGPU_ENCODE_SMALLER_FILES : 0u);
}

/* reference hap.c:506-604 */
unsigned int HapEncode(unsigned int count, const void **inputBuffers, unsigned long *inputBuffersBytes,
                       unsigned int *textureFormats, unsigned int *compressors, unsigned int *chunkCounts,
                       void *outputBuffer, unsigned long outputBufferBytes,
                       unsigned long *outputBufferBytesUsed)
{
    HapGpuContext *ctx;
    unsigned result = HapResult_Internal_Error, rc, flags, i;
    unsigned long used = 0;
    void *out = outputBuffer;
    if (count == 0 || count > 2 || !inputBuffers || !inputBuffersBytes || !textureFormats || !compressors ||
        !chunkCounts || !outputBuffer || outputBufferBytes == 0 || !outputBufferBytesUsed)
        return HapResult_Bad_Arguments;
    flags = env_encode_flags();
    /* A texture whose bytes do not divide by its chunk count is no real block texture; the reference's chunked form
       then drops the remainder (hap.c:433), and whether a frame takes that form or the raw one must not depend on
       the private table's few bytes: such textures are written without it, exactly as the reference decides. */
    for (i = 0; i < count; i++) {
        const unsigned n = chunkCounts[i] ? hapf_limit_chunk_count(inputBuffersBytes[i], textureFormats[i], chunkCounts[i]) : 0u;
        if (n == 0u || inputBuffersBytes[i] % n != 0u)
            flags &= ~HAPGPU_ENCODE_FRAGMENT_INDEX;
    }
    ctx = acquire_default_context();
    if (!ctx)
        return HapResult_Internal_Error;
    rc = hapb_encode(ctx, 1, count, (const void *const *)inputBuffers, inputBuffersBytes, textureFormats,
                     compressors, chunkCounts, &out, &outputBufferBytes, &used, &result, flags, NULL);
    release_default_context(ctx);
    if (rc == HapResult_No_Error)
        *outputBufferBytesUsed = used;
    return rc;
}

/* reference hap.c:993-1040 */
unsigned int HapDecode(const void *inputBuffer, unsigned long inputBufferBytes, unsigned int index,
                       HapDecodeCallback callback, void *info, void *outputBuffer,
                       unsigned long outputBufferBytes, unsigned long *outputBufferBytesUsed,
                       unsigned int *outputBufferTextureFormat)
{
    const HapbDecodeArgs client = {NULL, NULL, NULL, 0, NULL, 0u, callback, info};
    HapGpuContext *ctx;
    unsigned result = HapResult_Internal_Error, rc, fmt = 0;
    unsigned long used = 0;
    if (!inputBuffer || index > 1 || !callback || !outputBuffer || !outputBufferTextureFormat)
        return HapResult_Bad_Arguments;
    ctx = acquire_default_context();
    if (!ctx)
        return HapResult_Internal_Error;
    rc = hapb_decode(ctx, 1, &inputBuffer, &inputBufferBytes, index, &outputBuffer, &outputBufferBytes, &used,
                     &fmt, &result, 0, &client);
    release_default_context(ctx);
    /* the reference stores the format as soon as the section type has been read (hap.c:754) */
    *outputBufferTextureFormat = fmt;
    if (rc == HapResult_No_Error && outputBufferBytesUsed)
        *outputBufferBytesUsed = used;
    return rc;
}

/* The reference object also exports two helpers that hap.h does not declare (they are non-static in
 * hap.c:732 and hap.c:932); kept for link compatibility with clients that reach for them. */
int hap_get_section_at_index(const void *input_buffer, uint32_t input_buffer_bytes, unsigned int index,
                             const void **section, uint32_t *section_length, unsigned int *section_type)
{
    hapf_reader r;
    uint64_t off = 0;
    unsigned rc;
    hapf_reader_init_host(&r, input_buffer, input_buffer_bytes);
    *section = NULL;
    *section_length = 0;
    *section_type = 0;
    rc = hapf_locate(&r, input_buffer_bytes, index, &off, section_length, section_type);
    if (rc == HapResult_No_Error)
        *section = (const uint8_t *)input_buffer + off;
    hapf_reader_free(&r);
    return (int)rc;
}

unsigned int hap_decode_single_texture(const void *texture_section, uint32_t texture_section_length,
                                       unsigned int texture_section_type, HapDecodeCallback callback, void *info,
                                       void *outputBuffer, unsigned long outputBufferBytes,
                                       unsigned long *outputBufferBytesUsed, unsigned int *outputBufferTextureFormat)
{
    /* re-wrap the bare section in an 8-byte top-level header and take the normal path (host memory only) */
    uint8_t *frame;
    unsigned rc;
    if (!texture_section || !callback || !outputBuffer || !outputBufferTextureFormat)
        return HapResult_Bad_Arguments;
    frame = (uint8_t *)malloc((size_t)texture_section_length + 8u);
    if (!frame)
        return HapResult_Internal_Error;
    hapf_write_section(frame, 8u, texture_section_length, texture_section_type);
    memcpy(frame + 8, texture_section, texture_section_length);
    rc = HapDecode(frame, (unsigned long)texture_section_length + 8ul, 0, callback, info, outputBuffer,
                   outputBufferBytes, outputBufferBytesUsed, outputBufferTextureFormat);
    free(frame);
    return rc;
}

/* Inspectors read section headers only.  Host frames are parsed in place; for
 * device-resident frames the few header bytes are copied back. */
typedef struct inspect_fetch {
    HapGpuContext *ctx;
    const uint8_t *frame;
} inspect_fetch;

static int inspect_fetch_cb(void *user, uint64_t offset, uint64_t length, uint8_t *dst)
{
    inspect_fetch *f = (inspect_fetch *)user;
    int rc;
    hapgpu_rt_lock(f->ctx->rt);
    rc = hapgpu_rt_d2h(f->ctx->rt, dst, f->frame + offset, (size_t)length);
    if (!rc)
        rc = hapgpu_rt_sync(f->ctx->rt);
    hapgpu_rt_unlock(f->ctx->rt);
    return rc;
}

static void open_reader(hapf_reader *r, inspect_fetch *f, const void *frame, unsigned long bytes)
{
    /* classify without forcing a context into existence for plain host memory users */
    HapGpuContext *ctx = g_default;
    if (ctx && hapgpu_rt_is_device_ptr(ctx->rt, frame)) {
        hapf_reader_init_host(r, NULL, 0);
        f->ctx = ctx;
        f->frame = (const uint8_t *)frame;
        r->fetch = inspect_fetch_cb;
        r->user = f;
    } else {
        hapf_reader_init_host(r, frame, bytes);
    }
}

/* reference hap.c:1042-1087 (no NULL checks there either) */
unsigned int HapGetFrameTextureCount(const void *inputBuffer, unsigned long inputBufferBytes,
                                     unsigned int *outputTextureCount)
{
    hapf_reader r;
    inspect_fetch f;
    unsigned rc;
    open_reader(&r, &f, inputBuffer, inputBufferBytes);
    rc = hapf_texture_count(&r, inputBufferBytes, outputTextureCount);
    hapf_reader_free(&r);
    return rc;
}

/* reference hap.c:1089-1126 */
unsigned int HapGetFrameTextureFormat(const void *inputBuffer, unsigned long inputBufferBytes,
                                      unsigned int index, unsigned int *outputBufferTextureFormat)
{
    hapf_reader r;
    inspect_fetch f;
    uint64_t off;
    uint32_t len;
    unsigned type = 0, rc;
    if (!inputBuffer || index > 1 || !outputBufferTextureFormat)
        return HapResult_Bad_Arguments;
    open_reader(&r, &f, inputBuffer, inputBufferBytes);
    rc = hapf_locate(&r, (uint32_t)inputBufferBytes, index, &off, &len, &type);
    hapf_reader_free(&r);
    if (rc != HapResult_No_Error)
        return rc;
    *outputBufferTextureFormat = hapf_format_from_nibble(type & 0xFu);
    return *outputBufferTextureFormat ? HapResult_No_Error : HapResult_Bad_Frame;
}

/* reference hap.c:1128-1188 */
unsigned int HapGetFrameTextureChunkCount(const void *inputBuffer, unsigned long inputBufferBytes,
                                          unsigned int index, int *chunk_count)
{
    hapf_reader r;
    inspect_fetch f;
    hapf_texture_plan plan;
    *chunk_count = 0;                     /* before validation, like hap.c:1134 */
    if (!inputBuffer || index > 1)
        return HapResult_Bad_Arguments;
    open_reader(&r, &f, inputBuffer, inputBufferBytes);
    hapf_plan_texture(&r, (uint32_t)inputBufferBytes, index, 0, &plan);
    *chunk_count = plan.chunk_count;
    hapf_plan_free(&plan);
    hapf_reader_free(&r);
    return plan.result;
}

/* ----------------------------------------------------------- hap_gpu.h -- */

/* the whole-call refusal: every result set (a NULL results: none), Bad_Arguments returned */
static unsigned refuse_call(unsigned int *results, size_t count)
{
    size_t i;
    for (i = 0; results && i < count; i++)
        results[i] = HapResult_Bad_Arguments;
    return HapResult_Bad_Arguments;
}

/* a call down a road (hap_batch.h: HapbRoad) with the context's lock held: one texture, or frames */
static unsigned texture_down_road(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                  unsigned textureFormat, const void *alphaTexture, unsigned long alphaTextureBytes,
                                  unsigned width, unsigned height, void *picture, unsigned long rowBytes,
                                  const HapbRoad *road)
{
    unsigned r;
    hapgpu_rt_lock(context->rt);
    r = hapb_road_texture(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width, height,
                          picture, rowBytes, road);
    hapgpu_rt_unlock(context->rt);
    return r;
}

static unsigned frames_down_road(HapGpuContext *context, unsigned frameCount, const void *const *inputBuffers,
                                 const unsigned long *inputBuffersBytes, unsigned textureCount, void *const *pictures,
                                 unsigned width, unsigned height, unsigned long rowBytes, unsigned int *results,
                                 unsigned flags, const HapbRoad *road)
{
    unsigned r;
    hapgpu_rt_lock(context->rt);
    r = hapb_road_frames(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, pictures, width, height,
                         rowBytes, results, flags, road);
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* an encode call from a source (hap_batch.h: HapbSource): the context checked and its lock held; one texture, or frames */
static unsigned texture_from_source(HapGpuContext *context, const HapbSource *source, const void *picture,
                                    unsigned textureFormat, void *output, unsigned long outputBytes,
                                    unsigned long *outputBytesUsed, unsigned flags)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_source_texture(context, source, picture, textureFormat, output, outputBytes, outputBytesUsed, flags);
    hapgpu_rt_unlock(context->rt);
    return r;
}

static unsigned frames_from_source(HapGpuContext *context, const HapbSource *source, unsigned frameCount,
                                   const void *const *pictures, unsigned count, const unsigned *textureFormats,
                                   const unsigned *compressors, const unsigned *chunkCounts, void *const *outputBuffers,
                                   const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                   unsigned *results, unsigned flags, int defer)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_source_frames(context, source, frameCount, pictures, count, textureFormats, compressors, chunkCounts,
                           outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, defer);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuCompressRGBA(HapGpuContext *context, const void *rgba, unsigned int width,
                                unsigned int height, unsigned long rowBytes, unsigned int textureFormat,
                                void *output, unsigned long outputBytes, unsigned long *outputBytesUsed)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .width = width, .height = height, .row_bytes = rowBytes};
    return texture_from_source(context, &source, rgba, textureFormat, output, outputBytes, outputBytesUsed, 0u);
}

unsigned int HapGpuCompressRGBAFlags(HapGpuContext *context, const void *rgba, unsigned int width,
                                     unsigned int height, unsigned long rowBytes, unsigned int textureFormat,
                                     unsigned int flags, void *output, unsigned long outputBytes,
                                     unsigned long *outputBytesUsed)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .width = width, .height = height, .row_bytes = rowBytes};
    return texture_from_source(context, &source, rgba, textureFormat, output, outputBytes, outputBytesUsed, flags);
}

unsigned int HapGpuDecompressRGBA(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                  unsigned int textureFormat, const void *alphaTexture, unsigned long alphaBytes,
                                  unsigned int width, unsigned int height, void *rgba, unsigned long rowBytes)
{
    /* (one texture: BC7 is always taken; frames of it only with HAPGPU_DECODE_BPTC_PICTURES) */
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .bptc = 1};
    if (!context)
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaBytes, width, height, rgba,
                             rowBytes, &road);
}

/* one texture against its reference picture in device memory: the sums of the decoder's errors, no picture written */
unsigned int HapGpuMeasureTexture(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                  unsigned int textureFormat, const void *alphaTexture, unsigned long alphaTextureBytes,
                                  unsigned int width, unsigned int height, const void *rgba, unsigned long rowBytes,
                                  HapGpuPictureError *error)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .measure = error};
    if (!context || !error)
        return HapResult_Bad_Arguments;
    /* (the road's pictures are its third column whichever way the bytes go: this one only reads them) */
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width,
                             height, (void *)(uintptr_t)rgba, rowBytes, &road);
}

/* HapGpuDecompressRGBA of a block-aligned rectangle of the texture */
unsigned int HapGpuDecompressRGBARegion(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                        unsigned int textureFormat, const void *alphaTexture,
                                        unsigned long alphaTextureBytes, unsigned int width, unsigned int height,
                                        unsigned int regionX, unsigned int regionY, unsigned int regionWidth,
                                        unsigned int regionHeight, void *rgba, unsigned long rowBytes)
{
    const HapGpuRegion region = {width, regionX, regionY, regionWidth, regionHeight};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .bptc = 1, .region = &region};
    if (!context || !hapb_region_fits(&region, height))
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width,
                             height, rgba, rowBytes, &road);
}

/* HapGpuDecompressRGBA at half (scaleLog2 1) or quarter (2) size */
unsigned int HapGpuDecompressRGBAScaled(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                        unsigned int textureFormat, const void *alphaTexture,
                                        unsigned long alphaTextureBytes, unsigned int width, unsigned int height,
                                        unsigned int scaleLog2, void *rgba, unsigned long rowBytes)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .bptc = 1};
    if (!context || scaleLog2 < 1u || scaleLog2 > 2u)
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width,
                             height, rgba, rowBytes, &road);
}

/* one texture -> one NV12 video picture in device memory, at full, half or quarter size: the block decode of
   bc_decode_video.hip */
unsigned int HapGpuDecompressNV12(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                  unsigned int textureFormat, unsigned int width, unsigned int height,
                                  unsigned int scaleLog2, unsigned int matrix, unsigned int range, void *luma,
                                  unsigned long lumaRowBytes, void *chroma, unsigned long chromaRowBytes)
{
    const void *const chroma_plane = chroma;
    const HapbVideo video = {&chroma_plane, chromaRowBytes, matrix, range};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .video = &video};
    if (!context || !luma || !chroma || !hapb_video_decode_valid(width, height, scaleLog2, lumaRowBytes, &video))
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, NULL, 0ul, width, height, luma, lumaRowBytes,
                             &road);
}

/* 1: what the planar calls take of scaleLog2, channels, element, scale and bias */
static int planes_arguments_valid(unsigned scaleLog2, unsigned channels, unsigned element, const float *scale,
                                  const float *bias)
{
    return scaleLog2 <= 2u && channels >= 3u && channels <= 4u && element <= HapGpuPlaneElement_F32 && scale && bias;
}

/* one texture -> one planar float tensor in device memory */
unsigned int HapGpuDecompressPlanes(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                    unsigned int textureFormat, const void *alphaTexture,
                                    unsigned long alphaTextureBytes, unsigned int width, unsigned int height,
                                    unsigned int scaleLog2, unsigned int channels, unsigned int element, void *planes,
                                    unsigned long planeBytes, unsigned long rowBytes, const float *scale,
                                    const float *bias)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .planes = &layout};
    if (!context || !planes_arguments_valid(scaleLog2, channels, element, scale, bias))
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width,
                             height, planes, rowBytes, &road);
}

/* HapGpuDecompressPlanes of a block-aligned rectangle of the texture */
unsigned int HapGpuDecompressPlanesRegion(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                          unsigned int textureFormat, const void *alphaTexture,
                                          unsigned long alphaTextureBytes, unsigned int width, unsigned int height,
                                          unsigned int regionX, unsigned int regionY, unsigned int regionWidth,
                                          unsigned int regionHeight, unsigned int scaleLog2, unsigned int channels,
                                          unsigned int element, void *planes, unsigned long planeBytes,
                                          unsigned long rowBytes, const float *scale, const float *bias)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapGpuRegion region = {width, regionX, regionY, regionWidth, regionHeight};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .region = &region,
                           .planes = &layout};
    if (!context || !planes_arguments_valid(scaleLog2, channels, element, scale, bias) || !hapb_region_fits(&region, height))
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width,
                             height, planes, rowBytes, &road);
}

/* HapGpuDecompressPlanes of one crop of the scaled picture, at any texel position and size, resized to outWidth x
   outHeight */
unsigned int HapGpuDecompressPlanesResized(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                           unsigned int textureFormat, const void *alphaTexture,
                                           unsigned long alphaTextureBytes, unsigned int width, unsigned int height,
                                           unsigned int scaleLog2, unsigned int cropX, unsigned int cropY,
                                           unsigned int cropWidth, unsigned int cropHeight, unsigned int outWidth,
                                           unsigned int outHeight, unsigned int channels, unsigned int element,
                                           void *planes, unsigned long planeBytes, unsigned long rowBytes,
                                           const float *scale, const float *bias)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapbResize resize = {&cropX, &cropY, &cropWidth, &cropHeight, outWidth, outHeight};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .planes = &layout,
                           .resize = &resize};
    HapGpuRegion blocks;
    if (!context || !planes_arguments_valid(scaleLog2, channels, element, scale, bias) || (width & 3u) || (height & 3u) ||
        !hapb_resize_out_valid(&resize) || !hapb_resize_region(&resize, 0u, width, height, scaleLog2, &blocks))
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width,
                             height, planes, rowBytes, &road);
}

unsigned int HapGpuDecompressRGBAHalf(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                      unsigned int textureFormat, unsigned int width, unsigned int height,
                                      void *rgbaHalf, unsigned long rowBytes)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA16F};
    if (!context)
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, textureFormat, NULL, 0, width, height, rgbaHalf, rowBytes,
                             &road);
}

unsigned int HapGpuEncodeFrames(HapGpuContext *context, unsigned int frameCount, unsigned int count,
                                const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                const unsigned int *textureFormats, const unsigned int *compressors,
                                const unsigned int *chunkCounts, void *const *outputBuffers,
                                const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                unsigned int *results, unsigned int flags)
{
    unsigned r = HapResult_No_Error, done;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    /* (the kernels index frames with a grid dimension that holds 65535: larger batches go in slices) */
    if (frameCount <= HAP_SLICE_ENTRIES || !inputBuffers || !outputBuffers || !outputBuffersBytes || !outputBuffersBytesUsed || !results ||
        count == 0 || count > 2) {
        r = hapb_encode(context, frameCount, count, inputBuffers, inputBuffersBytes, textureFormats, compressors,
                        chunkCounts, outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, NULL);
    } else {
        for (done = 0; done < frameCount; done += HAP_SLICE_ENTRIES) {
            const unsigned n = frameCount - done < HAP_SLICE_ENTRIES ? frameCount - done : HAP_SLICE_ENTRIES;
            const unsigned rc = hapb_encode(context, n, count, inputBuffers + (size_t)done * count, inputBuffersBytes, textureFormats,
                                            compressors, chunkCounts, outputBuffers + done, outputBuffersBytes + done,
                                            outputBuffersBytesUsed + done, results + done, flags, NULL);
            if (r == HapResult_No_Error)
                r = rc;
        }
    }
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuEncodeFramesRGBA(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *rgbaFrames, unsigned int width, unsigned int height,
                                    unsigned long rowBytes, unsigned int count,
                                    const unsigned int *textureFormats, const unsigned int *compressors,
                                    const unsigned int *chunkCounts, void *const *outputBuffers,
                                    const unsigned long *outputBuffersBytes,
                                    unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                    unsigned int flags)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .width = width, .height = height, .row_bytes = rowBytes};
    return frames_from_source(context, &source, frameCount, rgbaFrames, count, textureFormats, compressors, chunkCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 0);
}

/* The two halves of HapGpuEncodeFramesRGBA / HapGpuEncodeFrames (include/hap_gpu.h): everything launched, nothing waited for. */
unsigned int HapGpuEncodeFramesRGBABegin(HapGpuContext *context, unsigned int frameCount,
                                         const void *const *rgbaFrames, unsigned int width, unsigned int height,
                                         unsigned long rowBytes, unsigned int count,
                                         const unsigned int *textureFormats, const unsigned int *compressors,
                                         const unsigned int *chunkCounts, void *const *outputBuffers,
                                         const unsigned long *outputBuffersBytes,
                                         unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                         unsigned int flags)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .width = width, .height = height, .row_bytes = rowBytes};
    return frames_from_source(context, &source, frameCount, rgbaFrames, count, textureFormats, compressors, chunkCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 1);
}

/* Planar float tensors -> textures and frames: the RGBA calls with the block encode of bc_encode_planes.hip */
unsigned int HapGpuCompressPlanes(HapGpuContext *context, const void *planes, unsigned long planeBytes,
                                  unsigned long rowBytes, unsigned int channels, unsigned int element,
                                  const float *scale, const float *bias, unsigned int width, unsigned int height,
                                  unsigned int textureFormat, void *output, unsigned long outputBytes,
                                  unsigned long *outputBytesUsed)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .planes = &layout, .width = width, .height = height,
                               .row_bytes = rowBytes};
    if (!planes || !output || !hapb_planes_encode_valid(width, height, rowBytes, &layout, 1u, &textureFormat))
        return HapResult_Bad_Arguments;
    return texture_from_source(context, &source, planes, textureFormat, output, outputBytes, outputBytesUsed, 0u);
}

/* what does not depend on a frame or on the context, checked before either is looked at: 0 = in order; else every
   results[f] is Bad_Arguments */
static unsigned planes_encode_refused(unsigned frameCount, const void *const *planeFrames, const HapbPlanes *layout,
                                      unsigned long rowBytes, unsigned width, unsigned height, unsigned count,
                                      const unsigned *textureFormats, const unsigned *compressors,
                                      const unsigned *chunkCounts, void *const *outputBuffers,
                                      const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                      unsigned *results)
{
    if (results && planeFrames && compressors && chunkCounts && outputBuffers && outputBuffersBytes &&
        outputBuffersBytesUsed && hapb_planes_encode_valid(width, height, rowBytes, layout, count, textureFormats))
        return 0u;
    refuse_call(results, frameCount);
    return 1u;
}

unsigned int HapGpuEncodeFramesPlanes(HapGpuContext *context, unsigned int frameCount,
                                      const void *const *planeFrames, unsigned int channels, unsigned int element,
                                      unsigned long planeBytes, unsigned long rowBytes, const float *scale,
                                      const float *bias, unsigned int width, unsigned int height, unsigned int count,
                                      const unsigned int *textureFormats, const unsigned int *compressors,
                                      const unsigned int *chunkCounts, void *const *outputBuffers,
                                      const unsigned long *outputBuffersBytes,
                                      unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                      unsigned int flags)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .planes = &layout, .width = width, .height = height,
                               .row_bytes = rowBytes};
    if (planes_encode_refused(frameCount, planeFrames, &layout, rowBytes, width, height, count, textureFormats, compressors,
                              chunkCounts, outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results))
        return HapResult_Bad_Arguments;
    return frames_from_source(context, &source, frameCount, planeFrames, count, textureFormats, compressors, chunkCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 0);
}

unsigned int HapGpuEncodeFramesPlanesBegin(HapGpuContext *context, unsigned int frameCount,
                                           const void *const *planeFrames, unsigned int channels,
                                           unsigned int element, unsigned long planeBytes, unsigned long rowBytes,
                                           const float *scale, const float *bias, unsigned int width,
                                           unsigned int height, unsigned int count,
                                           const unsigned int *textureFormats, const unsigned int *compressors,
                                           const unsigned int *chunkCounts, void *const *outputBuffers,
                                           const unsigned long *outputBuffersBytes,
                                           unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                           unsigned int flags)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .planes = &layout, .width = width, .height = height,
                               .row_bytes = rowBytes};
    if (frameCount > HAP_SLICE_ENTRIES ||
        planes_encode_refused(frameCount, planeFrames, &layout, rowBytes, width, height, count, textureFormats, compressors,
                              chunkCounts, outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results))
        return HapResult_Bad_Arguments;
    return frames_from_source(context, &source, frameCount, planeFrames, count, textureFormats, compressors, chunkCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 1);
}

/* NV12 video pictures -> textures and frames: the RGBA calls with the block encode of bc_encode_video.hip */
unsigned int HapGpuCompressNV12(HapGpuContext *context, const void *luma, unsigned long lumaRowBytes,
                                const void *chroma, unsigned long chromaRowBytes, unsigned int matrix,
                                unsigned int range, unsigned int width, unsigned int height,
                                unsigned int textureFormat, void *output, unsigned long outputBytes,
                                unsigned long *outputBytesUsed)
{
    const HapbVideo video = {&chroma, chromaRowBytes, matrix, range};
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .video = &video, .width = width, .height = height,
                               .row_bytes = lumaRowBytes};
    if (!luma || !chroma || !output || !hapb_video_encode_valid(width, height, lumaRowBytes, &video, 1u, &textureFormat))
        return HapResult_Bad_Arguments;
    return texture_from_source(context, &source, luma, textureFormat, output, outputBytes, outputBytesUsed, 0u);
}

/* what does not depend on a frame or on the context, checked before either is looked at: 0 = in order; else every
   results[f] is Bad_Arguments */
static unsigned video_encode_refused(unsigned frameCount, const void *const *lumaPlanes, const HapbVideo *video,
                                     unsigned long lumaRowBytes, unsigned width, unsigned height, unsigned count,
                                     const unsigned *textureFormats, const unsigned *compressors,
                                     const unsigned *chunkCounts, void *const *outputBuffers,
                                     const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                     unsigned *results)
{
    if (results && lumaPlanes && video->chroma && compressors && chunkCounts && outputBuffers && outputBuffersBytes &&
        outputBuffersBytesUsed && hapb_video_encode_valid(width, height, lumaRowBytes, video, count, textureFormats))
        return 0u;
    refuse_call(results, frameCount);
    return 1u;
}

unsigned int HapGpuEncodeFramesNV12(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *lumaPlanes, unsigned long lumaRowBytes,
                                    const void *const *chromaPlanes, unsigned long chromaRowBytes,
                                    unsigned int matrix, unsigned int range, unsigned int width, unsigned int height,
                                    unsigned int count, const unsigned int *textureFormats,
                                    const unsigned int *compressors, const unsigned int *chunkCounts,
                                    void *const *outputBuffers, const unsigned long *outputBuffersBytes,
                                    unsigned long *outputBuffersBytesUsed, unsigned int *results, unsigned int flags)
{
    const HapbVideo video = {chromaPlanes, chromaRowBytes, matrix, range};
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .video = &video, .width = width, .height = height,
                               .row_bytes = lumaRowBytes};
    if (video_encode_refused(frameCount, lumaPlanes, &video, lumaRowBytes, width, height, count, textureFormats, compressors,
                             chunkCounts, outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results))
        return HapResult_Bad_Arguments;
    return frames_from_source(context, &source, frameCount, lumaPlanes, count, textureFormats, compressors, chunkCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 0);
}

unsigned int HapGpuEncodeFramesNV12Begin(HapGpuContext *context, unsigned int frameCount,
                                         const void *const *lumaPlanes, unsigned long lumaRowBytes,
                                         const void *const *chromaPlanes, unsigned long chromaRowBytes,
                                         unsigned int matrix, unsigned int range, unsigned int width,
                                         unsigned int height, unsigned int count, const unsigned int *textureFormats,
                                         const unsigned int *compressors, const unsigned int *chunkCounts,
                                         void *const *outputBuffers, const unsigned long *outputBuffersBytes,
                                         unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                         unsigned int flags)
{
    const HapbVideo video = {chromaPlanes, chromaRowBytes, matrix, range};
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA8, .video = &video, .width = width, .height = height,
                               .row_bytes = lumaRowBytes};
    if (frameCount > HAP_SLICE_ENTRIES ||
        video_encode_refused(frameCount, lumaPlanes, &video, lumaRowBytes, width, height, count, textureFormats, compressors,
                             chunkCounts, outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results))
        return HapResult_Bad_Arguments;
    return frames_from_source(context, &source, frameCount, lumaPlanes, count, textureFormats, compressors, chunkCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 1);
}

/* RGBA16F pictures -> Hap HDR: the RGBA calls with 8-byte texels and one BC6H texture per frame */
unsigned int HapGpuCompressRGBAHalf(HapGpuContext *context, const void *rgbaHalf, unsigned int width,
                                    unsigned int height, unsigned long rowBytes, unsigned int textureFormat,
                                    void *output, unsigned long outputBytes, unsigned long *outputBytesUsed)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA16F, .width = width, .height = height, .row_bytes = rowBytes};
    return texture_from_source(context, &source, rgbaHalf, textureFormat, output, outputBytes, outputBytesUsed, 0u);
}

unsigned int HapGpuEncodeFramesRGBAHalf(HapGpuContext *context, unsigned int frameCount,
                                        const void *const *rgbaHalfFrames, unsigned int width, unsigned int height,
                                        unsigned long rowBytes, unsigned int textureFormat, unsigned int compressor,
                                        unsigned int chunkCount, void *const *outputBuffers,
                                        const unsigned long *outputBuffersBytes,
                                        unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                        unsigned int flags)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA16F, .width = width, .height = height, .row_bytes = rowBytes};
    return frames_from_source(context, &source, frameCount, rgbaHalfFrames, 1u, &textureFormat, &compressor, &chunkCount,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 0);
}

unsigned int HapGpuEncodeFramesRGBAHalfBegin(HapGpuContext *context, unsigned int frameCount,
                                             const void *const *rgbaHalfFrames, unsigned int width, unsigned int height,
                                             unsigned long rowBytes, unsigned int textureFormat, unsigned int compressor,
                                             unsigned int chunkCount, void *const *outputBuffers,
                                             const unsigned long *outputBuffersBytes,
                                             unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                             unsigned int flags)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_RGBA16F, .width = width, .height = height, .row_bytes = rowBytes};
    return frames_from_source(context, &source, frameCount, rgbaHalfFrames, 1u, &textureFormat, &compressor, &chunkCount,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 1);
}

/* A8 pictures -> Hap Alpha-Only: the RGBA calls with 1-byte texels and one RGTC1 texture per frame */
unsigned int HapGpuCompressAlpha(HapGpuContext *context, const void *alpha, unsigned int width, unsigned int height,
                                 unsigned long rowBytes, void *output, unsigned long outputBytes,
                                 unsigned long *outputBytesUsed)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_A8, .width = width, .height = height, .row_bytes = rowBytes};
    return texture_from_source(context, &source, alpha, HapTextureFormat_A_RGTC1, output, outputBytes, outputBytesUsed, 0u);
}

unsigned int HapGpuDecompressAlpha(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                   unsigned int width, unsigned int height, void *alpha, unsigned long rowBytes)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_A8};
    if (!context)
        return HapResult_Bad_Arguments;
    return texture_down_road(context, texture, textureBytes, HapTextureFormat_A_RGTC1, NULL, 0, width, height, alpha,
                             rowBytes,
                             &road);
}

unsigned int HapGpuEncodeFramesAlpha(HapGpuContext *context, unsigned int frameCount, const void *const *alphaFrames,
                                     unsigned int width, unsigned int height, unsigned long rowBytes,
                                     unsigned int compressor, unsigned int chunkCount, void *const *outputBuffers,
                                     const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                     unsigned int *results, unsigned int flags)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_A8, .width = width, .height = height, .row_bytes = rowBytes};
    const unsigned format = HapTextureFormat_A_RGTC1;
    return frames_from_source(context, &source, frameCount, alphaFrames, 1u, &format, &compressor, &chunkCount,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 0);
}

unsigned int HapGpuEncodeFramesAlphaBegin(HapGpuContext *context, unsigned int frameCount,
                                          const void *const *alphaFrames, unsigned int width, unsigned int height,
                                          unsigned long rowBytes, unsigned int compressor, unsigned int chunkCount,
                                          void *const *outputBuffers, const unsigned long *outputBuffersBytes,
                                          unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                          unsigned int flags)
{
    const HapbSource source = {.picture_kind = HAPGPU_PICTURE_A8, .width = width, .height = height, .row_bytes = rowBytes};
    const unsigned format = HapTextureFormat_A_RGTC1;
    return frames_from_source(context, &source, frameCount, alphaFrames, 1u, &format, &compressor, &chunkCount,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, 1);
}

unsigned int HapGpuEncodeFramesBegin(HapGpuContext *context, unsigned int frameCount, unsigned int count,
                                     const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                     const unsigned int *textureFormats, const unsigned int *compressors,
                                     const unsigned int *chunkCounts, void *const *outputBuffers,
                                     const unsigned long *outputBuffersBytes,
                                     unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                     unsigned int flags)
{
    const HapbEncodeArgs deferred = {0, NULL, 1, 0};
    unsigned r;
    if (!context || frameCount > HAP_SLICE_ENTRIES)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_encode(context, frameCount, count, inputBuffers, inputBuffersBytes, textureFormats, compressors, chunkCounts,
                    outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, results, flags, &deferred);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuEncodeFramesFinish(HapGpuContext *context)
{
    unsigned r = HapResult_No_Error;
    HapbEncodePending *pd;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    pd = context->pending_encode;
    context->pending_encode = NULL;
    if (pd)
        r = hapb_encode_complete(context, pd);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuDecodeFrames(HapGpuContext *context, unsigned int frameCount,
                                const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                unsigned int index, void *const *outputBuffers,
                                const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                unsigned int *outputTextureFormats, unsigned int *results, unsigned int flags)
{
    unsigned r = HapResult_No_Error, done;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    if (frameCount <= HAP_SLICE_ENTRIES || !inputBuffers || !inputBuffersBytes || !outputBuffers || !outputBuffersBytes || !results) {
        r = hapb_decode(context, frameCount, inputBuffers, inputBuffersBytes, index, outputBuffers,
                        outputBuffersBytes, outputBuffersBytesUsed, outputTextureFormats, results, flags, NULL);
    } else {
        for (done = 0; done < frameCount; done += HAP_SLICE_ENTRIES) {
            const unsigned n = frameCount - done < HAP_SLICE_ENTRIES ? frameCount - done : HAP_SLICE_ENTRIES;
            const unsigned rc = hapb_decode(context, n, inputBuffers + done, inputBuffersBytes + done, index, outputBuffers + done,
                                            outputBuffersBytes + done, outputBuffersBytesUsed ? outputBuffersBytesUsed + done : NULL,
                                            outputTextureFormats ? outputTextureFormats + done : NULL, results + done, flags, NULL);
            if (r == HapResult_No_Error)
                r = rc;
        }
    }
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuDecodeFrameTextures(HapGpuContext *context, unsigned int frameCount,
                                       const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                       unsigned int textureCount, void *const *outputBuffers,
                                       const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                       unsigned int *outputTextureFormats, unsigned int *results, unsigned int flags)
{
    unsigned r = HapResult_No_Error, f, t;
    const void **inputs;
    unsigned long *bytes;
    unsigned *indices;
    size_t entries, done;
    if (!context || !results || textureCount == 0 || textureCount > 2)
        return HapResult_Bad_Arguments;
    if (frameCount == 0)
        return HapResult_No_Error;
    entries = (size_t)frameCount * textureCount;
    if (!inputBuffers || !inputBuffersBytes || !outputBuffers || !outputBuffersBytes) {
        for (done = 0; done < entries; done++)
            results[done] = HapResult_Bad_Arguments;
        return HapResult_Bad_Arguments;
    }
    /* entry f * textureCount + t = texture t of frame f: one batch, so the frames' headers come to the host once
       and every texture's units go out in the same launches */
    inputs = (const void **)malloc(sizeof(*inputs) * entries);
    bytes = (unsigned long *)malloc(sizeof(*bytes) * entries);
    indices = (unsigned *)malloc(sizeof(*indices) * entries);
    if (!inputs || !bytes || !indices) {
        free(inputs); free(bytes); free(indices);
        for (done = 0; done < entries; done++)
            results[done] = HapResult_Internal_Error;
        return HapResult_Internal_Error;
    }
    for (f = 0; f < frameCount; f++)
        for (t = 0; t < textureCount; t++) {
            inputs[(size_t)f * textureCount + t] = inputBuffers[f];
            bytes[(size_t)f * textureCount + t] = inputBuffersBytes[f];
            indices[(size_t)f * textureCount + t] = t;
        }
    hapgpu_rt_lock(context->rt);
    for (done = 0; done < entries; done += HAP_SLICE_ENTRIES) {
        const unsigned n = (unsigned)(entries - done < HAP_SLICE_ENTRIES ? entries - done : HAP_SLICE_ENTRIES);
        const HapbDecodeArgs entries_of = {indices + done, NULL, NULL, 0, NULL, 0u, NULL, NULL};
        const unsigned rc = hapb_decode(context, n, inputs + done, bytes + done, 0, outputBuffers + done, outputBuffersBytes + done,
                                        outputBuffersBytesUsed ? outputBuffersBytesUsed + done : NULL,
                                        outputTextureFormats ? outputTextureFormats + done : NULL, results + done, flags,
                                        &entries_of);
        if (r == HapResult_No_Error)
            r = rc;
    }
    hapgpu_rt_unlock(context->rt);
    free(inputs); free(bytes); free(indices);
    return r;
}

unsigned int HapGpuDecodeFramesRGBA(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                    unsigned int textureCount, void *const *rgbaFrames, unsigned int width,
                                    unsigned int height, unsigned long rowBytes, unsigned int *results,
                                    unsigned int flags)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .bptc = (flags & HAPGPU_DECODE_BPTC_PICTURES) != 0};
    if (!context)
        return HapResult_Bad_Arguments;
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, rgbaFrames, width, height,
                            rowBytes, results, flags, &road);
}

/* frames against their reference pictures in device memory; a NULL errors refuses the whole call like a NULL results */
unsigned int HapGpuMeasureFrames(HapGpuContext *context, unsigned int frameCount, const void *const *inputBuffers,
                                 const unsigned long *inputBuffersBytes, unsigned int textureCount,
                                 const void *const *rgbaFrames, unsigned int width, unsigned int height,
                                 unsigned long rowBytes, HapGpuPictureError *errors, unsigned int *results,
                                 unsigned int flags)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .measure = errors};
    if (!context)
        return HapResult_Bad_Arguments;
    if (!errors)
        return refuse_call(results, frameCount);
    /* (the road's pictures are its third column whichever way the bytes go: this one only reads them.  Hap R frames
       are out of scope with or without the flag that asks for their pictures) */
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, (void *const *)rgbaFrames,
                            width, height, rowBytes, results,
                            flags & ~HAPGPU_DECODE_BPTC_PICTURES, &road);
}

/* layers of textures over a background colour: one picture, no decoded layer in between */
unsigned int HapGpuCompositeTextures(HapGpuContext *context, unsigned int layerCount, const void *const *textures,
                                     const unsigned long *texturesBytes, const unsigned int *textureFormats,
                                     const void *const *alphaTextures, const unsigned long *alphaTexturesBytes,
                                     const unsigned char *opacities, const unsigned char *background, unsigned int width,
                                     unsigned int height, void *rgba, unsigned long rowBytes)
{
    const HapbComposite composite = {.layer_count = layerCount, .width = width, .height = height, .background = background,
                                     .opacities = opacities, .row_bytes = rowBytes};
    void *const picture[1] = {rgba};
    unsigned r;
    /* (what is wrong with the call whatever its layers hold is seen before the context is looked at) */
    if (!context || !textures || !texturesBytes || !textureFormats || !rgba || !hapb_composite_valid(&composite, 1u, NULL, 0))
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_composite_textures(context, &composite, textures, texturesBytes, textureFormats, alphaTextures,
                                alphaTexturesBytes, picture, NULL, NULL);
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* layers of frames over a background colour: one picture per output frame; a NULL results refuses the whole call, and
   so does anything wrong with it whatever its frames hold -- every result set, before the context is looked at */
unsigned int HapGpuCompositeFrames(HapGpuContext *context, unsigned int frameCount, unsigned int layerCount,
                                   const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                   const unsigned int *textureCounts, const unsigned char *opacities,
                                   const unsigned char *background, void *const *rgbaFrames, unsigned int width,
                                   unsigned int height, unsigned long rowBytes, unsigned int *results, unsigned int flags)
{
    const HapbComposite composite = {.layer_count = layerCount, .width = width, .height = height, .background = background,
                                     .opacities = opacities, .row_bytes = rowBytes};
    unsigned r;
    if (!context || !results)
        return HapResult_Bad_Arguments;
    if (!inputBuffers || !inputBuffersBytes || !rgbaFrames || !hapb_composite_valid(&composite, frameCount, textureCounts, 1))
        return refuse_call(results, (size_t)frameCount * layerCount);
    hapgpu_rt_lock(context->rt);
    r = hapb_composite_frames(context, &composite, frameCount, inputBuffers, inputBuffersBytes, textureCounts, rgbaFrames,
                              NULL, NULL, results, NULL, flags);
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* ... with layers of sizes of their own, placed and clipped on the canvas: a layer size or a placement that is not in
   order refuses the call like everything above, before the context is looked at */
unsigned int HapGpuCompositeTexturesPlaced(HapGpuContext *context, unsigned int layerCount, const void *const *textures,
                                           const unsigned long *texturesBytes, const unsigned int *textureFormats,
                                           const void *const *alphaTextures, const unsigned long *alphaTexturesBytes,
                                           const unsigned int *layerWidths, const unsigned int *layerHeights,
                                           const HapGpuPlacement *placements, const unsigned char *opacities,
                                           const unsigned char *background, unsigned int width, unsigned int height,
                                           void *rgba, unsigned long rowBytes)
{
    const HapbComposite composite = {.layer_count = layerCount, .width = width, .height = height, .background = background,
                                     .opacities = opacities, .layer_widths = layerWidths, .layer_heights = layerHeights,
                                     .placements = placements, .row_bytes = rowBytes};
    void *const picture[1] = {rgba};
    unsigned r;
    /* (a description without layer sizes is the call above: this one has them) */
    if (!context || !textures || !texturesBytes || !textureFormats || !rgba || !layerWidths ||
        !hapb_composite_valid(&composite, 1u, NULL, 0))
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_composite_textures(context, &composite, textures, texturesBytes, textureFormats, alphaTextures,
                                alphaTexturesBytes, picture, NULL, NULL);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuCompositeFramesPlaced(HapGpuContext *context, unsigned int frameCount, unsigned int layerCount,
                                         const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                         const unsigned int *textureCounts, const unsigned int *layerWidths,
                                         const unsigned int *layerHeights, const HapGpuPlacement *placements,
                                         const unsigned char *opacities, const unsigned char *background,
                                         void *const *rgbaFrames, unsigned int width, unsigned int height,
                                         unsigned long rowBytes, unsigned int *results, unsigned int flags)
{
    const HapbComposite composite = {.layer_count = layerCount, .width = width, .height = height, .background = background,
                                     .opacities = opacities, .layer_widths = layerWidths, .layer_heights = layerHeights,
                                     .placements = placements, .row_bytes = rowBytes};
    unsigned r;
    if (!results)
        return HapResult_Bad_Arguments;
    /* (what is wrong with the call itself sets every result whatever the context is, a NULL one included) */
    if (!inputBuffers || !inputBuffersBytes || !rgbaFrames || !layerWidths ||
        !hapb_composite_valid(&composite, frameCount, textureCounts, 1))
        return refuse_call(results, (size_t)frameCount * layerCount);
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_composite_frames(context, &composite, frameCount, inputBuffers, inputBuffersBytes, textureCounts, rgbaFrames,
                              NULL, NULL, results, NULL, flags);
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* ... with the canvas encoded to textures, and to frames, instead of written as a picture: what is wrong with the call
   itself -- the placed calls' refusals, a destination set the kernel does not make, what the encoder refuses of the
   formats, compressors and chunk counts, a NULL results or layerResults -- is seen before the context is looked at, and
   sets every entry of every result array there is */
unsigned int HapGpuCompositeTexturesEncoded(HapGpuContext *context, unsigned int layerCount, const void *const *textures,
                                            const unsigned long *texturesBytes, const unsigned int *textureFormats,
                                            const void *const *alphaTextures, const unsigned long *alphaTexturesBytes,
                                            const unsigned int *layerWidths, const unsigned int *layerHeights,
                                            const HapGpuPlacement *placements, const unsigned char *opacities,
                                            const unsigned char *background, unsigned int width, unsigned int height,
                                            unsigned int count, const unsigned int *outputFormats, void *const *outputs,
                                            const unsigned long *outputsBytes, unsigned long *outputsBytesUsed)
{
    const HapbComposite composite = {.layer_count = layerCount, .width = width, .height = height, .background = background,
                                     .opacities = opacities, .layer_widths = layerWidths, .layer_heights = layerHeights,
                                     .placements = placements, .encoded = 1, .count = count, .formats = outputFormats};
    unsigned r;
    if (!context || !textures || !texturesBytes || !textureFormats || !outputs || !outputsBytes ||
        !hapb_composite_valid(&composite, 1u, NULL, 0))
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_composite_textures(context, &composite, textures, texturesBytes, textureFormats, alphaTextures,
                                alphaTexturesBytes, outputs, outputsBytes, outputsBytesUsed);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuCompositeFramesEncoded(HapGpuContext *context, unsigned int frameCount, unsigned int layerCount,
                                          const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                          const unsigned int *textureCounts, const unsigned int *layerWidths,
                                          const unsigned int *layerHeights, const HapGpuPlacement *placements,
                                          const unsigned char *opacities, const unsigned char *background,
                                          unsigned int width, unsigned int height, unsigned int count,
                                          const unsigned int *textureFormats, const unsigned int *compressors,
                                          const unsigned int *chunkCounts, void *const *outputBuffers,
                                          const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                          unsigned int *layerResults, unsigned int *results, unsigned int decodeFlags,
                                          unsigned int encodeFlags)
{
    const HapbComposite composite = {.layer_count = layerCount, .width = width, .height = height, .background = background,
                                     .opacities = opacities, .layer_widths = layerWidths, .layer_heights = layerHeights,
                                     .placements = placements, .encoded = 1, .count = count, .formats = textureFormats,
                                     .compressors = compressors, .chunk_counts = chunkCounts, .encode_flags = encodeFlags};
    unsigned r;
    if (!results || !layerResults || !inputBuffers || !inputBuffersBytes || !outputBuffers || !outputBuffersBytes ||
        !outputBuffersBytesUsed || !hapb_composite_valid(&composite, frameCount, textureCounts, 1)) {
        refuse_call(layerResults, (size_t)frameCount * layerCount);
        return refuse_call(results, frameCount);
    }
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_composite_frames(context, &composite, frameCount, inputBuffers, inputBuffersBytes, textureCounts,
                              outputBuffers, outputBuffersBytes, outputBuffersBytesUsed, layerResults, results, decodeFlags);
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* HapGpuDecodeFramesRGBA of a block-aligned rectangle of every frame; any other rectangle refuses the whole call */
unsigned int HapGpuDecodeFramesRGBARegion(HapGpuContext *context, unsigned int frameCount,
                                          const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                          unsigned int textureCount, void *const *rgbaFrames, unsigned int width,
                                          unsigned int height, unsigned int regionX, unsigned int regionY,
                                          unsigned int regionWidth, unsigned int regionHeight, unsigned long rowBytes,
                                          unsigned int *results, unsigned int flags)
{
    const HapGpuRegion region = {width, regionX, regionY, regionWidth, regionHeight};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .bptc = (flags & HAPGPU_DECODE_BPTC_PICTURES) != 0,
                           .region = &region};
    if (!context)
        return HapResult_Bad_Arguments;
    if (!hapb_region_fits(&region, height))
        return refuse_call(results, frameCount);
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, rgbaFrames, width, height,
                            rowBytes, results, flags, &road);
}

/* HapGpuDecodeFramesRGBA at half (scaleLog2 1) or quarter (2) size; any other scale refuses the whole call */
unsigned int HapGpuDecodeFramesRGBAScaled(HapGpuContext *context, unsigned int frameCount,
                                          const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                          unsigned int textureCount, void *const *rgbaFrames, unsigned int width,
                                          unsigned int height, unsigned int scaleLog2, unsigned long rowBytes,
                                          unsigned int *results, unsigned int flags)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2,
                           .bptc = (flags & HAPGPU_DECODE_BPTC_PICTURES) != 0};
    if (!context)
        return HapResult_Bad_Arguments;
    /* (the road underneath takes scale 0: that is HapGpuDecodeFramesRGBA's to ask for) */
    if (scaleLog2 < 1u || scaleLog2 > 2u)
        return refuse_call(results, frameCount);
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, rgbaFrames, width, height,
                            rowBytes, results, flags, &road);
}

/* frames -> NV12 video pictures in device memory; arguments outside the rules refuse the whole call, before the
   context is looked at */
unsigned int HapGpuDecodeFramesNV12(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                    unsigned int textureCount, void *const *lumaPlanes, unsigned long lumaRowBytes,
                                    void *const *chromaPlanes, unsigned long chromaRowBytes, unsigned int matrix,
                                    unsigned int range, unsigned int width, unsigned int height,
                                    unsigned int scaleLog2, unsigned int *results, unsigned int flags)
{
    const HapbVideo video = {(const void *const *)chromaPlanes, chromaRowBytes, matrix, range};
    /* (Hap R frames are out of scope with or without the flag that asks for their pictures: the road has no BC7) */
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .video = &video};
    if (!results)
        return HapResult_Bad_Arguments;
    if (!inputBuffers || !inputBuffersBytes || !lumaPlanes || !chromaPlanes || textureCount == 0 || textureCount > 2 ||
        !hapb_video_decode_valid(width, height, scaleLog2, lumaRowBytes, &video))
        return refuse_call(results, frameCount);
    if (!context)
        return HapResult_Bad_Arguments;
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, lumaPlanes, width, height,
                            lumaRowBytes, results, flags & ~HAPGPU_DECODE_BPTC_PICTURES, &road);
}

/* frames -> planar float tensors in device memory; arguments outside the rules refuse the whole call */
unsigned int HapGpuDecodeFramesPlanes(HapGpuContext *context, unsigned int frameCount,
                                      const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                      unsigned int textureCount, void *const *planeFrames, unsigned int width,
                                      unsigned int height, unsigned int scaleLog2, unsigned int channels,
                                      unsigned int element, unsigned long planeBytes, unsigned long rowBytes,
                                      const float *scale, const float *bias, unsigned int *results, unsigned int flags)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    /* (Hap R frames are out of scope with or without the flag that asks for their pictures: the road has no BC7) */
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .planes = &layout};
    if (!context)
        return HapResult_Bad_Arguments;
    if (!planes_arguments_valid(scaleLog2, channels, element, scale, bias))
        return refuse_call(results, frameCount);
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, planeFrames, width,
                            height, rowBytes, results, flags, &road);
}

/* HapGpuDecodeFramesPlanes of a block-aligned rectangle of every frame, frame f's at (regionXs[f], regionYs[f]); a size
   that is no rectangle of the frames refuses the whole call, an origin that puts it outside refuses its frame */
unsigned int HapGpuDecodeFramesPlanesRegion(HapGpuContext *context, unsigned int frameCount,
                                            const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                            unsigned int textureCount, void *const *planeFrames, unsigned int width,
                                            unsigned int height, const unsigned int *regionXs,
                                            const unsigned int *regionYs, unsigned int regionWidth,
                                            unsigned int regionHeight, unsigned int scaleLog2, unsigned int channels,
                                            unsigned int element, unsigned long planeBytes, unsigned long rowBytes,
                                            const float *scale, const float *bias, unsigned int *results,
                                            unsigned int flags)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapGpuRegion size = {width, 0u, 0u, regionWidth, regionHeight};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .region = &size,
                           .region_xs = regionXs, .region_ys = regionYs, .planes = &layout};
    if (!context)
        return HapResult_Bad_Arguments;
    /* (without origins the road would be the one-rectangle road at (0, 0)) */
    if (!planes_arguments_valid(scaleLog2, channels, element, scale, bias) || !regionXs || !regionYs ||
        !hapb_region_fits(&size, height))
        return refuse_call(results, frameCount);
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, planeFrames, width,
                            height, rowBytes, results, flags, &road);
}

/* HapGpuDecodeFramesPlanes of a crop per frame of the scaled picture, at any texel position and size, every one resized
   to outWidth x outHeight; a NULL crop array or an output size outside 1 .. 16384 refuses the whole call, a crop that is
   empty, past an edge or more than 4 x the output refuses its frame */
unsigned int HapGpuDecodeFramesPlanesResized(HapGpuContext *context, unsigned int frameCount,
                                             const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                             unsigned int textureCount, void *const *planeFrames, unsigned int width,
                                             unsigned int height, unsigned int scaleLog2, const unsigned int *cropXs,
                                             const unsigned int *cropYs, const unsigned int *cropWidths,
                                             const unsigned int *cropHeights, unsigned int outWidth,
                                             unsigned int outHeight, unsigned int channels, unsigned int element,
                                             unsigned long planeBytes, unsigned long rowBytes, const float *scale,
                                             const float *bias, unsigned int *results, unsigned int flags)
{
    const HapbPlanes layout = {channels, element, planeBytes, scale, bias};
    const HapbResize resize = {cropXs, cropYs, cropWidths, cropHeights, outWidth, outHeight};
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8, .scale_log2 = scaleLog2, .planes = &layout,
                           .resize = &resize};
    if (!context)
        return HapResult_Bad_Arguments;
    if (!planes_arguments_valid(scaleLog2, channels, element, scale, bias) || !cropXs || !cropYs || !cropWidths ||
        !cropHeights || !hapb_resize_out_valid(&resize))
        return refuse_call(results, frameCount);
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, textureCount, planeFrames, width,
                            height, rowBytes, results, flags, &road);
}

/* texture(s) -> texture(s) and frames -> frames of another flavour or size, without a picture in between */
unsigned int HapGpuTranscodeTexture(HapGpuContext *context, const void *texture, unsigned long textureBytes,
                                    unsigned int textureFormat, const void *alphaTexture, unsigned long alphaTextureBytes,
                                    unsigned int width, unsigned int height, unsigned int scaleLog2, unsigned int count,
                                    const unsigned int *outputFormats, void *const *outputs,
                                    const unsigned long *outputsBytes, unsigned long *outputsBytesUsed)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_transcode_texture(context, texture, textureBytes, textureFormat, alphaTexture, alphaTextureBytes, width, height,
                               scaleLog2, count, outputFormats, outputs, outputsBytes, outputsBytesUsed);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuTranscodeFrames(HapGpuContext *context, unsigned int frameCount, const void *const *inputBuffers,
                                   const unsigned long *inputBuffersBytes, unsigned int sourceTextureCount,
                                   unsigned int width, unsigned int height, unsigned int scaleLog2, unsigned int count,
                                   const unsigned int *textureFormats, const unsigned int *compressors,
                                   const unsigned int *chunkCounts, void *const *outputBuffers,
                                   const unsigned long *outputBuffersBytes, unsigned long *outputBuffersBytesUsed,
                                   unsigned int *results, unsigned int decodeFlags, unsigned int encodeFlags)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_transcode(context, frameCount, inputBuffers, inputBuffersBytes, sourceTextureCount, width, height, scaleLog2,
                       count, textureFormats, compressors, chunkCounts, outputBuffers, outputBuffersBytes,
                       outputBuffersBytesUsed, results, decodeFlags, encodeFlags);
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuDecodeFramesRGBAHalf(HapGpuContext *context, unsigned int frameCount,
                                        const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                        void *const *rgbaHalfFrames, unsigned int width, unsigned int height,
                                        unsigned long rowBytes, unsigned int *results, unsigned int flags)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA16F};
    if (!context)
        return HapResult_Bad_Arguments;
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, 1u, rgbaHalfFrames, width, height,
                            rowBytes, results, flags, &road);
}

unsigned int HapGpuDecodeFramesAlpha(HapGpuContext *context, unsigned int frameCount,
                                     const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                     void *const *alphaFrames, unsigned int width, unsigned int height,
                                     unsigned long rowBytes, unsigned int *results, unsigned int flags)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_A8};
    if (!context)
        return HapResult_Bad_Arguments;
    return frames_down_road(context, frameCount, inputBuffers, inputBuffersBytes, 1u, alphaFrames, width, height,
                            rowBytes, results, flags, &road);
}

unsigned int HapGpuJoinChunkGroupsDevice(HapGpuContext *context, unsigned int groupCount,
                                         const void *const *groupFrames, const unsigned long *groupFramesBytes,
                                         void *outputBuffer, unsigned long outputBufferBytes,
                                         unsigned long *outputBufferBytesUsed)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapb_join_device(context, groupCount, groupFrames, groupFramesBytes, outputBuffer, outputBufferBytes,
                         outputBufferBytesUsed);
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* callback that "runs" one contiguous group of chunks (hap.h:113-130 lets a client run any subset) */
typedef struct chunk_group {
    unsigned first, count;
} chunk_group;

static void run_chunk_group(HapDecodeWorkFunction function, void *p, unsigned int count, void *info)
{
    const chunk_group *g = (const chunk_group *)info;
    unsigned i;
    for (i = g->first; i < count && i - g->first < g->count; i++)
        function(p, i);
}

unsigned int HapGpuDecodeChunkGroup(HapGpuContext *context, const void *inputBuffer, unsigned long inputBufferBytes,
                                    unsigned int index, unsigned int firstChunk, unsigned int chunkCount,
                                    void *outputBuffer, unsigned long outputBufferBytes,
                                    unsigned long *outputBufferBytesUsed, unsigned int *outputBufferTextureFormat)
{
    chunk_group g = {firstChunk, chunkCount};
    const HapbDecodeArgs group = {NULL, NULL, NULL, 0, NULL, 0u, run_chunk_group, &g};
    unsigned result = HapResult_Internal_Error, rc, fmt = 0;
    unsigned long used = 0;
    if (!context || !inputBuffer || index > 1 || !outputBuffer)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    rc = hapb_decode(context, 1, &inputBuffer, &inputBufferBytes, index, &outputBuffer, &outputBufferBytes, &used,
                     &fmt, &result, 0, &group);
    hapgpu_rt_unlock(context->rt);
    if (outputBufferTextureFormat)
        *outputBufferTextureFormat = fmt;
    if (rc == HapResult_No_Error && outputBufferBytesUsed)
        *outputBufferBytesUsed = used;
    return rc;
}

/* decoded position of every chunk: the running sum the reference builds in hap.c:794-838 */
unsigned int HapGpuGetFrameTextureChunkLayout(const void *inputBuffer, unsigned long inputBufferBytes,
                                              unsigned int index, unsigned int capacity,
                                              unsigned long *decodedOffsets, unsigned int *chunkCount)
{
    hapf_reader r;
    inspect_fetch f;
    hapf_texture_plan plan;
    unsigned result, n, i;
    unsigned long cursor = 0;
    if (!inputBuffer || index > 1 || !decodedOffsets || !chunkCount)
        return HapResult_Bad_Arguments;
    *chunkCount = 0;
    open_reader(&r, &f, inputBuffer, inputBufferBytes);
    hapf_plan_texture(&r, (uint32_t)inputBufferBytes, index, 1, &plan);
    result = plan.result;
    n = plan.mode == HAPGPU_JOB_COMPLEX ? (unsigned)plan.chunk_count : 1u;
    if (result == HapResult_No_Error) {
        *chunkCount = n;
        if (capacity < n + 1u)
            result = HapResult_Buffer_Too_Small;
    }
    for (i = 0; result == HapResult_No_Error && i < n; i++) {
        uint64_t at = plan.mode == HAPGPU_JOB_COMPLEX ? plan.payload_offset + plan.chunks[i].src_off : plan.section_offset;
        uint32_t len = plan.mode == HAPGPU_JOB_COMPLEX ? plan.chunks[i].src_len : plan.section_length;
        unsigned codec = plan.mode == HAPGPU_JOB_COMPLEX ? (plan.chunks[i].codec & 0xFFu)
                         : plan.mode == HAPGPU_JOB_RAW ? HAP_NIBBLE_NONE : HAP_NIBBLE_SNAPPY;
        decodedOffsets[i] = cursor;
        if (codec == HAP_NIBBLE_NONE) {
            cursor += len;
        } else if (codec == HAP_NIBBLE_SNAPPY) {
            /* the stream's leading varint (snappy_uncompressed_length, hap.c:813) */
            const unsigned take = len < 5u ? len : 5u;
            const uint8_t *v = take ? hapf_need(&r, at, take) : NULL;
            uint64_t value = 0;
            unsigned k = 0, done = 0;
            while (v && k < take && !done) {
                value |= (uint64_t)(v[k] & 0x7Fu) << (7u * k);
                done = !(v[k] & 0x80u);
                k++;
            }
            if (!done || value > 0xFFFFFFFFull)
                result = v || !take ? HapResult_Bad_Frame : HapResult_Internal_Error;
            cursor += (unsigned long)value;
        } else {
            result = HapResult_Bad_Frame;             /* hap.c:637-640 */
        }
    }
    if (result == HapResult_No_Error)
        decodedOffsets[n] = cursor;
    hapf_plan_free(&plan);
    hapf_reader_free(&r);
    return result;
}

unsigned int HapGpuSetProfiling(HapGpuContext *context, unsigned int enable)
{
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    hapgpu_rt_set_profiling(context->rt, (int)enable);
    hapgpu_rt_unlock(context->rt);
    return HapResult_No_Error;
}

unsigned int HapGpuCollectProfileN(HapGpuContext *context, unsigned int classCount, unsigned long *launches, double *milliseconds)
{
    unsigned r;
    if (!context || !launches || !milliseconds)
        return HapResult_Bad_Arguments;
    if (classCount > HapGpuKernel_ClassCount)
        classCount = HapGpuKernel_ClassCount;
    hapgpu_rt_lock(context->rt);
    /* (events of classes beyond the caller's arrays are drained and dropped) */
    r = hapgpu_rt_collect_profile(context->rt, launches, milliseconds, classCount) ? HapResult_Internal_Error : HapResult_No_Error;
    hapgpu_rt_unlock(context->rt);
    return r;
}

/* The entry point of the first header (eight classes, no count argument): a client built against it has arrays of
   eight.  New code says how many entries its arrays have (HapGpuCollectProfileN). */
unsigned int HapGpuCollectProfile(HapGpuContext *context, unsigned long *launches, double *milliseconds)
{
    /* (the class count of the header this entry point was last released with: nine, encode_fused included -- ADVICE r05) */
    return HapGpuCollectProfileN(context, 9u, launches, milliseconds);
}

unsigned int HapGpuTimerStart(HapGpuContext *context)
{
    unsigned r;
    if (!context)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapgpu_rt_timer_start(context->rt) ? HapResult_Internal_Error : HapResult_No_Error;
    hapgpu_rt_unlock(context->rt);
    return r;
}

unsigned int HapGpuTimerStop(HapGpuContext *context, double *milliseconds)
{
    unsigned r;
    if (!context || !milliseconds)
        return HapResult_Bad_Arguments;
    hapgpu_rt_lock(context->rt);
    r = hapgpu_rt_timer_stop(context->rt, milliseconds) ? HapResult_Internal_Error : HapResult_No_Error;
    hapgpu_rt_unlock(context->rt);
    return r;
}
