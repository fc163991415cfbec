/*
 * hap_batch_private.h -- what hap_batch.c (frames to textures and back) and hap_pictures.c (everything that goes on from
 * block textures) share and nobody else sees: the names of the runtime's scratch slots and a few small helpers.  Pure C.
 */
#ifndef HAP_BATCH_PRIVATE_H
#define HAP_BATCH_PRIVATE_H

#include "hap_batch.h"
#include <stddef.h>

enum {
    D_FRAMES = 0, D_SLOTS, D_FRAGSIZES, D_COPIES, D_TEX_STAGE, D_FRAME_STAGE, D_BC_TEX, D_RGBA_STAGE,
    D_JOBS, D_CHUNKS, D_UNITS, D_IN_STAGE, D_OUT_STAGE, D_PTRS, D_PREFIX, D_BC_PTRS
};
#define D_GROUPTABLES D_PTRS   /* encode-only arenas in decode-only slots: one call never needs both */
#define D_PACK D_PREFIX
#define D_CHUNK_ACC D_JOBS
#define D_SCAN D_SLOTS       /* ... and the decoder's block-scan arena in an encode-only one */
#define D_GUESS D_FRAGSIZES  /* ... and the group tables the decoder makes for fragments that came without */
#define D_TRANSCODED D_RGBA_STAGE /* ... and the textures a transcode call makes, where the calls with pictures stage those: it
                                     has none, and D_BC_TEX holds its source textures until its encode half is done */
#define D_MEASURE D_RGBA_STAGE    /* ... and the totals and partial sums of a measuring call: its pictures are never staged */
#define P_SCAN P_FRAMES
enum { P_FRAMES = 0, P_JOBS, P_CHUNKS, P_PREFIX, P_PTRS, P_BC_PTRS, P_PREFIX2 };   /* (8, 9: hap_sequence.c) */

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static inline int is_dev(HapGpuContext *c, const void *p) { return hapgpu_rt_is_device_ptr(c->rt, p); }

/* A context whose last encode call has been begun and not finished (HapGpuEncodeFramesRGBABegin) holds that call's
   tables and scratch: it takes no other call until HapGpuEncodeFramesFinish.  1: busy, and every result set (hap_batch.c) */
int context_busy(HapGpuContext *c, unsigned *results, unsigned frame_count);

/* What hapb_encode asks of a call's textures whatever its frames are (reference hap.c:518-559, and per texture
   hap.c:367-385): Bad_Arguments refuses the whole call.  count 1 or 2.  (hap_batch.c) */
unsigned encode_textures_valid(unsigned count, const unsigned long *input_bytes, const unsigned *formats,
                               const unsigned *compressors, const unsigned *chunk_counts, unsigned flags);

#endif
