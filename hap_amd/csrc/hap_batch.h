/*
 * hap_batch.h -- internal interface between hap_api.c (public symbols) and
 * hap_batch.c / hap_pictures.c (GPU orchestration).  Pure C.
 */
#ifndef HAP_BATCH_H
#define HAP_BATCH_H

#include "../../include/hap_gpu.h"
#include "hap_frame.h"
#include "hap_slice.h"
#include "hapgpu_abi.h"

struct HapGpuContext {
    hapgpu_rt *rt;
    unsigned frag_log2;
    unsigned byte_granular;   /* HAP_AMD_BYTE_GRANULAR=1: never emit 16-bit granular element streams */
    unsigned position_lanes;  /* HAP_AMD_POSITION_LANES: never use the field-per-lane compressor */
    unsigned rgtc1_fields;    /* layout of RGTC1 planes for the block compressor: 26 = [2, 6] (default), 44 = [4, 4], 0 = position lanes (HAP_AMD_RGTC1_LAYOUT) */
    unsigned no_block_scan;   /* HAP_AMD_NO_BLOCK_SCAN: whole-stream units stay whole (A/B runs) */
    unsigned no_fusion;       /* HAP_AMD_NO_FUSION: RGBA calls run the block encoder as a pass of its own (A/B runs) */
    unsigned placing_min_frames; /* HAP_AMD_PLACING_MIN_FRAMES (default 8; 12 until round 5): batches below it gather (with most of a
                                    frame in flight at once its wavefronts wait for each other longer than the gather pass
                                    takes; at 8 frames the two break even for a call by itself, and in a pipelined step --
                                    the next batch's decode kernels fill the waiting wavefronts' slots -- placing wins:
                                    0.545 against 0.559 ms per step of 8 8K frames) */
    unsigned placing_holdoff; /* calls left that gather although they could place: the last placing call encoded most frames twice */
    unsigned placing_holdoff_calls; /* HAP_AMD_PLACING_HOLDOFF (default 8): how many */
    unsigned no_placing;      /* HAP_AMD_NO_PLACING: compressed fragments go to slots and are gathered (A/B runs); a single
                                 call asks for the same with HapbEncodeArgs.never_place */
    unsigned no_wide_planes;  /* HAP_AMD_NO_WIDE_PLANES: A8 pictures take the one-block-per-lane road of alpha_plane.hip even
                                 where they are 16-byte aligned (A/B runs) */
    unsigned no_half_tiles;   /* HAP_AMD_NO_HALF_TILES: fragment table version 1 even for field streams (A/B runs) */
    unsigned long placement_retries; /* frames encoded a second time, through slots (a chunk of theirs was stored raw) */
    unsigned long placement_timeouts; /* ... of which: a wavefront waited for its predecessors' sizes longer than the bound */
    unsigned placing_off;     /* after such a timeout: encode calls left that gather before placing is tried again */
    unsigned long table_fallbacks;   /* frames decoded again without their fragment table (it did not match) */
    /* HapGpuEncodeFramesRGBABegin / HapGpuEncodeFramesFinish: the launched half of an encode call whose results have
       not been asked for yet; while there is one the context takes no other call */
    struct HapbEncodePending *pending_encode;
};

/* The tensors of the planar roads (include/hap_gpu.h: HapGpuDecompressPlanes, HapGpuDecodeFramesPlanes,
   HapGpuCompressPlanes, HapGpuEncodeFramesPlanes): what one
   call's tensors share.  Their rows are the calls' row_bytes apart. */
typedef struct HapbPlanes {
    unsigned channels;              /* planes of a tensor: 3 (R, G, B) or 4 (+ A) */
    unsigned element;               /* HapGpuPlaneElement */
    unsigned long plane_bytes;      /* from one plane of a tensor to the next */
    const float *scale, *bias;      /* `channels` floats each.  Decoding: element = (float)byte * scale[c] + bias[c], two
                                       roundings; encoding: byte = quantise(element * scale[c] + bias[c]), two roundings
                                       (plane_quantise.hpp) */
} HapbPlanes;

/* The NV12 pictures of the video roads (include/hap_gpu.h: HapGpuCompressNV12, HapGpuEncodeFramesNV12): what lies beside
   the Y planes, which are the call's pictures with the call's row_bytes as their pitch. */
typedef struct HapbVideo {
    const void *const *chroma;      /* chroma[f]: the plane of interleaved Cb, Cr pairs of pictures[f], f counted from the
                                       call's first frame (one texture: one entry) */
    unsigned long chroma_row_bytes; /* the pitch of its rows */
    unsigned matrix, range;         /* HapGpuYCbCrMatrix, HapGpuYCbCrRange */
} HapbVideo;

/* What an encode call's textures are made from: the mirror of HapbRoad, filled the same way. */
typedef struct HapbSource {
    unsigned picture_kind;      /* HAPGPU_PICTURE_*: RGBA8, RGBA16F, A8 */
    const HapbPlanes *planes;   /* NULL: interleaved pictures of picture_kind; else (RGBA8: they make what those make)
                                   planar tensors in device memory: row_bytes is the pitch of a plane's rows */
    const HapbVideo *video;     /* NULL: as above; else (RGBA8: they make what those make; no planes) NV12 pictures in
                                   device memory: the pictures are Y planes and row_bytes is the pitch of their rows */
    unsigned width, height;
    unsigned long row_bytes;
} HapbSource;

typedef struct HapbBlockEncodeJob {
    const uint64_t *host_table;    /* pinned: [sources][outputs of texture 0][of texture 1], frame_count each */
    uint64_t *device_table;
    unsigned frame_count, count, formats[2];
    /* source.planes != NULL: the sources are planar tensors in device memory, not pictures: the block encode is
       hapgpu_k_block_encode_planes' and never part of the block compressor; source.picture_kind and wide mean nothing.
       Only RGBA8 pictures are ever fused into the block compressor.  scale and bias are kept here (source.planes->scale
       and ->bias are the caller's, which need not outlive the first half of a call in two halves: not looked at after
       hapb_source_frames has returned).
       source.video != NULL: the sources are NV12 pictures in device memory, Y planes in the table's first column and
       CbCr planes in its third: the block encode is hapgpu_k_block_encode_video's, never part of the block compressor
       either; source.video->chroma is not looked at (the table holds the addresses). */
    HapbSource source;
    int wide;
    float plane_scale[4], plane_bias[4];
} HapbBlockEncodeJob;

/* What hapb_encode leaves for hapb_encode_complete: the call's arguments (copies: the client's arrays need not outlive
   the first half -- except the two it fills, output_used and results) and the state of its launches. */
typedef struct HapbEncodePending {
    unsigned frame_count, count, flags, live, placed, first_error, launch_rc;
    int inputs_are_device, has_job;
    const void **inputs;
    void **outputs;
    unsigned long *output_bytes;
    unsigned long input_bytes[2];
    unsigned formats[2], compressors[2], chunk_counts[2];
    unsigned long *output_used;       /* the client's */
    unsigned *results;                /* the client's */
    unsigned *live_index;
    size_t *stage_off_out;
    HapGpuFrameEnc *hframes;          /* pinned scratch: stays as it is while the context takes no other call */
    uint8_t *out_stage;
    HapbBlockEncodeJob job;           /* a call that started from pictures (has_job) */
    HapbPlanes planes;                /* ... from tensors: what job.source.planes points to (the caller's is gone) */
    HapbVideo video;                  /* ... from video pictures: what job.source.video points to */
} HapbEncodePending;
unsigned hapb_encode_complete(HapGpuContext *ctx, HapbEncodePending *pending);
/* ... or lets go of it without touching the client's arrays (the context is being destroyed): waits for the launches, frees `pending` */
void hapb_encode_abandon(HapGpuContext *ctx, HapbEncodePending *pending);

/* What one hapb_encode call is told beyond its frames.  NULL stands for all zero: textures that may lie anywhere, made by
   the client, results before the call returns, placing where the context and the geometry allow it. */
typedef struct HapbEncodeArgs {
    int inputs_are_device;          /* != 0: every input pointer is known to be device memory (skips classification); 2: and
                                       pictures were staged for them, so the launches are not recorded as a graph */
    const HapbBlockEncodeJob *job;  /* the block encode that makes the textures, issued at the head of the call's launches:
                                       the whole call is one launch sequence (recorded and replayed as one HIP graph) */
    int defer;                      /* 1: return once everything is launched and leave the rest in ctx->pending_encode */
    int never_place;                /* 1: fragments go to slots and are gathered, as with ctx->no_placing */
} HapbEncodeArgs;
unsigned hapb_encode(HapGpuContext *ctx, unsigned frame_count, unsigned count,
                     const void *const *inputs, const unsigned long *input_bytes,
                     const unsigned *formats, const unsigned *compressors, const unsigned *chunk_counts,
                     void *const *outputs, const unsigned long *output_bytes,
                     unsigned long *output_used, unsigned *results, unsigned flags,
                     const HapbEncodeArgs *args);
/* one picture or planar tensor -> one texture (host or device), results before it returns.  Pictures (host or device):
   RGBA8 and the DXT / RGTC1 formats (BC7 with HAPGPU_ENCODE_BPTC_BLOCKS), RGBA16F and a BC6H format, or A8 and A_RGTC1
   (hapb_source_frames' rules); HAPGPU_ENCODE_REFINE_ENDPOINTS in flags goes down to the block kernel, which looks at it
   for DXT1 and DXT5.  A tensor (device memory): DXT1, DXT5, YCoCg-DXT5, or RGTC1 from the fourth plane (255 where there
   are three); flags are not looked at.  A video picture (device memory; `picture` its Y plane, source->video->chroma[0]
   its CbCr plane): DXT1 or YCoCg-DXT5; flags are not looked at */
unsigned hapb_source_texture(HapGpuContext *ctx, const HapbSource *source, const void *picture, unsigned format,
                             void *output, unsigned long output_bytes, unsigned long *used, unsigned flags);
/* The crops of the resized planar roads (include/hap_gpu.h: HapGpuDecompressPlanesResized,
   HapGpuDecodeFramesPlanesResized): entry f's crop is (xs[f], ys[f], ws[f], hs[f]) in texels of the scaled picture, f
   counted from the call's first frame, and every tensor is out_w x out_h elements */
typedef struct HapbResize {
    const unsigned *xs, *ys, *ws, *hs;
    unsigned out_w, out_h;
} HapbResize;
/* 1: out_w and out_h are sizes the resized roads take (1 to 16384) */
int hapb_resize_out_valid(const HapbResize *resize);
/* 1: crop f of `resize` is one of a width x height texture at scale_log2 -- not empty, inside the scaled picture, at most
   4 x the output per axis; *region then gets it in full-size texels, rounded outward to the block grid: a rectangle of
   hapb_region_fits */
int hapb_resize_region(const HapbResize *resize, size_t f, unsigned width, unsigned height, unsigned scale_log2,
                       HapGpuRegion *region);
/* what the planar encode calls ask whatever their tensors are: 1 = channels, element, scale, bias, the geometry, the
   pitches and the set of texture formats are in order (include/hap_gpu.h: HapGpuCompressPlanes,
   HapGpuEncodeFramesPlanes).  Touches no device. */
int hapb_planes_encode_valid(unsigned width, unsigned height, unsigned long row_bytes, const HapbPlanes *planes,
                             unsigned count, const unsigned *formats);
/* ... and the video encode calls whatever their planes are: 1 = matrix, range, the geometry, both pitches and the set of
   texture formats are in order (include/hap_gpu.h: HapGpuCompressNV12, HapGpuEncodeFramesNV12).  Touches no device. */
int hapb_video_encode_valid(unsigned width, unsigned height, unsigned long row_bytes, const HapbVideo *video,
                            unsigned count, const unsigned *formats);
/* ... and the video decode calls whatever their frames and planes are: 1 = scale_log2, matrix, range, the geometry
   (multiples of 4 << scale_log2, at most 65535 block rows of the output) and both pitches are in order
   (include/hap_gpu.h: HapGpuDecompressNV12, HapGpuDecodeFramesNV12).  Touches no device. */
int hapb_video_decode_valid(unsigned width, unsigned height, unsigned scale_log2, unsigned long row_bytes,
                            const HapbVideo *video);
/* 1: region is a block-aligned, non-empty rectangle inside region->width x height */
int hapb_region_fits(const HapGpuRegion *region, unsigned height);
/* pictures or planar tensors -> frames, HAP_SLICE_ENTRIES frames at a time: every slice reports for itself and the first
   slice's error is returned.  Pictures of kind RGBA8: the DXT / RGTC1 formats (BC7 with HAPGPU_ENCODE_BPTC_BLOCKS);
   RGBA16F (rows and device addresses 16-byte aligned): one BC6H texture; A8 (rows and device addresses 4-byte aligned):
   one RGTC1 texture.  Tensors (hapb_planes_encode_valid): count 1: DXT1, DXT5, YCoCg-DXT5 or RGTC1; count 2: YCoCg-DXT5
   then RGTC1; a NULL, host or misaligned tensor makes its frame Bad_Arguments.  Video pictures
   (hapb_video_encode_valid): count 1: DXT1 or YCoCg-DXT5; a NULL, host or misaligned Y or CbCr plane makes its frame
   Bad_Arguments; HAPGPU_ENCODE_BPTC_BLOCKS is ignored.  HAPGPU_ENCODE_REFINE_ENDPOINTS in flags:
   hapb_encode hands it to the block kernels of one-texture frames and does not fuse a DXT5 texture.  defer:
   HapbEncodeArgs.defer of the call's hapb_encode; such a call takes one slice at most */
unsigned hapb_source_frames(HapGpuContext *ctx, const HapbSource *source, unsigned frame_count,
                            const void *const *pictures, unsigned count, const unsigned *formats,
                            const unsigned *compressors, const unsigned *chunk_counts, void *const *outputs,
                            const unsigned long *output_bytes, unsigned long *output_used, unsigned *results,
                            unsigned flags, int defer);
/* What one hapb_decode call is told beyond its frames.  NULL stands for all zero: texture `index` of every entry, whole
   textures, nobody to ask which chunks are wanted. */
typedef struct HapbDecodeArgs {
    const unsigned *indices;        /* texture index of every entry (NULL: the `index` argument for all) */
    const HapGpuRegion *region;     /* the rectangle the textures are wanted for (NULL: all of them): units that hold none
                                       of its blocks stay undecoded */
    const HapGpuRegion *regions;    /* ... or a rectangle per entry (NULL: `region` for all): an entry that skips nothing
                                       carries the whole of its texture */
    int region_uncounted;           /* 1: the call is a frame's second pass, whose first pass has counted what it skipped
                                       (HapGpuSkippedTextureBytes counts a frame once) */
    const unsigned char *marks;     /* mark_count chunk marks the client's callback has given for this frame already: a
                                       second pass uses them, so that the callback runs once per HapDecode */
    unsigned mark_count;
    HapDecodeCallback callback;     /* only honoured for frame_count == 1 (the hap.h HapDecode path) */
    void *callback_info;
} HapbDecodeArgs;
unsigned hapb_decode(HapGpuContext *ctx, unsigned frame_count, const void *const *inputs,
                     const unsigned long *input_bytes, unsigned index, void *const *outputs,
                     const unsigned long *output_bytes, unsigned long *output_used,
                     unsigned *output_formats, unsigned *results, unsigned flags, const HapbDecodeArgs *args);

/* A road from block textures to pictures: what the caller wants made of every texture (+ RGTC1 alpha plane) or frame.
   Filled with designated initialisers, everything not named being 0 / NULL: RGBA8 pictures of the textures' size.
   Which texture formats the road takes follows from it (hap_pictures.c: road_formats) -- RGBA8: DXT1, DXT5 and
   YCoCg-DXT5, each with an optional alpha plane, and with `bptc` BC7; RGBA16F: BC6H unsigned or signed; A8: RGTC1. */
typedef struct HapbRoad {
    unsigned picture_kind;      /* HAPGPU_PICTURE_*: the pictures' layout, and with it the size of a texel */
    unsigned scale_log2;        /* 0: pictures of the textures' size; 1 / 2 (RGBA8 only): half / quarter size, of
                                   (width >> scale_log2) x (height >> scale_log2); rows and device pictures are then
                                   aligned to 16 >> scale_log2 bytes */
    int bptc;                   /* != 0 (interleaved RGBA8 pictures only): BC7 textures are taken too */
    const HapGpuRegion *region; /* NULL: the whole of every texture; else (RGBA8; interleaved pictures: scale_log2 0;
                                   region->width == width) pictures of region->w x region->h, planar tensors of
                                   (region->w >> scale_log2) x (region->h >> scale_log2): that rectangle of every texture,
                                   and only its blocks are read */
    const unsigned *region_xs, *region_ys;  /* NULL: region->x, region->y for every frame; else (planes only, frames only)
                                   frame f's rectangle begins at (region_xs[f], region_ys[f]), f counted from the call's
                                   first frame, and region->x, region->y are 0 */
    const HapbPlanes *planes;   /* NULL: interleaved pictures of picture_kind; else (RGBA8, scale_log2 0 to 2) planar
                                   tensors in device memory: a "texel" is then one element of one plane and row_bytes
                                   the pitch of a plane's rows */
    const HapbResize *resize;   /* NULL: tensors of the rectangle's or the textures' (scaled) size; else (planes only, no
                                   region) tensors of resize->out_w x resize->out_h, entry f's crop of the scaled picture
                                   resized */
    const HapbVideo *video;     /* NULL: as above; else (RGBA8, scale_log2 0 to 2; no bptc, region, planes, resize or
                                   measure) NV12 pictures in device memory are WRITTEN: the road's pictures are their Y
                                   planes, a "texel" one byte and row_bytes the pitch of a Y plane's rows; video->chroma[f]
                                   is the CbCr plane of pictures[f], f counted from the call's first frame (one texture:
                                   one entry).  It travels in the alpha column of the launch's HapGpuPictureTable, free
                                   here: the RGTC1 plane of a frame is never block-decoded */
    HapGpuPictureError *measure; /* NULL: the pictures are written; else (RGBA8, scale_log2 0, no region, no planes) they
                                   are reference pictures in device memory and are READ: measure[f] gets the sums of
                                   frame f against its picture, f counted from the call's first frame, all zero for a
                                   frame whose result is not No_Error (one texture: *measure, written on No_Error only) */
} HapbRoad;
/* one texture (host or device; + RGTC1 alpha plane) down a road: to one picture, one planar tensor, or one set of sums */
unsigned hapb_road_texture(HapGpuContext *ctx, const void *texture, unsigned long texture_bytes, unsigned format,
                           const void *alpha, unsigned long alpha_bytes, unsigned width, unsigned height, void *picture,
                           unsigned long row_bytes, const HapbRoad *road);
/* frames down a road, one picture each (texture_count 2: Hap Q Alpha frames, colour + RGTC1 alpha plane; width and
   height are the frames') */
unsigned hapb_road_frames(HapGpuContext *ctx, unsigned frame_count, const void *const *inputs,
                          const unsigned long *input_bytes, unsigned texture_count, void *const *pictures, unsigned width,
                          unsigned height, unsigned long row_bytes, unsigned *results, unsigned flags,
                          const HapbRoad *road);

/* frames -> frames of the texture formats `formats` (count 1 or 2) at (width >> scale_log2) x (height >> scale_log2),
   without a picture in between (include/hap_gpu.h: HapGpuTranscodeFrames); texture_count: the textures read of every
   frame, as for hapb_road_frames */
unsigned hapb_transcode(HapGpuContext *ctx, unsigned frame_count, const void *const *inputs,
                        const unsigned long *input_bytes, unsigned texture_count, unsigned width, unsigned height,
                        unsigned scale_log2, unsigned count, const unsigned *formats, const unsigned *compressors,
                        const unsigned *chunk_counts, void *const *outputs, const unsigned long *output_bytes,
                        unsigned long *output_used, unsigned *results, unsigned decode_flags, unsigned encode_flags);
/* ... one texture (+ RGTC1 alpha plane) -> `count` textures (HapGpuTranscodeTexture) */
unsigned hapb_transcode_texture(HapGpuContext *ctx, const void *texture, unsigned long texture_bytes, unsigned format,
                                const void *alpha, unsigned long alpha_bytes, unsigned width, unsigned height,
                                unsigned scale_log2, unsigned count, const unsigned *formats, void *const *outputs,
                                const unsigned long *output_bytes, unsigned long *output_used);

/* A compositing call: the canvas, what the layers are on it and where the canvas goes.  Filled with designated
   initialisers, everything not named being 0 / NULL: layers of the canvas's size, whole at (0, 0), fully opaque over
   opaque black, to RGBA8 pictures.  What follows from it -- the rules, the descriptors, the kernel -- is decided in one
   place each (hap_pictures.c: hapb_composite_valid, composite_descriptor, launch_composite). */
typedef struct HapbComposite {
    unsigned layer_count;               /* layer 0 at the bottom */
    unsigned width, height;             /* the canvas */
    const unsigned char *background;    /* 4 bytes R, G, B, A (NULL: 0, 0, 0, 255) */
    const unsigned char *opacities;     /* one byte per layer of every output frame (NULL: all 255) */
    const unsigned *layer_widths, *layer_heights;   /* NULL: every layer has the canvas's size (HapGpuCompositeTextures,
                                           HapGpuCompositeFrames); else layer l is layer_widths[l] x layer_heights[l] */
    const HapGpuPlacement *placements;  /* (layer sizes only) one per layer of every output frame: the rectangle of the
                                           layer and where it goes, clipped to the canvas (hap_place.h); NULL: every layer
                                           whole at (0, 0) */
    /* the destination, one of two: RGBA8 pictures, host or device, rows row_bytes apart ... */
    unsigned long row_bytes;
    /* ... or (encoded != 0; layer sizes only) the canvas encoded to `count` block textures of `formats`, one of the four
       destination sets of hapb_transcode's kernel, never written as a picture -- and, for frames, made frames of by
       hapb_encode with compressors, chunk_counts and encode_flags */
    int encoded;
    unsigned count;
    const unsigned *formats, *compressors, *chunk_counts;
    unsigned encode_flags;
} HapbComposite;
/* what a compositing call asks whatever its layers hold: 1 = the layer count, the canvas, the pitch, every texture count
   (frames; NULL: all 1), every layer's size and every one of the frame_count * layer_count placements (hap_place.h) are
   in order; encoded: at most 65535 block rows and a destination set the kernel makes, and for `frames` compressors and
   chunk counts that hapb_encode takes with it (include/hap_gpu.h: HapGpuCompositeTextures to
   HapGpuCompositeFramesEncoded).  Touches no device. */
int hapb_composite_valid(const HapbComposite *composite, size_t frame_count, const unsigned *texture_counts, int frames);
/* layer_count textures (+ RGTC1 alpha planes; host or device) -> one canvas: outputs[0] the picture, or outputs[i]
   destination texture i (host or device) of output_bytes[i], output_used[i] (NULL: not wanted) the bytes written; a
   call to pictures takes neither */
unsigned hapb_composite_textures(HapGpuContext *ctx, const HapbComposite *composite, const void *const *textures,
                                 const unsigned long *texture_bytes, const unsigned *formats,
                                 const void *const *alphas, const unsigned long *alpha_bytes, void *const *outputs,
                                 const unsigned long *output_bytes, unsigned long *output_used);
/* ... of frames: entry f * layer_count + l is layer l of output frame f, texture_counts[l] textures read of it, its
   result layer_results[f * layer_count + l]; outputs[f] the picture of output frame f -- a NULL or misaligned one fails
   every layer entry of its frame, and results is NULL -- or, encoded, its frame with output_bytes, output_used and
   results as hapb_transcode has them, the result of an output frame with a failed layer being that layer's */
unsigned hapb_composite_frames(HapGpuContext *ctx, const HapbComposite *composite, unsigned frame_count,
                               const void *const *inputs, const unsigned long *input_bytes,
                               const unsigned *texture_counts, void *const *outputs, const unsigned long *output_bytes,
                               unsigned long *output_used, unsigned *layer_results, unsigned *results,
                               unsigned decode_flags);

/* groups and output in device memory: tables through the host, payloads device to device */
unsigned hapb_join_device(HapGpuContext *ctx, unsigned group_count, const void *const *frames,
                          const unsigned long *frame_bytes, void *output, unsigned long output_bytes,
                          unsigned long *output_used);

/* hap_join.c: the join proper, reading the groups' headers through `readers` (host views, or device frames with a
 * fetch callback) and writing through a sink: `put` = bytes made here to output offset, `move` = bytes of group g's
 * frame to output offset.  Non-zero from a sink callback ends the join with Internal_Error. */
typedef struct hapj_sink {
    void *user;
    int (*put)(void *user, uint64_t dst_off, const void *src, size_t len);
    int (*move)(void *user, unsigned group, uint64_t src_off, uint64_t dst_off, size_t len);
} hapj_sink;
unsigned hapj_join(unsigned groupCount, hapf_reader *readers, const unsigned long *groupFramesBytes,
                   const hapj_sink *sink, unsigned long outputBufferBytes, unsigned long *outputBufferBytesUsed);

#endif
