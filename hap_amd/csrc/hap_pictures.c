/*
 * hap_pictures.c -- everything that goes on from block textures (pure C99): the roads from textures and frames to
 * pictures, planar tensors and error sums, compositing, and transcoding.  hap_batch.c undoes the second stage of a
 * slice of frames into texture scratch (hapb_decode) and makes frames of textures (hapb_encode); what lies between
 * the two is here.  A road is described by the caller (HapbRoad, hap_batch.h); which block-decode launch it takes,
 * which texture formats and what of its pictures follow from that description in one place each.
 */
#include "hap_batch_private.h"
#include "hap_place.h"
#include "hap_region.h"
#include "hap_slice.h"
#include <stdlib.h>
#include <string.h>

/* RGBA8 pictures (BC7 last: frames of it only with HAPGPU_DECODE_BPTC_PICTURES), RGBA16F ones and A8 ones */
static const unsigned k_rgba_kinds[4] = {HapTextureFormat_RGB_DXT1, HapTextureFormat_RGBA_DXT5, HapTextureFormat_YCoCg_DXT5,
                                         HapTextureFormat_RGBA_BPTC_UNORM};
static const unsigned k_half_kinds[2] = {HapTextureFormat_RGB_BPTC_UNSIGNED_FLOAT, HapTextureFormat_RGB_BPTC_SIGNED_FLOAT};
static const unsigned k_alpha_kinds[1] = {HapTextureFormat_A_RGTC1};

/* What block textures a road takes (one block-decode launch per format present in a slice of frames): *kinds gets
   the list, *paired (where asked for) the formats that may come with an RGTC1 alpha plane (bit k: kinds[k]); returns
   their number.  The planar and measuring roads are the RGBA8 road's without BC7. */
static unsigned road_formats(const HapbRoad *road, const unsigned **kinds, unsigned *paired)
{
    const int half = road->picture_kind == HAPGPU_PICTURE_RGBA16F, a8 = road->picture_kind == HAPGPU_PICTURE_A8;
    *kinds = half ? k_half_kinds : a8 ? k_alpha_kinds : k_rgba_kinds;
    if (paired)
        *paired = half || a8 ? 0u : 0x7u;
    if (half || a8)
        return half ? 2u : 1u;
    return road->bptc && !road->planes && !road->measure ? 4u : 3u;
}

/* the place of `format` among `kinds`; kind_count: not one of them */
static unsigned kind_of(const unsigned *kinds, unsigned kind_count, unsigned format)
{
    unsigned k;
    for (k = 0; k < kind_count && kinds[k] != format; k++)
        ;
    return k;
}

/* the road as the code below reads it: only RGBA8 pictures come scaled or as rectangles, and interleaved pictures of a
   rectangle have the rectangle's size */
static HapbRoad road_taken(const HapbRoad *road)
{
    HapbRoad r = *road;
    if (r.picture_kind != HAPGPU_PICTURE_RGBA8)
        r.region = NULL;
    if (r.picture_kind != HAPGPU_PICTURE_RGBA8 || (r.region && !r.planes))
        r.scale_log2 = 0u;
    return r;
}

/* a measuring road's device scratch for `pictures` pictures: [pictures][8] 64-bit totals, then the workgroups' partials */
static unsigned long long *measure_scratch(hapgpu_rt *rt, unsigned pictures, unsigned width, unsigned height,
                                           uint32_t **partials)
{
    const size_t totals_bytes = align_up(sizeof(unsigned long long) * 8u * pictures, 256);
    uint8_t *s = (uint8_t *)hapgpu_rt_device_scratch(rt, D_MEASURE, totals_bytes +
                                                     hapgpu_block_measure_partial_bytes(width, height) * pictures);
    *partials = s ? (uint32_t *)(s + totals_bytes) : NULL;
    return (unsigned long long *)s;
}

/* a picture's eight totals (sse R, G, B, A, then sad) as the caller's struct */
static void measure_result(HapGpuPictureError *error, const unsigned long long *totals, unsigned width, unsigned height)
{
    unsigned c;
    for (c = 0; c < 4u; c++) {
        error->sse[c] = totals[c];
        error->sad[c] = totals[4u + c];
    }
    error->texels = (unsigned long long)width * height;
}

int hapb_resize_out_valid(const HapbResize *resize)
{
    return resize->out_w >= 1u && resize->out_w <= 16384u && resize->out_h >= 1u && resize->out_h <= 16384u;
}

int hapb_resize_region(const HapbResize *resize, size_t f, unsigned width, unsigned height, unsigned scale_log2,
                       HapGpuRegion *region)
{
    const unsigned x = resize->xs[f], y = resize->ys[f], w = resize->ws[f], h = resize->hs[f];
    const unsigned level_w = width >> scale_log2, level_h = height >> scale_log2;
    if (scale_log2 > 2u || w == 0u || h == 0u || x > level_w || w > level_w - x || y > level_h || h > level_h - y ||
        w > 4u * resize->out_w || h > 4u * resize->out_h)
        return 0;
    /* (outward to the grid: width and height are multiples of 4, so the far edges stay inside) */
    region->width = width;
    region->x = (x << scale_log2) & ~3u;
    region->y = (y << scale_log2) & ~3u;
    region->w = ((((x + w) << scale_log2) + 3u) & ~3u) - region->x;
    region->h = ((((y + h) << scale_log2) + 3u) & ~3u) - region->y;
    return hapb_region_fits(region, height);
}

/* bytes of what a road's row_bytes counts: a texel of an interleaved picture, an element of a plane */
static size_t picture_texel_bytes(const HapbRoad *road)
{
    if (road->planes)
        return road->planes->element == HapGpuPlaneElement_F32 ? 4u : 2u;
    if (road->video)
        return 1u;          /* (a Y sample) */
    return HAPGPU_PICTURE_TEXEL_BYTES(road->picture_kind);
}

/* the geometry of a road's pictures, from the textures' */
static unsigned picture_width_of(const HapbRoad *road, unsigned width)
{
    if (road->resize)
        return road->resize->out_w;
    return (road->region ? road->region->w : width) >> road->scale_log2;
}

static unsigned picture_height_of(const HapbRoad *road, unsigned height)
{
    if (road->resize)
        return road->resize->out_h;
    return (road->region ? road->region->h : height) >> road->scale_log2;
}

/* 1: the region is a block-aligned rectangle inside width x height (hap_region.h's rules and the texture's height) */
int hapb_region_fits(const HapGpuRegion *region, unsigned height)
{
    return hap_region_geometry_valid(region->width, region->x, region->y, region->w, region->h) && region->y <= height &&
           region->h <= height - region->y;
}

int hapb_video_decode_valid(unsigned width, unsigned height, unsigned scale_log2, unsigned long row_bytes,
                            const HapbVideo *video)
{
    unsigned step, out_width;
    if (scale_log2 > 2u || video->matrix > HapGpuYCbCrMatrix_BT709 || video->range > HapGpuYCbCrRange_Full)
        return 0;
    step = 4u << scale_log2;
    out_width = width >> scale_log2;
    /* (width / 2 pairs of two bytes: a chroma row is as long as a luma row) */
    return width && height && !(width % step) && !(height % step) && height / step <= 65535u && row_bytes >= out_width &&
           video->chroma_row_bytes >= out_width && !(row_bytes & 3u) && !(video->chroma_row_bytes & 3u);
}

/* 1: `plane` is where a video road can write a CbCr plane: in device memory, dword aligned */
static int chroma_plane_fits(HapGpuContext *ctx, const void *plane)
{
    return plane && is_dev(ctx, plane) && !((uintptr_t)plane & 3u);
}

/* what the block decoders ask of a picture's address (in device memory) and row pitch when they write it: 16-byte
   stores for RGBA8 and RGBA16F; A8 pictures take dword stores, and 16-byte ones where address and pitch allow; a scaled
   picture takes the 16 >> scale_log2 bytes a lane has for each of its rows, a plane its 4 >> scale_log2 elements -- or,
   resized, the one element a lane stores; the planes of a video picture take dword stores */
static unsigned picture_align_mask(const HapbRoad *road)
{
    if (road->resize)
        return (unsigned)picture_texel_bytes(road) - 1u;
    if (road->planes)
        return (4u >> road->scale_log2) * (unsigned)picture_texel_bytes(road) - 1u;
    if (road->video)
        return 3u;          /* (at every size: a lane stores a destination block's rows) */
    if (road->scale_log2)
        return (16u >> road->scale_log2) - 1u;
    return road->picture_kind == HAPGPU_PICTURE_A8 ? 3u : 15u;
}

/* 1: a planar road's tensors are what the calls take (include/hap_gpu.h: HapGpuDecompressPlanes) -- planes that hold
   their rows and, like the rows, keep every lane's store aligned; pixel_row: the bytes of one row of a plane */
static int planes_fit(const HapbRoad *road, size_t pixel_row, unsigned picture_height, unsigned long row_bytes)
{
    const HapbPlanes *p = road->planes;
    return p->channels >= 3u && p->channels <= 4u && p->element <= HapGpuPlaneElement_F32 && road->scale_log2 <= 2u &&
           p->scale && p->bias && picture_height && !(p->plane_bytes & picture_align_mask(road)) &&
           p->plane_bytes >= (size_t)row_bytes * (picture_height - 1u) + pixel_row;
}

/* the texture block a rectangle begins at */
static uint32_t region_first_block(unsigned width, unsigned x, unsigned y)
{
    return (uint32_t)((y / 4u) * (width / 4u) + x / 4u);
}

/* A picture in host memory is made in D_RGBA_STAGE and copied back: what the copy needs to know of it */
typedef struct picture_shape {
    size_t row_bytes, pixel_row, bytes;     /* the caller's pitch; the bytes of a row that are the picture's; first to last byte */
    unsigned rows;
} picture_shape;

/* where picture f of the n a call stages lies, `stride` bytes apart; *stage: the scratch, asked for with the first.
   NULL: no scratch */
static uint8_t *picture_stage(hapgpu_rt *rt, uint8_t **stage, size_t stride, unsigned n, unsigned f)
{
    if (!*stage)
        *stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_RGBA_STAGE, stride * n);
    return *stage ? *stage + stride * f : NULL;
}

/* ... and back to the caller's: row by row when the caller's rows are longer than the picture's -- what lies between
   them (the rest of a larger image, perhaps) is not the call's to overwrite */
static int picture_unstage(hapgpu_rt *rt, void *picture, const void *staged, const picture_shape *p)
{
    if (p->row_bytes == p->pixel_row)
        return hapgpu_rt_d2h(rt, picture, staged, p->bytes);
    return hapgpu_rt_d2h_rows(rt, picture, p->row_bytes, staged, p->row_bytes, p->pixel_row, p->rows);
}

/* the block-decode launch of a road: pictures of the frames' size, scaled ones, a rectangle's, planar tensors (the
   alpha plane is read only where a fourth plane is written) or video pictures (whose CbCr planes are the table's second
   column; with_alpha is not looked at).  origins: a planar road with a rectangle per frame -- the
   device array of the pictures' first blocks, or, resized, of their crops (four words each; NULL: the road's first crop
   for all); partials, totals: a measuring road's scratch (measure_scratch) */
static int launch_block_decode(hapgpu_rt *rt, const HapbRoad *road, const HapGpuPictureTable *t, unsigned pictures,
                               int with_alpha, unsigned width, unsigned height, unsigned format, size_t row_bytes, int wide,
                               const uint32_t *origins, uint32_t *partials, unsigned long long *totals)
{
    /* (a measuring road: the block kernel with the pictures as its third column, read, and the reduction behind it) */
    if (road->video)
        return hapgpu_k_block_decode_video(rt, t, pictures, width, height, format, road->scale_log2, row_bytes,
                                           road->video->chroma_row_bytes, road->video->matrix, road->video->range);
    if (road->measure)
        return hapgpu_k_block_measure(rt, t, pictures, with_alpha, width, height, format, row_bytes, partials, totals);
    if (road->resize) {
        const unsigned crop[4] = {road->resize->xs[0], road->resize->ys[0], road->resize->ws[0], road->resize->hs[0]};
        return hapgpu_k_block_decode_planes_resized(rt, t, pictures, with_alpha && road->planes->channels == 4u, width, height,
                                                    format, origins, origins ? NULL : crop, road->resize->out_w,
                                                    road->resize->out_h, road->scale_log2, road->planes->channels,
                                                    road->planes->element, road->planes->plane_bytes, row_bytes,
                                                    road->planes->scale, road->planes->bias);
    }
    if (road->planes && road->region)
        return hapgpu_k_block_decode_planes_region(rt, t, pictures, with_alpha && road->planes->channels == 4u, width, height,
                                                   format, origins,
                                                   origins ? 0u : region_first_block(width, road->region->x, road->region->y),
                                                   road->region->w, road->region->h, road->scale_log2, road->planes->channels,
                                                   road->planes->element, road->planes->plane_bytes, row_bytes,
                                                   road->planes->scale, road->planes->bias);
    if (road->planes)
        return hapgpu_k_block_decode_planes(rt, t, pictures, with_alpha && road->planes->channels == 4u, width, height, format,
                                            road->scale_log2, road->planes->channels, road->planes->element,
                                            road->planes->plane_bytes, row_bytes, road->planes->scale, road->planes->bias);
    if (road->region)
        return hapgpu_k_block_decode_region(rt, t, pictures, with_alpha, width, height, format, road->region->x, road->region->y,
                                            road->region->w, road->region->h, row_bytes);
    if (road->scale_log2)
        return hapgpu_k_block_decode_scaled(rt, t, pictures, with_alpha, width, height, format, road->scale_log2, row_bytes);
    return hapgpu_k_block_decode(rt, t, pictures, with_alpha, width, height, format, row_bytes, wide, road->picture_kind);
}

/* one texture (+ RGTC1 alpha plane) down a road (DESIGN.md's `decompress_picture`) */
unsigned hapb_road_texture(HapGpuContext *ctx, const void *texture, unsigned long texture_bytes, unsigned format,
                           const void *alpha, unsigned long alpha_bytes, unsigned width, unsigned height, void *picture,
                           unsigned long row_bytes, const HapbRoad *const proad)
{
    const HapbRoad road = road_taken(proad);
    const unsigned picture_kind = road.picture_kind;
    const unsigned *kinds;
    unsigned paired;
    const unsigned kind_count = road_formats(&road, &kinds, &paired);
    const unsigned align = picture_align_mask(&road);
    hapgpu_rt *rt = ctx->rt;
    /* (the picture's geometry: the texture's, a scaled road's fraction of it, or the rectangle's) */
    const unsigned picture_height = picture_height_of(&road, height);
    const size_t block = hapf_block_bytes(format),
                 pixel_row = (size_t)picture_width_of(&road, width) * picture_texel_bytes(&road);
    HapGpuPictureTable t = {{NULL, NULL, NULL}, {0u, 0u, 0u}};
    picture_shape shape = {row_bytes, pixel_row, 0u, picture_height};
    size_t need, alpha_need;
    const void *src = texture, *asrc = alpha;
    uint8_t *stage = NULL;
    void *dst = picture;
    uint32_t *partials = NULL;
    unsigned long long *totals = NULL, *htotals = NULL;
    HapGpuRegion resized;       /* (a resized road's crop as a rectangle of blocks: only asked whether there is one) */
    unsigned k;
    int rc;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    k = kind_of(kinds, kind_count, format);
    if (!texture || !picture || width == 0 || height == 0 || (width & 3u) || (height & 3u) || row_bytes < pixel_row ||
        (road.region && (road.region->width != width || !hapb_region_fits(road.region, height))) ||
        (road.resize && (!hapb_resize_out_valid(road.resize) ||
                         !hapb_resize_region(road.resize, 0u, width, height, road.scale_log2, &resized))) ||
        k == kind_count || (alpha && !(paired >> k & 1u)) ||
        /* (tensors live in device memory: no host staging road) */
        (road.planes && (!planes_fit(&road, pixel_row, picture_height, row_bytes) || !is_dev(ctx, picture))) ||
        /* (and so do reference pictures) */
        (road.measure && !is_dev(ctx, picture)) ||
        /* (and video pictures, both planes; no alpha plane is taken) */
        (road.video && (alpha || !hapb_video_decode_valid(width, height, road.scale_log2, row_bytes, road.video) ||
                        !is_dev(ctx, picture) || !chroma_plane_fits(ctx, road.video->chroma[0]))))
        return HapResult_Bad_Arguments;
    need = (size_t)(width / 4u) * (height / 4u) * block;
    alpha_need = (size_t)(width / 4u) * (height / 4u) * 8u;
    if (texture_bytes < need || (alpha && alpha_bytes < alpha_need))
        return HapResult_Bad_Arguments;
    /* rows a multiple of 16 bytes; device textures aligned to their blocks, alpha planes to 8 bytes, pictures to 16
       (A8 pictures: rows and device pictures to 4 bytes, and at most 65535 block rows; scaled pictures: rows and device
       pictures to 8 bytes at half, 4 at quarter size) */
    if ((row_bytes & align) || (is_dev(ctx, texture) && ((uintptr_t)texture & (block - 1u))) ||
        /* (a video road's lane reads what of a block row lies under its destination block in one load) */
        (road.video && is_dev(ctx, texture) && ((uintptr_t)texture & ((block << road.scale_log2) - 1u) & 15u)) ||
        (alpha && is_dev(ctx, alpha) && ((uintptr_t)alpha & 7u)) || (is_dev(ctx, picture) && ((uintptr_t)picture & align)) ||
        (picture_kind == HAPGPU_PICTURE_A8 && height / 4u > 65535u))
        return HapResult_Bad_Arguments;
    shape.bytes = (size_t)row_bytes * (picture_height - 1u) + pixel_row;
    if (!is_dev(ctx, texture)) {
        void *s = hapgpu_rt_device_scratch(rt, D_BC_TEX, need + alpha_need + 256);
        if (!s || hapgpu_rt_h2d(rt, s, texture, need))
            return HapResult_Internal_Error;
        src = s;
        if (alpha && !is_dev(ctx, alpha)) {
            uint8_t *a = (uint8_t *)s + align_up(need, 256);
            if (hapgpu_rt_h2d(rt, a, alpha, alpha_need))
                return HapResult_Internal_Error;
            asrc = a;
        }
    } else if (alpha && !is_dev(ctx, alpha)) {
        void *a = hapgpu_rt_device_scratch(rt, D_BC_TEX, alpha_need);
        if (!a || hapgpu_rt_h2d(rt, a, alpha, alpha_need))
            return HapResult_Internal_Error;
        asrc = a;
    }
    if (!is_dev(ctx, picture) && !(dst = picture_stage(rt, &stage, shape.bytes, 1u, 0u)))
        return HapResult_Internal_Error;
    t.one[0] = (uint64_t)(uintptr_t)src;
    t.one[1] = (uint64_t)(uintptr_t)(road.video ? road.video->chroma[0] : asrc);
    t.one[2] = (uint64_t)(uintptr_t)dst;
    if (road.measure) {
        /* (after the textures' scratch: growing an arena waits for the stream, not for copies yet to be issued) */
        totals = measure_scratch(rt, 1u, width, height, &partials);
        htotals = (unsigned long long *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, sizeof(*htotals) * 8u);
        if (!totals || !htotals)
            return HapResult_Internal_Error;
    }
    rc = launch_block_decode(rt, &road, &t, 1u, alpha != NULL, width, height, format, row_bytes,
                             (((uintptr_t)dst | row_bytes) & 15u) == 0 && !ctx->no_wide_planes, NULL, partials, totals);
    if (rc == 1)
        return HapResult_Bad_Arguments;
    if (rc)
        return HapResult_Internal_Error;
    if (road.measure) {
        if (hapgpu_rt_d2h(rt, htotals, totals, sizeof(*htotals) * 8u) || hapgpu_rt_sync(rt))
            return HapResult_Internal_Error;
        measure_result(road.measure, htotals, width, height);
        return HapResult_No_Error;
    }
    if (dst != picture && picture_unstage(rt, picture, dst, &shape))
        return HapResult_Internal_Error;
    if (hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    return HapResult_No_Error;
}

/* ============================================================= frames to pixels */
/* Hap frames -> RGBA8 pictures with nothing but frames going in and pixels coming out: the second stage of a slice of
   frames is undone into a scratch of block textures (one batch through hapb_decode: texture 0, and the RGTC1 alpha
   plane of Hap Q Alpha frames), then every picture is expanded by the block decoder on the same stream.  What a
   player without texture sampling of its own asks of a Hap decoder (the reference leaves this step to the GPU's
   texture units, hap.h:92-95 "the texture format the frame decodes to"). */
#define PICTURE_KINDS_MAX 4u                    /* texture formats one road decodes */
typedef char slice_members_hold_layers[HAPGPU_COMPOSITE_MAX_LAYERS <= HAP_SLICE_MEMBERS_MAX ? 1 : -1];

/* The second stage of a slice of a call's output frames into texture scratch, for everything that goes on from block
   textures (hapb_road_frames, hapb_composite_frames, hapb_transcode).  An output frame has at.member_count members --
   one, or a layer each --, member m of the call's output frame f being the call's input f * member_count + m.  Entry
   f * at.entries_per_frame + at.entry_of[m] + t is texture t of member m of the slice's frame f: the colour texture at
   at.per_frame * f + at.offset_of[m] of the slice's D_BC_TEX scratch, the RGTC1 alpha plane at + at.alpha_off
   (hap_slice.h).  The textures of one member stay adjacent: hapb_decode uploads a host frame once for them. */
typedef struct slice_textures {
    hap_slice_layout at;
    const hap_place_layout *placed;         /* (members of sizes of their own: their blocks and planes; else NULL) */
    unsigned width, height;
    /* per entry, one allocation (`in` is its start): what hapb_decode is given ... */
    const void **in;
    unsigned long *in_bytes, *caps;
    unsigned *idx;
    HapGpuRegion *decode_regions;           /* (a call with a rectangle per frame; else NULL) */
    /* ... and what it gives back: the texture's address, bytes, format and result */
    void **outs;
    unsigned long *used;
    unsigned *fmts, *res;
} slice_textures;

/* the blocks of member m's textures, and how far behind its colour texture its plane lies */
static size_t member_blocks(const slice_textures *s, unsigned m)
{
    return s->placed ? s->placed->blocks_of[m] : s->at.blocks;
}

static size_t member_alpha_off(const slice_textures *s, unsigned m)
{
    return s->placed ? s->placed->alpha_off_of[m] : s->at.alpha_off;
}

/* the arrays of a slice's entries, s->at being laid out.  0: out of memory */
static int slice_textures_alloc(slice_textures *s, int rectangles)
{
    const size_t entries = s->at.slice * s->at.entries_per_frame;
    s->in = (const void **)malloc(entries * (2u * sizeof(void *) + 3u * sizeof(unsigned long) + 3u * sizeof(unsigned) +
                                             (rectangles ? sizeof(HapGpuRegion) : 0u)));
    if (!s->in)
        return 0;
    s->outs = (void **)(s->in + entries);
    s->in_bytes = (unsigned long *)(s->outs + entries);
    s->caps = s->in_bytes + entries;
    s->used = s->caps + entries;
    s->idx = (unsigned *)(s->used + entries);
    s->fmts = s->idx + entries;
    s->res = s->fmts + entries;
    s->decode_regions = rectangles ? (HapGpuRegion *)(s->res + entries) : NULL;
    return 1;
}

/* counts: the members' texture counts (NULL: all 1); extra_per_frame: what else the caller holds per frame while a
   slice's textures are held; rectangles != 0: room for a rectangle per entry.  0: out of memory */
static int slice_textures_init(slice_textures *s, unsigned frame_count, unsigned member_count, const unsigned *counts,
                               unsigned width, unsigned height, size_t extra_per_frame, int rectangles)
{
    s->placed = NULL;
    s->width = width;
    s->height = height;
    hap_slice_layout_of(&s->at, member_count, counts, width, height, extra_per_frame, frame_count);
    return slice_textures_alloc(s, rectangles);
}

/* ... for members of sizes of their own (`placed`: their layout, which the caller keeps while s is used); whole frames
   alone: width and height are no member's and 0 */
static int slice_textures_init_placed(slice_textures *s, const hap_place_layout *placed)
{
    s->placed = placed;
    s->width = 0u;
    s->height = 0u;
    s->at = placed->at;
    return slice_textures_alloc(s, 0);
}

/* Output frames done .. done + n of the call (n <= s->at.slice) into `textures`, at.per_frame * n bytes of D_BC_TEX
   scratch.  road (NULL: whole textures) -- its region: the rectangle wanted of every frame -- or, with region_xs and
   region_ys, its size alone, frame f's origin being (xs[f], ys[f]): a frame whose origin puts the rectangle off the grid or
   past an edge goes to hapb_decode with a NULL input, its Bad_Arguments, and nothing of it is decoded.  Its resize: frame
   f's rectangle is its crop at scale_log2 rounded outward to the blocks (hapb_resize_region), and a crop that is none
   refuses its frame alike. */
static void slice_textures_decode(HapGpuContext *ctx, const slice_textures *s, uint8_t *textures, const void *const *inputs,
                                  const unsigned long *input_bytes, size_t done, unsigned n, const HapbRoad *road,
                                  unsigned flags)
{
    const unsigned width = s->width, height = s->height, members = s->at.member_count;
    const HapGpuRegion whole = {width, 0u, 0u, width, height};
    const HapGpuRegion *const region = road ? road->region : NULL;
    const unsigned *const xs = road ? road->region_xs : NULL, *const ys = road ? road->region_ys : NULL;
    const HapbResize *const resize = road ? road->resize : NULL;
    const unsigned scale_log2 = road ? road->scale_log2 : 0u;
    HapbDecodeArgs args = {s->idx, NULL, NULL, 0, NULL, 0u, NULL, NULL};
    unsigned f, m, t;
    int any_skip = 0;
    for (f = 0; f < n; f++) {
        /* (frame done + f of the call: the origins are the call's, not the slice's) */
        HapGpuRegion own = whole;
        int refused = 0;
        if (xs) {
            own.x = xs[done + f];
            own.y = ys[done + f];
            own.w = region->w;
            own.h = region->h;
            refused = !hapb_region_fits(&own, height);
        } else if (resize) {
            refused = !hapb_resize_region(resize, done + f, width, height, scale_log2, &own);
        }
        if (refused)
            own = whole;
        else if (own.x != 0u || own.y != 0u || own.w != width || own.h != height)
            any_skip = 1;
        for (m = 0; m < members; m++)
            for (t = 0; t < s->at.count_of[m]; t++) {
                const size_t e = (size_t)f * s->at.entries_per_frame + s->at.entry_of[m] + t;
                if (s->decode_regions)
                    s->decode_regions[e] = own;
                s->in[e] = refused ? NULL : inputs[(done + f) * members + m];
                s->in_bytes[e] = input_bytes[(done + f) * members + m];
                s->outs[e] = textures + s->at.per_frame * f + s->at.offset_of[m] + (t ? member_alpha_off(s, m) : 0u);
                s->caps[e] = (unsigned long)(t ? member_blocks(s, m) * 8u : member_blocks(s, m) * 16u);
                s->idx[e] = t;
                s->used[e] = 0;
                s->fmts[e] = 0;
            }
    }
    /* (rectangles that are all the whole frame skip nothing -- one that is among others needs everything -- and nor does
       one rectangle for all that is the whole frame) */
    if (xs || resize)
        args.regions = any_skip ? s->decode_regions : NULL;
    else if (region && !(region->x == 0u && region->y == 0u && region->w == width && region->h == height))
        args.region = region;
    hapb_decode(ctx, n * s->at.entries_per_frame, s->in, s->in_bytes, 0, s->outs, s->caps, s->used, s->fmts, s->res,
                flags & ~HAPGPU_DECODE_BPTC_PICTURES, &args);
}

/* 1: entry e of a decoded slice (and, count 2, entry e + 1) holds what the caller's geometry says: a colour texture of
   `kinds`, of exactly width x height, and (two textures) an RGTC1 plane of the same geometry */
static int slice_entry_fits(const slice_textures *s, size_t e, unsigned count, const unsigned *kinds, unsigned kind_count)
{
    const unsigned fmt = s->fmts[e];
    return kind_of(kinds, kind_count, fmt) != kind_count && s->used[e] == s->at.blocks * hapf_block_bytes(fmt) &&
           (count != 2u || (s->fmts[e + 1] == HapTextureFormat_A_RGTC1 && s->used[e + 1] == s->at.blocks * 8u));
}

/* ... for member m of a slice whose members have sizes of their own: exactly that member's blocks */
static int slice_entry_fits_member(const slice_textures *s, size_t e, unsigned m, const unsigned *kinds, unsigned kind_count)
{
    const unsigned fmt = s->fmts[e];
    const size_t blocks = member_blocks(s, m);
    return kind_of(kinds, kind_count, fmt) != kind_count && s->used[e] == blocks * hapf_block_bytes(fmt) &&
           (s->at.count_of[m] != 2u || (s->fmts[e + 1] == HapTextureFormat_A_RGTC1 && s->used[e + 1] == blocks * 8u));
}

/* frames down a road (DESIGN.md's `decode_pictures`, its roads' descriptions being `picture_road`s): one picture each */
unsigned hapb_road_frames(HapGpuContext *ctx, unsigned frame_count, const void *const *inputs,
                          const unsigned long *input_bytes, unsigned texture_count, void *const *rgba_frames,
                          unsigned width, unsigned height, unsigned long row_bytes, unsigned *results, unsigned flags,
                          const HapbRoad *proad)
{
    const HapbRoad taken = road_taken(proad), *const road = &taken;
    hapgpu_rt *rt = ctx->rt;
    const unsigned *kinds;
    unsigned paired;
    const unsigned kind_count = road_formats(road, &kinds, &paired);
    size_t done;
    unsigned first_error = HapResult_No_Error, f;
    slice_textures s;
    /* (the pictures' geometry: the frames', a scaled road's fraction of it, or the rectangle's) */
    const unsigned picture_height = picture_height_of(road, height);
    const size_t pixel_row = (size_t)picture_width_of(road, width) * picture_texel_bytes(road);
    const unsigned align = picture_align_mask(road);
    const int per_frame_regions = road->region_xs != NULL || road->resize != NULL;
    const size_t frame_words = road->resize ? 4u : 1u;      /* what travels behind the table per frame */
    picture_shape shape = {row_bytes, pixel_row, 0u, picture_height};
    if (frame_count == 0)
        return HapResult_No_Error;
    if (!results)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, results, frame_count))
        return HapResult_Internal_Error;
    if (!inputs || !input_bytes || !rgba_frames || texture_count == 0 || texture_count > 2 || width == 0 ||
        height == 0 || (width & 3u) || (height & 3u) || row_bytes < pixel_row || (row_bytes & align) ||
        (road->region && (road->region->width != width || !hapb_region_fits(road->region, height))) ||
        (road->resize && (!hapb_resize_out_valid(road->resize) || !road->resize->xs || !road->resize->ys ||
                          !road->resize->ws || !road->resize->hs)) ||
        (road->planes && !planes_fit(road, pixel_row, picture_height, row_bytes)) ||
        (road->video && (!road->video->chroma ||
                         !hapb_video_decode_valid(width, height, road->scale_log2, row_bytes, road->video))) ||
        (road->picture_kind == HAPGPU_PICTURE_A8 && height / 4u > 65535u)) {
        for (f = 0; f < frame_count; f++)
            results[f] = HapResult_Bad_Arguments;
        return HapResult_Bad_Arguments;
    }
    /* (a measuring road: a frame that is not measured has an all-zero struct) */
    if (road->measure)
        memset(road->measure, 0, sizeof(*road->measure) * frame_count);
    shape.bytes = (size_t)row_bytes * (picture_height - 1u) + pixel_row;
    if (!slice_textures_init(&s, frame_count, 1u, &texture_count, width, height, 0u, per_frame_regions)) {
        for (f = 0; f < frame_count; f++)
            results[f] = HapResult_Internal_Error;
        return HapResult_Internal_Error;
    }
    for (done = 0; done < frame_count; done += s.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.at.slice ? frame_count - done : s.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.at.per_frame * n);
        uint8_t *stage = NULL;
        const unsigned long long *htotals_of_slice = NULL;
        int rc = 0;
        if (!textures) {
            for (f = 0; f < n; f++)
                results[done + f] = HapResult_Internal_Error;
            first_error = first_error ? first_error : HapResult_Internal_Error;
            continue;
        }
        slice_textures_decode(ctx, &s, textures, inputs, input_bytes, done, n, road, flags);
        {
            /* one block-decode launch per texture format present in the slice: [textures][alpha planes][pictures] in a
               small device table, pictures of other formats (or that failed) with a texture address of 0 */
            /* ... and behind the table, in the same copy, a rectangle per frame's first texture block of every picture -- or,
               resized, every picture's crop: four words, x, y, w, h */
            /* ... and, in the pinned copy alone, a measuring road's totals of every picture on their way back */
            const size_t ptr_words = (size_t)3u * PICTURE_KINDS_MAX * n;
            const size_t tab_bytes = sizeof(uint64_t) * ptr_words + (per_frame_regions ? sizeof(uint32_t) * frame_words * n : 0u);
            const size_t totals_bytes = road->measure ? sizeof(unsigned long long) * 8u * n : 0u;
            uint64_t *htab = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, align_up(tab_bytes, 8) + totals_bytes);
            uint64_t *dtab = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, tab_bytes);
            uint32_t *partials = NULL;
            unsigned long long *totals = road->measure ? measure_scratch(rt, n, width, height, &partials) : NULL;
            const unsigned long long *htotals = htab ? (const unsigned long long *)((const uint8_t *)htab + align_up(tab_bytes, 8)) : NULL;
            uint32_t *horigins = per_frame_regions && htab ? (uint32_t *)(htab + ptr_words) : NULL;
            const uint32_t *dorigins = per_frame_regions && dtab ? (const uint32_t *)(dtab + ptr_words) : NULL;
            unsigned present = 0, k;
            int wide = (row_bytes & 15u) == 0 && !ctx->no_wide_planes;      /* A8 pictures: every one of the slice 16-byte aligned, and the pitch */
            if (!htab || !dtab || (road->measure && !totals)) {
                for (f = 0; f < n; f++)
                    results[done + f] = HapResult_Internal_Error;
                first_error = first_error ? first_error : HapResult_Internal_Error;
                continue;
            }
            memset(htab, 0, tab_bytes);
            for (f = 0; f < n; f++) {
                const size_t e = (size_t)f * texture_count;
                void *dst = rgba_frames[done + f];
                unsigned r = s.res[e];
                k = kind_of(kinds, kind_count, s.fmts[e]);
                if (r == HapResult_No_Error && texture_count == 2)
                    r = s.res[e + 1];
                /* (no Hap variant pairs a BC7 texture with a second one) */
                if (texture_count == 2 && s.res[e] == HapResult_No_Error && k < kind_count && !(paired >> k & 1u))
                    r = HapResult_Bad_Arguments;
                if (r == HapResult_No_Error && !dst)
                    r = HapResult_Bad_Arguments;
                /* the frame must hold what the caller's geometry says, in a format of the road (BC7 only when the caller
                   asked for Hap R pictures) */
                if (r == HapResult_No_Error && !slice_entry_fits(&s, e, texture_count, kinds, kind_count))
                    r = HapResult_Bad_Arguments;
                /* (a video picture's other plane: NULL, in host memory or misaligned refuses the frame) */
                if (r == HapResult_No_Error && road->video && !chroma_plane_fits(ctx, road->video->chroma[done + f]))
                    r = HapResult_Bad_Arguments;
                if (r == HapResult_No_Error && (road->planes || road->measure || road->video) && !is_dev(ctx, dst)) {
                    r = HapResult_Bad_Arguments;        /* tensors, reference and video pictures live in device memory: no host staging road */
                } else if (r == HapResult_No_Error && !is_dev(ctx, dst)) {
                    dst = picture_stage(rt, &stage, align_up(shape.bytes, 256), n, f);
                    if (!dst)
                        r = HapResult_Internal_Error;
                } else if (r == HapResult_No_Error && ((uintptr_t)dst & align)) {
                    r = HapResult_Bad_Arguments;
                }
                if (r == HapResult_No_Error) {
                    present |= 1u << k;
                    if ((uintptr_t)dst & 15u)
                        wide = 0;
                    htab[(size_t)k * 3u * n + f] = (uint64_t)(uintptr_t)s.outs[e];
                    htab[(size_t)k * 3u * n + n + f] = road->video ? (uint64_t)(uintptr_t)road->video->chroma[done + f] :
                                                       texture_count == 2 ? (uint64_t)(uintptr_t)s.outs[e + 1] : 0u;
                    htab[(size_t)k * 3u * n + 2u * n + f] = (uint64_t)(uintptr_t)dst;
                    if (horigins && road->resize) {     /* (a crop of the frame: a refused one never gets here) */
                        horigins[4u * f] = road->resize->xs[done + f];
                        horigins[4u * f + 1u] = road->resize->ys[done + f];
                        horigins[4u * f + 2u] = road->resize->ws[done + f];
                        horigins[4u * f + 3u] = road->resize->hs[done + f];
                    } else if (horigins) {              /* (inside the frame: a refused origin never gets here) */
                        horigins[f] = region_first_block(width, road->region_xs[done + f], road->region_ys[done + f]);
                    }
                }
                results[done + f] = r;
            }
            if (present) {
                rc |= hapgpu_rt_h2d(rt, dtab, htab, tab_bytes);
                for (k = 0; k < kind_count; k++)
                    if (present & (1u << k)) {
                        const uint64_t *col = dtab + (size_t)k * 3u * n;
                        const HapGpuPictureTable t = {{col, col + n, col + 2u * (size_t)n}, {0u, 0u, 0u}};
                        rc |= launch_block_decode(rt, road, &t, n, texture_count == 2, width, height, kinds[k], row_bytes,
                                                  wide, dorigins, partials, totals);
                    }
                if (road->measure) {
                    rc |= hapgpu_rt_d2h(rt, (void *)htotals, totals, totals_bytes);
                    htotals_of_slice = htotals;
                }
                for (f = 0; f < n; f++)
                    if (results[done + f] == HapResult_No_Error && stage && !is_dev(ctx, rgba_frames[done + f]))
                        rc |= picture_unstage(rt, rgba_frames[done + f], stage + align_up(shape.bytes, 256) * f, &shape);
            }
        }
        rc |= hapgpu_rt_sync(rt);
        if (rc)
            for (f = 0; f < n; f++)
                if (results[done + f] == HapResult_No_Error)
                    results[done + f] = HapResult_Internal_Error;
        /* (the totals have arrived: every picture of a launch got its own eight) */
        if (road->measure && htotals_of_slice)
            for (f = 0; f < n; f++)
                if (results[done + f] == HapResult_No_Error)
                    measure_result(&road->measure[done + f], htotals_of_slice + 8u * (size_t)f, width, height);
        for (f = 0; f < n; f++)
            if (results[done + f] != HapResult_No_Error && first_error == HapResult_No_Error)
                first_error = results[done + f];
    }
    free(s.in);
    return first_error;
}

/* ============================================================= compositing */
/* Layers of textures or frames "over" a background colour -> one RGBA8 picture per output frame, by bc_composite.hip:
   the layers' pictures never exist.  The textures form stages what lies in host memory into D_BC_TEX; the frames form
   runs the second stage of all frameCount * layerCount frames of a slice in one batch into D_BC_TEX, as hapb_road_frames
   does, a layer being a member of slice_textures with a texture count of its own, and one composite launch per slice
   follows.  The descriptors and the pictures' addresses go out in one small table. */

static const unsigned char k_composite_background[4] = {0u, 0u, 0u, 255u};
/* (the public limit is the kernel's) */
typedef char composite_limits_agree[HAPGPU_COMPOSITE_MAX_LAYERS == HAPGPU_COMPOSITE_LAYERS_MAX ? 1 : -1];

/* the colour formats a layer may have */
static int composite_format(unsigned format)
{
    return format == HapTextureFormat_RGB_DXT1 || format == HapTextureFormat_RGBA_DXT5 || format == HapTextureFormat_YCoCg_DXT5;
}

int hapb_composite_valid(unsigned layer_count, unsigned width, unsigned height, unsigned long row_bytes,
                         const unsigned *texture_counts)
{
    unsigned l;
    if (layer_count == 0 || layer_count > HAPGPU_COMPOSITE_MAX_LAYERS || width == 0 || height == 0 || (width & 3u) ||
        (height & 3u) || row_bytes < (unsigned long)width * 4u || (row_bytes & 15u))
        return 0;
    for (l = 0; texture_counts && l < layer_count; l++)
        if (texture_counts[l] != 1u && texture_counts[l] != 2u)
            return 0;
    return 1;
}

/* the table of a composite launch for n pictures of layer_count layers: [n] picture addresses, then [n][layer_count]
   descriptors; *device gets its device copy's address (filled by the caller's h2d of `bytes`) */
static uint64_t *composite_table(hapgpu_rt *rt, unsigned n, unsigned layer_count, uint64_t **device, size_t *bytes)
{
    uint64_t *htab;
    *bytes = sizeof(uint64_t) * n + sizeof(HapGpuCompositeLayer) * (size_t)n * layer_count;
    htab = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, *bytes);
    *device = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, *bytes);
    if (!htab || !*device)
        return NULL;
    memset(htab, 0, *bytes);
    return htab;
}

unsigned hapb_composite_textures(HapGpuContext *ctx, unsigned layer_count, const void *const *textures,
                                 const unsigned long *texture_bytes, const unsigned *formats,
                                 const void *const *alphas, const unsigned long *alpha_bytes,
                                 const unsigned char *opacities, const unsigned char *background, unsigned width,
                                 unsigned height, void *picture, unsigned long row_bytes)
{
    hapgpu_rt *rt = ctx->rt;
    const size_t blocks = (size_t)(width / 4u) * (height / 4u), pixel_row = (size_t)width * 4u;
    const picture_shape shape = {row_bytes, pixel_row, (size_t)row_bytes * (height ? height - 1u : 0u) + pixel_row, height};
    size_t staged = 0, tab_bytes, at = 0;
    uint64_t *htab, *dtab;
    HapGpuCompositeLayer *hlayers;
    uint8_t *stage = NULL, *picture_staged = NULL;
    void *dst = picture;
    unsigned l;
    int rc;
    if (!hapb_composite_valid(layer_count, width, height, row_bytes, NULL) || !textures || !texture_bytes || !formats ||
        !picture)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    /* every layer: HapGpuDecompressRGBA's rules for its texture and its plane */
    for (l = 0; l < layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL;
        const size_t need = composite_format(formats[l]) ? blocks * hapf_block_bytes(formats[l]) : 0u;
        if (!textures[l] || !need || texture_bytes[l] < need || (alpha && (!alpha_bytes || alpha_bytes[l] < blocks * 8u)) ||
            (is_dev(ctx, textures[l]) && ((uintptr_t)textures[l] & (hapf_block_bytes(formats[l]) - 1u))) ||
            (alpha && is_dev(ctx, alpha) && ((uintptr_t)alpha & 7u)))
            return HapResult_Bad_Arguments;
        if (!is_dev(ctx, textures[l]))
            staged += align_up(need, 256);
        if (alpha && !is_dev(ctx, alpha))
            staged += align_up(blocks * 8u, 256);
    }
    if (is_dev(ctx, picture) && ((uintptr_t)picture & 15u))
        return HapResult_Bad_Arguments;
    /* (one request for all that is staged: an arena that grows forgets what it held) */
    if (staged && !(stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, staged)))
        return HapResult_Internal_Error;
    if (!is_dev(ctx, picture) && !(dst = picture_stage(rt, &picture_staged, shape.bytes, 1u, 0u)))
        return HapResult_Internal_Error;
    htab = composite_table(rt, 1u, layer_count, &dtab, &tab_bytes);
    if (!htab)
        return HapResult_Internal_Error;
    hlayers = (HapGpuCompositeLayer *)(htab + 1);
    htab[0] = (uint64_t)(uintptr_t)dst;
    for (l = 0; l < layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL, *src = textures[l];
        if (!is_dev(ctx, src)) {
            const size_t need = blocks * hapf_block_bytes(formats[l]);
            if (hapgpu_rt_h2d(rt, stage + at, src, need))
                return HapResult_Internal_Error;
            src = stage + at;
            at += align_up(need, 256);
        }
        if (alpha && !is_dev(ctx, alpha)) {
            if (hapgpu_rt_h2d(rt, stage + at, alpha, blocks * 8u))
                return HapResult_Internal_Error;
            alpha = stage + at;
            at += align_up(blocks * 8u, 256);
        }
        hlayers[l].texture = (uint64_t)(uintptr_t)src;
        hlayers[l].alpha = (uint64_t)(uintptr_t)alpha;
        hlayers[l].format = formats[l];
        hlayers[l].opacity = opacities ? opacities[l] : 255u;
    }
    if (hapgpu_rt_h2d(rt, dtab, htab, tab_bytes))
        return HapResult_Internal_Error;
    rc = hapgpu_k_block_composite(rt, (const HapGpuCompositeLayer *)(dtab + 1), layer_count, dtab, 1u,
                                  background ? background : k_composite_background, width, height, row_bytes);
    if (rc == 1)
        return HapResult_Bad_Arguments;
    if (rc)
        return HapResult_Internal_Error;
    if (dst != picture && picture_unstage(rt, picture, dst, &shape))
        return HapResult_Internal_Error;
    if (hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    return HapResult_No_Error;
}

unsigned hapb_composite_frames(HapGpuContext *ctx, unsigned frame_count, unsigned layer_count, const void *const *inputs,
                               const unsigned long *input_bytes, const unsigned *texture_counts,
                               const unsigned char *opacities, const unsigned char *background, void *const *rgba_frames,
                               unsigned width, unsigned height, unsigned long row_bytes, unsigned *results, unsigned flags)
{
    hapgpu_rt *rt = ctx->rt;
    const size_t pixel_row = (size_t)width * 4u;
    const picture_shape shape = {row_bytes, pixel_row, (size_t)row_bytes * (height ? height - 1u : 0u) + pixel_row, height};
    const size_t total = (size_t)frame_count * layer_count;
    size_t done, i;
    unsigned first_error = HapResult_No_Error, f, l;
    slice_textures s;
    if (!results)
        return HapResult_Bad_Arguments;
    if (!hapb_composite_valid(layer_count, width, height, row_bytes, texture_counts) || !inputs || !input_bytes ||
        !rgba_frames) {
        for (i = 0; i < total; i++)
            results[i] = HapResult_Bad_Arguments;
        return HapResult_Bad_Arguments;
    }
    if (frame_count == 0)
        return HapResult_No_Error;
    /* output frames of a slice: at most 4 GiB of block textures and 32768 entries of the second stage at a time */
    if (context_busy(ctx, NULL, 0) || !slice_textures_init(&s, frame_count, layer_count, texture_counts, width, height, 0u, 0)) {
        for (i = 0; i < total; i++)
            results[i] = HapResult_Internal_Error;
        return HapResult_Internal_Error;
    }
    for (done = 0; done < frame_count; done += s.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.at.slice ? frame_count - done : s.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.at.per_frame * n);
        uint8_t *stage = NULL;
        uint64_t *htab = NULL, *dtab = NULL;
        HapGpuCompositeLayer *hlayers;
        size_t tab_bytes = 0;
        unsigned present = 0;
        int rc = 0;
        if (textures) {
            /* the second stage of every layer of every output frame of the slice, one batch */
            slice_textures_decode(ctx, &s, textures, inputs, input_bytes, done, n, NULL, flags);
            /* (after the second stage, which has tables of its own) */
            htab = composite_table(rt, n, layer_count, &dtab, &tab_bytes);
        }
        if (!htab) {
            for (i = done * layer_count; i < (done + n) * layer_count; i++)
                results[i] = HapResult_Internal_Error;
            first_error = first_error ? first_error : HapResult_Internal_Error;
            continue;
        }
        hlayers = (HapGpuCompositeLayer *)(htab + n);
        for (f = 0; f < n; f++) {
            unsigned *frame_results = results + (done + f) * layer_count;
            void *dst = rgba_frames[done + f];
            unsigned picture = HapResult_No_Error, all = HapResult_No_Error;
            for (l = 0; l < layer_count; l++) {
                const unsigned count = s.at.count_of[l];
                const size_t e = (size_t)f * s.at.entries_per_frame + s.at.entry_of[l];
                HapGpuCompositeLayer *d = &hlayers[(size_t)f * layer_count + l];
                unsigned r = s.res[e];
                if (r == HapResult_No_Error && count == 2u)
                    r = s.res[e + 1];
                /* the frame must hold what the caller's geometry says, in one of the three formats a layer may have */
                if (r == HapResult_No_Error && !slice_entry_fits(&s, e, count, k_rgba_kinds, 3u))
                    r = HapResult_Bad_Arguments;
                frame_results[l] = r;
                if (r != HapResult_No_Error && all == HapResult_No_Error)
                    all = r;
                d->texture = (uint64_t)(uintptr_t)s.outs[e];
                d->alpha = count == 2u ? (uint64_t)(uintptr_t)s.outs[e + 1] : 0u;
                d->format = s.fmts[e];
                d->opacity = opacities ? opacities[(done + f) * layer_count + l] : 255u;
            }
            /* the picture: NULL or misaligned fails every layer's entry; host pictures are staged */
            if (!dst || (is_dev(ctx, dst) && ((uintptr_t)dst & 15u))) {
                picture = HapResult_Bad_Arguments;
            } else if (all == HapResult_No_Error && !is_dev(ctx, dst)) {
                dst = picture_stage(rt, &stage, align_up(shape.bytes, 256), n, f);
                if (!dst)
                    picture = HapResult_Internal_Error;
            }
            if (picture != HapResult_No_Error)
                for (l = 0; l < layer_count; l++)
                    frame_results[l] = picture;
            /* (an output frame that is not written: picture address 0 skips it) */
            if (picture == HapResult_No_Error && all == HapResult_No_Error) {
                htab[f] = (uint64_t)(uintptr_t)dst;
                present = 1;
            }
        }
        if (present) {
            rc |= hapgpu_rt_h2d(rt, dtab, htab, tab_bytes);
            rc |= hapgpu_k_block_composite(rt, (const HapGpuCompositeLayer *)(dtab + n), layer_count, dtab, n,
                                           background ? background : k_composite_background, width, height, row_bytes);
            for (f = 0; f < n; f++)
                if (htab[f] && !is_dev(ctx, rgba_frames[done + f]))
                    rc |= picture_unstage(rt, rgba_frames[done + f], stage + align_up(shape.bytes, 256) * f, &shape);
        }
        rc |= hapgpu_rt_sync(rt);
        for (i = done * layer_count; i < (done + n) * layer_count; i++) {
            if (rc && results[i] == HapResult_No_Error && htab[i / layer_count - done])
                results[i] = HapResult_Internal_Error;
            if (results[i] != HapResult_No_Error && first_error == HapResult_No_Error)
                first_error = results[i];
        }
    }
    free(s.in);
    return first_error;
}

/* ------------------------------------------------------------- ... of layers placed on the canvas */
/* The two calls above for layers of sizes of their own, each with a rectangle of it placed and clipped on the canvas
   (hap_place.h: the rules and the clip; bc_composite.hip's placed kernel).  A descriptor carries its layer's clip in
   blocks; the second stage still decodes every layer's whole frame, into a scratch laid out by hap_place_layout_of. */

int hapb_composite_placed_valid(unsigned layer_count, const unsigned *layer_widths, const unsigned *layer_heights,
                                const HapGpuPlacement *placements, size_t frame_count, unsigned width, unsigned height,
                                unsigned long row_bytes, const unsigned *texture_counts)
{
    size_t f;
    unsigned l;
    if (!hapb_composite_valid(layer_count, width, height, row_bytes, texture_counts) || !layer_widths || !layer_heights ||
        !hap_place_layer_valid(width, height))
        return 0;
    for (l = 0; l < layer_count; l++)
        if (!hap_place_layer_valid(layer_widths[l], layer_heights[l]))
            return 0;
    for (f = 0; placements && f < frame_count; f++)
        for (l = 0; l < layer_count; l++) {
            const HapGpuPlacement *p = &placements[f * layer_count + l];
            if (!hap_place_valid(p->srcX, p->srcY, p->width, p->height, p->dstX, p->dstY, layer_widths[l], layer_heights[l]))
                return 0;
        }
    return 1;
}

/* a descriptor's six clip words: placement p (NULL: the layer whole at (0, 0)) of a layer_w x layer_h layer on the canvas */
static void placed_layer_clip(HapGpuPlacedLayer *d, const HapGpuPlacement *p, unsigned layer_w, unsigned layer_h,
                              unsigned width, unsigned height)
{
    const HapGpuPlacement whole = {0u, 0u, layer_w, layer_h, 0, 0};
    hap_place_clip c;
    if (!p)
        p = &whole;
    hap_place_clip_of(&c, p->srcX, p->srcY, p->width, p->height, p->dstX, p->dstY, layer_w, width, height);
    d->cx0 = c.cx0;
    d->cy0 = c.cy0;
    d->cw = c.cw;
    d->ch = c.ch;
    d->first = c.first;
    d->layer_blocks_x = c.layer_blocks_x;
}

/* composite_table's for placed layers */
static uint64_t *composite_placed_table(hapgpu_rt *rt, unsigned n, unsigned layer_count, uint64_t **device, size_t *bytes)
{
    uint64_t *htab;
    *bytes = sizeof(uint64_t) * n + sizeof(HapGpuPlacedLayer) * (size_t)n * layer_count;
    htab = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, *bytes);
    *device = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, *bytes);
    if (!htab || !*device)
        return NULL;
    memset(htab, 0, *bytes);
    return htab;
}

unsigned hapb_composite_textures_placed(HapGpuContext *ctx, unsigned layer_count, const void *const *textures,
                                        const unsigned long *texture_bytes, const unsigned *formats,
                                        const void *const *alphas, const unsigned long *alpha_bytes,
                                        const unsigned *layer_widths, const unsigned *layer_heights,
                                        const HapGpuPlacement *placements, const unsigned char *opacities,
                                        const unsigned char *background, unsigned width, unsigned height, void *picture,
                                        unsigned long row_bytes)
{
    hapgpu_rt *rt = ctx->rt;
    const size_t pixel_row = (size_t)width * 4u;
    const picture_shape shape = {row_bytes, pixel_row, (size_t)row_bytes * (height ? height - 1u : 0u) + pixel_row, height};
    size_t staged = 0, tab_bytes, at = 0;
    uint64_t *htab, *dtab;
    HapGpuPlacedLayer *hlayers;
    uint8_t *stage = NULL, *picture_staged = NULL;
    void *dst = picture;
    unsigned l;
    int rc;
    if (!hapb_composite_placed_valid(layer_count, layer_widths, layer_heights, placements, 1u, width, height, row_bytes, NULL) ||
        !textures || !texture_bytes || !formats || !picture)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    /* every layer: HapGpuDecompressRGBA's rules for its texture and its plane, at the layer's own size */
    for (l = 0; l < layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL;
        const size_t blocks = (size_t)(layer_widths[l] / 4u) * (layer_heights[l] / 4u);
        const size_t need = composite_format(formats[l]) ? blocks * hapf_block_bytes(formats[l]) : 0u;
        if (!textures[l] || !need || texture_bytes[l] < need || (alpha && (!alpha_bytes || alpha_bytes[l] < blocks * 8u)) ||
            (is_dev(ctx, textures[l]) && ((uintptr_t)textures[l] & (hapf_block_bytes(formats[l]) - 1u))) ||
            (alpha && is_dev(ctx, alpha) && ((uintptr_t)alpha & 7u)))
            return HapResult_Bad_Arguments;
        if (!is_dev(ctx, textures[l]))
            staged += align_up(need, 256);
        if (alpha && !is_dev(ctx, alpha))
            staged += align_up(blocks * 8u, 256);
    }
    if (is_dev(ctx, picture) && ((uintptr_t)picture & 15u))
        return HapResult_Bad_Arguments;
    /* (one request for all that is staged: an arena that grows forgets what it held) */
    if (staged && !(stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, staged)))
        return HapResult_Internal_Error;
    if (!is_dev(ctx, picture) && !(dst = picture_stage(rt, &picture_staged, shape.bytes, 1u, 0u)))
        return HapResult_Internal_Error;
    htab = composite_placed_table(rt, 1u, layer_count, &dtab, &tab_bytes);
    if (!htab)
        return HapResult_Internal_Error;
    hlayers = (HapGpuPlacedLayer *)(htab + 1);
    htab[0] = (uint64_t)(uintptr_t)dst;
    for (l = 0; l < layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL, *src = textures[l];
        const size_t blocks = (size_t)(layer_widths[l] / 4u) * (layer_heights[l] / 4u);
        if (!is_dev(ctx, src)) {
            const size_t need = blocks * hapf_block_bytes(formats[l]);
            if (hapgpu_rt_h2d(rt, stage + at, src, need))
                return HapResult_Internal_Error;
            src = stage + at;
            at += align_up(need, 256);
        }
        if (alpha && !is_dev(ctx, alpha)) {
            if (hapgpu_rt_h2d(rt, stage + at, alpha, blocks * 8u))
                return HapResult_Internal_Error;
            alpha = stage + at;
            at += align_up(blocks * 8u, 256);
        }
        hlayers[l].texture = (uint64_t)(uintptr_t)src;
        hlayers[l].alpha = (uint64_t)(uintptr_t)alpha;
        hlayers[l].format = formats[l];
        hlayers[l].opacity = opacities ? opacities[l] : 255u;
        placed_layer_clip(&hlayers[l], placements ? &placements[l] : NULL, layer_widths[l], layer_heights[l], width, height);
    }
    if (hapgpu_rt_h2d(rt, dtab, htab, tab_bytes))
        return HapResult_Internal_Error;
    rc = hapgpu_k_block_composite_placed(rt, (const HapGpuPlacedLayer *)(dtab + 1), layer_count, dtab, 1u,
                                         background ? background : k_composite_background, width, height, row_bytes);
    if (rc == 1)
        return HapResult_Bad_Arguments;
    if (rc)
        return HapResult_Internal_Error;
    if (dst != picture && picture_unstage(rt, picture, dst, &shape))
        return HapResult_Internal_Error;
    if (hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    return HapResult_No_Error;
}

unsigned hapb_composite_frames_placed(HapGpuContext *ctx, unsigned frame_count, unsigned layer_count,
                                      const void *const *inputs, const unsigned long *input_bytes,
                                      const unsigned *texture_counts, const unsigned *layer_widths,
                                      const unsigned *layer_heights, const HapGpuPlacement *placements,
                                      const unsigned char *opacities, const unsigned char *background,
                                      void *const *rgba_frames, unsigned width, unsigned height, unsigned long row_bytes,
                                      unsigned *results, unsigned flags)
{
    hapgpu_rt *rt = ctx->rt;
    const size_t pixel_row = (size_t)width * 4u;
    const picture_shape shape = {row_bytes, pixel_row, (size_t)row_bytes * (height ? height - 1u : 0u) + pixel_row, height};
    const size_t total = (size_t)frame_count * layer_count;
    size_t done, i;
    unsigned first_error = HapResult_No_Error, f, l;
    hap_place_layout layout;
    slice_textures s;
    if (!results)
        return HapResult_Bad_Arguments;
    if (!hapb_composite_placed_valid(layer_count, layer_widths, layer_heights, placements, frame_count, width, height,
                                     row_bytes, texture_counts) || !inputs || !input_bytes || !rgba_frames) {
        for (i = 0; i < total; i++)
            results[i] = HapResult_Bad_Arguments;
        return HapResult_Bad_Arguments;
    }
    if (frame_count == 0)
        return HapResult_No_Error;
    /* output frames of a slice: at most 4 GiB of block textures and 32768 entries of the second stage at a time */
    hap_place_layout_of(&layout, layer_count, texture_counts, layer_widths, layer_heights, 0u, frame_count);
    if (context_busy(ctx, NULL, 0) || !slice_textures_init_placed(&s, &layout)) {
        for (i = 0; i < total; i++)
            results[i] = HapResult_Internal_Error;
        return HapResult_Internal_Error;
    }
    for (done = 0; done < frame_count; done += s.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.at.slice ? frame_count - done : s.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.at.per_frame * n);
        uint8_t *stage = NULL;
        uint64_t *htab = NULL, *dtab = NULL;
        HapGpuPlacedLayer *hlayers;
        size_t tab_bytes = 0;
        unsigned present = 0;
        int rc = 0;
        if (textures) {
            /* the second stage of every layer of every output frame of the slice, one batch: whole frames */
            slice_textures_decode(ctx, &s, textures, inputs, input_bytes, done, n, NULL, flags);
            /* (after the second stage, which has tables of its own) */
            htab = composite_placed_table(rt, n, layer_count, &dtab, &tab_bytes);
        }
        if (!htab) {
            for (i = done * layer_count; i < (done + n) * layer_count; i++)
                results[i] = HapResult_Internal_Error;
            first_error = first_error ? first_error : HapResult_Internal_Error;
            continue;
        }
        hlayers = (HapGpuPlacedLayer *)(htab + n);
        for (f = 0; f < n; f++) {
            unsigned *frame_results = results + (done + f) * layer_count;
            void *dst = rgba_frames[done + f];
            unsigned picture = HapResult_No_Error, all = HapResult_No_Error;
            for (l = 0; l < layer_count; l++) {
                const unsigned count = s.at.count_of[l];
                const size_t e = (size_t)f * s.at.entries_per_frame + s.at.entry_of[l];
                HapGpuPlacedLayer *d = &hlayers[(size_t)f * layer_count + l];
                unsigned r = s.res[e];
                if (r == HapResult_No_Error && count == 2u)
                    r = s.res[e + 1];
                /* the frame must hold exactly its layer's geometry, in one of the three formats a layer may have: a
                   texture with more blocks than the layer's room holds is of another size like one with fewer */
                if (r == HapResult_Buffer_Too_Small ||
                    (r == HapResult_No_Error && !slice_entry_fits_member(&s, e, l, k_rgba_kinds, 3u)))
                    r = HapResult_Bad_Arguments;
                frame_results[l] = r;
                if (r != HapResult_No_Error && all == HapResult_No_Error)
                    all = r;
                d->texture = (uint64_t)(uintptr_t)s.outs[e];
                d->alpha = count == 2u ? (uint64_t)(uintptr_t)s.outs[e + 1] : 0u;
                d->format = s.fmts[e];
                d->opacity = opacities ? opacities[(done + f) * layer_count + l] : 255u;
                placed_layer_clip(d, placements ? &placements[(done + f) * layer_count + l] : NULL, layer_widths[l],
                                  layer_heights[l], width, height);
            }
            /* the picture: NULL or misaligned fails every layer's entry; host pictures are staged */
            if (!dst || (is_dev(ctx, dst) && ((uintptr_t)dst & 15u))) {
                picture = HapResult_Bad_Arguments;
            } else if (all == HapResult_No_Error && !is_dev(ctx, dst)) {
                dst = picture_stage(rt, &stage, align_up(shape.bytes, 256), n, f);
                if (!dst)
                    picture = HapResult_Internal_Error;
            }
            if (picture != HapResult_No_Error)
                for (l = 0; l < layer_count; l++)
                    frame_results[l] = picture;
            /* (an output frame that is not written: picture address 0 skips it) */
            if (picture == HapResult_No_Error && all == HapResult_No_Error) {
                htab[f] = (uint64_t)(uintptr_t)dst;
                present = 1;
            }
        }
        if (present) {
            rc |= hapgpu_rt_h2d(rt, dtab, htab, tab_bytes);
            rc |= hapgpu_k_block_composite_placed(rt, (const HapGpuPlacedLayer *)(dtab + n), layer_count, dtab, n,
                                                  background ? background : k_composite_background, width, height,
                                                  row_bytes);
            for (f = 0; f < n; f++)
                if (htab[f] && !is_dev(ctx, rgba_frames[done + f]))
                    rc |= picture_unstage(rt, rgba_frames[done + f], stage + align_up(shape.bytes, 256) * f, &shape);
        }
        rc |= hapgpu_rt_sync(rt);
        for (i = done * layer_count; i < (done + n) * layer_count; i++) {
            if (rc && results[i] == HapResult_No_Error && htab[i / layer_count - done])
                results[i] = HapResult_Internal_Error;
            if (results[i] != HapResult_No_Error && first_error == HapResult_No_Error)
                first_error = results[i];
        }
    }
    free(s.in);
    return first_error;
}

/* ============================================================= transcode */
/* Frames -> frames of other texture formats or of half / quarter size: hapb_decode into D_BC_TEX as in hapb_road_frames,
   the transcode kernel from there into D_TRANSCODED (one launch per source format present in the slice), hapb_encode on
   those textures -- or, for a frame that holds the wanted formats already, on its own.  No picture anywhere. */

/* the destination sets the kernel makes: 1 DXT1, 2 DXT5, 3 YCoCg-DXT5, 4 YCoCg-DXT5 + RGTC1 (Hap Q Alpha); 0: none of them */
static unsigned transcode_set(unsigned count, const unsigned *formats)
{
    if (count == 1u)
        return formats[0] == HapTextureFormat_RGB_DXT1 ? 1u : formats[0] == HapTextureFormat_RGBA_DXT5 ? 2u :
               formats[0] == HapTextureFormat_YCoCg_DXT5 ? 3u : 0u;
    return count == 2u && formats[0] == HapTextureFormat_YCoCg_DXT5 && formats[1] == HapTextureFormat_A_RGTC1 ? 4u : 0u;
}

static void transcode_refuse(unsigned *results, unsigned frame_count, unsigned code)
{
    unsigned f;
    for (f = 0; results && f < frame_count; f++)
        results[f] = code;
}

unsigned hapb_transcode(HapGpuContext *ctx, unsigned frame_count, const void *const *inputs,
                        const unsigned long *input_bytes, unsigned texture_count, unsigned width, unsigned height,
                        unsigned scale_log2, unsigned count, const unsigned *formats, const unsigned *compressors,
                        const unsigned *chunk_counts, void *const *outputs, const unsigned long *output_bytes,
                        unsigned long *output_used, unsigned *results, unsigned decode_flags, unsigned encode_flags)
{
    hapgpu_rt *rt = ctx->rt;
    /* the three source formats of the kernel, each with or without an alpha plane: the picture road's without BC7 */
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8};
    const unsigned *kinds;
    const unsigned kind_count = road_formats(&road, &kinds, NULL);
    const HapbEncodeArgs device_textures = {1, NULL, 0, 0};
    size_t out_per_frame = 0, out_off[2] = {0, 0}, done;
    unsigned long out_bytes[2] = {0, 0};
    unsigned first_error = HapResult_No_Error, f, i, set;
    slice_textures s;
    const void **tex;       /* per frame and destination texture: what the encode half reads */
    unsigned *decoded;      /* per frame: what its decode half came to */
    if (frame_count == 0)
        return HapResult_No_Error;
    if (!results)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, results, frame_count))
        return HapResult_Internal_Error;
    if (!inputs || !input_bytes || !formats || !compressors || !chunk_counts || !outputs || !output_bytes || !output_used ||
        texture_count == 0 || texture_count > 2 || count == 0 || count > 2 || scale_log2 > 2u || width == 0 || height == 0 ||
        width % (4u << scale_log2) || height % (4u << scale_log2) || (height >> scale_log2) / 4u > 65535u) {
        transcode_refuse(results, frame_count, HapResult_Bad_Arguments);
        return HapResult_Bad_Arguments;
    }
    /* a destination the kernel does not make is one a frame can only have already: legal at the frames' own size */
    set = transcode_set(count, formats);
    if (!set && scale_log2) {
        transcode_refuse(results, frame_count, HapResult_Bad_Arguments);
        return HapResult_Bad_Arguments;
    }
    for (i = 0; i < count; i++) {
        out_bytes[i] = (unsigned long)((size_t)((width >> scale_log2) / 4u) * ((height >> scale_log2) / 4u) * hapf_block_bytes(formats[i]));
        out_off[i] = out_per_frame;
        out_per_frame += align_up(out_bytes[i], 256);
    }
    /* (the destination blocks are the default encode's: no BC7, no refined end points) */
    encode_flags &= ~(HAPGPU_ENCODE_BPTC_BLOCKS | HAPGPU_ENCODE_REFINE_ENDPOINTS);
    if (encode_textures_valid(count, out_bytes, formats, compressors, chunk_counts, encode_flags) != HapResult_No_Error) {
        transcode_refuse(results, frame_count, HapResult_Bad_Arguments);
        return HapResult_Bad_Arguments;
    }
    if (!slice_textures_init(&s, frame_count, 1u, &texture_count, width, height, out_per_frame, 0)) {
        transcode_refuse(results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    tex = (const void **)malloc((sizeof(*tex) * count + sizeof(*decoded)) * s.at.slice);
    if (!tex) {
        free(s.in);
        transcode_refuse(results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    decoded = (unsigned *)(tex + s.at.slice * count);
    for (done = 0; done < frame_count; done += s.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.at.slice ? frame_count - done : s.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.at.per_frame * n);
        uint8_t *transcoded = set ? (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out_per_frame * n) : NULL;
        /* [source textures][source planes][destination textures][destination planes] per source format */
        const size_t tab_bytes = sizeof(uint64_t) * 4u * PICTURE_KINDS_MAX * n;
        uint64_t *htab = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, tab_bytes);
        uint64_t *dtab = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, tab_bytes);
        unsigned present = 0, k;
        int rc = 0;
        if (!textures || (set && !transcoded) || !htab || !dtab) {
            transcode_refuse(results + done, n, HapResult_Internal_Error);
            first_error = first_error ? first_error : HapResult_Internal_Error;
            continue;
        }
        slice_textures_decode(ctx, &s, textures, inputs, input_bytes, done, n, NULL, decode_flags);
        memset(htab, 0, tab_bytes);
        for (f = 0; f < n; f++) {
            const size_t e = (size_t)f * texture_count;
            unsigned r = s.res[e];
            int pass = 0;
            k = kind_count;
            if (r == HapResult_No_Error && texture_count == 2)
                r = s.res[e + 1];
            if (r == HapResult_No_Error) {
                /* the frame's own formats are the wanted ones, at its own size: its textures go on as they are */
                pass = scale_log2 == 0u && texture_count == count;
                for (i = 0; pass && i < count; i++)
                    if (s.fmts[e + i] != formats[i] || s.used[e + i] != out_bytes[i])
                        pass = 0;
                k = kind_of(kinds, kind_count, s.fmts[e]);
                /* else it must hold what the caller's geometry says, as for hapb_road_frames, in a format the kernel reads */
                if (!pass && (!set || !slice_entry_fits(&s, e, texture_count, kinds, kind_count)))
                    r = HapResult_Bad_Arguments;
            }
            decoded[f] = r;
            for (i = 0; i < count; i++)
                tex[(size_t)f * count + i] = r != HapResult_No_Error ? NULL :
                                             pass ? s.outs[e + i] : (const void *)(transcoded + out_per_frame * f + out_off[i]);
            /* (a frame whose output hapb_encode will refuse is not worth the kernel's time either) */
            if (r == HapResult_No_Error && !pass && outputs[done + f] && output_bytes[done + f]) {
                uint64_t *col = htab + (size_t)k * 4u * n;
                present |= 1u << k;
                col[f] = (uint64_t)(uintptr_t)s.outs[e];
                col[n + f] = texture_count == 2 ? (uint64_t)(uintptr_t)s.outs[e + 1] : 0u;
                col[2u * n + f] = (uint64_t)(uintptr_t)tex[(size_t)f * count];
                col[3u * n + f] = count == 2 ? (uint64_t)(uintptr_t)tex[(size_t)f * count + 1] : 0u;
            }
        }
        if (present) {
            rc |= hapgpu_rt_h2d(rt, dtab, htab, tab_bytes);
            for (k = 0; k < kind_count; k++)
                if (present & (1u << k)) {
                    const uint64_t *col = dtab + (size_t)k * 4u * n;
                    const HapGpuTranscodeTable tt = {{col, col + n, col + 2u * (size_t)n, col + 3u * (size_t)n}, {0u, 0u, 0u, 0u}};
                    rc |= hapgpu_k_block_transcode(rt, &tt, n, kinds[k], texture_count == 2, width, height, scale_log2,
                                                   formats[0], count == 2);
                }
        }
        if (rc)     /* (nothing of this slice's kernel output may be trusted: its frames fail, the pass-through ones included) */
            memset(tex, 0, sizeof(*tex) * (size_t)n * count);
        /* the encode half on the same stream, behind the kernel; it ends with the slice's second and last wait */
        hapb_encode(ctx, n, count, tex, out_bytes, formats, compressors, chunk_counts, outputs + done, output_bytes + done,
                    output_used + done, results + done, encode_flags, &device_textures);
        for (f = 0; f < n; f++) {
            if (decoded[f] != HapResult_No_Error)
                results[done + f] = decoded[f];
            else if (rc && (results[done + f] == HapResult_No_Error || results[done + f] == HapResult_Bad_Arguments))
                results[done + f] = HapResult_Internal_Error;
            if (results[done + f] != HapResult_No_Error && first_error == HapResult_No_Error)
                first_error = results[done + f];
        }
    }
    free(s.in); free(tex);
    return first_error;
}

/* One texture (+ alpha plane) -> `count` textures of one of the kernel's destination sets; the set the source is
   already, at its own size, is copied. */
unsigned hapb_transcode_texture(HapGpuContext *ctx, const void *texture, unsigned long texture_bytes, unsigned format,
                                const void *alpha, unsigned long alpha_bytes, unsigned width, unsigned height,
                                unsigned scale_log2, unsigned count, const unsigned *formats, void *const *outputs,
                                const unsigned long *output_bytes, unsigned long *output_used)
{
    const HapbRoad road = {.picture_kind = HAPGPU_PICTURE_RGBA8};
    const unsigned *kinds;
    const unsigned kind_count = road_formats(&road, &kinds, NULL);
    hapgpu_rt *rt = ctx->rt;
    const size_t block = hapf_block_bytes(format);
    HapGpuTranscodeTable t = {{NULL, NULL, NULL, NULL}, {0u, 0u, 0u, 0u}};
    size_t need, alpha_need, out_need[2] = {0, 0}, out_off[2] = {0, 0}, out_total = 0;
    const void *src = texture, *asrc = alpha;
    uint8_t *staged = NULL;
    unsigned i, k, set, align;
    int rc = 0, pass;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    k = kind_of(kinds, kind_count, format);
    if (!texture || !formats || !outputs || !output_bytes || count == 0 || count > 2 || scale_log2 > 2u || width == 0 ||
        height == 0 || width % (4u << scale_log2) || height % (4u << scale_log2) || (height >> scale_log2) / 4u > 65535u ||
        k == kind_count)
        return HapResult_Bad_Arguments;
    set = transcode_set(count, formats);
    if (!set)
        return HapResult_Bad_Arguments;
    need = (size_t)(width / 4u) * (height / 4u) * block;
    alpha_need = (size_t)(width / 4u) * (height / 4u) * 8u;
    if (texture_bytes < need || (alpha && alpha_bytes < alpha_need))
        return HapResult_Bad_Arguments;
    for (i = 0; i < count; i++) {
        if (!outputs[i])
            return HapResult_Bad_Arguments;
        out_need[i] = (size_t)((width >> scale_log2) / 4u) * ((height >> scale_log2) / 4u) * hapf_block_bytes(formats[i]);
        out_off[i] = out_total;
        out_total += align_up(out_need[i], 256);
    }
    for (i = 0; i < count; i++)
        if (output_bytes[i] < out_need[i])
            return HapResult_Buffer_Too_Small;
    /* device sources aligned to what a lane reads of a block row (the block << scale_log2, at most 16 bytes), device
       outputs to their blocks */
    align = (unsigned)(block << scale_log2) > 16u ? 16u : (unsigned)(block << scale_log2);
    if ((is_dev(ctx, texture) && ((uintptr_t)texture & (align - 1u))) ||
        (alpha && is_dev(ctx, alpha) && ((uintptr_t)alpha & ((8u << scale_log2 > 16u ? 16u : 8u << scale_log2) - 1u))))
        return HapResult_Bad_Arguments;
    for (i = 0; i < count; i++)
        if (is_dev(ctx, outputs[i]) && ((uintptr_t)outputs[i] & (hapf_block_bytes(formats[i]) - 1u)))
            return HapResult_Bad_Arguments;
    if (!is_dev(ctx, texture) || (alpha && !is_dev(ctx, alpha))) {
        uint8_t *s = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, align_up(need, 256) + alpha_need);
        if (!s)
            return HapResult_Internal_Error;
        if (!is_dev(ctx, texture)) {
            if (hapgpu_rt_h2d(rt, s, texture, need))
                return HapResult_Internal_Error;
            src = s;
        }
        if (alpha && !is_dev(ctx, alpha)) {
            if (hapgpu_rt_h2d(rt, s + align_up(need, 256), alpha, alpha_need))
                return HapResult_Internal_Error;
            asrc = s + align_up(need, 256);
        }
    }
    /* the source is the destination set already (its alpha plane counted), at its own size: no generation loss */
    pass = scale_log2 == 0u && formats[0] == format && (count == 2) == (alpha != NULL);
    for (i = 0; i < count; i++)
        if (!is_dev(ctx, outputs[i]) && !pass && !staged) {
            staged = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out_total);
            if (!staged)
                return HapResult_Internal_Error;
        }
    if (pass) {
        for (i = 0; i < count; i++) {
            const void *from = i ? asrc : src;
            rc |= is_dev(ctx, outputs[i]) ? hapgpu_rt_d2d(rt, outputs[i], from, out_need[i])
                                          : hapgpu_rt_d2h(rt, outputs[i], from, out_need[i]);
        }
    } else {
        t.one[0] = (uint64_t)(uintptr_t)src;
        t.one[1] = (uint64_t)(uintptr_t)asrc;
        for (i = 0; i < count; i++)
            t.one[2u + i] = (uint64_t)(uintptr_t)(is_dev(ctx, outputs[i]) ? (uint8_t *)outputs[i] : staged + out_off[i]);
        rc = hapgpu_k_block_transcode(rt, &t, 1u, format, alpha != NULL, width, height, scale_log2, formats[0], count == 2);
        if (rc == 1)
            return HapResult_Bad_Arguments;
        for (i = 0; !rc && i < count; i++)
            if (!is_dev(ctx, outputs[i]))
                rc |= hapgpu_rt_d2h(rt, outputs[i], staged + out_off[i], out_need[i]);
    }
    if (rc || hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    for (i = 0; output_used && i < count; i++)
        output_used[i] = (unsigned long)out_need[i];
    return HapResult_No_Error;
}

/* ============================================================= compositing to frames */
/* Layers of frames -> frames, and layers of textures -> textures: the placed compositing calls up to their launch, then
   hapb_transcode from its launch on.  hapgpu_k_block_composite_encode takes the descriptors of
   hapgpu_k_block_composite_placed and, where that has the pictures' addresses, the destination textures' -- a slice's lie
   in D_TRANSCODED --, and hapb_encode follows on those textures on the same stream.  No picture anywhere. */

int hapb_composite_encode_textures_valid(unsigned layer_count, const unsigned *layer_widths, const unsigned *layer_heights,
                                         const HapGpuPlacement *placements, size_t frame_count, unsigned width,
                                         unsigned height, const unsigned *texture_counts, unsigned count,
                                         const unsigned *formats)
{
    /* (the canvas is the placed calls' with rows of exactly width * 4 bytes; a block row per blockIdx.y of the kernel) */
    return hapb_composite_placed_valid(layer_count, layer_widths, layer_heights, placements, frame_count, width, height,
                                       (unsigned long)width * 4u, texture_counts) &&
           height / 4u <= 65535u && formats && count != 0 && count <= 2 && transcode_set(count, formats);
}

int hapb_composite_encode_frames_valid(unsigned layer_count, const unsigned *layer_widths, const unsigned *layer_heights,
                                       const HapGpuPlacement *placements, size_t frame_count, unsigned width,
                                       unsigned height, const unsigned *texture_counts, unsigned count,
                                       const unsigned *formats, const unsigned *compressors,
                                       const unsigned *chunk_counts, unsigned encode_flags)
{
    unsigned long out_bytes[2] = {0, 0};
    unsigned i;
    if (!compressors || !chunk_counts ||
        !hapb_composite_encode_textures_valid(layer_count, layer_widths, layer_heights, placements, frame_count, width,
                                              height, texture_counts, count, formats))
        return 0;
    for (i = 0; i < count; i++)
        out_bytes[i] = (unsigned long)((size_t)(width / 4u) * (height / 4u) * hapf_block_bytes(formats[i]));
    encode_flags &= ~(HAPGPU_ENCODE_BPTC_BLOCKS | HAPGPU_ENCODE_REFINE_ENDPOINTS);
    return encode_textures_valid(count, out_bytes, formats, compressors, chunk_counts, encode_flags) == HapResult_No_Error;
}

/* the table of a composite-encode launch for n canvases of layer_count layers: [n] destination textures, [n] destination
   planes, then [n][layer_count] descriptors; as composite_placed_table */
static uint64_t *composite_encode_table(hapgpu_rt *rt, unsigned n, unsigned layer_count, uint64_t **device, size_t *bytes)
{
    uint64_t *htab;
    *bytes = sizeof(uint64_t) * 2u * n + sizeof(HapGpuPlacedLayer) * (size_t)n * layer_count;
    htab = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, *bytes);
    *device = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, *bytes);
    if (!htab || !*device)
        return NULL;
    memset(htab, 0, *bytes);
    return htab;
}

static void composite_encode_refuse(unsigned *layer_results, size_t layer_entries, unsigned *results, size_t frame_count,
                                    unsigned code)
{
    size_t i;
    for (i = 0; layer_results && i < layer_entries; i++)
        layer_results[i] = code;
    for (i = 0; results && i < frame_count; i++)
        results[i] = code;
}

unsigned hapb_composite_encode_textures(HapGpuContext *ctx, unsigned layer_count, const void *const *textures,
                                        const unsigned long *texture_bytes, const unsigned *formats,
                                        const void *const *alphas, const unsigned long *alpha_bytes,
                                        const unsigned *layer_widths, const unsigned *layer_heights,
                                        const HapGpuPlacement *placements, const unsigned char *opacities,
                                        const unsigned char *background, unsigned width, unsigned height, unsigned count,
                                        const unsigned *out_formats, void *const *outputs,
                                        const unsigned long *output_bytes, unsigned long *output_used)
{
    hapgpu_rt *rt = ctx->rt;
    size_t staged = 0, tab_bytes, at = 0, out_need[2] = {0, 0}, out_off[2] = {0, 0}, out_total = 0;
    uint64_t *htab, *dtab;
    HapGpuPlacedLayer *hlayers;
    uint8_t *stage = NULL, *out_stage = NULL;
    unsigned l, i;
    int rc, any_host_output = 0;
    if (!hapb_composite_encode_textures_valid(layer_count, layer_widths, layer_heights, placements, 1u, width, height, NULL,
                                              count, out_formats) ||
        !textures || !texture_bytes || !formats || !outputs || !output_bytes)
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    /* every layer: HapGpuDecompressRGBA's rules for its texture and its plane, at the layer's own size */
    for (l = 0; l < layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL;
        const size_t blocks = (size_t)(layer_widths[l] / 4u) * (layer_heights[l] / 4u);
        const size_t need = composite_format(formats[l]) ? blocks * hapf_block_bytes(formats[l]) : 0u;
        if (!textures[l] || !need || texture_bytes[l] < need || (alpha && (!alpha_bytes || alpha_bytes[l] < blocks * 8u)) ||
            (is_dev(ctx, textures[l]) && ((uintptr_t)textures[l] & (hapf_block_bytes(formats[l]) - 1u))) ||
            (alpha && is_dev(ctx, alpha) && ((uintptr_t)alpha & 7u)))
            return HapResult_Bad_Arguments;
        if (!is_dev(ctx, textures[l]))
            staged += align_up(need, 256);
        if (alpha && !is_dev(ctx, alpha))
            staged += align_up(blocks * 8u, 256);
    }
    /* every output: HapGpuTranscodeTexture's rules */
    for (i = 0; i < count; i++) {
        if (!outputs[i])
            return HapResult_Bad_Arguments;
        out_need[i] = (size_t)(width / 4u) * (height / 4u) * hapf_block_bytes(out_formats[i]);
        out_off[i] = out_total;
        out_total += align_up(out_need[i], 256);
    }
    for (i = 0; i < count; i++)
        if (output_bytes[i] < out_need[i])
            return HapResult_Buffer_Too_Small;
    for (i = 0; i < count; i++) {
        if (is_dev(ctx, outputs[i]) && ((uintptr_t)outputs[i] & (hapf_block_bytes(out_formats[i]) - 1u)))
            return HapResult_Bad_Arguments;
        if (!is_dev(ctx, outputs[i]))
            any_host_output = 1;
    }
    /* (one request for all that is staged: an arena that grows forgets what it held) */
    if (staged && !(stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, staged)))
        return HapResult_Internal_Error;
    if (any_host_output && !(out_stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out_total)))
        return HapResult_Internal_Error;
    htab = composite_encode_table(rt, 1u, layer_count, &dtab, &tab_bytes);
    if (!htab)
        return HapResult_Internal_Error;
    hlayers = (HapGpuPlacedLayer *)(htab + 2);
    for (i = 0; i < count; i++)
        htab[i] = (uint64_t)(uintptr_t)(is_dev(ctx, outputs[i]) ? (uint8_t *)outputs[i] : out_stage + out_off[i]);
    for (l = 0; l < layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL, *src = textures[l];
        const size_t blocks = (size_t)(layer_widths[l] / 4u) * (layer_heights[l] / 4u);
        if (!is_dev(ctx, src)) {
            const size_t need = blocks * hapf_block_bytes(formats[l]);
            if (hapgpu_rt_h2d(rt, stage + at, src, need))
                return HapResult_Internal_Error;
            src = stage + at;
            at += align_up(need, 256);
        }
        if (alpha && !is_dev(ctx, alpha)) {
            if (hapgpu_rt_h2d(rt, stage + at, alpha, blocks * 8u))
                return HapResult_Internal_Error;
            alpha = stage + at;
            at += align_up(blocks * 8u, 256);
        }
        hlayers[l].texture = (uint64_t)(uintptr_t)src;
        hlayers[l].alpha = (uint64_t)(uintptr_t)alpha;
        hlayers[l].format = formats[l];
        hlayers[l].opacity = opacities ? opacities[l] : 255u;
        placed_layer_clip(&hlayers[l], placements ? &placements[l] : NULL, layer_widths[l], layer_heights[l], width, height);
    }
    if (hapgpu_rt_h2d(rt, dtab, htab, tab_bytes))
        return HapResult_Internal_Error;
    rc = hapgpu_k_block_composite_encode(rt, (const HapGpuPlacedLayer *)(dtab + 2), layer_count, dtab, dtab + 1, 1u,
                                         background ? background : k_composite_background, width, height, out_formats[0],
                                         count == 2);
    if (rc == 1)
        return HapResult_Bad_Arguments;
    for (i = 0; !rc && i < count; i++)
        if (!is_dev(ctx, outputs[i]))
            rc |= hapgpu_rt_d2h(rt, outputs[i], out_stage + out_off[i], out_need[i]);
    if (rc || hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    for (i = 0; output_used && i < count; i++)
        output_used[i] = (unsigned long)out_need[i];
    return HapResult_No_Error;
}

unsigned hapb_composite_encode_frames(HapGpuContext *ctx, unsigned frame_count, unsigned layer_count,
                                      const void *const *inputs, const unsigned long *input_bytes,
                                      const unsigned *texture_counts, const unsigned *layer_widths,
                                      const unsigned *layer_heights, const HapGpuPlacement *placements,
                                      const unsigned char *opacities, const unsigned char *background, unsigned width,
                                      unsigned height, unsigned count, const unsigned *formats,
                                      const unsigned *compressors, const unsigned *chunk_counts, void *const *outputs,
                                      const unsigned long *output_bytes, unsigned long *output_used,
                                      unsigned *layer_results, unsigned *results, unsigned decode_flags,
                                      unsigned encode_flags)
{
    hapgpu_rt *rt = ctx->rt;
    const HapbEncodeArgs device_textures = {1, NULL, 0, 0};
    const size_t total = (size_t)frame_count * layer_count;
    size_t out_per_frame = 0, out_off[2] = {0, 0}, done, i;
    unsigned long out_bytes[2] = {0, 0};
    unsigned first_error = HapResult_No_Error, f, l;
    hap_place_layout layout;
    slice_textures s;
    const void **tex;       /* per output frame and destination texture: what the encode half reads */
    unsigned *composited;   /* per output frame: what its layers came to */
    if (!results || !layer_results)
        return HapResult_Bad_Arguments;
    if (!hapb_composite_encode_frames_valid(layer_count, layer_widths, layer_heights, placements, frame_count, width, height,
                                            texture_counts, count, formats, compressors, chunk_counts, encode_flags) ||
        !inputs || !input_bytes || !outputs || !output_bytes || !output_used) {
        composite_encode_refuse(layer_results, total, results, frame_count, HapResult_Bad_Arguments);
        return HapResult_Bad_Arguments;
    }
    if (frame_count == 0)
        return HapResult_No_Error;
    /* (the destination blocks are the default encode's: no BC7, no refined end points) */
    encode_flags &= ~(HAPGPU_ENCODE_BPTC_BLOCKS | HAPGPU_ENCODE_REFINE_ENDPOINTS);
    for (i = 0; i < count; i++) {
        out_bytes[i] = (unsigned long)((size_t)(width / 4u) * (height / 4u) * hapf_block_bytes(formats[i]));
        out_off[i] = out_per_frame;
        out_per_frame += align_up(out_bytes[i], 256);
    }
    /* output frames of a slice: at most 4 GiB of block textures, the canvases' among them, and 32768 entries of the second
       stage at a time */
    hap_place_layout_of(&layout, layer_count, texture_counts, layer_widths, layer_heights, out_per_frame, frame_count);
    if (context_busy(ctx, NULL, 0) || !slice_textures_init_placed(&s, &layout)) {
        composite_encode_refuse(layer_results, total, results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    tex = (const void **)malloc((sizeof(*tex) * count + sizeof(*composited)) * s.at.slice);
    if (!tex) {
        free(s.in);
        composite_encode_refuse(layer_results, total, results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    composited = (unsigned *)(tex + s.at.slice * count);
    for (done = 0; done < frame_count; done += s.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.at.slice ? frame_count - done : s.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.at.per_frame * n);
        uint8_t *encoded = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out_per_frame * n);
        uint64_t *htab = NULL, *dtab = NULL;
        HapGpuPlacedLayer *hlayers;
        size_t tab_bytes = 0;
        unsigned present = 0;
        int rc = 0;
        if (textures && encoded) {
            /* the second stage of every layer of every output frame of the slice, one batch: whole frames */
            slice_textures_decode(ctx, &s, textures, inputs, input_bytes, done, n, NULL, decode_flags);
            /* (after the second stage, which has tables of its own) */
            htab = composite_encode_table(rt, n, layer_count, &dtab, &tab_bytes);
        }
        if (!htab) {
            composite_encode_refuse(layer_results + done * layer_count, (size_t)n * layer_count, results + done, n,
                                    HapResult_Internal_Error);
            for (f = 0; f < n; f++)
                output_used[done + f] = 0;
            first_error = first_error ? first_error : HapResult_Internal_Error;
            continue;
        }
        hlayers = (HapGpuPlacedLayer *)(htab + 2u * (size_t)n);
        for (f = 0; f < n; f++) {
            unsigned *frame_results = layer_results + (done + f) * layer_count;
            unsigned all = HapResult_No_Error;
            for (l = 0; l < layer_count; l++) {
                const unsigned layer_textures = s.at.count_of[l];
                const size_t e = (size_t)f * s.at.entries_per_frame + s.at.entry_of[l];
                HapGpuPlacedLayer *d = &hlayers[(size_t)f * layer_count + l];
                unsigned r = s.res[e];
                if (r == HapResult_No_Error && layer_textures == 2u)
                    r = s.res[e + 1];
                /* the placed call's checks: exactly the layer's geometry, in one of the three formats a layer may have */
                if (r == HapResult_Buffer_Too_Small ||
                    (r == HapResult_No_Error && !slice_entry_fits_member(&s, e, l, k_rgba_kinds, 3u)))
                    r = HapResult_Bad_Arguments;
                frame_results[l] = r;
                if (r != HapResult_No_Error && all == HapResult_No_Error)
                    all = r;
                d->texture = (uint64_t)(uintptr_t)s.outs[e];
                d->alpha = layer_textures == 2u ? (uint64_t)(uintptr_t)s.outs[e + 1] : 0u;
                d->format = s.fmts[e];
                d->opacity = opacities ? opacities[(done + f) * layer_count + l] : 255u;
                placed_layer_clip(d, placements ? &placements[(done + f) * layer_count + l] : NULL, layer_widths[l],
                                  layer_heights[l], width, height);
            }
            composited[f] = all;
            /* (an output frame with a failed layer has NULL textures: hapb_encode leaves it out) */
            for (i = 0; i < count; i++)
                tex[(size_t)f * count + i] = all != HapResult_No_Error ? NULL :
                                             (const void *)(encoded + out_per_frame * f + out_off[i]);
            /* (a frame whose output hapb_encode will refuse is not worth the kernel's time either: address 0 skips it) */
            if (all == HapResult_No_Error && outputs[done + f] && output_bytes[done + f]) {
                htab[f] = (uint64_t)(uintptr_t)tex[(size_t)f * count];
                htab[n + f] = count == 2 ? (uint64_t)(uintptr_t)tex[(size_t)f * count + 1] : 0u;
                present = 1;
            }
        }
        if (present) {
            rc |= hapgpu_rt_h2d(rt, dtab, htab, tab_bytes);
            rc |= hapgpu_k_block_composite_encode(rt, (const HapGpuPlacedLayer *)(dtab + 2u * (size_t)n), layer_count, dtab,
                                                  dtab + n, n, background ? background : k_composite_background, width,
                                                  height, formats[0], count == 2);
        }
        if (rc)     /* (nothing of this slice's kernel output may be trusted: its frames fail) */
            memset(tex, 0, sizeof(*tex) * (size_t)n * count);
        /* the encode half on the same stream, behind the kernel; it ends with the slice's second and last wait */
        hapb_encode(ctx, n, count, tex, out_bytes, formats, compressors, chunk_counts, outputs + done, output_bytes + done,
                    output_used + done, results + done, encode_flags, &device_textures);
        for (f = 0; f < n; f++) {
            if (composited[f] != HapResult_No_Error) {
                results[done + f] = composited[f];
                output_used[done + f] = 0;
            } else if (rc && (results[done + f] == HapResult_No_Error || results[done + f] == HapResult_Bad_Arguments)) {
                results[done + f] = HapResult_Internal_Error;
            }
            if (results[done + f] != HapResult_No_Error && first_error == HapResult_No_Error)
                first_error = results[done + f];
        }
    }
    free(s.in); free(tex);
    return first_error;
}
