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
   one, or a layer each, of a size of its own --, member m of the call's output frame f being the call's input
   f * member_count + m.  Entry f * at.entries_per_frame + at.entry_of[m] + t is texture t of member m of the slice's
   frame f: the colour texture at at.per_frame * f + at.offset_of[m] of the slice's D_BC_TEX scratch, the RGTC1 alpha
   plane at + layout.alpha_off_of[m] (hap_place.h; `at` is layout.at).  The textures of one member stay adjacent:
   hapb_decode uploads a host frame once for them. */
typedef struct slice_textures {
    hap_place_layout layout;
    unsigned width, height;                 /* (member 0's: a road with rectangles has one member) */
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

/* The arrays of a slice's entries and its layout.  counts: the members' texture counts (NULL: all 1); widths, heights:
   their sizes, one each; extra_per_frame: what else the caller holds per frame while a slice's textures are held;
   rectangles != 0: room for a rectangle per entry.  0: out of memory */
static int slice_textures_init(slice_textures *s, unsigned frame_count, unsigned member_count, const unsigned *counts,
                               const unsigned *widths, const unsigned *heights, size_t extra_per_frame, int rectangles)
{
    size_t entries;
    s->width = widths[0];
    s->height = heights[0];
    hap_place_layout_of(&s->layout, member_count, counts, widths, heights, extra_per_frame, frame_count);
    entries = s->layout.at.slice * s->layout.at.entries_per_frame;
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

/* Output frames done .. done + n of the call (n <= at.slice) into `textures`, at.per_frame * n bytes of D_BC_TEX
   scratch.  road (NULL: whole textures) -- its region: the rectangle wanted of every frame -- or, with region_xs and
   region_ys, its size alone, frame f's origin being (xs[f], ys[f]): a frame whose origin puts the rectangle off the grid or
   past an edge goes to hapb_decode with a NULL input, its Bad_Arguments, and nothing of it is decoded.  Its resize: frame
   f's rectangle is its crop at scale_log2 rounded outward to the blocks (hapb_resize_region), and a crop that is none
   refuses its frame alike. */
static void slice_textures_decode(HapGpuContext *ctx, const slice_textures *s, uint8_t *textures, const void *const *inputs,
                                  const unsigned long *input_bytes, size_t done, unsigned n, const HapbRoad *road,
                                  unsigned flags)
{
    const hap_slice_layout *const at = &s->layout.at;
    const unsigned width = s->width, height = s->height, members = at->member_count;
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
            for (t = 0; t < at->count_of[m]; t++) {
                const size_t e = (size_t)f * at->entries_per_frame + at->entry_of[m] + t;
                if (s->decode_regions)
                    s->decode_regions[e] = own;
                s->in[e] = refused ? NULL : inputs[(done + f) * members + m];
                s->in_bytes[e] = input_bytes[(done + f) * members + m];
                s->outs[e] = textures + at->per_frame * f + at->offset_of[m] + (t ? s->layout.alpha_off_of[m] : 0u);
                s->caps[e] = (unsigned long)(s->layout.blocks_of[m] * (t ? 8u : 16u));
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
    hapb_decode(ctx, n * at->entries_per_frame, s->in, s->in_bytes, 0, s->outs, s->caps, s->used, s->fmts, s->res,
                flags & ~HAPGPU_DECODE_BPTC_PICTURES, &args);
}

/* 1: entry e of a decoded slice, member m's first (and, two textures read of it, entry e + 1), holds what the caller's
   geometry says: a colour texture of `kinds`, of exactly the member's blocks, and (two textures) an RGTC1 plane of the
   same geometry */
static int slice_entry_fits(const slice_textures *s, size_t e, unsigned m, const unsigned *kinds, unsigned kind_count)
{
    const unsigned fmt = s->fmts[e];
    const size_t blocks = s->layout.blocks_of[m];
    return kind_of(kinds, kind_count, fmt) != kind_count && s->used[e] == blocks * hapf_block_bytes(fmt) &&
           (s->layout.at.count_of[m] != 2u || (s->fmts[e + 1] == HapTextureFormat_A_RGTC1 && s->used[e + 1] == blocks * 8u));
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
    if (!slice_textures_init(&s, frame_count, 1u, &texture_count, &width, &height, 0u, per_frame_regions)) {
        for (f = 0; f < frame_count; f++)
            results[f] = HapResult_Internal_Error;
        return HapResult_Internal_Error;
    }
    for (done = 0; done < frame_count; done += s.layout.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.layout.at.slice ? frame_count - done : s.layout.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.layout.at.per_frame * n);
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
                if (r == HapResult_No_Error && !slice_entry_fits(&s, e, 0u, kinds, kind_count))
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

/* ============================================================= destinations of block textures */
/* What the calls that end in block textures or in frames of them share (transcoding, compositing to textures): the sets
   of textures their kernels make, where a call's destination textures lie, and the encode half of a slice. */

/* the destination sets the kernels make: 1 DXT1, 2 DXT5, 3 YCoCg-DXT5, 4 YCoCg-DXT5 + RGTC1 (Hap Q Alpha); 0: none of them */
static unsigned transcode_set(unsigned count, const unsigned *formats)
{
    if (count == 1u)
        return formats[0] == HapTextureFormat_RGB_DXT1 ? 1u : formats[0] == HapTextureFormat_RGBA_DXT5 ? 2u :
               formats[0] == HapTextureFormat_YCoCg_DXT5 ? 3u : 0u;
    return count == 2u && formats[0] == HapTextureFormat_YCoCg_DXT5 && formats[1] == HapTextureFormat_A_RGTC1 ? 4u : 0u;
}

/* (the destination blocks are the default encode's: no BC7, no refined end points) */
#define DESTINATION_ENCODE_FLAGS(flags) ((flags) & ~(unsigned)(HAPGPU_ENCODE_BPTC_BLOCKS | HAPGPU_ENCODE_REFINE_ENDPOINTS))

/* the `count` destination textures of one frame: their sizes, and where they lie, 256-byte aligned, in scratch of `total`
   bytes a frame (D_TRANSCODED) */
typedef struct destination_layout {
    unsigned long bytes[2];
    size_t off[2], total;
} destination_layout;

static void destination_layout_of(destination_layout *d, unsigned count, const unsigned *formats, unsigned width,
                                  unsigned height)
{
    unsigned i;
    memset(d, 0, sizeof(*d));
    for (i = 0; i < count; i++) {
        d->bytes[i] = (unsigned long)((size_t)(width / 4u) * (height / 4u) * hapf_block_bytes(formats[i]));
        d->off[i] = d->total;
        d->total += align_up(d->bytes[i], 256);
    }
}

/* every output of a call that writes textures, HapGpuTranscodeTexture's rules: there, large enough, and in device memory
   aligned to its blocks */
static unsigned destination_textures_fit(HapGpuContext *ctx, const destination_layout *d, unsigned count,
                                         const unsigned *formats, void *const *outputs, const unsigned long *output_bytes)
{
    unsigned i;
    for (i = 0; i < count; i++)
        if (!outputs[i])
            return HapResult_Bad_Arguments;
    for (i = 0; i < count; i++)
        if (output_bytes[i] < d->bytes[i])
            return HapResult_Buffer_Too_Small;
    for (i = 0; i < count; i++)
        if (is_dev(ctx, outputs[i]) && ((uintptr_t)outputs[i] & (hapf_block_bytes(formats[i]) - 1u)))
            return HapResult_Bad_Arguments;
    return HapResult_No_Error;
}

/* The encode half of a slice of n frames, on the same stream behind the kernel; it ends with the slice's second and last
   wait.  tex: per frame and destination texture, what hapb_encode reads (device memory; NULL: the frame is left out);
   first_half[f]: what frame f's decode or compositing half came to, which is its result where it failed -- and, with
   failed_use_nothing, its output_used is then 0 whatever hapb_encode left there; rc: the slice's launches and copies.
   results, outputs, output_bytes, output_used: the slice's. */
static void slice_encode_half(HapGpuContext *ctx, unsigned n, const void **tex, const unsigned *first_half, int rc,
                              int failed_use_nothing, const destination_layout *d, unsigned count, const unsigned *formats,
                              const unsigned *compressors, const unsigned *chunk_counts, unsigned encode_flags,
                              void *const *outputs, const unsigned long *output_bytes, unsigned long *output_used,
                              unsigned *results, unsigned *first_error)
{
    const HapbEncodeArgs device_textures = {1, NULL, 0, 0};
    unsigned f;
    if (rc)     /* (nothing of this slice's kernel output may be trusted: its frames fail, the pass-through ones included) */
        memset(tex, 0, sizeof(*tex) * (size_t)n * count);
    hapb_encode(ctx, n, count, tex, d->bytes, formats, compressors, chunk_counts, outputs, output_bytes, output_used, results,
                DESTINATION_ENCODE_FLAGS(encode_flags), &device_textures);
    for (f = 0; f < n; f++) {
        if (first_half[f] != HapResult_No_Error) {
            results[f] = first_half[f];
            if (failed_use_nothing)
                output_used[f] = 0;
        } else if (rc && (results[f] == HapResult_No_Error || results[f] == HapResult_Bad_Arguments)) {
            results[f] = HapResult_Internal_Error;
        }
        if (results[f] != HapResult_No_Error && *first_error == HapResult_No_Error)
            *first_error = results[f];
    }
}

/* ============================================================= compositing */
/* Layers of textures or frames "over" a background colour -> one canvas per output frame, by bc_composite.hip and
   bc_composite_encode.hip: the layers' pictures never exist.  The call is its caller's description (HapbComposite,
   hap_batch.h): layers of the canvas's size or of sizes of their own, placed and clipped (hap_place.h: the rules and the
   clip), and a canvas that is written as an RGBA8 picture or goes to the block encoder in registers and comes out as
   textures, which the frames form hands to hapb_encode as hapb_transcode does -- no picture anywhere.  The textures
   form stages what lies in host memory into D_BC_TEX; the frames form runs the second stage of all frameCount *
   layerCount frames of a slice in one batch into D_BC_TEX, as hapb_road_frames does, a layer being a member of
   slice_textures with a texture count and a size of its own -- whole frames, whatever of them is visible --, and one
   composite launch per slice follows.  The destinations' addresses and the descriptors go out in one small table. */

static const unsigned char k_composite_background[4] = {0u, 0u, 0u, 255u};
/* (the public limit is the kernel's) */
typedef char composite_limits_agree[HAPGPU_COMPOSITE_MAX_LAYERS == HAPGPU_COMPOSITE_LAYERS_MAX ? 1 : -1];
/* (a placed descriptor begins as a plain one: composite_descriptor writes both) */
typedef char placed_layer_begins_plain[offsetof(HapGpuPlacedLayer, texture) == offsetof(HapGpuCompositeLayer, texture) &&
                                       offsetof(HapGpuPlacedLayer, alpha) == offsetof(HapGpuCompositeLayer, alpha) &&
                                       offsetof(HapGpuPlacedLayer, format) == offsetof(HapGpuCompositeLayer, format) &&
                                       offsetof(HapGpuPlacedLayer, opacity) == offsetof(HapGpuCompositeLayer, opacity) &&
                                       offsetof(HapGpuPlacedLayer, cx0) == sizeof(HapGpuCompositeLayer) ? 1 : -1];

/* the colour formats a layer may have */
static int composite_format(unsigned format)
{
    return format == HapTextureFormat_RGB_DXT1 || format == HapTextureFormat_RGBA_DXT5 || format == HapTextureFormat_YCoCg_DXT5;
}

/* what the calls that end in textures ask on top (a block row per blockIdx.y of the kernel), and the frames form of them
   on top of that */
static int composite_destination_valid(const HapbComposite *c, int frames)
{
    destination_layout out;
    if (!c->layer_widths || c->height / 4u > 65535u || !c->formats || c->count == 0 || c->count > 2 ||
        !transcode_set(c->count, c->formats))
        return 0;
    if (!frames)
        return 1;
    if (!c->compressors || !c->chunk_counts)
        return 0;
    destination_layout_of(&out, c->count, c->formats, c->width, c->height);
    return encode_textures_valid(c->count, out.bytes, c->formats, c->compressors, c->chunk_counts,
                                 DESTINATION_ENCODE_FLAGS(c->encode_flags)) == HapResult_No_Error;
}

int hapb_composite_valid(const HapbComposite *c, size_t frame_count, const unsigned *texture_counts, int frames)
{
    const unsigned layer_count = c->layer_count, width = c->width, height = c->height;
    size_t f;
    unsigned l;
    if (layer_count == 0 || layer_count > HAPGPU_COMPOSITE_MAX_LAYERS || width == 0 || height == 0 || (width & 3u) ||
        (height & 3u))
        return 0;
    /* (an encoded canvas has rows of exactly width * 4 bytes, and nobody's pitch to ask about) */
    if (!c->encoded && (c->row_bytes < (unsigned long)width * 4u || (c->row_bytes & 15u)))
        return 0;
    for (l = 0; texture_counts && l < layer_count; l++)
        if (texture_counts[l] != 1u && texture_counts[l] != 2u)
            return 0;
    if (c->encoded && !composite_destination_valid(c, frames))
        return 0;
    if (!c->layer_widths)
        return 1;
    if (!c->layer_heights || !hap_place_layer_valid(width, height))
        return 0;
    for (l = 0; l < layer_count; l++)
        if (!hap_place_layer_valid(c->layer_widths[l], c->layer_heights[l]))
            return 0;
    for (f = 0; c->placements && f < frame_count; f++)
        for (l = 0; l < layer_count; l++) {
            const HapGpuPlacement *p = &c->placements[f * layer_count + l];
            if (!hap_place_valid(p->srcX, p->srcY, p->width, p->height, p->dstX, p->dstY, c->layer_widths[l],
                                 c->layer_heights[l]))
                return 0;
        }
    return 1;
}

/* what a launch's table holds in front of the descriptors, n addresses each: the pictures, or the destination textures
   and their planes; and a descriptor's size: a placed one where layers have sizes of their own */
static unsigned composite_columns(const HapbComposite *c)
{
    return c->encoded ? 2u : 1u;
}

static size_t composite_stride(const HapbComposite *c)
{
    return c->layer_widths ? sizeof(HapGpuPlacedLayer) : sizeof(HapGpuCompositeLayer);
}

/* the table of a composite launch for n canvases: [columns][n] addresses, then [n][layer_count] descriptors of `stride`
   bytes; *device gets its device copy's address (filled by the caller's h2d of `bytes`) */
static uint64_t *composite_table(hapgpu_rt *rt, unsigned columns, unsigned n, unsigned layer_count, size_t stride,
                                 uint64_t **device, size_t *bytes)
{
    uint64_t *htab;
    *bytes = sizeof(uint64_t) * columns * n + stride * (size_t)n * layer_count;
    htab = (uint64_t *)hapgpu_rt_pinned_scratch(rt, P_BC_PTRS, *bytes);
    *device = (uint64_t *)hapgpu_rt_device_scratch(rt, D_BC_PTRS, *bytes);
    if (!htab || !*device)
        return NULL;
    memset(htab, 0, *bytes);
    return htab;
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

/* Descriptor `slot` of a host table (htab) for n canvases: layer l of the call's output frame f, its texture and plane
   (NULL: none) in device memory.  A placed descriptor begins with a plain one's four members, and has its clip where the
   layers have sizes. */
static void composite_descriptor(const HapbComposite *c, uint64_t *htab, unsigned n, size_t slot, size_t f, unsigned l,
                                 const void *texture, const void *alpha, unsigned format)
{
    void *const at = (uint8_t *)(htab + (size_t)composite_columns(c) * n) + composite_stride(c) * slot;
    HapGpuCompositeLayer *const d = (HapGpuCompositeLayer *)at;
    const size_t entry = f * c->layer_count + l;
    d->texture = (uint64_t)(uintptr_t)texture;
    d->alpha = (uint64_t)(uintptr_t)alpha;
    d->format = format;
    d->opacity = c->opacities ? c->opacities[entry] : 255u;
    if (c->layer_widths)
        placed_layer_clip((HapGpuPlacedLayer *)at, c->placements ? &c->placements[entry] : NULL, c->layer_widths[l],
                          c->layer_heights[l], c->width, c->height);
}

/* the composite launch of a description for the n canvases of a device table: layers of the canvas's size keep the
   kernel and the 24-byte descriptors they have had from the start */
static int launch_composite(hapgpu_rt *rt, const HapbComposite *c, const uint64_t *dtab, unsigned n)
{
    const unsigned char *const background = c->background ? c->background : k_composite_background;
    const void *const layers = dtab + (size_t)composite_columns(c) * n;
    if (c->encoded)
        return hapgpu_k_block_composite_encode(rt, (const HapGpuPlacedLayer *)layers, c->layer_count, dtab, dtab + n, n,
                                               background, c->width, c->height, c->formats[0], c->count == 2);
    if (c->layer_widths)
        return hapgpu_k_block_composite_placed(rt, (const HapGpuPlacedLayer *)layers, c->layer_count, dtab, n, background,
                                               c->width, c->height, c->row_bytes);
    return hapgpu_k_block_composite(rt, (const HapGpuCompositeLayer *)layers, c->layer_count, dtab, n, background, c->width,
                                    c->height, c->row_bytes);
}

/* the blocks of layer l's textures */
static size_t composite_layer_blocks(const HapbComposite *c, unsigned l)
{
    return c->layer_widths ? (size_t)(c->layer_widths[l] / 4u) * (c->layer_heights[l] / 4u)
                           : (size_t)(c->width / 4u) * (c->height / 4u);
}

/* The layers of the textures form.  Every layer: HapGpuDecompressRGBA's rules for its texture and its plane, at the
   layer's own size.  Then what lies in host memory is staged into D_BC_TEX: src[l] and asrc[l] get layer l's texture and
   plane (NULL: none) in device memory.  refused_otherwise: what the caller has against its destination, No_Error if
   nothing -- the call's answer once the layers are in order.  Returns a HapResult. */
static unsigned composite_layers_staged(HapGpuContext *ctx, const HapbComposite *c, const void *const *textures,
                                        const unsigned long *texture_bytes, const unsigned *formats,
                                        const void *const *alphas, const unsigned long *alpha_bytes,
                                        unsigned refused_otherwise, const void **src, const void **asrc)
{
    hapgpu_rt *rt = ctx->rt;
    size_t staged = 0, at = 0;
    uint8_t *stage = NULL;
    unsigned l;
    for (l = 0; l < c->layer_count; l++) {
        const void *alpha = alphas ? alphas[l] : NULL;
        const size_t blocks = composite_layer_blocks(c, l);
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
    /* (what the caller refuses of its destination comes behind the layers' refusals and before any copy) */
    if (refused_otherwise != HapResult_No_Error)
        return refused_otherwise;
    /* (one request for all that is staged: an arena that grows forgets what it held) */
    if (staged && !(stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, staged)))
        return HapResult_Internal_Error;
    for (l = 0; l < c->layer_count; l++) {
        const size_t blocks = composite_layer_blocks(c, l);
        src[l] = textures[l];
        asrc[l] = alphas ? alphas[l] : NULL;
        if (!is_dev(ctx, src[l])) {
            const size_t need = blocks * hapf_block_bytes(formats[l]);
            if (hapgpu_rt_h2d(rt, stage + at, src[l], need))
                return HapResult_Internal_Error;
            src[l] = stage + at;
            at += align_up(need, 256);
        }
        if (asrc[l] && !is_dev(ctx, asrc[l])) {
            if (hapgpu_rt_h2d(rt, stage + at, asrc[l], blocks * 8u))
                return HapResult_Internal_Error;
            asrc[l] = stage + at;
            at += align_up(blocks * 8u, 256);
        }
    }
    return HapResult_No_Error;
}

unsigned hapb_composite_textures(HapGpuContext *ctx, const HapbComposite *c, const void *const *textures,
                                 const unsigned long *texture_bytes, const unsigned *formats,
                                 const void *const *alphas, const unsigned long *alpha_bytes, void *const *outputs,
                                 const unsigned long *output_bytes, unsigned long *output_used)
{
    hapgpu_rt *rt = ctx->rt;
    const size_t pixel_row = (size_t)c->width * 4u;
    const picture_shape shape = {c->row_bytes, pixel_row, (size_t)c->row_bytes * (c->height ? c->height - 1u : 0u) + pixel_row,
                                 c->height};
    const unsigned count = c->encoded ? c->count : 1u;
    const void *src[HAPGPU_COMPOSITE_MAX_LAYERS], *asrc[HAPGPU_COMPOSITE_MAX_LAYERS];
    destination_layout out = {{0, 0}, {0, 0}, 0};
    size_t tab_bytes;
    uint64_t *htab, *dtab;
    uint8_t *stage = NULL;              /* (of the destinations that lie in host memory) */
    unsigned refused = HapResult_No_Error, l, i, r;
    int rc, any_host_output = 0;
    if (!hapb_composite_valid(c, 1u, NULL, 0) || !textures || !texture_bytes || !formats || !outputs ||
        (c->encoded ? !output_bytes : !outputs[0]))
        return HapResult_Bad_Arguments;
    if (context_busy(ctx, NULL, 0))
        return HapResult_Internal_Error;
    /* every output: HapGpuTranscodeTexture's rules; a picture in device memory: 16-byte aligned */
    if (c->encoded) {
        destination_layout_of(&out, count, c->formats, c->width, c->height);
        refused = destination_textures_fit(ctx, &out, count, c->formats, outputs, output_bytes);
    } else if (is_dev(ctx, outputs[0]) && ((uintptr_t)outputs[0] & 15u)) {
        refused = HapResult_Bad_Arguments;
    }
    r = composite_layers_staged(ctx, c, textures, texture_bytes, formats, alphas, alpha_bytes, refused, src, asrc);
    if (r != HapResult_No_Error)
        return r;
    for (i = 0; i < count; i++)
        if (!is_dev(ctx, outputs[i]))
            any_host_output = 1;
    /* (a destination in host memory is made in scratch and copied back) */
    if (any_host_output) {
        if (c->encoded)
            stage = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out.total);
        else
            (void)picture_stage(rt, &stage, shape.bytes, 1u, 0u);
        if (!stage)
            return HapResult_Internal_Error;
    }
    htab = composite_table(rt, composite_columns(c), 1u, c->layer_count, composite_stride(c), &dtab, &tab_bytes);
    if (!htab)
        return HapResult_Internal_Error;
    for (i = 0; i < count; i++)
        htab[i] = (uint64_t)(uintptr_t)(is_dev(ctx, outputs[i]) ? (uint8_t *)outputs[i] : c->encoded ? stage + out.off[i] : stage);
    for (l = 0; l < c->layer_count; l++)
        composite_descriptor(c, htab, 1u, l, 0u, l, src[l], asrc[l], formats[l]);
    if (hapgpu_rt_h2d(rt, dtab, htab, tab_bytes))
        return HapResult_Internal_Error;
    rc = launch_composite(rt, c, dtab, 1u);
    if (rc == 1)
        return HapResult_Bad_Arguments;
    for (i = 0; !rc && i < count; i++)
        if (!is_dev(ctx, outputs[i]))
            rc |= c->encoded ? hapgpu_rt_d2h(rt, outputs[i], stage + out.off[i], out.bytes[i])
                             : picture_unstage(rt, outputs[0], stage, &shape);
    if (rc || hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    for (i = 0; c->encoded && output_used && i < count; i++)
        output_used[i] = out.bytes[i];
    return HapResult_No_Error;
}

/* every entry of the result arrays a refusal sets (results: NULL for a call to pictures) */
static void composite_refuse(unsigned *layer_results, size_t layer_entries, unsigned *results, size_t frame_count,
                             unsigned code)
{
    size_t i;
    for (i = 0; i < layer_entries; i++)
        layer_results[i] = code;
    for (i = 0; results && i < frame_count; i++)
        results[i] = code;
}

unsigned hapb_composite_frames(HapGpuContext *ctx, const HapbComposite *c, unsigned frame_count,
                               const void *const *inputs, const unsigned long *input_bytes,
                               const unsigned *texture_counts, void *const *outputs, const unsigned long *output_bytes,
                               unsigned long *output_used, unsigned *layer_results, unsigned *results,
                               unsigned decode_flags)
{
    hapgpu_rt *rt = ctx->rt;
    const unsigned layer_count = c->layer_count, count = c->count;
    const size_t pixel_row = (size_t)c->width * 4u;
    const picture_shape shape = {c->row_bytes, pixel_row, (size_t)c->row_bytes * (c->height ? c->height - 1u : 0u) + pixel_row,
                                 c->height};
    const size_t total = (size_t)frame_count * layer_count;
    destination_layout out = {{0, 0}, {0, 0}, 0};
    unsigned canvas_widths[HAPGPU_COMPOSITE_MAX_LAYERS], canvas_heights[HAPGPU_COMPOSITE_MAX_LAYERS];
    size_t done, i;
    unsigned first_error = HapResult_No_Error, f, l;
    slice_textures s;
    const void **tex = NULL;    /* (encoded) per output frame and destination texture: what the encode half reads */
    unsigned *composited = NULL;    /* ... and per output frame: what its layers came to */
    if (!layer_results || (c->encoded && !results))
        return HapResult_Bad_Arguments;
    if (!hapb_composite_valid(c, frame_count, texture_counts, 1) || !inputs || !input_bytes || !outputs ||
        (c->encoded && (!output_bytes || !output_used))) {
        composite_refuse(layer_results, total, results, frame_count, HapResult_Bad_Arguments);
        return HapResult_Bad_Arguments;
    }
    if (frame_count == 0)
        return HapResult_No_Error;
    if (c->encoded)
        destination_layout_of(&out, count, c->formats, c->width, c->height);
    for (l = 0; l < layer_count; l++) {
        canvas_widths[l] = c->width;
        canvas_heights[l] = c->height;
    }
    /* output frames of a slice: at most 4 GiB of block textures, an encoded canvas's among them, and 32768 entries of the
       second stage at a time */
    if (context_busy(ctx, NULL, 0) ||
        !slice_textures_init(&s, frame_count, layer_count, texture_counts, c->layer_widths ? c->layer_widths : canvas_widths,
                             c->layer_widths ? c->layer_heights : canvas_heights, out.total, 0)) {
        composite_refuse(layer_results, total, results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    if (c->encoded) {
        tex = (const void **)malloc((sizeof(*tex) * count + sizeof(*composited)) * s.layout.at.slice);
        if (!tex) {
            free(s.in);
            composite_refuse(layer_results, total, results, frame_count, HapResult_Internal_Error);
            return HapResult_Internal_Error;
        }
        composited = (unsigned *)(tex + s.layout.at.slice * count);
    }
    for (done = 0; done < frame_count; done += s.layout.at.slice) {
        const hap_slice_layout *const at = &s.layout.at;
        const unsigned n = (unsigned)(frame_count - done < at->slice ? frame_count - done : at->slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, at->per_frame * n);
        uint8_t *encoded = c->encoded ? (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out.total * n) : NULL;
        uint8_t *stage = NULL;
        uint64_t *htab = NULL, *dtab = NULL;
        size_t tab_bytes = 0;
        unsigned present = 0;
        int rc = 0;
        if (textures && (encoded || !c->encoded)) {
            /* the second stage of every layer of every output frame of the slice, one batch: whole frames */
            slice_textures_decode(ctx, &s, textures, inputs, input_bytes, done, n, NULL, decode_flags);
            /* (after the second stage, which has tables of its own) */
            htab = composite_table(rt, composite_columns(c), n, layer_count, composite_stride(c), &dtab, &tab_bytes);
        }
        if (!htab) {
            composite_refuse(layer_results + done * layer_count, (size_t)n * layer_count, results ? results + done : NULL, n,
                             HapResult_Internal_Error);
            for (f = 0; c->encoded && f < n; f++)
                output_used[done + f] = 0;
            first_error = first_error ? first_error : HapResult_Internal_Error;
            continue;
        }
        for (f = 0; f < n; f++) {
            unsigned *frame_results = layer_results + (done + f) * layer_count;
            unsigned all = HapResult_No_Error;
            for (l = 0; l < layer_count; l++) {
                const size_t e = (size_t)f * at->entries_per_frame + at->entry_of[l];
                unsigned r = s.res[e];
                if (r == HapResult_No_Error && at->count_of[l] == 2u)
                    r = s.res[e + 1];
                /* the frame must hold exactly its layer's geometry, in one of the three formats a layer may have.  Where
                   layers have sizes of their own, a texture with more blocks than the layer's room holds is of another
                   size like one with fewer; a layer of the canvas's size keeps the second stage's code for that */
                if ((r == HapResult_Buffer_Too_Small && c->layer_widths) ||
                    (r == HapResult_No_Error && !slice_entry_fits(&s, e, l, k_rgba_kinds, 3u)))
                    r = HapResult_Bad_Arguments;
                frame_results[l] = r;
                if (r != HapResult_No_Error && all == HapResult_No_Error)
                    all = r;
                composite_descriptor(c, htab, n, (size_t)f * layer_count + l, done + f, l, s.outs[e],
                                     at->count_of[l] == 2u ? s.outs[e + 1] : NULL, s.fmts[e]);
            }
            if (c->encoded) {
                composited[f] = all;
                /* (an output frame with a failed layer has NULL textures: hapb_encode leaves it out) */
                for (i = 0; i < count; i++)
                    tex[(size_t)f * count + i] = all != HapResult_No_Error ? NULL :
                                                 (const void *)(encoded + out.total * f + out.off[i]);
                /* (a frame whose output hapb_encode will refuse is not worth the kernel's time either: address 0 skips it) */
                if (all == HapResult_No_Error && outputs[done + f] && output_bytes[done + f]) {
                    htab[f] = (uint64_t)(uintptr_t)tex[(size_t)f * count];
                    htab[n + f] = count == 2 ? (uint64_t)(uintptr_t)tex[(size_t)f * count + 1] : 0u;
                    present = 1;
                }
            } else {
                void *dst = outputs[done + f];
                unsigned picture = HapResult_No_Error;
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
        }
        if (present) {
            rc |= hapgpu_rt_h2d(rt, dtab, htab, tab_bytes);
            rc |= launch_composite(rt, c, dtab, n);
            for (f = 0; !c->encoded && f < n; f++)
                if (htab[f] && !is_dev(ctx, outputs[done + f]))
                    rc |= picture_unstage(rt, outputs[done + f], stage + align_up(shape.bytes, 256) * f, &shape);
        }
        if (c->encoded) {
            slice_encode_half(ctx, n, tex, composited, rc, 1, &out, count, c->formats, c->compressors, c->chunk_counts,
                              c->encode_flags, outputs + done, output_bytes + done, output_used + done, results + done,
                              &first_error);
            continue;
        }
        rc |= hapgpu_rt_sync(rt);
        for (i = done * layer_count; i < (done + n) * layer_count; i++) {
            if (rc && layer_results[i] == HapResult_No_Error && htab[i / layer_count - done])
                layer_results[i] = HapResult_Internal_Error;
            if (layer_results[i] != HapResult_No_Error && first_error == HapResult_No_Error)
                first_error = layer_results[i];
        }
    }
    free(s.in); free(tex);
    return first_error;
}

/* ============================================================= transcode */
/* Frames -> frames of other texture formats or of half / quarter size: hapb_decode into D_BC_TEX as in hapb_road_frames,
   the transcode kernel from there into D_TRANSCODED (one launch per source format present in the slice), hapb_encode on
   those textures -- or, for a frame that holds the wanted formats already, on its own.  No picture anywhere. */

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
    destination_layout out;
    size_t done;
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
    destination_layout_of(&out, count, formats, width >> scale_log2, height >> scale_log2);
    if (encode_textures_valid(count, out.bytes, formats, compressors, chunk_counts,
                              DESTINATION_ENCODE_FLAGS(encode_flags)) != HapResult_No_Error) {
        transcode_refuse(results, frame_count, HapResult_Bad_Arguments);
        return HapResult_Bad_Arguments;
    }
    if (!slice_textures_init(&s, frame_count, 1u, &texture_count, &width, &height, out.total, 0)) {
        transcode_refuse(results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    tex = (const void **)malloc((sizeof(*tex) * count + sizeof(*decoded)) * s.layout.at.slice);
    if (!tex) {
        free(s.in);
        transcode_refuse(results, frame_count, HapResult_Internal_Error);
        return HapResult_Internal_Error;
    }
    decoded = (unsigned *)(tex + s.layout.at.slice * count);
    for (done = 0; done < frame_count; done += s.layout.at.slice) {
        const unsigned n = (unsigned)(frame_count - done < s.layout.at.slice ? frame_count - done : s.layout.at.slice);
        uint8_t *textures = (uint8_t *)hapgpu_rt_device_scratch(rt, D_BC_TEX, s.layout.at.per_frame * n);
        uint8_t *transcoded = set ? (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out.total * n) : NULL;
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
                    if (s.fmts[e + i] != formats[i] || s.used[e + i] != out.bytes[i])
                        pass = 0;
                k = kind_of(kinds, kind_count, s.fmts[e]);
                /* else it must hold what the caller's geometry says, as for hapb_road_frames, in a format the kernel reads */
                if (!pass && (!set || !slice_entry_fits(&s, e, 0u, kinds, kind_count)))
                    r = HapResult_Bad_Arguments;
            }
            decoded[f] = r;
            for (i = 0; i < count; i++)
                tex[(size_t)f * count + i] = r != HapResult_No_Error ? NULL :
                                             pass ? s.outs[e + i] : (const void *)(transcoded + out.total * f + out.off[i]);
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
        /* (a frame whose decode half failed keeps what hapb_encode leaves in output_used) */
        slice_encode_half(ctx, n, tex, decoded, rc, 0, &out, count, formats, compressors, chunk_counts, encode_flags,
                          outputs + done, output_bytes + done, output_used + done, results + done, &first_error);
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
    destination_layout out;
    size_t need, alpha_need;
    const void *src = texture, *asrc = alpha;
    uint8_t *staged = NULL;
    unsigned i, k, set, align, r;
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
    /* every output there, large enough and, in device memory, aligned to its blocks; device sources aligned to what a
       lane reads of a block row (the block << scale_log2, at most 16 bytes) */
    destination_layout_of(&out, count, formats, width >> scale_log2, height >> scale_log2);
    r = destination_textures_fit(ctx, &out, count, formats, outputs, output_bytes);
    if (r != HapResult_No_Error)
        return r;
    align = (unsigned)(block << scale_log2) > 16u ? 16u : (unsigned)(block << scale_log2);
    if ((is_dev(ctx, texture) && ((uintptr_t)texture & (align - 1u))) ||
        (alpha && is_dev(ctx, alpha) && ((uintptr_t)alpha & ((8u << scale_log2 > 16u ? 16u : 8u << scale_log2) - 1u))))
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
            staged = (uint8_t *)hapgpu_rt_device_scratch(rt, D_TRANSCODED, out.total);
            if (!staged)
                return HapResult_Internal_Error;
        }
    if (pass) {
        for (i = 0; i < count; i++) {
            const void *from = i ? asrc : src;
            rc |= is_dev(ctx, outputs[i]) ? hapgpu_rt_d2d(rt, outputs[i], from, out.bytes[i])
                                          : hapgpu_rt_d2h(rt, outputs[i], from, out.bytes[i]);
        }
    } else {
        t.one[0] = (uint64_t)(uintptr_t)src;
        t.one[1] = (uint64_t)(uintptr_t)asrc;
        for (i = 0; i < count; i++)
            t.one[2u + i] = (uint64_t)(uintptr_t)(is_dev(ctx, outputs[i]) ? (uint8_t *)outputs[i] : staged + out.off[i]);
        rc = hapgpu_k_block_transcode(rt, &t, 1u, format, alpha != NULL, width, height, scale_log2, formats[0], count == 2);
        if (rc == 1)
            return HapResult_Bad_Arguments;
        for (i = 0; !rc && i < count; i++)
            if (!is_dev(ctx, outputs[i]))
                rc |= hapgpu_rt_d2h(rt, outputs[i], staged + out.off[i], out.bytes[i]);
    }
    if (rc || hapgpu_rt_sync(rt))
        return HapResult_Internal_Error;
    for (i = 0; output_used && i < count; i++)
        output_used[i] = out.bytes[i];
    return HapResult_No_Error;
}
