/*
 * hap_place.h -- the geometry of compositing placed layers (include/hap_gpu.h: HapGpuPlacement,
 * HapGpuCompositeTexturesPlaced, HapGpuCompositeFramesPlaced): what a placement must be, what of it is visible on a
 * canvas, and how layers of sizes of their own lie in a slice's scratch.  Plain C arithmetic, no runtime: one definition
 * for the calls and for the stand-alone program that walks it (tests/c/place_layout.c).
 *
 * Everything is on the grid of 4 x 4 blocks, so a canvas block has at most one block of a layer under it.  Offsets on
 * the canvas are signed and at most HAP_PLACE_DST_MAX in magnitude; sizes are unsigned 32-bit numbers of texels, at most
 * 2^30 blocks a side; the clip is worked out in long long blocks, which holds every sum and product of these (the
 * largest, a layer's block index, is below 2^60), and what it gives fits 32 bits because a layer has fewer than 2^32
 * blocks (hap_place_layer_valid).
 */
#ifndef HAP_PLACE_H
#define HAP_PLACE_H

#include "hap_slice.h"

#define HAP_PLACE_DST_MAX (1 << 20)

/* 1: a layer's (or a canvas's) size is one the calls take: not 0, multiples of 4, fewer than 2^32 blocks */
static inline int hap_place_layer_valid(unsigned width, unsigned height)
{
    return width != 0u && height != 0u && !(width & 3u) && !(height & 3u) &&
           (unsigned long long)(width / 4u) * (height / 4u) <= 0xFFFFFFFFull;
}

/* 1: the placement is one of a layer_w x layer_h layer (itself valid): all six fields multiples of 4, a rectangle that
   is not empty and does not leave the layer, an offset of at most HAP_PLACE_DST_MAX either way */
static inline int hap_place_valid(unsigned src_x, unsigned src_y, unsigned width, unsigned height, int dst_x, int dst_y,
                                  unsigned layer_w, unsigned layer_h)
{
    /* (two's complement: a negative multiple of 4 has its low two bits clear as well) */
    if (((src_x | src_y | width | height | (unsigned)dst_x | (unsigned)dst_y) & 3u) || width == 0u || height == 0u)
        return 0;
    if (src_x > layer_w || width > layer_w - src_x || src_y > layer_h || height > layer_h - src_y)
        return 0;
    return dst_x >= -HAP_PLACE_DST_MAX && dst_x <= HAP_PLACE_DST_MAX && dst_y >= -HAP_PLACE_DST_MAX &&
           dst_y <= HAP_PLACE_DST_MAX;
}

/* What of a placement is visible, in blocks: canvas blocks cx0 <= bx < cx0 + cw, cy0 <= by < cy0 + ch (cw == 0, and ch:
   nothing), and under canvas block (bx, by) the layer's block first + (by - cy0) * layer_blocks_x + (bx - cx0). */
typedef struct hap_place_clip {
    unsigned cx0, cy0, cw, ch;
    unsigned first, layer_blocks_x;
} hap_place_clip;

/* the placement valid (hap_place_valid) for its layer, the canvas canvas_w x canvas_h (hap_place_layer_valid) */
static inline void hap_place_clip_of(hap_place_clip *c, unsigned src_x, unsigned src_y, unsigned width, unsigned height,
                                     int dst_x, int dst_y, unsigned layer_w, unsigned canvas_w, unsigned canvas_h)
{
    const long long dx = dst_x / 4, dy = dst_y / 4;                     /* (exact: multiples of 4) */
    const long long x0 = dx > 0 ? dx : 0, y0 = dy > 0 ? dy : 0;
    long long x1 = dx + (long long)(width / 4u), y1 = dy + (long long)(height / 4u);
    if (x1 > (long long)(canvas_w / 4u))
        x1 = (long long)(canvas_w / 4u);
    if (y1 > (long long)(canvas_h / 4u))
        y1 = (long long)(canvas_h / 4u);
    c->layer_blocks_x = layer_w / 4u;
    if (x1 <= x0 || y1 <= y0) {
        c->cx0 = c->cy0 = c->cw = c->ch = c->first = 0u;
        return;
    }
    c->cx0 = (unsigned)x0;
    c->cy0 = (unsigned)y0;
    c->cw = (unsigned)(x1 - x0);
    c->ch = (unsigned)(y1 - y0);
    c->first = (unsigned)(((long long)(src_y / 4u) + (y0 - dy)) * (long long)(layer_w / 4u) + (long long)(src_x / 4u) + (x0 - dx));
}

/* The scratch of one output frame whose members (layers) have sizes of their own: hap_slice_layout's, with a block
   count and a distance from colour texture to plane per member.  at.blocks and at.alpha_off are no member's and 0; the
   rest of `at` reads as hap_slice.h says, and the slice keeps its rule: at most 4 GiB and 32768 entries. */
typedef struct hap_place_layout {
    hap_slice_layout at;
    size_t blocks_of[HAP_SLICE_MEMBERS_MAX];        /* blocks of member m's textures */
    size_t alpha_off_of[HAP_SLICE_MEMBERS_MAX];     /* member m's colour texture to its plane */
} hap_place_layout;

/* counts: member_count texture counts (NULL: all 1); widths, heights: the members' sizes; frame_count: at least 1 */
static inline void hap_place_layout_of(hap_place_layout *p, unsigned member_count, const unsigned *counts,
                                       const unsigned *widths, const unsigned *heights, size_t extra_per_frame,
                                       size_t frame_count)
{
    hap_slice_layout *s = &p->at;
    unsigned m;
    s->member_count = member_count;
    s->blocks = 0u;
    s->alpha_off = 0u;
    s->entries_per_frame = 0u;
    s->per_frame = 0u;
    for (m = 0; m < member_count; m++) {
        p->blocks_of[m] = (size_t)(widths[m] / 4u) * (heights[m] / 4u);
        p->alpha_off_of[m] = hap_slice_align(p->blocks_of[m] * 16u);
        s->count_of[m] = counts ? counts[m] : 1u;
        s->entry_of[m] = s->entries_per_frame;
        s->offset_of[m] = s->per_frame;
        s->entries_per_frame += s->count_of[m];
        s->per_frame += p->alpha_off_of[m] + (s->count_of[m] == 2u ? hap_slice_align(p->blocks_of[m] * 8u) : 0u);
    }
    s->slice = HAP_SLICE_BYTES / (s->per_frame + extra_per_frame);
    if (s->slice == 0)
        s->slice = 1;
    if (s->slice > frame_count)
        s->slice = frame_count;
    if (s->slice * s->entries_per_frame > HAP_SLICE_ENTRIES)
        s->slice = HAP_SLICE_ENTRIES / s->entries_per_frame;
}

#endif
