/*
 * place_layout.c -- hap_place.h walked over its inputs by a plain program (built with -fsanitize=address,undefined by
 * tests/test_composite_place_host.py; nothing is preloaded).
 *
 * The clip: every block-aligned placement of layers of 1, 2, 5 and 17 blocks a side (sides mixed) on canvases of 1, 2, 4
 * and 17 blocks a side (sides mixed), every source rectangle of 1, 2 and all blocks a side at every place in its layer,
 * dst from one block beyond the left / top edge (the rectangle wholly outside, not even touching) to one beyond the
 * right / bottom, and 1 << 20 and its negative.  hap_place_clip_of is compared with a walk of the definition block by
 * block: per axis the definition says, texel by texel, which layer column (row) lies under a canvas column (row), and
 * every canvas block of every placement is then asked whether it is covered and which layer block is under it.
 * The refusals: every rule of hap_place_valid and hap_place_layer_valid, at its edge.
 * The scratch layout: hap_place_layout_of against arithmetic written out here, the way slice_layout.c does it --
 * offsets 256-byte aligned, no member's bytes another's, a slice's textures within 4 GiB and its entries within 32768.
 */
#include "hap_place.h"
#include <limits.h>
#include <stdio.h>

static unsigned long failures;
#define CHECK(cond) do { if (!(cond)) { failures++; if (failures < 20u) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

#define SIDE_MAX 17

/* one axis of a placement, in texels, and what the definition says of it: under[b] is the layer's block column (row)
   under canvas block column (row) b, -1 for none.  Texel by texel: canvas texel x is covered when dst <= x < dst + size
   and then has the layer's texel src + x - dst; on the grid, a block's four texels agree. */
typedef struct axis {
    unsigned src, size;
    int dst;
    unsigned layer, canvas;     /* sides in texels */
    int under[SIDE_MAX];
} axis;

static void axis_by_definition(axis *a)
{
    unsigned b, t;
    for (b = 0; b < a->canvas / 4u; b++) {
        int found = -2;
        for (t = 0; t < 4u; t++) {
            const long long x = (long long)(4u * b + t);
            int here = -1;
            if ((long long)a->dst <= x && x < (long long)a->dst + (long long)a->size)
                here = (int)(((long long)a->src + x - (long long)a->dst) / 4);
            CHECK(found == -2 || found == here);
            found = here;
        }
        a->under[b] = found;
    }
}

static unsigned long placements_walked, blocks_walked;

static void walk_placement(const axis *x, const axis *y)
{
    hap_place_clip c;
    unsigned bx, by;
    CHECK(hap_place_valid(x->src, y->src, x->size, y->size, x->dst, y->dst, x->layer, y->layer));
    hap_place_clip_of(&c, x->src, y->src, x->size, y->size, x->dst, y->dst, x->layer, x->canvas, y->canvas);
    CHECK(c.layer_blocks_x == x->layer / 4u);
    CHECK((c.cw == 0u) == (c.ch == 0u));
    CHECK((unsigned long long)c.cx0 + c.cw <= x->canvas / 4u && (unsigned long long)c.cy0 + c.ch <= y->canvas / 4u);
    for (by = 0; by < y->canvas / 4u; by++)
        for (bx = 0; bx < x->canvas / 4u; bx++) {
            const int covered = x->under[bx] >= 0 && y->under[by] >= 0;
            /* (the kernel's test: unsigned, so a block left of or above the clip wraps to a large number) */
            const unsigned ux = bx - c.cx0, uy = by - c.cy0;
            const int inside = ux < c.cw && uy < c.ch;
            CHECK(inside == covered);
            if (inside && covered) {
                const unsigned under = c.first + uy * c.layer_blocks_x + ux;
                CHECK(under == (unsigned)y->under[by] * (x->layer / 4u) + (unsigned)x->under[bx]);
                CHECK(under < (x->layer / 4u) * (y->layer / 4u));
            }
        }
    placements_walked++;
    blocks_walked += (unsigned long)(x->canvas / 4u) * (y->canvas / 4u);
}

/* every axis of a layer side and a canvas side (blocks): rectangles of 1, 2 and all blocks at every place, dst from one
   block beyond the near edge to one beyond the far edge, and +- 1 << 20 */
#define AXES_MAX 4096
static axis axes_x[AXES_MAX], axes_y[AXES_MAX];

static unsigned axes_of(axis *out, unsigned layer_blocks, unsigned canvas_blocks)
{
    const unsigned sizes[3] = {1u, 2u, layer_blocks};
    unsigned n = 0, k, s;
    int d;
    for (k = 0; k < 3u; k++) {
        const unsigned size = sizes[k];
        if (size > layer_blocks || (k < 2u && size == layer_blocks) || (k == 1u && size == 1u))
            continue;           /* (each size once: "all" is the last) */
        for (s = 0; s + size <= layer_blocks; s++) {
            const int lo = -(int)size - 1, hi = (int)canvas_blocks + 1;
            for (d = lo; d <= hi + 2; d++) {
                axis *a = &out[n++];
                a->src = 4u * s;
                a->size = 4u * size;
                a->dst = d <= hi ? 4 * d : d == hi + 1 ? HAP_PLACE_DST_MAX : -HAP_PLACE_DST_MAX;
                a->layer = 4u * layer_blocks;
                a->canvas = 4u * canvas_blocks;
                axis_by_definition(a);
            }
        }
    }
    return n;
}

static void walk_clips(void)
{
    static const unsigned layer_sides[4] = {1u, 2u, 5u, 17u}, canvas_sides[4] = {1u, 2u, 4u, 17u};
    unsigned lx, ly, cx, cy, i, j;
    for (lx = 0; lx < 4u; lx++)
        for (cx = 0; cx < 4u; cx++) {
            const unsigned nx = axes_of(axes_x, layer_sides[lx], canvas_sides[cx]);
            CHECK(nx > 0u && nx <= AXES_MAX);
            for (ly = 0; ly < 4u; ly++)
                for (cy = 0; cy < 4u; cy++) {
                    const unsigned ny = axes_of(axes_y, layer_sides[ly], canvas_sides[cy]);
                    for (i = 0; i < nx; i++)
                        for (j = 0; j < ny; j++)
                            walk_placement(&axes_x[i], &axes_y[j]);
                }
        }
}

/* the clip at the bounds of its arithmetic: the largest layer a call takes, its last block at a canvas's first and last */
static void walk_extremes(void)
{
    const unsigned lw = 0xFFFFFFFCu, lh = 16u;      /* 2^30 - 1 blocks a row, 4 rows: fewer than 2^32 blocks */
    hap_place_clip c;
    CHECK(hap_place_layer_valid(lw, lh));
    CHECK(hap_place_valid(lw - 4u, lh - 4u, 4u, 4u, 0, 0, lw, lh));
    hap_place_clip_of(&c, lw - 4u, lh - 4u, 4u, 4u, 0, 0, lw, 8u, 8u);
    CHECK(c.cx0 == 0u && c.cy0 == 0u && c.cw == 1u && c.ch == 1u && c.layer_blocks_x == lw / 4u);
    CHECK(c.first == 4u * (lw / 4u) - 1u);
    /* the whole layer a long way up and left: its last block under the canvas's first */
    CHECK(hap_place_valid(0u, 0u, 1u << 20, 16u, 4 - HAP_PLACE_DST_MAX, -12, 1u << 20, 16u));
    hap_place_clip_of(&c, 0u, 0u, 1u << 20, 16u, 4 - HAP_PLACE_DST_MAX, -12, 1u << 20, 8u, 8u);
    CHECK(c.cx0 == 0u && c.cy0 == 0u && c.cw == 1u && c.ch == 1u && c.first == 4u * (1u << 18) - 1u);
    /* a long way down and right of the largest canvas side that still meets it */
    hap_place_clip_of(&c, 0u, 0u, 8u, 8u, HAP_PLACE_DST_MAX, HAP_PLACE_DST_MAX, 8u, (unsigned)HAP_PLACE_DST_MAX + 4u,
                      (unsigned)HAP_PLACE_DST_MAX + 4u);
    CHECK(c.cx0 == (1u << 18) && c.cy0 == (1u << 18) && c.cw == 1u && c.ch == 1u && c.first == 0u);
    hap_place_clip_of(&c, 0u, 0u, 8u, 8u, HAP_PLACE_DST_MAX, 0, 8u, (unsigned)HAP_PLACE_DST_MAX, 8u);
    CHECK(c.cw == 0u && c.ch == 0u);
}

static void walk_refusals(void)
{
    const unsigned L = 32u;     /* a 32 x 32 layer */
    unsigned f, off;
    CHECK(hap_place_valid(0u, 0u, L, L, 0, 0, L, L));
    CHECK(hap_place_valid(4u, 8u, 28u, 24u, -4, 4, L, L));
    /* any of the six fields off the grid */
    for (f = 0; f < 6u; f++)
        for (off = 1u; off < 4u; off++) {
            unsigned v[4] = {4u, 4u, 8u, 8u};
            int d[2] = {8, -8};
            if (f < 4u)
                v[f] += off;
            else
                d[f - 4u] += (int)off;
            CHECK(!hap_place_valid(v[0], v[1], v[2], v[3], d[0], d[1], L, L));
            if (f >= 4u) {
                d[f - 4u] -= 2 * (int)off;
                CHECK(!hap_place_valid(v[0], v[1], v[2], v[3], d[0], d[1], L, L));
            }
        }
    /* a width or height of 0 */
    CHECK(!hap_place_valid(0u, 0u, 0u, 4u, 0, 0, L, L) && !hap_place_valid(0u, 0u, 4u, 0u, 0, 0, L, L));
    CHECK(!hap_place_valid(L, L, 0u, 0u, 0, 0, L, L));
    /* a rectangle that leaves its layer: by a block, from its far corner, and by a sum that wraps */
    CHECK(hap_place_valid(L - 4u, L - 4u, 4u, 4u, 0, 0, L, L));
    CHECK(!hap_place_valid(L - 4u, 0u, 8u, 4u, 0, 0, L, L) && !hap_place_valid(0u, L - 4u, 4u, 8u, 0, 0, L, L));
    CHECK(!hap_place_valid(L, 0u, 4u, 4u, 0, 0, L, L) && !hap_place_valid(0u, L, 4u, 4u, 0, 0, L, L));
    CHECK(!hap_place_valid(0u, 0u, L + 4u, L, 0, 0, L, L) && !hap_place_valid(0u, 0u, L, L + 4u, 0, 0, L, L));
    CHECK(!hap_place_valid(0xFFFFFFFCu, 0u, 8u, 4u, 0, 0, L, L) && !hap_place_valid(0u, 0xFFFFFFFCu, 4u, 8u, 0, 0, L, L));
    CHECK(!hap_place_valid(8u, 0u, 0xFFFFFFFCu, 4u, 0, 0, L, L) && !hap_place_valid(0u, 8u, 4u, 0xFFFFFFFCu, 0, 0, L, L));
    /* |dst| above 1 << 20 */
    CHECK(hap_place_valid(0u, 0u, 4u, 4u, HAP_PLACE_DST_MAX, -HAP_PLACE_DST_MAX, L, L));
    CHECK(hap_place_valid(0u, 0u, 4u, 4u, -HAP_PLACE_DST_MAX, HAP_PLACE_DST_MAX, L, L));
    CHECK(!hap_place_valid(0u, 0u, 4u, 4u, HAP_PLACE_DST_MAX + 4, 0, L, L) && !hap_place_valid(0u, 0u, 4u, 4u, 0, HAP_PLACE_DST_MAX + 4, L, L));
    CHECK(!hap_place_valid(0u, 0u, 4u, 4u, -HAP_PLACE_DST_MAX - 4, 0, L, L) && !hap_place_valid(0u, 0u, 4u, 4u, 0, -HAP_PLACE_DST_MAX - 4, L, L));
    CHECK(!hap_place_valid(0u, 0u, 4u, 4u, INT_MIN, 0, L, L) && !hap_place_valid(0u, 0u, 4u, 4u, 0, INT_MIN, L, L));
    CHECK(!hap_place_valid(0u, 0u, 4u, 4u, INT_MAX - 3, 0, L, L) && !hap_place_valid(0u, 0u, 4u, 4u, 0, INT_MAX - 3, L, L));
    /* a layer size that is 0, no multiple of 4, or of 2^32 blocks and more */
    CHECK(hap_place_layer_valid(4u, 4u) && hap_place_layer_valid(0xFFFFFFFCu, 16u) && hap_place_layer_valid(1u << 18, (1u << 18) - 4u));
    CHECK(!hap_place_layer_valid(0u, 4u) && !hap_place_layer_valid(4u, 0u) && !hap_place_layer_valid(0u, 0u));
    for (off = 1u; off < 4u; off++)
        CHECK(!hap_place_layer_valid(4u + off, 4u) && !hap_place_layer_valid(4u, 4u + off));
    /* (2^16 x 2^16 blocks are 2^32; (2^30 - 1) x 5 blocks are more) */
    CHECK(!hap_place_layer_valid(1u << 18, 1u << 18) && !hap_place_layer_valid(0xFFFFFFFCu, 20u) && !hap_place_layer_valid(20u, 0xFFFFFFFCu));
}

static size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }

static unsigned long layouts_walked, one_size_walked, one_size_with_extra_walked, one_member_walked;

static void walk_layout(unsigned members, const unsigned *counts, const unsigned *ws, const unsigned *hs, size_t extra, size_t frames)
{
    hap_place_layout p;
    size_t per_frame = 0, slice;
    unsigned entries = 0, m, o;
    hap_place_layout_of(&p, members, counts, ws, hs, extra, frames);
    CHECK(p.at.member_count == members && p.at.blocks == 0u && p.at.alpha_off == 0u);
    for (m = 0; m < members; m++) {
        const unsigned count = counts ? counts[m] : 1u;
        const size_t blocks = (size_t)(ws[m] / 4u) * (hs[m] / 4u);
        const size_t end = p.at.offset_of[m] + p.alpha_off_of[m] + (count == 2u ? blocks * 8u : 0u);
        CHECK(p.blocks_of[m] == blocks && p.alpha_off_of[m] == up256(blocks * 16u));
        CHECK(p.at.count_of[m] == count && p.at.entry_of[m] == entries);
        CHECK(p.at.offset_of[m] % 256u == 0 && (p.at.offset_of[m] + p.alpha_off_of[m]) % 256u == 0);
        CHECK(p.at.offset_of[m] == per_frame && end <= p.at.per_frame);
        /* the colour texture ends where the plane begins at the latest, and no member's bytes are another's */
        CHECK(blocks * 16u <= p.alpha_off_of[m]);
        for (o = 0; o < members; o++) {
            const size_t other_blocks = (size_t)(ws[o] / 4u) * (hs[o] / 4u);
            const size_t other_end = p.at.offset_of[o] + p.alpha_off_of[o] + ((counts ? counts[o] : 1u) == 2u ? other_blocks * 8u : 0u);
            CHECK(o == m || p.at.offset_of[o] >= end || other_end <= p.at.offset_of[m]);
        }
        entries += count;
        per_frame += up256(blocks * 16u) + (count == 2u ? up256(blocks * 8u) : 0u);
    }
    CHECK(p.at.entries_per_frame == entries && p.at.per_frame == per_frame);
    /* the slice by the rule: 4 GiB / (per_frame + extra), at least 1, at most frame_count, then at most 32768 / entries */
    slice = ((size_t)4u << 30) / (per_frame + extra);
    if (slice == 0)
        slice = 1;
    if (slice > frames)
        slice = frames;
    if (slice * entries > 32768u)
        slice = 32768u / entries;
    CHECK(p.at.slice == slice);
    CHECK(p.at.slice >= 1u && p.at.slice <= frames && p.at.slice * entries <= 32768u);
    CHECK(p.at.slice == 1u || p.at.slice * (per_frame + extra) <= ((size_t)4u << 30));
    /* members of one size: hap_slice.h's layout, number for number -- what lets every road lay its slices out with
       hap_place_layout_of, the roads whose members have one size included */
    for (m = 1; m < members && ws[m] == ws[0] && hs[m] == hs[0]; m++)
        ;
    if (m == members) {
        hap_slice_layout s;
        hap_slice_layout_of(&s, members, counts, ws[0], hs[0], extra, frames);
        CHECK(s.member_count == p.at.member_count);
        CHECK(s.per_frame == p.at.per_frame && s.slice == p.at.slice && s.entries_per_frame == p.at.entries_per_frame);
        for (m = 0; m < members; m++)
            CHECK(s.offset_of[m] == p.at.offset_of[m] && s.entry_of[m] == p.at.entry_of[m] && s.count_of[m] == p.at.count_of[m] &&
                  s.alpha_off == p.alpha_off_of[m] && s.blocks == p.blocks_of[m]);
        one_size_walked++;
        if (extra)
            one_size_with_extra_walked++;
        if (members == 1u)
            one_member_walked++;
    }
    layouts_walked++;
}

static void walk_layouts(void)
{
    static const unsigned sides[][2] = {{4, 4}, {8, 4}, {4, 8}, {260, 12}, {68, 64}, {1920, 1080}, {7680, 4320}, {16384, 4}, {16384, 16384}};
    const unsigned n_sides = (unsigned)(sizeof(sides) / sizeof(sides[0]));
    unsigned ws[16], hs[16], counts[16];
    unsigned members, shift, pattern, x, m;
    for (members = 1; members <= 16u; members += members < 3u ? 1u : 13u)         /* 1, 2, 3, 16 */
        for (shift = 0; shift < n_sides; shift++)
            for (pattern = 0; pattern < 4u; pattern++)
                for (x = 0; x < 2u; x++) {
                    hap_place_layout whole;
                    size_t extra;
                    /* member m: the m-th size from `shift` on (pattern 3: all of one size); counts all 1, all 2, mixed, NULL */
                    for (m = 0; m < members; m++) {
                        const unsigned g = pattern == 3u ? shift : (shift + m) % n_sides;
                        ws[m] = sides[g][0];
                        hs[m] = sides[g][1];
                        counts[m] = pattern == 0u ? 1u : pattern == 1u ? 2u : 1u + (m & 1u);
                    }
                    extra = x ? up256((size_t)(ws[0] / 4u) * (hs[0] / 4u) * 16u) : 0u;
                    hap_place_layout_of(&whole, members, pattern == 3u ? NULL : counts, ws, hs, extra, (size_t)1u << 40);
                    walk_layout(members, pattern == 3u ? NULL : counts, ws, hs, extra, 1u);
                    walk_layout(members, pattern == 3u ? NULL : counts, ws, hs, extra, whole.at.slice);
                    walk_layout(members, pattern == 3u ? NULL : counts, ws, hs, extra, whole.at.slice + 1u);
                }
}

int main(void)
{
    walk_clips();
    walk_extremes();
    walk_refusals();
    walk_layouts();
    /* (the agreement with hap_slice.h was asked for: one member, several of one size, and with something else held per frame) */
    CHECK(one_member_walked != 0 && one_size_walked > one_member_walked && one_size_with_extra_walked != 0);
    if (failures) {
        fprintf(stderr, "%lu checks failed\n", failures);
        return 1;
    }
    printf("%lu placements and %lu canvas blocks walked, %lu layouts: ok\n", placements_walked, blocks_walked, layouts_walked);
    return 0;
}
