/*
 * hap_slice.h -- how a call that goes on from block textures (hap_pictures.c) lays the textures of one output frame
 * out in scratch, and how many output frames it holds at a time.  Plain C arithmetic, no runtime: one definition for
 * the calls and for the stand-alone program that walks it (tests/c/slice_layout.c).
 *
 * An output frame has `member_count` members (one for the picture and transcode roads, one per layer for compositing),
 * each a frame read with 1 or 2 textures: a colour texture, in room for 16-byte blocks whatever its format, and for 2
 * the RGTC1 alpha plane behind it, both 256-byte aligned.  A slice holds at most 4 GiB of these textures together with
 * whatever else the caller keeps per frame, and at most 32768 entries of the second stage (a texture is one entry).
 */
#ifndef HAP_SLICE_H
#define HAP_SLICE_H

#include <stddef.h>

#define HAP_SLICE_BYTES ((size_t)4u << 30)
#define HAP_SLICE_ENTRIES 32768u
#define HAP_SLICE_MEMBERS_MAX 16u

typedef struct hap_slice_layout {
    unsigned member_count, entries_per_frame;
    unsigned count_of[HAP_SLICE_MEMBERS_MAX];   /* textures read of member m: 1 or 2 */
    unsigned entry_of[HAP_SLICE_MEMBERS_MAX];   /* member m's first entry within its frame's */
    size_t offset_of[HAP_SLICE_MEMBERS_MAX];    /* member m's colour texture within its frame's scratch; its plane: + alpha_off */
    size_t blocks, alpha_off, per_frame;        /* blocks of a texture; colour texture to plane; scratch bytes of a frame */
    size_t slice;                               /* output frames of a slice at most */
} hap_slice_layout;

static inline size_t hap_slice_align(size_t v) { return (v + 255u) / 256u * 256u; }

/* counts: member_count texture counts (NULL: all 1); extra_per_frame: what else the caller holds per frame while a
   slice's textures are held; frame_count: the call's, at least 1.  The library itself lays every slice out with
   hap_place.h's hap_place_layout_of, members of one size included, and no longer calls this: it stays as the definition
   of the one-size layout, which tests/c/slice_layout.c walks and tests/c/place_layout.c holds hap_place_layout_of
   against, member by member. */
static inline void hap_slice_layout_of(hap_slice_layout *s, unsigned member_count, const unsigned *counts, unsigned width,
                                       unsigned height, size_t extra_per_frame, size_t frame_count)
{
    unsigned m;
    s->member_count = member_count;
    s->blocks = (size_t)(width / 4u) * (height / 4u);
    s->alpha_off = hap_slice_align(s->blocks * 16u);
    s->entries_per_frame = 0u;
    s->per_frame = 0u;
    for (m = 0; m < member_count; m++) {
        s->count_of[m] = counts ? counts[m] : 1u;
        s->entry_of[m] = s->entries_per_frame;
        s->offset_of[m] = s->per_frame;
        s->entries_per_frame += s->count_of[m];
        s->per_frame += s->alpha_off + (s->count_of[m] == 2u ? hap_slice_align(s->blocks * 8u) : 0u);
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
