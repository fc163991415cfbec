/*
 * slice_layout.c -- hap_slice.h walked over its inputs by a plain program (built with -fsanitize=address,undefined by
 * tests/test_host_sanitizers.py): member counts {1}, {2}, {1, 2} and 16 members of 2; geometries from 4 x 4 to
 * 16384 x 16384; nothing else held per frame, and one texture more; 1 frame, exactly a slice, a slice and one.  Every
 * property is asserted against arithmetic written out here, and for one member against numbers recorded from the
 * function this header replaced.
 */
#include "hap_slice.h"
#include <stdio.h>

static unsigned long failures;
#define CHECK(cond) do { if (!(cond)) { failures++; fprintf(stderr, "line %d: %s (members %u, %u x %u, extra %zu, frames %zu)\n", \
                                                            __LINE__, #cond, members, w, h, extra, frames); } } while (0)

static size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }

/* the slice by the rule: 4 GiB / (per_frame + extra), at least 1, at most frame_count, then at most 32768 / entries */
static size_t slice_by_rule(size_t per_frame, size_t extra, size_t frames, unsigned entries)
{
    size_t slice = ((size_t)4u << 30) / (per_frame + extra);
    if (slice == 0)
        slice = 1;
    if (slice > frames)
        slice = frames;
    if (slice * entries > 32768u)
        slice = 32768u / entries;
    return slice;
}

static void walk(unsigned members, const unsigned *counts, unsigned w, unsigned h, size_t extra, size_t frames)
{
    const size_t blocks = (size_t)(w / 4u) * (h / 4u);
    hap_slice_layout s;
    size_t per_frame = 0;
    unsigned entries = 0, m, o;
    hap_slice_layout_of(&s, members, counts, w, h, extra, frames);
    CHECK(s.member_count == members && s.blocks == blocks && s.alpha_off == up256(blocks * 16u) && s.alpha_off % 256u == 0);
    for (m = 0; m < members; m++) {
        const unsigned count = counts ? counts[m] : 1u;
        const size_t end = s.offset_of[m] + s.alpha_off + (count == 2u ? blocks * 8u : 0u);
        CHECK(s.count_of[m] == count && s.entry_of[m] == entries);
        CHECK(s.offset_of[m] % 256u == 0 && (s.offset_of[m] + s.alpha_off) % 256u == 0);
        CHECK(s.offset_of[m] == per_frame && end <= s.per_frame);
        /* the colour texture ends where the plane begins at the latest, and no member's bytes are another's */
        CHECK(blocks * 16u <= s.alpha_off);
        for (o = 0; o < members; o++) {
            const size_t other_end = s.offset_of[o] + s.alpha_off + ((counts ? counts[o] : 1u) == 2u ? blocks * 8u : 0u);
            CHECK(o == m || s.offset_of[o] >= end || other_end <= s.offset_of[m]);
        }
        entries += count;
        per_frame += up256(blocks * 16u) + (count == 2u ? up256(blocks * 8u) : 0u);
    }
    CHECK(s.entries_per_frame == entries && s.per_frame == per_frame);
    CHECK(s.slice == slice_by_rule(per_frame, extra, frames, entries));
    CHECK(s.slice >= 1u && s.slice <= frames && s.slice * entries <= 32768u);
}

int main(void)
{
    static const unsigned one[1] = {1u}, two[1] = {2u}, mixed[2] = {1u, 2u};
    static const unsigned sixteen[16] = {2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u};
    static const struct { unsigned members; const unsigned *counts; } sets[] = {{1u, one}, {1u, two}, {2u, mixed}, {16u, sixteen},
                                                                                {1u, NULL}};
    static const unsigned sides[][2] = {{4, 4}, {8, 4}, {4, 8}, {260, 12}, {68, 64}, {1920, 1080}, {7680, 4320}, {16384, 4}, {16384, 16384}};
    /* tc, width, height, extra, frames -> alpha_off, per_frame, slice: what slice_textures_init gave before this header */
    static const struct { unsigned count, w, h; size_t extra, frames, alpha_off, per_frame, slice; } recorded[] = {
        {1, 4, 4, 0, 40000, 256, 256, 32768},
        {2, 4, 4, 0, 40000, 256, 512, 16384},
        {1, 16384, 16384, 0, 100, 268435456, 268435456, 16},
        {2, 16384, 16384, 268435456, 100, 268435456, 402653184, 6},
        {2, 260, 12, 0, 7, 3328, 5120, 7},
        {1, 1920, 1080, 2073600, 5000, 2073600, 2073600, 1035},
    };
    unsigned long walked = 0;
    unsigned i, g, x;
    for (i = 0; i < sizeof(sets) / sizeof(sets[0]); i++)
        for (g = 0; g < sizeof(sides) / sizeof(sides[0]); g++)
            for (x = 0; x < 2u; x++) {
                const unsigned w = sides[g][0], h = sides[g][1];
                const size_t extra = x ? up256((size_t)(w / 4u) * (h / 4u) * 16u) : 0u;
                hap_slice_layout whole;
                /* (a call of more frames than anything holds: its slice is what a slice holds at most) */
                hap_slice_layout_of(&whole, sets[i].members, sets[i].counts, w, h, extra, (size_t)1u << 40);
                walk(sets[i].members, sets[i].counts, w, h, extra, 1u);
                walk(sets[i].members, sets[i].counts, w, h, extra, whole.slice);
                walk(sets[i].members, sets[i].counts, w, h, extra, whole.slice + 1u);
                walked += 3u;
            }
    for (i = 0; i < sizeof(recorded) / sizeof(recorded[0]); i++) {
        const unsigned members = 1u, w = recorded[i].w, h = recorded[i].h;
        const size_t extra = recorded[i].extra, frames = recorded[i].frames;
        hap_slice_layout s;
        hap_slice_layout_of(&s, members, &recorded[i].count, w, h, extra, frames);
        CHECK(s.alpha_off == recorded[i].alpha_off && s.per_frame == recorded[i].per_frame && s.slice == recorded[i].slice);
        CHECK(s.entries_per_frame == recorded[i].count && s.offset_of[0] == 0u && s.entry_of[0] == 0u);
    }
    if (failures) {
        fprintf(stderr, "%lu checks failed\n", failures);
        return 1;
    }
    printf("%lu layouts walked, %u recorded ones equal: ok\n", walked, (unsigned)(sizeof(recorded) / sizeof(recorded[0])));
    return 0;
}
