// resample_taps_host.hip -- hap_amd/csrc/resample_taps.hpp compiled for the host (hipcc --offload-host-only -shared): the
// taps of an axis, and the blend both as the definition writes it and in the packed form the kernel runs, for
// tests/test_resample_taps_host.py.
#include <stddef.h>
#include <stdint.h>

#include "resample_taps.hpp"

using namespace hapbc::resample;

// i0[i], i1[i], w[i] = the taps of element i = 0 .. o - 1 of an axis of o elements over c texels
extern "C" void resample_taps(unsigned o, unsigned c, uint32_t *i0, uint32_t *i1, uint32_t *w)
{
    for (unsigned i = 0; i < o; i++) {
        const tap t = tap_of(i, o, c);
        i0[i] = t.i0;
        i1[i] = t.i1;
        w[i] = t.w;
    }
}

// out[(a << 8 | b) * 257 + w]: a blended with b at weight w along one axis, the other axis's weight 0.  kernel_form 0: the
// definition's blend_channel; 1: blend_texel, with a and b in all four channels of their texels (each channel's byte
// must come out) and other bytes in the two texels of weight 0.  vertical: the axis is y
extern "C" void resample_blend_axis_sweep(int kernel_form, int vertical, uint16_t *out)
{
    for (unsigned a = 0; a < 256u; a++)
        for (unsigned b = 0; b < 256u; b++)
            for (unsigned w = 0; w <= 256u; w++) {
                // (channel k of a's texel is a rotated by k: every channel sees every pair over the sweep)
                const unsigned pa = a | ((a + 1u) & 255u) << 8 | ((a + 2u) & 255u) << 16 | ((a + 3u) & 255u) << 24;
                const unsigned pb = b | ((b + 1u) & 255u) << 8 | ((b + 2u) & 255u) << 16 | ((b + 3u) & 255u) << 24;
                const unsigned junk0 = ~pa, junk1 = pb ^ 0x5AA5C33Cu;
                const unsigned p00 = pa, p01 = vertical ? junk0 : pb, p10 = vertical ? pb : junk0, p11 = junk1;
                const unsigned wx = vertical ? 0u : w, wy = vertical ? w : 0u;
                unsigned v;
                if (kernel_form) {
                    const unsigned t = blend_texel(p00, p01, p10, p11, wx, wy);
                    // channel k must be the blend of (a + k, b + k): all four folded into one 16-bit value that is the
                    // first channel's byte only where the other three are right
                    v = t & 255u;
                    for (unsigned k = 1; k < 4u; k++)
                        if (((t >> (8u * k)) & 255u) != blend_channel(p00, p01, p10, p11, k, wx, wy))
                            v = 0xFFFFu;
                } else {
                    v = blend_channel(p00, p01, p10, p11, 0u, wx, wy);
                }
                out[(size_t)(a << 8 | b) * 257u + w] = (uint16_t)v;
            }
}

// out[j] = the texel of four packed taps and two weights; kernel_form 0: four blend_channel, 1: blend_texel
extern "C" void resample_blend_texels(int kernel_form, size_t n, const uint32_t *p00, const uint32_t *p01, const uint32_t *p10,
                                      const uint32_t *p11, const uint32_t *wx, const uint32_t *wy, uint32_t *out)
{
    for (size_t j = 0; j < n; j++) {
        if (kernel_form) {
            out[j] = blend_texel(p00[j], p01[j], p10[j], p11[j], wx[j], wy[j]);
        } else {
            unsigned v = 0;
            for (unsigned k = 0; k < 4u; k++)
                v |= blend_channel(p00[j], p01[j], p10[j], p11[j], k, wx[j], wy[j]) << (8u * k);
            out[j] = v;
        }
    }
}
