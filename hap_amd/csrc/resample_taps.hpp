// resample_taps.hpp -- where an output texel of a resized crop samples, and how its four taps are blended
// (include/hap_gpu.h: HapGpuDecompressPlanesResized, HapGpuDecodeFramesPlanesResized): bilinear with pixel centres
// (align_corners = false) in integers only.  __host__ __device__: the kernel (bc_resample_planes.hip) and the host sweep
// of tests/c/resample_taps_host.hip run the same text.
//
// An output axis of o elements over a crop axis of c texels, element i = 0 .. o - 1:
//     num  = max((2 * i + 1) * c - o, 0)
//     i0   = min(num / (2 * o), c - 1)      i1 = min(i0 + 1, c - 1)      taps never leave the crop: edge texels repeat
//     frac = num % (2 * o)                  w  = (frac * 256 + o) / (2 * o)       0 .. 256, nearest, halves up
// With x0, x1, wx of the columns and y0, y1, wy of the rows, a channel's byte is
//     top = P[y0][x0] * (256 - wx) + P[y0][x1] * wx         (0 .. 65280)
//     bot = P[y1][x0] * (256 - wx) + P[y1][x1] * wx
//     v   = (top * (256 - wy) + bot * wy + 32768) >> 16     (0 .. 255)
// o is at most 16384 and c at most 4 * o: (2 * i + 1) * c < 2 * o * c <= 2^31 and frac * 256 + o < 2^24, so 32 bits hold
// every intermediate.  The divisions are plain unsigned divisions: exact.
//
// The first half is the definition as it is written; the second half is the horizontal step two channels at a time --
// R and B (or G and A) in the 16-bit halves of a dword, which a sum of at most 65280 never leaves --, which is what the
// kernel runs.
#pragma once
#include <hip/hip_runtime.h>

namespace hapbc {
namespace resample {

struct tap {
    unsigned i0, i1, w;       // the two texels of the crop axis and the second one's weight, 0 .. 256
};

// ---- the definition
__host__ __device__ __forceinline__ tap tap_of(unsigned i, unsigned o, unsigned c)
{
    const unsigned a = (2u * i + 1u) * c, num = a > o ? a - o : 0u, q = num / (2u * o), frac = num - q * (2u * o);
    tap t;
    t.i0 = q < c - 1u ? q : c - 1u;
    t.i1 = t.i0 + 1u < c - 1u ? t.i0 + 1u : c - 1u;
    t.w = (frac * 256u + o) / (2u * o);
    return t;
}

__host__ __device__ __forceinline__ unsigned blend_axis(unsigned a, unsigned b, unsigned w) { return a * (256u - w) + b * w; }

__host__ __device__ __forceinline__ unsigned blend_rows(unsigned top, unsigned bot, unsigned wy)
{
    return (top * (256u - wy) + bot * wy + 32768u) >> 16;
}

// one channel (k = 0 .. 3) of four packed texels R | G << 8 | B << 16 | A << 24
__host__ __device__ __forceinline__ unsigned blend_channel(unsigned p00, unsigned p01, unsigned p10, unsigned p11, unsigned k,
                                                           unsigned wx, unsigned wy)
{
    const unsigned s = 8u * k;
    return blend_rows(blend_axis((p00 >> s) & 255u, (p01 >> s) & 255u, wx), blend_axis((p10 >> s) & 255u, (p11 >> s) & 255u, wx), wy);
}

// ---- the kernel's form
// blend_axis of channels k and k + 2 of two packed texels at once (`odd`: k = 1, else k = 0): channel k's sum in the low
// half, channel k + 2's in the high half
__host__ __device__ __forceinline__ unsigned blend_axis_pair(unsigned a, unsigned b, unsigned w, bool odd)
{
    const unsigned a2 = (odd ? a >> 8 : a) & 0x00FF00FFu, b2 = (odd ? b >> 8 : b) & 0x00FF00FFu;
    return a2 * (256u - w) + b2 * w;
}

// the texel R | G << 8 | B << 16 | A << 24 of the four taps
__host__ __device__ __forceinline__ unsigned blend_texel(unsigned p00, unsigned p01, unsigned p10, unsigned p11, unsigned wx,
                                                         unsigned wy)
{
    const unsigned top_rb = blend_axis_pair(p00, p01, wx, false), top_ga = blend_axis_pair(p00, p01, wx, true);
    const unsigned bot_rb = blend_axis_pair(p10, p11, wx, false), bot_ga = blend_axis_pair(p10, p11, wx, true);
    return blend_rows(top_rb & 0xFFFFu, bot_rb & 0xFFFFu, wy) | blend_rows(top_ga & 0xFFFFu, bot_ga & 0xFFFFu, wy) << 8 |
           blend_rows(top_rb >> 16, bot_rb >> 16, wy) << 16 | blend_rows(top_ga >> 16, bot_ga >> 16, wy) << 24;
}

} // namespace resample
} // namespace hapbc
