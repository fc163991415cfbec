// rgb_ycbcr.hpp -- how RGBA8 texels become the 8-bit Y, Cb, Cr samples of an NV12 video picture (include/hap_gpu.h:
// HapGpuDecompressNV12): the way back of ycbcr_rgb.hpp.  __host__ __device__: the kernel (bc_decode_video.hip) and the
// host sweep of tests/c/rgb_ycbcr_host.hip run the same text; tests/_video_planes.py is the numpy form.
//
// In 32-bit signed integers, >> arithmetic, with Rs, Gs, Bs the sums of R, G, B over a pair's 2 x 2 texels (0 .. 1020):
//     Y  = lo + ((yr * R + yg * G + yb * B + 32768) >> 16)                                   (never outside 0 .. 255)
//     Cb = clamp255((-cbr * Rs - cbg * Gs + ch * Bs + (128 << 18) + (1 << 17)) >> 18)
//     Cr = clamp255(( ch * Rs - crg * Gs - crb * Bs + (128 << 18) + (1 << 17)) >> 18)
// The coefficients are the standards' exact rationals times 65536 -- Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722
// (BT.709), limited range scaling luma by 219/255 and chroma by 224/255 -- rounded to nearest, but yg, cbg and crg by
// subtraction (yg = round(65536 sy) - yr - yb, cbg = ch - cbr, crg = ch - crb): every row sums exactly, so greys give
// Cb = Cr = 128 and white and black 235 / 16 or 255 / 0.  The luma accumulator stays below 2^24, the chroma ones within
// 0 .. 2^26 -- full range reaches exactly 2^26, 256 after the shift: the clamp is part of the definition.
//
// Every factor fits 24 signed bits (46871 < 2^23, sums <= 1020), so on the device the products are the full-rate
// v_mul_i32_i24's: the same integers.
#pragma once
#include <hip/hip_runtime.h>

namespace hapbc {
namespace video {

// (HapGpuYCbCrMatrix: 0 BT601, 1 BT709; HapGpuYCbCrRange: 0 Limited, 1 Full -- ycbcr_rgb.hpp's enums)

// what a (matrix, range) pair comes to on the way to samples: wave-uniform, kernel arguments
struct sample_coefficients {
    int yr, yg, yb, cbr, cbg, ch, crg, crb, lo;
};

// (matrix and range inside their enums)
__host__ __device__ constexpr sample_coefficients sample_coefficients_of(unsigned matrix, unsigned range)
{
    //                                                         yr     yg    yb    cbr    cbg     ch    crg   crb  lo
    return matrix == 0u ? (range == 0u ? sample_coefficients{16829, 33039, 6416, 9714, 19070, 28784, 24103, 4681, 16}    // BT601 Limited
                                       : sample_coefficients{19595, 38470, 7471, 11058, 21710, 32768, 27439, 5329, 0})   // BT601 Full
                        : (range == 0u ? sample_coefficients{11966, 40254, 4064, 6596, 22188, 28784, 26145, 2639, 16}    // BT709 Limited
                                       : sample_coefficients{13933, 46871, 4732, 7509, 25259, 32768, 29763, 3005, 0});   // BT709 Full
}

// a product of two factors within 24 signed bits
__host__ __device__ __forceinline__ int sample_product(int a, int b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// Y of the texel R | G << 8 | B << 16 | A << 24 (alpha is not looked at)
__host__ __device__ __forceinline__ unsigned luma_of(unsigned texel, const sample_coefficients &k)
{
    const int r = (int)(texel & 0xFFu), g = (int)(texel >> 8 & 0xFFu), b = (int)(texel >> 16 & 0xFFu);
    return (unsigned)(k.lo + ((sample_product(k.yr, r) + sample_product(k.yg, g) + sample_product(k.yb, b) + 32768) >> 16));
}

// The sums of a pair's four texels, two channels to a word: rb = Rs | Bs << 16, ga = Gs | As << 16 (each at most 1020)
struct texel_sums {
    unsigned rb, ga;
};

__host__ __device__ __forceinline__ texel_sums sums_of(unsigned t0, unsigned t1, unsigned t2, unsigned t3)
{
    texel_sums s;
    s.rb = (t0 & 0x00FF00FFu) + (t1 & 0x00FF00FFu) + (t2 & 0x00FF00FFu) + (t3 & 0x00FF00FFu);
    s.ga = (t0 >> 8 & 0x00FF00FFu) + (t1 >> 8 & 0x00FF00FFu) + (t2 >> 8 & 0x00FF00FFu) + (t3 >> 8 & 0x00FF00FFu);
    return s;
}

// An accumulator held to 0 .. 0x3FFFFFF: shifted right by 18 it is clamp255(x >> 18) -- the shift is monotonic, a
// negative x stays below zero and 0x3FFFFFF >> 18 is 255.  (Held before the shift, as ycbcr_rgb.hpp's held(): the clamp
// written after the shift is what hipcc once turned into gfx950 code that differed from the definition.)
__host__ __device__ __forceinline__ unsigned held26(int x) { return (unsigned)(x < 0 ? 0 : x > 0x3FFFFFF ? 0x3FFFFFF : x); }

// the pair Cb | Cr << 8 of the sums Rs, Gs, Bs
__host__ __device__ __forceinline__ unsigned pair_of(int rs, int gs, int bs, const sample_coefficients &k)
{
    const int bias = (128 << 18) + (1 << 17);
    const int cb = sample_product(k.ch, bs) - sample_product(k.cbr, rs) - sample_product(k.cbg, gs) + bias;
    const int cr = sample_product(k.ch, rs) - sample_product(k.crg, gs) - sample_product(k.crb, bs) + bias;
    return held26(cb) >> 18 | (held26(cr) >> 18) << 8;
}

__host__ __device__ __forceinline__ unsigned pair_of(const texel_sums &s, const sample_coefficients &k)
{
    return pair_of((int)(s.rb & 0xFFFFu), (int)(s.ga & 0xFFFFu), (int)(s.rb >> 16), k);
}

// What a 4 x 4 block of texels p[4 * row + column] comes to: four rows of four Y samples and two rows of two pairs, each
// row one little-endian word as the planes hold it
__host__ __device__ __forceinline__ void samples_of_block(const unsigned (&p)[16], const sample_coefficients &k,
                                                          unsigned (&luma)[4], unsigned (&chroma)[2])
{
#pragma unroll
    for (int r = 0; r < 4; r++)
        luma[r] = luma_of(p[4 * r], k) | luma_of(p[4 * r + 1], k) << 8 | luma_of(p[4 * r + 2], k) << 16 |
                  luma_of(p[4 * r + 3], k) << 24;
#pragma unroll
    for (int j = 0; j < 2; j++)
        chroma[j] = pair_of(sums_of(p[8 * j], p[8 * j + 1], p[8 * j + 4], p[8 * j + 5]), k) |
                    pair_of(sums_of(p[8 * j + 2], p[8 * j + 3], p[8 * j + 6], p[8 * j + 7]), k) << 16;
}

} // namespace video
} // namespace hapbc
