// ycbcr_rgb.hpp -- how an 8-bit Y, Cb, Cr sample of a video picture becomes an RGBA8 texel (include/hap_gpu.h:
// HapGpuCompressNV12).  __host__ __device__: the kernel (bc_encode_video.hip) and the host sweep of
// tests/c/ycbcr_rgb_host.hip run the same text; tests/_video_pictures.py is the numpy form.
//
// With y' = Y - luma_offset (16 limited, 0 full), u = Cb - 128, v = Cr - 128, in 32-bit signed integers, >> arithmetic:
//     R = clamp255((cy * y' + crv * v           + 32768) >> 16)
//     G = clamp255((cy * y' - cgu * u - cgv * v + 32768) >> 16)
//     B = clamp255((cy * y' + cbu * u           + 32768) >> 16)        A = 255
// The coefficients are the standards' exact rationals times 65536, rounded to nearest: with Kr, Kb = 0.299, 0.114
// (BT.601) or 0.2126, 0.0722 (BT.709) and Kg = 1 - Kr - Kb: crv = 2 (1 - Kr), cbu = 2 (1 - Kb), cgu = cbu Kb / Kg,
// cgv = crv Kr / Kg, cy = 1; limited range scales cy by 255/219 and the other four by 255/224.  The accumulators stay
// below 3.6e7 in magnitude, and before the clamp every channel is within 0.5016 of the exact real value.
//
// The chroma terms are those of a CbCr pair and are shared by the 2 x 2 luma samples it is replicated over: a block is
// 4 pairs and 16 luma samples, 20 + 16 multiplies.  Every factor fits 24 signed bits (138438 < 2^23, |y'|, |u|, |v| <=
// 255), so on the device the products are the full-rate v_mul_i32_i24's: the same integers.
#pragma once
#include <hip/hip_runtime.h>

namespace hapbc {
namespace video {

enum { kBT601 = 0, kBT709 = 1 };        // HapGpuYCbCrMatrix
enum { kLimited = 0, kFull = 1 };       // HapGpuYCbCrRange

// what a (matrix, range) pair comes to: wave-uniform, kernel arguments
struct coefficients {
    int cy, crv, cbu, cgu, cgv, luma_offset;
};

// (matrix and range inside their enums)
__host__ __device__ constexpr coefficients coefficients_of(unsigned matrix, unsigned range)
{
    //                                                          cy     crv     cbu    cgu    cgv
    return matrix == kBT601 ? (range == kLimited ? coefficients{76309, 104597, 132201, 25675, 53279, 16}    // BT601 Limited
                                                 : coefficients{65536, 91881, 116130, 22553, 46802, 0})     // BT601 Full
                            : (range == kLimited ? coefficients{76309, 117489, 138438, 13975, 34925, 16}    // BT709 Limited
                                                 : coefficients{65536, 103206, 121609, 12276, 30679, 0});   // BT709 Full
}

// a product of two factors within 24 signed bits
__host__ __device__ __forceinline__ int product(int a, int b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// An accumulator held to 0 .. 0xFFFFFF: bits 16 to 23 of it are clamp255(x >> 16) -- the shift is monotonic, a negative
// x stays below zero and 0xFFFFFF >> 16 is 255 -- so a channel is one v_med3_i32 and lands in its byte with a mask.
// (Not the clamp after the shift: for a pair of those hipcc picks gfx950's v_ashr_pk_u8_i32, and the one kernel it did
// that in, the Hap Q one, made other blocks than the definition's on the device.)
__host__ __device__ __forceinline__ unsigned held(int x) { return (unsigned)(x < 0 ? 0 : x > 0xFFFFFF ? 0xFFFFFF : x); }

// what a CbCr pair adds to the three channels of its luma samples, the rounding constant included
struct chroma_terms {
    int r, g, b;
};

__host__ __device__ __forceinline__ chroma_terms chroma_of(unsigned cb, unsigned cr, const coefficients &k)
{
    const int u = (int)cb - 128, v = (int)cr - 128;
    chroma_terms t;
    t.r = product(k.crv, v) + 32768;
    t.g = 32768 - product(k.cgu, u) - product(k.cgv, v);
    t.b = product(k.cbu, u) + 32768;
    return t;
}

// the texel R | G << 8 | B << 16 | 0xFF000000 of one luma sample under its pair's terms
__host__ __device__ __forceinline__ unsigned rgba_of_luma(unsigned y, const chroma_terms &t, const coefficients &k)
{
    const int l = product(k.cy, (int)y - k.luma_offset);
    return held(l + t.r) >> 16 | (held(l + t.g) >> 8 & 0x0000FF00u) | (held(l + t.b) & 0x00FF0000u) | 0xFF000000u;
}

// ... of one (Y, Cb, Cr) sample: the definition
__host__ __device__ __forceinline__ unsigned rgba_of(unsigned y, unsigned cb, unsigned cr, const coefficients &k)
{
    return rgba_of_luma(y, chroma_of(cb, cr, k), k);
}
__host__ __device__ __forceinline__ unsigned rgba_of(unsigned y, unsigned cb, unsigned cr, unsigned matrix, unsigned range)
{
    return rgba_of(y, cb, cr, coefficients_of(matrix, range));
}

} // namespace video
} // namespace hapbc
