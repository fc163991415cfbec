// plane_quantise.hpp -- how an element of a planar float tensor becomes a texel byte (include/hap_gpu.h:
// HapGpuCompressPlanes): the inverse of bc_decode_planes.hip's element_of.  __host__ __device__: the kernel
// (bc_encode_planes.hip) and the host sweep of tests/c/plane_quantise_host.hip run the same text.
//
// For x, the element's value as binary32 (the conversion from half or bfloat16 is exact, subnormals kept):
//     t = x * scale         one binary32 multiply, round to nearest even
//     r = t + bias          one binary32 add, round to nearest even -- NOT a fused multiply-add
//     v = 0                 if not (r > 0): NaN, -0, everything negative, -Inf
//         255               if r >= 255: +Inf too
//         rint(r)           otherwise, halves to even (0.5 -> 0, 1.5 -> 2, 254.5 -> 254)
#pragma once
#include <hip/hip_runtime.h>

namespace hapbc {
namespace planes {

enum { kF16 = 0, kBF16 = 1, kF32 = 2 };     // HapGpuPlaneElement

// an element's bit pattern -> its value: all three exact
__host__ __device__ __forceinline__ float value_of_half(unsigned short bits)
{
    return (float)__builtin_bit_cast(_Float16, bits);                  // v_cvt_f32_f16: subnormal halves kept
}
__host__ __device__ __forceinline__ float value_of_bfloat(unsigned short bits)
{
    return __builtin_bit_cast(float, (unsigned)bits << 16);
}
__host__ __device__ __forceinline__ float value_of_float(unsigned bits) { return __builtin_bit_cast(float, bits); }

__host__ __device__ __forceinline__ unsigned quantise(float x, float scale, float bias)
{
    float r;
    {
        // the definition's two roundings: the multiply and the add stay apart
#pragma clang fp contract(off)
        const float t = x * scale;
        r = t + bias;
    }
    // The comparisons as the definition writes them (a NaN fails the first); in between, rounding to nearest even and
    // the conversion are exact.  (No v_med3_f32 / v_cvt_pk_u8_f32: what they make of a NaN and of the ties is theirs.)
    if (!(r > 0.0f))
        return 0u;
    if (r >= 255.0f)
        return 255u;
    return (unsigned)__builtin_rintf(r);
}

} // namespace planes
} // namespace hapbc
