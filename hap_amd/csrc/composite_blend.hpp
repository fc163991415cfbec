// composite_blend.hpp -- how a layer's texel goes over the canvas (include/hap_gpu.h: HapGpuCompositeTextures,
// HapGpuCompositeFrames): "over" in integer arithmetic on bytes.  __host__ __device__: the kernel (bc_composite.hip)
// and the host sweep of tests/c/composite_blend_host.hip run the same text.
//
// The canvas (Rd, Gd, Bd, Ad) is premultiplied by its alpha; a layer's texel (Rs, Gs, Bs, As) is straight alpha, o the
// layer's opacity byte:
//     a  = rdiv255(As * o)
//     Cd = rdiv255(Cs * a + Cd * (255 - a))      for C = R, G, B
//     Ad = a + rdiv255(Ad * (255 - a))
// rdiv255(x) is the integer nearest to x / 255 for 0 <= x <= 65025 (255 is odd: no x lies on a tie).
//
// The first half is the definition as it is written; the second half is the same values two at a time in packed
// 16-bit lanes, which is what the kernel runs -- every intermediate stays below 65536.
#pragma once
#include <hip/hip_runtime.h>

namespace hapbc {
namespace composite {

// ---- the definition
__host__ __device__ __forceinline__ unsigned rdiv255(unsigned x)
{
    const unsigned t = x + 128u;
    return (t + (t >> 8)) >> 8;
}
__host__ __device__ __forceinline__ unsigned layer_alpha(unsigned As, unsigned o) { return rdiv255(As * o); }
__host__ __device__ __forceinline__ unsigned blend_colour(unsigned Cs, unsigned Cd, unsigned a)
{
    return rdiv255(Cs * a + Cd * (255u - a));
}
__host__ __device__ __forceinline__ unsigned blend_alpha(unsigned Ad, unsigned a) { return a + rdiv255(Ad * (255u - a)); }

// ---- the kernel's forms
typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
__host__ __device__ __forceinline__ pk_u16 as_pk_u16(unsigned v) { return __builtin_bit_cast(pk_u16, v); }
__host__ __device__ __forceinline__ unsigned as_dword(pk_u16 v) { return __builtin_bit_cast(unsigned, v); }

// A layer's opacity as its kernel constant: o * 257 (below 65536)
__host__ __device__ __forceinline__ unsigned opacity_scaled(unsigned o) { return o * 257u; }
// a = layer_alpha(As, o) in bits 16 .. 23 of the result and nothing above them: rdiv255(x) = ((x + 128) * 257) >> 16,
// since (t + (t >> 8)) >> 8 = floor((t + t / 256) / 256) whether t / 256 is rounded down first or not; and
// (As * o + 128) * 257 = As * (o * 257) + 32896 < 2^24 is ONE 24-bit multiply-add.  The kernel picks the byte with the
// v_perm_b32 that doubles it.
__host__ __device__ __forceinline__ unsigned layer_alpha_in_byte_2(unsigned As, unsigned o257)
{
    return As * o257 + 32896u;
}
// two lanes of rdiv255(s * a + d * (255 - a)): s, d, a bytes in 16-bit lanes, inv = 255 - a.  Colour channels as they
// are; the canvas's alpha with s = 255, since rdiv255(255 * a + y) = a + rdiv255(y) for an integer a.
// s * a + d * inv <= 255 * 255 = 65025; + 128 = 65153; + (t >> 8) <= 65407: no lane overflows.
__host__ __device__ __forceinline__ pk_u16 blend_pair(pk_u16 s, pk_u16 d, pk_u16 a, pk_u16 inv)
{
    const pk_u16 k128 = {128, 128}, k8 = {8, 8};
    pk_u16 t = s * a + k128;
#if defined(__HIP_DEVICE_COMPILE__)
    // (the value itself, not a sum to be regrouped: two v_pk_mad_u16 instead of multiply, multiply-add and add)
    asm("" : "+v"(t));
#endif
    t = d * inv + t;
    return (t + (t >> k8)) >> k8;
}

} // namespace composite
} // namespace hapbc
