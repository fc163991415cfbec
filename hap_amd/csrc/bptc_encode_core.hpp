// bptc_encode_core.hpp -- what the two BPTC encoders share: bptc_encode.hip (RGBA8 -> BC7) and bc6h_encode.hip
// (RGBA16F -> BC6H).  The byte-packed weight tables, a set's packed indices and its index field, the 128-bit block and
// the small integer helpers are stated here once.  Everything is __host__ __device__ and force-inlined: the files'
// block functions also run in a host build (tests/c/bptc_block_host.hip includes both files into one translation unit).
//
// Both kernels are bound by vector instruction issue, so the header takes only what leaves the instruction streams of
// all four kernels exactly as they were.  These are the same rule in both files and still stay in each, because a
// shared form changed a stream (one 4x4 block per lane unrolls to 31 000 / 54 000 vector instructions, and the order in
// which the compiler meets the same operations decides its schedule and register count):
//   rdiv and refit       one template over the top value and signedness, BC7's early-outs: BC7 identical, BC6H + 47
//                        vector instructions; BC6H's early-outs: BC7 not identical
//   the anchor rule      (index inversion by nibble mask, endpoint swap) BC6H <true> 424 VGPRs for 434
//   the index merge      BC7 - 4, BC6H + 54 vector instructions
//   index thresholds     (numerator from a callable) BC7 + 46 vector instructions
//   partition search     (over 16 packed sums) BC7 314 VGPRs for 315
// box_endpoints differs in earnest: BC6H shifts its covariance terms by a run-time `cs` that BC7 would compute only to
// find it zero.  So do the texel representations, the quantisers, the projection, sse, the tie rules and the mode
// assemblers.
#ifndef HAPGPU_BPTC_ENCODE_CORE_HPP
#define HAPGPU_BPTC_ENCODE_CORE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bptc_tables.hpp"

#define HD __host__ __device__ __forceinline__      // (stays defined: the two encoder files use it too)

namespace {
namespace hapbptc {

typedef unsigned long long u64;

HD int imin(int a, int b) { return a < b ? a : b; }
HD int imax(int a, int b) { return a > b ? a : b; }
HD int iabs(int a) { return a < 0 ? -a : a; }
HD int bitlen(int v) { return v > 0 ? 32 - __builtin_clz((unsigned)v) : 0; }

HD bool wave_any(bool v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_ballot_w64(v) != 0ull;
#else
    return v;
#endif
}

// weight of index i in the BPTC table of B bits, from byte-packed constants (no memory table: i varies per lane)
template <int B> HD int wgt(int i)
{
    const unsigned u = (unsigned)i;
    unsigned w;
    if (B == 2)
        w = 0x402B1500u;
    else if (B == 3)
        w = (u & 4u) ? 0x40372E25u : 0x1B120900u;
    else
        w = (u & 8u) ? ((u & 4u) ? 0x403C3733u : 0x2F2B2622u) : ((u & 4u) ? 0x1E1A1511u : 0x0D090400u);
    return (int)((w >> (8u * (u & 3u))) & 0xFFu);
}

// a set's indices: 4 bits per texel, texels 0..7 in lo, 8..15 in hi
HD unsigned idx_of(unsigned lo, unsigned hi, int t) { return ((t < 8 ? lo : hi) >> (4 * (t & 7))) & 15u; }

// the index field: B bits per texel, B - 1 at texel 0 and at texel a1 (a1 = 0: no second anchor)
template <int B> HD u64 index_field(unsigned lo, unsigned hi, int a1)
{
    u64 acc = 0ull;
    int at = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        acc |= (u64)idx_of(lo, hi, t) << at;
        at += (t == 0 || t == a1) ? B - 1 : B;
    }
    return acc;
}

// 128 bits, least significant first; positions are compile-time constants after unrolling
struct bits128 {
    u64 lo = 0, hi = 0;
    HD void put(u64 v, int pos, int n)
    {
        v &= n == 64 ? ~0ull : ((1ull << n) - 1ull);
        if (pos < 64) {
            lo |= v << pos;
            if (pos + n > 64)
                hi |= v >> (64 - pos);
        } else {
            hi |= v << (pos - 64);
        }
    }
    HD uint4 words() const { return make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)); }
};

} // namespace hapbptc
} // namespace

#endif
