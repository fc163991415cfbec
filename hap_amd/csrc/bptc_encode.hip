// bptc_encode.hip -- RGBA8 -> BC7 (RGBA_BPTC_UNORM, Hap R) block compression for gfx950.
//
// The integer algorithm is the one defined by tests/_bc7_encode.py (its docstring states every rounding rule and
// tie-break); results are bit-identical.  Opaque blocks: mode 6 with p-bits 1 against mode 1 on the partition of the
// best masked-sum estimate; blocks with alpha: mode 6 with searched p-bits against mode 5 (rotation 0).  Each candidate:
// bounding-box diagonal (covariance signs about the box centre, pivot = widest channel), nearest-weight indices by
// projection, one integer least-squares refit, indices again, the anchor rule, and the exact SSE of what the decoder
// will produce.
//
// Shape of bc_encode.hip: one 4x4 block per lane, a wavefront per 64 blocks of a block row, 16-byte row loads when the
// source allows.  Every lane runs one straight-line path for the candidates it may need; the only branches skip mode 1
// (no opaque block in the wave) or mode 5 (no block with alpha), and both conditions are ballots, uniform over the wave.
// Per-lane arrays are indexed by unrolled constants only, so nothing goes to scratch.
// The weight tables, index packing and the 128-bit block are bptc_encode_core.hpp's, shared with bc6h_encode.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapgpu_runtime.hpp"
#include "bptc_encode_core.hpp"

namespace {
namespace hapbc7 {

using namespace hapbptc;

HD int chan(unsigned px, int c) { return (int)((px >> (8 * c)) & 0xFFu); }

HD int unq(int code, int bits)
{
    const int v = code << (8 - bits);
    return v | (v >> bits);
}

// nearest code of cb bits (with p-bit p when HAS_P) to v: candidates floor(v / 2^(8 - cb)) - 1 .. + 1, ties to the lower
template <int CB, bool HAS_P>
HD void quant_channel(int v, int p, int &q, int &u)
{
    const int top = (1 << CB) - 1, base = v >> (8 - CB);
    int bq = 0, bu = 0, be = 1 << 20;
#pragma unroll
    for (int dq = -1; dq <= 1; dq++) {
        const int c = imin(imax(base + dq, 0), top);
        const int uu = HAS_P ? unq((c << 1) | p, CB + 1) : unq(c, CB);
        const int e = uu > v ? uu - v : v - uu;
        const bool take = e < be || (e == be && c < bq);
        bq = take ? c : bq;
        bu = take ? uu : bu;
        be = take ? e : be;
    }
    q = bq;
    u = bu;
}

// endpoint values -> codes and decoded values for one quantiser.  KIND 6: RGBA 7 + p per endpoint (forced 1 when
// opaque); KIND 1: RGB 6 + one p for both endpoints; KIND 7 / 8: plain 7 / 8 bits.
template <int KIND, int NC>
struct quantised {
    int q0[NC], q1[NC], d0[NC], d1[NC];
    int p0, p1;
};

template <int KIND, int NC>
HD void quantise(const int (&e0)[NC], const int (&e1)[NC], bool opaque, quantised<KIND, NC> &r)
{
    if (KIND == 6 || KIND == 1) {
        constexpr int CB = KIND == 6 ? 7 : 6;
        int qa0[NC], ua0[NC], qb0[NC], ub0[NC], qa1[NC], ua1[NC], qb1[NC], ub1[NC];
        int ea0 = 0, eb0 = 0, ea1 = 0, eb1 = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            quant_channel<CB, true>(e0[c], 0, qa0[c], ua0[c]);
            quant_channel<CB, true>(e0[c], 1, qb0[c], ub0[c]);
            quant_channel<CB, true>(e1[c], 0, qa1[c], ua1[c]);
            quant_channel<CB, true>(e1[c], 1, qb1[c], ub1[c]);
            ea0 += (ua0[c] - e0[c]) * (ua0[c] - e0[c]);
            eb0 += (ub0[c] - e0[c]) * (ub0[c] - e0[c]);
            ea1 += (ua1[c] - e1[c]) * (ua1[c] - e1[c]);
            eb1 += (ub1[c] - e1[c]) * (ub1[c] - e1[c]);
        }
        bool s0, s1;
        if (KIND == 6) {
            s0 = opaque || eb0 < ea0;
            s1 = opaque || eb1 < ea1;
        } else {
            s0 = s1 = (eb0 + eb1) < (ea0 + ea1);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            r.q0[c] = s0 ? qb0[c] : qa0[c];
            r.d0[c] = s0 ? ub0[c] : ua0[c];
            r.q1[c] = s1 ? qb1[c] : qa1[c];
            r.d1[c] = s1 ? ub1[c] : ua1[c];
        }
        r.p0 = s0 ? 1 : 0;
        r.p1 = s1 ? 1 : 0;
    } else {
        constexpr int CB = KIND;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            quant_channel<CB, false>(e0[c], 0, r.q0[c], r.d0[c]);
            quant_channel<CB, false>(e1[c], 0, r.q1[c], r.d1[c]);
        }
        r.p0 = r.p1 = 0;
    }
}

// steps 1-3: the bounding-box diagonal of the texels in m (a 16-bit mask, never empty) on channels C0 .. C0 + NC - 1
template <int C0, int NC>
HD void box_endpoints(const unsigned (&px)[16], unsigned m, int (&e0)[NC], int (&e1)[NC])
{
    int lo[NC], hi[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        lo[c] = 256;
        hi[c] = -1;
    }
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const bool in = (m >> t) & 1u;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int v = chan(px[t], C0 + c);
            lo[c] = in ? imin(lo[c], v) : lo[c];
            hi[c] = in ? imax(hi[c], v) : hi[c];
        }
    }
    int pivot = 0, prange = hi[0] - lo[0], plo = lo[0], phi = hi[0];
#pragma unroll
    for (int c = 1; c < NC; c++) {
        const bool take = hi[c] - lo[c] > prange;
        pivot = take ? c : pivot;
        prange = take ? hi[c] - lo[c] : prange;
        plo = take ? lo[c] : plo;
        phi = take ? hi[c] : phi;
    }
    int cov[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        cov[c] = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const bool in = (m >> t) & 1u;
        const int pv = 2 * chan(px[t], C0 + pivot) - plo - phi;
#pragma unroll
        for (int c = 0; c < NC; c++)
            cov[c] += in ? (2 * chan(px[t], C0 + c) - lo[c] - hi[c]) * pv : 0;
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const bool flip = cov[c] < 0 && c != pivot;
        e0[c] = flip ? hi[c] : lo[c];
        e1[c] = flip ? lo[c] : hi[c];
    }
}

// step 5: nearest-weight indices, 4 bits per texel (texels 0..7 in lo, 8..15 in hi)
template <int C0, int NC, int B>
HD void indices(const unsigned (&px)[16], const int (&d0)[NC], const int (&d1)[NC], unsigned &lo, unsigned &hi)
{
    int d[NC], den = 0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        d[c] = d1[c] - d0[c];
        den += d[c] * d[c];
    }
    int thr[(1 << B) - 1];
#pragma unroll
    for (int k = 1; k < (1 << B); k++)
        thr[k - 1] = (wgt<B>(k - 1) + wgt<B>(k)) * den;
    lo = hi = 0u;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        int num = 0;
#pragma unroll
        for (int c = 0; c < NC; c++)
            num += (chan(px[t], C0 + c) - d0[c]) * d[c];
        num *= 128;
        unsigned idx = 0u;
#pragma unroll
        for (int k = 0; k < (1 << B) - 1; k++)
            idx += num > thr[k] ? 1u : 0u;
        if (t < 8)
            lo |= idx << (4 * t);
        else
            hi |= idx << (4 * (t - 8));
    }
}

// rdiv(n, d) = 0 for n <= 0, else min(255, floor((n + floor(d / 2)) / d)); d > 0, n < 2^42
HD int rdiv(long long n, long long d)
{
    if (n <= 0)
        return 0;
    const long long n2 = n + d / 2;
    if (n2 >= 256 * d)
        return 255;
#ifdef __HIP_DEVICE_COMPILE__
    const float inv = __builtin_amdgcn_rcpf((float)d);
#else
    const float inv = 1.0f / (float)d;
#endif
    long long q = (long long)((float)n2 * inv);          // within 1 of the quotient: made exact below
    q = q < 0 ? 0 : q > 256 ? 256 : q;
    if (q * d > n2)
        q -= 1;
    else if ((q + 1) * d <= n2)
        q += 1;
    return q > 255 ? 255 : (int)q;
}

// step 6: least-squares endpoints from the indices of the texels in m; e0 / e1 stay when det = 0
template <int C0, int NC, int B>
HD void refit(const unsigned (&px)[16], unsigned m, unsigned lo, unsigned hi, int (&e0)[NC], int (&e1)[NC])
{
    int a = 0, b = 0, cc = 0, X[NC], Y[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        X[c] = Y[c] = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const bool in = (m >> t) & 1u;
        const int w = in ? wgt<B>((int)idx_of(lo, hi, t)) : 0, v = in ? 64 - w : 0;
        a += v * v;
        b += v * w;
        cc += w * w;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int x = chan(px[t], C0 + c);
            X[c] += v * x;
            Y[c] += w * x;
        }
    }
    const long long det = (long long)a * cc - (long long)b * b;
    if (det > 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            e0[c] = rdiv(64 * ((long long)cc * X[c] - (long long)b * Y[c]), det);
            e1[c] = rdiv(64 * ((long long)a * Y[c] - (long long)b * X[c]), det);
        }
    }
}

// steps 1-7 for one set of texels; the anchor rule (step 8) is the caller's
template <int C0, int NC, int B, int KIND>
HD void fit(const unsigned (&px)[16], unsigned m, bool opaque, quantised<KIND, NC> &r, unsigned &lo, unsigned &hi)
{
    int e0[NC], e1[NC];
    box_endpoints<C0, NC>(px, m, e0, e1);
    quantise<KIND, NC>(e0, e1, opaque, r);
    indices<C0, NC, B>(px, r.d0, r.d1, lo, hi);
    refit<C0, NC, B>(px, m, lo, hi, e0, e1);
    quantise<KIND, NC>(e0, e1, opaque, r);
    indices<C0, NC, B>(px, r.d0, r.d1, lo, hi);
}

// step 8 for the texels in m whose anchor is texel `anchor`: swap the endpoints and invert the indices
template <int KIND, int NC, int B>
HD void anchor_rule(quantised<KIND, NC> &r, unsigned m, int anchor, unsigned &lo, unsigned &hi)
{
    const unsigned top = 1u << (B - 1);
    const bool swap = (idx_of(lo, hi, anchor) & top) != 0u;
    // m as a nibble mask over the packed indices, times the inversion constant (2^B - 1) per nibble
    unsigned mlo = 0u, mhi = 0u;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        mlo |= ((m >> t) & 1u) * ((1u << B) - 1u) << (4 * t);
        mhi |= ((m >> (t + 8)) & 1u) * ((1u << B) - 1u) << (4 * t);
    }
    lo ^= swap ? mlo : 0u;                     // (2^B - 1 - i) = i xor (2^B - 1) for B-bit i
    hi ^= swap ? mhi : 0u;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int q0 = r.q0[c], d0 = r.d0[c];
        r.q0[c] = swap ? r.q1[c] : q0;
        r.q1[c] = swap ? q0 : r.q1[c];
        r.d0[c] = swap ? r.d1[c] : d0;
        r.d1[c] = swap ? d0 : r.d1[c];
    }
    const int p0 = r.p0;
    r.p0 = swap ? r.p1 : p0;
    r.p1 = swap ? p0 : r.p1;
}

// bits128 filled from bit 0 upwards
struct bits_appended : bits128 {
    int pos = 0;
    using bits128::put;
    HD void put(u64 v, int n)
    {
        put(v, pos, n);
        pos += n;
    }
};

template <int C0, int NC, int B>
HD int sse(const unsigned (&px)[16], const int (&d0)[NC], const int (&d1)[NC], unsigned m, unsigned lo, unsigned hi)
{
    int e = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const int w = wgt<B>((int)idx_of(lo, hi, t));
        int s = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int dec = ((64 - w) * d0[c] + w * d1[c] + 32) >> 6;
            const int diff = dec - chan(px[t], C0 + c);
            s += diff * diff;
        }
        e += ((m >> t) & 1u) ? s : 0;
    }
    return e;
}

HD int partition_of_block(const unsigned (&px)[16])
{
    // packed sums: R | G << 16 and B (at most 16 * 255 each)
    unsigned tot_rg = 0u, tot_b = 0u;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        tot_rg += (px[t] & 0xFFu) | ((px[t] & 0xFF00u) << 8);
        tot_b += (px[t] >> 16) & 0xFFu;
    }
    int best = 0;
    unsigned long long bs = 0ull, bd = 1ull;
#pragma unroll
    for (int p = 0; p < 64; p++) {
        const unsigned mask = k_partition2_masks[p];
        unsigned s_rg = 0u, s_b = 0u;
#pragma unroll
        for (int t = 0; t < 16; t++)
            if ((mask >> t) & 1u) {
                s_rg += (px[t] & 0xFFu) | ((px[t] & 0xFF00u) << 8);
                s_b += (px[t] >> 16) & 0xFFu;
            }
        const int n1 = __builtin_popcount(mask), n0 = 16 - n1;
        const unsigned o_rg = tot_rg - s_rg, o_b = tot_b - s_b;
        const unsigned r1 = s_rg & 0xFFFFu, g1 = s_rg >> 16, r0 = o_rg & 0xFFFFu, g0 = o_rg >> 16;
        const unsigned q1 = r1 * r1 + g1 * g1 + s_b * s_b, q0 = r0 * r0 + g0 * g0 + o_b * o_b;
        const unsigned long long score = (unsigned long long)q0 * (unsigned)n1 + (unsigned long long)q1 * (unsigned)n0;
        const unsigned den = (unsigned)(n0 * n1);
        const bool better = p == 0 || score * bd > bs * den;
        best = better ? p : best;
        bs = better ? score : bs;
        bd = better ? den : bd;
    }
    return best;
}

struct candidate {
    uint4 block;
    int err;
};

HD candidate mode6(const unsigned (&px)[16], bool opaque)
{
    quantised<6, 4> r;
    unsigned lo, hi;
    fit<0, 4, 4, 6>(px, 0xFFFFu, opaque, r, lo, hi);
    anchor_rule<6, 4, 4>(r, 0xFFFFu, 0, lo, hi);
    bits_appended o;
    o.put(1u << 6, 7);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        o.put((unsigned)r.q0[c], 7);
        o.put((unsigned)r.q1[c], 7);
    }
    o.put((unsigned)r.p0, 1);
    o.put((unsigned)r.p1, 1);
    o.put(index_field<4>(lo, hi, 0), 63);
    return {o.words(), sse<0, 4, 4>(px, r.d0, r.d1, 0xFFFFu, lo, hi)};
}

HD candidate mode1(const unsigned (&px)[16])
{
    const int part = partition_of_block(px);
    const unsigned m1 = k_partition2_masks[part], m0 = ~m1 & 0xFFFFu;
    const int a1 = (int)k_anchor2[part];
    quantised<1, 3> r0, r1;
    unsigned lo0, hi0, lo1, hi1;
    fit<0, 3, 3, 1>(px, m0, true, r0, lo0, hi0);
    anchor_rule<1, 3, 3>(r0, m0, 0, lo0, hi0);
    fit<0, 3, 3, 1>(px, m1, true, r1, lo1, hi1);
    anchor_rule<1, 3, 3>(r1, m1, a1, lo1, hi1);
    // texel t's index from its subset's set
    unsigned ml = 0u, mh = 0u;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        ml |= ((m1 >> t) & 1u) * 15u << (4 * t);
        mh |= ((m1 >> (t + 8)) & 1u) * 15u << (4 * t);
    }
    const unsigned lo = (lo0 & ~ml) | (lo1 & ml), hi = (hi0 & ~mh) | (hi1 & mh);
    bits_appended o;
    o.put(2u, 2);
    o.put((unsigned)part, 6);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o.put((unsigned)r0.q0[c], 6);
        o.put((unsigned)r0.q1[c], 6);
        o.put((unsigned)r1.q0[c], 6);
        o.put((unsigned)r1.q1[c], 6);
    }
    o.put((unsigned)r0.p0, 1);
    o.put((unsigned)r1.p0, 1);
    o.put(index_field<3>(lo, hi, a1), 46);
    const int err = sse<0, 3, 3>(px, r0.d0, r0.d1, m0, lo0, hi0) + sse<0, 3, 3>(px, r1.d0, r1.d1, m1, lo1, hi1);
    return {o.words(), err};
}

HD candidate mode5(const unsigned (&px)[16])
{
    quantised<7, 3> rc;
    quantised<8, 1> ra;
    unsigned clo, chi, alo, ahi;
    fit<0, 3, 2, 7>(px, 0xFFFFu, false, rc, clo, chi);
    anchor_rule<7, 3, 2>(rc, 0xFFFFu, 0, clo, chi);
    fit<3, 1, 2, 8>(px, 0xFFFFu, false, ra, alo, ahi);
    anchor_rule<8, 1, 2>(ra, 0xFFFFu, 0, alo, ahi);
    bits_appended o;
    o.put(1u << 5, 6);
    o.put(0u, 2);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o.put((unsigned)rc.q0[c], 7);
        o.put((unsigned)rc.q1[c], 7);
    }
    o.put((unsigned)ra.q0[0], 8);
    o.put((unsigned)ra.q1[0], 8);
    o.put(index_field<2>(clo, chi, 0), 31);
    o.put(index_field<2>(alo, ahi, 0), 31);
    return {o.words(), sse<0, 3, 2>(px, rc.d0, rc.d1, 0xFFFFu, clo, chi) + sse<3, 1, 2>(px, ra.d0, ra.d1, 0xFFFFu, alo, ahi)};
}

// one block: 16 RGBA8 texels (row-major, R in the low byte) -> the 16 BC7 bytes as four little-endian dwords.  Host and
// device alike (the HIP launch and a CPU build of this file run the same code).
HD uint4 hapgpu_bc7_encode_block(const unsigned (&px)[16])
{
    bool opaque = true;
#pragma unroll
    for (int t = 0; t < 16; t++)
        opaque = opaque && (px[t] >> 24) == 255u;
    candidate best = mode6(px, opaque);
    // (the lower mode wins a tie: mode 1 or 5 replaces mode 6 at equal error)
    if (wave_any(opaque)) {
        const candidate c = mode1(px);
        const bool take = opaque && c.err <= best.err;
        best.block = take ? c.block : best.block;
        best.err = take ? c.err : best.err;
    }
    if (wave_any(!opaque)) {
        const candidate c = mode5(px);
        const bool take = !opaque && c.err <= best.err;
        best.block = take ? c.block : best.block;
        best.err = take ? c.err : best.err;
    }
    return best.block;
}

template <bool WIDE>
__device__ __forceinline__ void encode_block(const uint8_t *__restrict__ rgba, size_t row_bytes, unsigned blocks_x,
                                             uint8_t *__restrict__ out)
{
    // one wavefront per 64 blocks of one block row: the row's address is scalar
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    const size_t id = (size_t)by * blocks_x + bx;
    const uint8_t *src = rgba + (size_t)(4u * by) * row_bytes + 16u * bx;
    unsigned p[16];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (WIDE) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)r * row_bytes);
            p[4 * r + 0] = v.x; p[4 * r + 1] = v.y; p[4 * r + 2] = v.z; p[4 * r + 3] = v.w;
        } else {
            const unsigned *q = reinterpret_cast<const unsigned *>(src + (size_t)r * row_bytes);
            p[4 * r + 0] = q[0]; p[4 * r + 1] = q[1]; p[4 * r + 2] = q[2]; p[4 * r + 3] = q[3];
        }
    }
    *reinterpret_cast<uint4 *>(out + id * 16u) = hapgpu_bc7_encode_block(p);
}

// pictures of one geometry in one launch: picture blockIdx.z, addresses from a HapGpuPictureTable (0: skip the picture)
template <bool WIDE>
__global__ __launch_bounds__(64) void bptc_encode_kernel(HapGpuPictureTable t, size_t row_bytes, unsigned blocks_x)
{
    const uint8_t *rgba = (const uint8_t *)picture_address(t, 0);
    uint8_t *out = (uint8_t *)picture_address(t, 1);
    if (!rgba || !out)
        return;
    encode_block<WIDE>(rgba, row_bytes, blocks_x, out);
}

} // namespace hapbc7
} // namespace

#ifndef HAPGPU_BPTC_ENCODE_HOST_ONLY
// RGBA_BPTC_UNORM of hapgpu_k_block_encode (bc_encode.hip): outputs 16-byte aligned
void hapgpu_launch_bptc_encode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                               size_t row_bytes, bool wide, hipStream_t stream)
{
    const dim3 grid((bx + 63u) / 64u, by, pictures), block(64);
    if (wide)
        hipLaunchKernelGGL(hapbc7::bptc_encode_kernel<true>, grid, block, 0, stream, t, row_bytes, bx);
    else
        hipLaunchKernelGGL(hapbc7::bptc_encode_kernel<false>, grid, block, 0, stream, t, row_bytes, bx);
}
#endif
