// bc6h_encode.hip -- RGBA16F -> BC6H (RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT, Hap HDR) block compression for
// gfx950.
//
// The integer algorithm is the one defined by tests/_bc6h_encode.py (its docstring states every rounding rule and
// tie-break); results are bit-identical.  Each channel is normalised (NaN, Inf, negatives of the unsigned format) and
// taken to the 16-bit domain in front of the decoder's finish, where interpolation is linear.  One region: one fit
// (bounding-box diagonal, projection indices, one integer least-squares refit), then modes 0x03, 0x07, 0x0B and 0x0F
// each quantise its endpoints, index again and measure the exact error of what the decoder will produce; a transformed
// mode counts only where its deltas fit after the anchor rule.  Two regions (modes 0x1E, 0x01, 0x00 on the partition
// of the best masked-sum estimate) run when a block of the wave asks for them: that is a ballot, uniform over the wave.
//
// One 4x4 block per lane as in bptc_encode.hip, a wavefront per 64 blocks of a block row, eight 16-byte row loads
// per lane (a block row is 32 bytes), one 16-byte store.  Every lane runs one straight-line path.  The working values
// are kept two to a dword; the header layouts are compile-time run tables (the rows of bc6h_decode.hip's k_modes read
// the other way), so every field lands with constant shifts.  Per-lane arrays are indexed by unrolled constants only.
// The weight tables, index packing and the 128-bit block are bptc_encode_core.hpp's, shared with bptc_encode.hip; the
// fit itself (rdiv, refit, the anchor rule, the partition search) is that file's rule restated for 16-bit values.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapgpu_runtime.hpp"
#include "bptc_encode_core.hpp"

namespace {
namespace hapbc6h {

using namespace hapbptc;

// the block's working values: R | G << 16 and B, 16 bits each (two's complement in the signed format)
struct texels {
    unsigned rg[16], b[16];
};

template <bool S> HD int chan(const texels &x, int t, int c)
{
    const unsigned v = c == 2 ? x.b[t] : x.rg[t];
    if (S)
        return c == 1 ? (int)v >> 16 : (int)(short)(v & 0xFFFFu);
    return c == 1 ? (int)(v >> 16) : (int)(v & 0xFFFFu);
}

// a half bit pattern -> the normalised value in the working domain
template <bool S> HD int working(unsigned half)
{
    const unsigned mag = half & 0x7FFFu;
    const bool nan = mag > 0x7C00u, neg = (half & 0x8000u) != 0u;
    const unsigned h = mag > 0x7BFFu ? 0x7BFFu : mag;
    if (S) {
        const int u = (int)((32u * h + 30u) / 31u);
        return nan ? 0 : neg ? -u : u;
    }
    return nan || neg ? 0 : (int)((64u * h + 30u) / 31u);
}

// a 16-bit value -> the signed integer of the half pattern the decoder's finish writes
template <bool S> HD int finish(int v)
{
    if (S)
        return v < 0 ? -((-v * 31) >> 5) : (v * 31) >> 5;
    return (int)(((unsigned)v * 31u) >> 6);
}

// nearest code of PREC bits to v (the magnitude's, in the signed format): floor candidate - 1 .. + 1, ties to the lower
template <bool S, int PREC> HD void quant(int v, int &q, int &u)
{
    if (PREC >= (S ? 16 : 15)) {
        q = u = v;
        return;
    }
    constexpr int top = (1 << (S ? PREC - 1 : PREC)) - 1;
    const int mag = iabs(v), base = mag >> (16 - PREC);
    int bq = 0, bu = 0, be = 1 << 20;
#pragma unroll
    for (int dq = -1; dq <= 1; dq++) {
        const int c = imin(imax(base + dq, 0), top);
        const int mid = S ? ((c << 15) + 0x4000) >> (PREC - 1) : (int)((((unsigned)c << 16) + 0x8000u) >> PREC);
        const int uu = c == 0 ? 0 : c >= top ? (S ? 0x7FFF : 0xFFFF) : mid;
        const int e = iabs(uu - mag);
        const bool take = e < be || (e == be && c < bq);
        bq = take ? c : bq;
        bu = take ? uu : bu;
        be = take ? e : be;
    }
    q = v < 0 ? -bq : bq;
    u = v < 0 ? -bu : bu;
}

// what the first pass of a set of texels leaves for the final precisions: refitted endpoints and the set's box
struct fitted {
    int e0[3], e1[3], lo[3], hi[3];
};

// endpoint codes, unquantised endpoints and packed indices (4 bits a texel: 0..7 in lo, 8..15 in hi) of a set
struct region {
    int q0[3], q1[3], d0[3], d1[3];
    unsigned lo, hi;
};

// steps 1-3: the bounding-box diagonal of the texels in m (a 16-bit mask, never empty)
template <bool S> HD void box_endpoints(const texels &x, unsigned m, fitted &f)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        f.lo[c] = 1 << 20;
        f.hi[c] = -(1 << 20);
    }
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const bool in = (m >> t) & 1u;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int v = chan<S>(x, t, c);
            f.lo[c] = in ? imin(f.lo[c], v) : f.lo[c];
            f.hi[c] = in ? imax(f.hi[c], v) : f.hi[c];
        }
    }
    int pivot = 0, prange = f.hi[0] - f.lo[0], plo = f.lo[0], phi = f.hi[0];
#pragma unroll
    for (int c = 1; c < 3; c++) {
        const bool take = f.hi[c] - f.lo[c] > prange;
        pivot = take ? c : pivot;
        prange = take ? f.hi[c] - f.lo[c] : prange;
        plo = take ? f.lo[c] : plo;
        phi = take ? f.hi[c] : phi;
    }
    const int cs = imax(0, bitlen(prange) - 11);
    int cov[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const bool in = (m >> t) & 1u;
        const int xp = pivot == 0 ? chan<S>(x, t, 0) : pivot == 1 ? chan<S>(x, t, 1) : chan<S>(x, t, 2);
        const int pv = in ? (2 * xp - plo - phi) >> cs : 0;
#pragma unroll
        for (int c = 0; c < 3; c++)
            cov[c] += (in ? (2 * chan<S>(x, t, c) - f.lo[c] - f.hi[c]) >> cs : 0) * pv;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const bool flip = cov[c] < 0 && c != pivot;
        f.e0[c] = flip ? f.hi[c] : f.lo[c];
        f.e1[c] = flip ? f.lo[c] : f.hi[c];
    }
}

// step 5: nearest-weight indices on the segment d0 -> d1, in the set's own scale (texels outside the set get indices
// nobody reads: their products may wrap, so they are formed unsigned)
template <bool S, int B>
HD void indices(const texels &x, const fitted &f, const int (&d0)[3], const int (&d1)[3], unsigned &lo, unsigned &hi)
{
    int d[3], big = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d[c] = d1[c] - d0[c];
        big = imax(big, imax(iabs(d[c]), imax(iabs(f.lo[c] - d0[c]), iabs(f.hi[c] - d0[c]))));
    }
    const int s = imax(0, bitlen(big) - 10);
    int den = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d[c] >>= s;
        den += d[c] * d[c];
    }
    int thr[(1 << B) - 1];
#pragma unroll
    for (int k = 1; k < (1 << B); k++)
        thr[k - 1] = (wgt<B>(k - 1) + wgt<B>(k)) * den;
    lo = hi = 0u;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        unsigned acc = 0u;
#pragma unroll
        for (int c = 0; c < 3; c++)
            acc += (unsigned)((chan<S>(x, t, c) - d0[c]) >> s) * (unsigned)d[c];
        const int num = (int)(acc * 128u);
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

// rdiv(n, d) = sign(n) min(top, floor((|n| + floor(d / 2)) / d)), 0 for n < 0 in the unsigned format; 0 < d < 2^32
template <bool S> HD int rdiv(long long n, long long d)
{
    constexpr long long top = S ? 0x7FFF : 0xFFFF;
    const bool neg = n < 0;
    if (!S && neg)
        return 0;
    const long long n2 = (neg ? -n : n) + d / 2;
    long long q;
    if (n2 >= (top + 1) * d) {
        q = top;
    } else {
#ifdef __HIP_DEVICE_COMPILE__
        const float inv = __builtin_amdgcn_rcpf((float)d);
#else
        const float inv = 1.0f / (float)d;
#endif
        q = (long long)((float)n2 * inv);                 // within 1 of the quotient: made exact below
        q = q < 0 ? 0 : q > top + 1 ? top + 1 : q;
        if (q * d > n2)
            q -= 1;
        else if ((q + 1) * d <= n2)
            q += 1;
        q = q > top ? top : q;
    }
    return neg ? -(int)q : (int)q;
}

// step 6: least-squares endpoints from the indices of the texels in m; e0 / e1 stay when det = 0
template <bool S, int B> HD void refit(const texels &x, unsigned m, unsigned lo, unsigned hi, fitted &f)
{
    int a = 0, b = 0, cc = 0, X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const bool in = (m >> t) & 1u;
        const int w = in ? wgt<B>((int)idx_of(lo, hi, t)) : 0, v = in ? 64 - w : 0;
        a += v * v;
        b += v * w;
        cc += w * w;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int xv = chan<S>(x, t, c);
            X[c] += v * xv;
            Y[c] += w * xv;
        }
    }
    const long long det = (long long)a * cc - (long long)b * b;
    if (det > 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            f.e0[c] = rdiv<S>(64 * ((long long)cc * X[c] - (long long)b * Y[c]), det);
            f.e1[c] = rdiv<S>(64 * ((long long)a * Y[c] - (long long)b * X[c]), det);
        }
    }
}

// steps 1-6 for one set of texels, first precision P0
template <bool S, int B, int P0> HD void first_pass(const texels &x, unsigned m, fitted &f)
{
    box_endpoints<S>(x, m, f);
    int q, d0[3], d1[3];
    unsigned lo, hi;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        quant<S, P0>(f.e0[c], q, d0[c]);
        quant<S, P0>(f.e1[c], q, d1[c]);
    }
    indices<S, B>(x, f, d0, d1, lo, hi);
    refit<S, B>(x, m, lo, hi, f);
}

// steps 7-8 at one final precision: quantise, index again, and the anchor rule for the set m anchored at `anchor`
template <bool S, int B, int PREC> HD void final_pass(const texels &x, const fitted &f, unsigned m, int anchor, region &r)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        quant<S, PREC>(f.e0[c], r.q0[c], r.d0[c]);
        quant<S, PREC>(f.e1[c], r.q1[c], r.d1[c]);
    }
    indices<S, B>(x, f, r.d0, r.d1, r.lo, r.hi);
    const bool swap = (idx_of(r.lo, r.hi, anchor) >> (B - 1)) != 0u;
    // m as a nibble mask over the packed indices, times the inversion constant (2^B - 1) per nibble
    unsigned mlo = 0u, mhi = 0u;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        mlo |= ((m >> t) & 1u) * ((1u << B) - 1u) << (4 * t);
        mhi |= ((m >> (t + 8)) & 1u) * ((1u << B) - 1u) << (4 * t);
    }
    r.lo ^= swap ? mlo : 0u;                   // (2^B - 1 - i) = i xor (2^B - 1) for B-bit i
    r.hi ^= swap ? mhi : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int q0 = r.q0[c], d0 = r.d0[c];
        r.q0[c] = swap ? r.q1[c] : q0;
        r.q1[c] = swap ? q0 : r.q1[c];
        r.d0[c] = swap ? r.d1[c] : d0;
        r.d1[c] = swap ? d0 : r.d1[c];
    }
}

// the exact error of the texels in m: decoded against normalised input, both as integers of their half patterns
template <bool S, int B> HD u64 sse(const texels &x, const region &r, unsigned m)
{
    u64 e = 0ull;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const int w = wgt<B>((int)idx_of(r.lo, r.hi, t));
        const bool in = (m >> t) & 1u;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int dec = finish<S>(((64 - w) * r.d0[c] + w * r.d1[c] + 32) >> 6);
            const unsigned diff = (unsigned)iabs(dec - finish<S>(chan<S>(x, t, c)));      // < 2^16
            e += in ? (u64)(diff * diff) : 0ull;
        }
    }
    return e;
}

// ---- the header layouts: {block bit, length, field, first field bit, reversed} per run, the specification's table.
// Fields: w, x of region 0, y, z of region 1, per channel.
enum : int { RW, GW, BW, RX, GX, BX, RY, GY, BY, RZ, GZ, BZ };
struct run {
    int src, len, field, bit, rev;
};
struct mode_layout {
    int value, prec, dr, dg, db, transformed, runs;
    run r[24];
};
#define F(src, len, f, bit) {src, len, f, bit, 0}
#define R(src, len, f, bit) {src, len, f, bit, 1}
constexpr mode_layout k_mode03 = {0x03, 10, 10, 10, 10, 0, 6,
    {F(5, 10, RW, 0), F(15, 10, GW, 0), F(25, 10, BW, 0), F(35, 10, RX, 0), F(45, 10, GX, 0), F(55, 10, BX, 0)}};
constexpr mode_layout k_mode07 = {0x07, 11, 9, 9, 9, 1, 9,
    {F(5, 10, RW, 0), F(15, 10, GW, 0), F(25, 10, BW, 0), F(35, 9, RX, 0), F(44, 1, RW, 10), F(45, 9, GX, 0),
     F(54, 1, GW, 10), F(55, 9, BX, 0), F(64, 1, BW, 10)}};
constexpr mode_layout k_mode0B = {0x0B, 12, 8, 8, 8, 1, 9,
    {F(5, 10, RW, 0), F(15, 10, GW, 0), F(25, 10, BW, 0), F(35, 8, RX, 0), R(43, 2, RW, 10), F(45, 8, GX, 0),
     R(53, 2, GW, 10), F(55, 8, BX, 0), R(63, 2, BW, 10)}};
constexpr mode_layout k_mode0F = {0x0F, 16, 4, 4, 4, 1, 9,
    {F(5, 10, RW, 0), F(15, 10, GW, 0), F(25, 10, BW, 0), F(35, 4, RX, 0), R(39, 6, RW, 10), F(45, 4, GX, 0),
     R(49, 6, GW, 10), F(55, 4, BX, 0), R(59, 6, BW, 10)}};
constexpr mode_layout k_mode1E = {0x1E, 6, 6, 6, 6, 0, 21,
    {F(5, 6, RW, 0), F(15, 6, GW, 0), F(25, 6, BW, 0), F(35, 6, RX, 0), F(45, 6, GX, 0), F(55, 6, BX, 0),
     F(21, 1, GY, 5), F(24, 1, GY, 4), F(41, 4, GY, 0), F(65, 6, RY, 0), F(14, 1, BY, 4), F(22, 1, BY, 5), F(61, 4, BY, 0),
     F(71, 6, RZ, 0), F(11, 1, GZ, 4), F(12, 2, BZ, 0), F(23, 1, BZ, 2), F(31, 1, GZ, 5), F(32, 1, BZ, 3), R(33, 2, BZ, 4),
     F(51, 4, GZ, 0)}};
constexpr mode_layout k_mode01 = {0x01, 7, 6, 6, 6, 1, 20,
    {F(5, 7, RW, 0), F(15, 7, GW, 0), F(25, 7, BW, 0), F(35, 6, RX, 0), F(45, 6, GX, 0), F(55, 6, BX, 0),
     F(2, 1, GY, 5), F(24, 1, GY, 4), F(41, 4, GY, 0), F(65, 6, RY, 0), F(14, 1, BY, 4), F(22, 1, BY, 5), F(61, 4, BY, 0),
     F(71, 6, RZ, 0), F(3, 2, GZ, 4), F(12, 2, BZ, 0), F(23, 1, BZ, 2), F(32, 1, BZ, 3), R(33, 2, BZ, 4), F(51, 4, GZ, 0)}};
constexpr mode_layout k_mode00 = {0x00, 10, 5, 5, 5, 1, 19,
    {F(5, 10, RW, 0), F(15, 10, GW, 0), F(25, 10, BW, 0), F(35, 5, RX, 0), F(45, 5, GX, 0), F(55, 5, BX, 0),
     F(2, 1, GY, 4), F(41, 4, GY, 0), F(65, 5, RY, 0), F(3, 1, BY, 4), F(61, 4, BY, 0), F(71, 5, RZ, 0),
     F(4, 1, BZ, 4), F(40, 1, GZ, 4), F(50, 1, BZ, 0), F(51, 4, GZ, 0), F(60, 1, BZ, 1), F(70, 1, BZ, 2), F(76, 1, BZ, 3)}};
#undef F
#undef R

// every header bit of a layout is written exactly once: bits 2 / 5 .. 64 (one region) or .. 76 (two regions)
constexpr bool covers(const mode_layout &l, int first, int end)
{
    u64 lo = 0, hi = 0;
    for (int i = 0; i < l.runs; i++)
        for (int k = 0; k < l.r[i].len; k++) {
            const int p = l.r[i].src + k;
            u64 &w = p < 64 ? lo : hi;
            if (p < first || p >= end || (w >> (p & 63)) & 1)
                return false;
            w |= 1ull << (p & 63);
        }
    for (int p = first; p < end; p++)
        if (!(((p < 64 ? lo : hi) >> (p & 63)) & 1))
            return false;
    return true;
}
static_assert(covers(k_mode03, 5, 65) && covers(k_mode07, 5, 65) && covers(k_mode0B, 5, 65) && covers(k_mode0F, 5, 65),
              "a one-region layout leaves a header bit out or writes one twice");
static_assert(covers(k_mode1E, 5, 77) && covers(k_mode01, 2, 77) && covers(k_mode00, 2, 77),
              "a two-region layout leaves a header bit out or writes one twice");

// the mode bits and the endpoint fields (as stored: deltas already taken) by the mode's run table
template <const mode_layout &l> HD void put_header(bits128 &o, const int (&field)[12])
{
    o.put((unsigned)l.value, 0, l.value < 2 ? 2 : 5);
#pragma unroll
    for (int i = 0; i < 24; i++) {
        if (i >= l.runs)
            break;
        const run k = l.r[i];
        unsigned v = ((unsigned)field[k.field] >> k.bit) & ((1u << k.len) - 1u);
        if (k.rev)
            v = __builtin_bitreverse32(v) >> (32 - k.len);
        o.put(v, k.src, k.len);
    }
}

HD bool delta_fits(int d, int bits) { return d >= -(1 << (bits - 1)) && d <= (1 << (bits - 1)) - 1; }

struct candidate {
    uint4 block;
    u64 err;
};

HD void keep_better(candidate &best, bool allowed, const bits128 &o, u64 err)
{
    const bool take = allowed && err < best.err;          // (a tie stays with the earlier candidate)
    const uint4 w = o.words();
    best.block = take ? w : best.block;
    best.err = take ? err : best.err;
}

// one one-region mode from the shared first pass (`first`: mode 0x03, which every block has)
template <bool S, int PREC, const mode_layout &l>
HD void try_one_region(const texels &x, const fitted &f, candidate &best, bool first)
{
    region r;
    final_pass<S, 4, PREC>(x, f, 0xFFFFu, 0, r);
    int field[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool fits = true;
    const int db[3] = {l.dr, l.dg, l.db};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        field[RW + c] = r.q0[c];
        field[RX + c] = l.transformed ? r.q1[c] - r.q0[c] : r.q1[c];
        if (l.transformed)
            fits = fits && delta_fits(r.q1[c] - r.q0[c], db[c]);
    }
    bits128 o;
    put_header<l>(o, field);
    o.put(index_field<4>(r.lo, r.hi, 0), 65, 63);
    const u64 err = sse<S, 4>(x, r, 0xFFFFu);
    if (first) {
        best.block = o.words();
        best.err = err;
    } else {
        keep_better(best, fits, o, err);
    }
}

// the partition of the largest masked-sum score (tests/_bc6h_encode.py: best_partition), on 10-bit offsets from the
// block's box so that a channel's sums keep to 14 bits and |S|^2 to 32
template <bool S> HD int partition_of_block(const texels &x)
{
    int lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        lo[c] = 1 << 20;
        hi[c] = -(1 << 20);
    }
#pragma unroll
    for (int t = 0; t < 16; t++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = imin(lo[c], chan<S>(x, t, c));
            hi[c] = imax(hi[c], chan<S>(x, t, c));
        }
    const int ps = imax(0, bitlen(imax(hi[0] - lo[0], imax(hi[1] - lo[1], hi[2] - lo[2]))) - 10);
    unsigned y_rg[16], y_b[16], tot_rg = 0u, tot_b = 0u;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        y_rg[t] = (unsigned)((chan<S>(x, t, 0) - lo[0]) >> ps) | ((unsigned)((chan<S>(x, t, 1) - lo[1]) >> ps) << 16);
        y_b[t] = (unsigned)((chan<S>(x, t, 2) - lo[2]) >> ps);
        tot_rg += y_rg[t];
        tot_b += y_b[t];
    }
    int best = 0;
    u64 bs = 0ull, bd = 1ull;
#pragma unroll
    for (int p = 0; p < 32; p++) {
        const unsigned mask = k_partition2_masks[p];
        unsigned s_rg = 0u, s_b = 0u;
#pragma unroll
        for (int t = 0; t < 16; t++)
            if ((mask >> t) & 1u) {
                s_rg += y_rg[t];
                s_b += y_b[t];
            }
        const int n1 = __builtin_popcount(mask), n0 = 16 - n1;
        const unsigned o_rg = tot_rg - s_rg, o_b = tot_b - s_b;
        const unsigned r1 = s_rg & 0xFFFFu, g1 = s_rg >> 16, r0 = o_rg & 0xFFFFu, g0 = o_rg >> 16;
        const unsigned q1 = r1 * r1 + g1 * g1 + s_b * s_b, q0 = r0 * r0 + g0 * g0 + o_b * o_b;
        const u64 score = (u64)q0 * (unsigned)n1 + (u64)q1 * (unsigned)n0;
        const unsigned den = (unsigned)(n0 * n1);
        const bool better = p == 0 || score * bd > bs * den;
        best = better ? p : best;
        bs = better ? score : bs;
        bd = better ? den : bd;
    }
    return best;
}

template <bool S, int PREC, const mode_layout &l>
HD void try_two_regions(const texels &x, const fitted &f0, const fitted &f1, unsigned m0, unsigned m1, int part, int a1,
                        bool asked, candidate &best)
{
    region r0, r1;
    final_pass<S, 3, PREC>(x, f0, m0, 0, r0);
    final_pass<S, 3, PREC>(x, f1, m1, a1, r1);
    int field[12];
    bool fits = true;
    const int db[3] = {l.dr, l.dg, l.db};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int w = r0.q0[c], e[3] = {r0.q1[c], r1.q0[c], r1.q1[c]};
        field[RW + c] = w;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            field[RX + 3 * k + c] = l.transformed ? e[k] - w : e[k];
            if (l.transformed)
                fits = fits && delta_fits(e[k] - w, db[c]);
        }
    }
    // texel t's index from its region's set
    unsigned ml = 0u, mh = 0u;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        ml |= ((m1 >> t) & 1u) * 15u << (4 * t);
        mh |= ((m1 >> (t + 8)) & 1u) * 15u << (4 * t);
    }
    const unsigned lo = (r0.lo & ~ml) | (r1.lo & ml), hi = (r0.hi & ~mh) | (r1.hi & mh);
    bits128 o;
    put_header<l>(o, field);
    o.put((unsigned)part, 77, 5);
    o.put(index_field<3>(lo, hi, a1), 82, 46);
    keep_better(best, asked && fits, o, sse<S, 3>(x, r0, m0) + sse<S, 3>(x, r1, m1));
}

// blocks whose best one-region error exceeds this ask for the two-region modes (TWO_REGION_ERROR of the definition)
constexpr u64 kTwoRegionError = 48ull * 16ull * 16ull;

// one block: 16 RGBA16F texels (row-major; dword 2t = R | G << 16, dword 2t + 1 = B | A << 16) -> the 16 BC6H bytes as
// four little-endian dwords.  Host and device alike.
template <bool S> HD uint4 hapgpu_bc6h_encode_block(const unsigned (&px)[32])
{
    texels x;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const unsigned r = (unsigned)working<S>(px[2 * t] & 0xFFFFu) & 0xFFFFu;
        const unsigned g = (unsigned)working<S>(px[2 * t] >> 16) & 0xFFFFu;
        x.rg[t] = r | (g << 16);
        x.b[t] = (unsigned)working<S>(px[2 * t + 1] & 0xFFFFu) & 0xFFFFu;
    }
    candidate best;
    {
        fitted f;
        first_pass<S, 4, 10>(x, 0xFFFFu, f);
        try_one_region<S, 10, k_mode03>(x, f, best, true);
        try_one_region<S, 11, k_mode07>(x, f, best, false);
        try_one_region<S, 12, k_mode0B>(x, f, best, false);
        try_one_region<S, 16, k_mode0F>(x, f, best, false);
    }
    const bool asked = best.err > kTwoRegionError;
    if (wave_any(asked)) {
        const int part = partition_of_block<S>(x);
        const unsigned m1 = k_partition2_masks[part], m0 = ~m1 & 0xFFFFu;
        const int a1 = (int)k_anchor2[part];
        fitted f0, f1;
        first_pass<S, 3, 6>(x, m0, f0);
        first_pass<S, 3, 6>(x, m1, f1);
        try_two_regions<S, 6, k_mode1E>(x, f0, f1, m0, m1, part, a1, asked, best);
        try_two_regions<S, 7, k_mode01>(x, f0, f1, m0, m1, part, a1, asked, best);
        try_two_regions<S, 10, k_mode00>(x, f0, f1, m0, m1, part, a1, asked, best);
    }
    return best.block;
}

// pictures of one geometry in one launch: picture blockIdx.z, addresses from a HapGpuPictureTable (0: skip the picture)
template <bool S>
__global__ __launch_bounds__(64) void bc6h_encode_kernel(HapGpuPictureTable t, size_t row_bytes, unsigned blocks_x)
{
    const uint8_t *rgbah = (const uint8_t *)picture_address(t, 0);
    uint8_t *out = (uint8_t *)picture_address(t, 1);
    if (!rgbah || !out)
        return;
    // one wavefront per 64 blocks of one block row: the row's address is scalar
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    const size_t id = (size_t)by * blocks_x + bx;
    const uint8_t *src = rgbah + (size_t)(4u * by) * row_bytes + 32u * (size_t)bx;
    unsigned p[32];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint4 a = *reinterpret_cast<const uint4 *>(src + (size_t)r * row_bytes);
        const uint4 b = *reinterpret_cast<const uint4 *>(src + (size_t)r * row_bytes + 16u);
        p[8 * r + 0] = a.x; p[8 * r + 1] = a.y; p[8 * r + 2] = a.z; p[8 * r + 3] = a.w;
        p[8 * r + 4] = b.x; p[8 * r + 5] = b.y; p[8 * r + 6] = b.z; p[8 * r + 7] = b.w;
    }
    *reinterpret_cast<uint4 *>(out + id * 16u) = hapgpu_bc6h_encode_block<S>(p);
}

} // namespace hapbc6h
} // namespace

#ifndef HAPGPU_BC6H_ENCODE_HOST_ONLY
// RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT of hapgpu_k_block_encode (bc_encode.hip): RGBA16F pictures, rows and
// addresses 16-byte aligned
void hapgpu_launch_bc6h_encode(const HapGpuPictureTable &t, unsigned pictures, bool is_signed, unsigned bx, unsigned by,
                               size_t row_bytes, hipStream_t stream)
{
    const dim3 grid((bx + 63u) / 64u, by, pictures), block(64);
    if (is_signed)
        hipLaunchKernelGGL(hapbc6h::bc6h_encode_kernel<true>, grid, block, 0, stream, t, row_bytes, bx);
    else
        hipLaunchKernelGGL(hapbc6h::bc6h_encode_kernel<false>, grid, block, 0, stream, t, row_bytes, bx);
}
#endif
