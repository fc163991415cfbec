// bc_encode_core.hpp -- the block math of the RGBA8 -> DXT1 / DXT5 / scaled YCoCg-DXT5 / RGTC1 encoder: sixteen pixels of
// a lane in, the block's bits out.  Shared by bc_encode.hip (one block per lane, texture to memory) and the fused
// kernel of snappy_compress_blocks.hip (the block goes straight into the second stage).  The integer algorithm is the
// one defined by oracle/bc_oracle.c; results are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_refine_core.hpp"

namespace hapbc {

constexpr int kFmtDXT1 = 0, kFmtDXT5 = 1, kFmtYCoCg = 2, kFmtRGTC1 = 3;
constexpr int kFmtYCoCgAlpha = 4;      // Hap Q Alpha: scaled YCoCg-DXT5 + RGTC1 alpha plane from one read of the RGBA

// Inline-asm helpers below must never consume the result of a v_dot4 directly: gfx950 needs wait states between
// a dot product and a different VALU reader, and the compiler does not see through the asm to insert them.
// a * b + c on the 24-bit multiplier (full rate; the 32-bit one is quarter rate); |a|, |b| < 2^23
__device__ __forceinline__ int mad24(int a, int b, int c)
{
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
template <int K>      // K: inline constant (-16..64)
__device__ __forceinline__ int mad24k(int a, int c)
{
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "i"(K), "v"(c));
    return r;
}
// a * b + c on the unsigned 24-bit multiplier: the low 24 bits of a and of b, the low 32 bits of the sum
__device__ __forceinline__ unsigned mad24u(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
template <int K>      // a * K + K, K an inline constant: K (a + 1)
__device__ __forceinline__ unsigned mad24uk(unsigned a)
{
    unsigned r;
    asm("v_mad_u32_u24 %0, %1, %2, %2" : "=v"(r) : "v"(a), "i"(K));
    return r;
}

__device__ __forceinline__ int quant5(int v) { int t = mad24k<31>(v, 128); return (t + (t >> 8)) >> 8; }
__device__ __forceinline__ int quant6(int v) { int t = mad24k<63>(v, 128); return (t + (t >> 8)) >> 8; }
__device__ __forceinline__ int expand5(int q) { return (q << 3) | (q >> 2); }
__device__ __forceinline__ int expand6(int q) { return (q << 2) | (q >> 4); }

// two 16-bit halves of one register: the Co | Cg pairs of a scaled YCoCg block
typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
typedef short pk_i16 __attribute__((ext_vector_type(2)));

// both halves of v shifted left by the same count (the low half of sh's register serves both: op_sel_hi)
__device__ __forceinline__ pk_u16 pk_shl(pk_u16 v, unsigned sh)
{
    unsigned r;
    asm("v_pk_lshlrev_b16 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(sh), "v"(__builtin_bit_cast(unsigned, v)));
    return __builtin_bit_cast(pk_u16, r);
}


// Eight 3-bit fields holding (r + 1) mod 8 of the ramp positions r = 0..7 -> their S3TC codes 0->0, 7->1, r->r+1, all at
// once: (r + 1) mod 8 is the code already for r = 1..6; the two ends come out as 1 and 0 and want 0 and 1 -- the fields
// whose upper two bits are clear get their low bit turned over.  (Was a byte-table v_perm per pixel.)
__device__ __forceinline__ unsigned ramp_codes(unsigned w)
{
    return w ^ (~((w >> 1) | (w >> 2)) & 0x249249u);
}

// 8-byte alpha-style block: a0, a1, 16 x 3-bit codes (S3TC alpha / RGTC1 layout).  a[] holds the values less BIAS (the
// centred luma of a scaled YCoCg block: BIAS 128): box, range and ramp use only differences, the two end bytes get the
// BIAS back once per block.
template <int BIAS = 0>
__device__ __forceinline__ uint2 alpha_block(const int (&a)[16])
{
    int lo = a[0], hi = a[0];
#pragma unroll
    for (int i = 1; i < 16; i++) {
        lo = min(lo, a[i]);
        hi = max(hi, a[i]);
    }
    const int a0 = hi, a1 = lo;            // (the exact range: every pixel lies on the ramp, no position needs clamping)
    unsigned lo24 = 0, hi24 = 0;       // 3-bit codes of pixels 0..7 and 8..15
    if (a0 != a1) {
        // oracle/bc_oracle.c: with d = a0 - a1 and u = a0 - a (0..d), the ramp position is
        // r = ((14 u + max(d - 6, 0)) * m) >> 20, m = floor(2^19 / d) + 1 -- the pixel's place on the ramp rounded to
        // the nearest of its 8 steps (x * m >> 20 = x / 2d), thresholds moved by the 3/7 the decoder's steps are
        // rounded down on average; 0..7 by construction.  Per pixel: one multiply-add, shift, insert; the codes eight pixels at a time.
        const int d = a0 - a1;
        // floor(2^19 / d) from v_rcp_f32, exact as it comes for d = 1..255: where d does not divide 2^19 the quotient
        // lies 1 / d or more from a whole number, the reciprocal's one unit in the last place moves it by 1 / (16 d)
        // at most (2^19 / d x 2^-23; the product with 2^19 is exact), and a power of two has an exact reciprocal.
        // (tools/micro/rcp_floor_probe.hip asks the instruction: all 255 right; the luma-range sweep of
        // tests/test_packed_endpoints_gpu.py holds every d with every position against the definition.)
        const unsigned m = (unsigned)(524288.0f * __builtin_amdgcn_rcpf((float)d)) + 1u;
        // x = (14 (a0 - a) + bias) m as one multiply-add in a
        const int neg_m14 = -(int)(14u * m);                             // |.| < 2^23
        // (+ 2^20: the position comes out as r + 1, 1..8, and x stays below 2^24)
        const int start = mad24(a0, (int)(14u * m), (int)__umul24((unsigned)max(d - 6, 0), m)) + (1 << 20);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const unsigned r1 = (unsigned)mad24(a[i], neg_m14, start) >> 20;
            // three bits in from the top (the funnel shift drops bit 3 of an 8): after 8 pixels the fields occupy
            // bits 31:8, pixel 0 lowest
            if (i < 8)
                lo24 = __builtin_amdgcn_alignbit(r1, lo24, 3);
            else
                hi24 = __builtin_amdgcn_alignbit(r1, hi24, 3);
        }
        lo24 = ramp_codes(lo24 >> 8);
        hi24 = ramp_codes(hi24 >> 8);
    }
    const unsigned long long bits = (unsigned long long)lo24 | ((unsigned long long)hi24 << 24);
    // a0 + BIAS | (a1 + BIAS) << 8 as one sum: the two bytes do not meet
    const unsigned long long v = (unsigned long long)(unsigned)(a0 + (a1 << 8) + BIAS * 257) | (bits << 16);
    return make_uint2((unsigned)v, (unsigned)(v >> 32));
}

// The luma half of a scaled YCoCg block from NEGATED luma in byte 1: v[i] = 256 (255 - Y), what row 0 of the BIASED
// matrix form delivers less its junk byte (ycocg_weight_rows_biased(); the fused kernel alone).  The same block as
// alpha_block<128> makes from Y - 128, at two instructions a pixel for the ramp where that has three.
// With n = 255 - Y the definition's u = a0 - a is n - min n, so the box is taken on v as it stands and
//     x = (14 u + max(d - 6, 0)) m + 2^20  =  14 m n + start,   start = max(d - 6, 0) m + 2^20 - 14 m min n,
// whose bits 22..20 are (r + 1) mod 8 (x is below 2^24; its bit 23, set for r = 7 alone, is what the field drops anyway).
// v (2 * 14 m) = 512 * 14 m n: the unsigned 24-bit multiply-add (v below 2^16, 28 m at most 28 (2^19 + 1), below 2^24)
// leaves x << 9 modulo 2^32 when it starts from start << 9, so the field stands in the TOP three bits of the result and
// the funnel shift takes it from there, v_alignbit(acc, x9, 29) = acc << 3 | field -- the form gather_indices has, and
// like it walking each eight pixels from the last to the first.  The codes then stand in bits 23..0, pixel 0 lowest.
// Once a block the two end bytes come back as 255 - n, minimum and maximum changing places.
// (tests/test_luma_row_identity.py: the row for every R, G, B, and this form against alpha_block's and the
// definition's for every range, offset and pixel value.)
__device__ __forceinline__ uint2 luma_block_negated(const unsigned (&v)[16])
{
    unsigned lo = v[0], hi = v[0];
#pragma unroll
    for (int i = 1; i < 16; i++) {
        lo = min(lo, v[i]);
        hi = max(hi, v[i]);
    }
    unsigned lo24 = 0, hi24 = 0;       // 3-bit codes of pixels 0..7 and 8..15
    if (lo != hi) {
        const unsigned d = (hi - lo) >> 8;
        // m = floor(2^19 / d) + 1 as in alpha_block; the products on the 24-bit multiplier by name (left to itself the
        // compiler folds the + 1 into 64-bit multiply-adds, quarter rate)
        const unsigned m1 = (unsigned)(524288.0f * __builtin_amdgcn_rcpf((float)d));          // m - 1
        const unsigned m28 = mad24uk<28>(m1);
        const unsigned d6 = (unsigned)max((int)d - 6, 0);
        const unsigned start9 = ((mad24u(d6, m1, d6) << 9) + (1u << 29)) - mad24u(lo, m28, 0u);   // modulo 2^32
#pragma unroll
        for (int i = 7; i >= 0; i--) {
            lo24 = __builtin_amdgcn_alignbit(lo24, mad24u(v[i], m28, start9), 29);
            hi24 = __builtin_amdgcn_alignbit(hi24, mad24u(v[i + 8], m28, start9), 29);
        }
        lo24 = ramp_codes(lo24);
        hi24 = ramp_codes(hi24);
    }
    const unsigned long long bits = (unsigned long long)lo24 | ((unsigned long long)hi24 << 24);
    // a0 | a1 << 8 = 255 - min n | (255 - max n) << 8: min n from byte 1 of lo to byte 0, max n where it stands
    const unsigned long long w = (unsigned long long)(((lo >> 8) | hi) ^ 0xFFFFu) | (bits << 16);
    return make_uint2((unsigned)w, (unsigned)(w >> 32));
}

// 2-bit indices of 16 pixels for the palette p0, p1, (2 p0 + p1) / 3, (p0 + 2 p1) / 3 (oracle/bc_oracle.c,
// pick_indices): the entries lie at 3/3, 0/3, 2/3, 1/3 of the segment p1 .. p0, so the pixel is projected onto it,
//     t = (pixel - p1) . dir + len2 / 6 clamped to 0 .. len2 + len2 / 6,   dir = p0 - p1, len2 = |dir|^2,
//     pos = (t * floor(3 * 2^24 / len2)) >> 24,                            index = {1, 3, 2, 0}[pos].
// One unsigned byte dot product per pixel: channels whose direction is negative enter complemented (`flip` has 0xFF
// in those bytes, XOR-ed into the pixel unless FLIPPED says the caller did that already), the constants of the
// complement and of p1 . dir ride in the dot product's accumulator.  px, p0, p1: packed bytes, top byte zero.
struct projection {
    unsigned adir;      // |dir| per channel, packed
    unsigned flip;      // 0xFF where dir < 0
    int start;          // accumulator start: len2 / 6 - p1 . dir - 255 * (sum of |dir| over flipped channels)
    int top;            // len2 + len2 / 6
    unsigned m24;       // floor(3 * 2^24 / len2)
};

// floor(3 * 2^24 / len2) from the float reciprocal, corrected with the integer remainder (off by one at most)
__device__ __forceinline__ unsigned index_scale(unsigned len2)
{
    unsigned m = (unsigned)(50331648.0f * __builtin_amdgcn_rcpf((float)len2));
    const int rem = (int)(50331648u - m * len2);
    m += (rem >= (int)len2 ? 1u : 0u) - (rem < 0 ? 1u : 0u);
    return m;
}

// CHANNELS: 3, or 2 for the pairs of a scaled YCoCg block, whose third byte is zero on both sides (a channel with
// direction 0 adds nothing to any of the sums)
template <int CHANNELS = 3>
__device__ __forceinline__ projection make_projection(unsigned p0, unsigned p1)
{
    projection pr;
    // per-byte |p0 - p1| and the sign bytes: 9-bit lanes of a 32-bit subtraction would borrow across bytes, so per channel
    int dir[CHANNELS];
    unsigned adir = 0, flip = 0;
    int neg = 0, base = 0;
#pragma unroll
    for (int c = 0; c < CHANNELS; c++) {
        const int a = (int)((p0 >> (8 * c)) & 255u), b = (int)((p1 >> (8 * c)) & 255u);
        dir[c] = a - b;
        const int ad = abs(dir[c]);
        adir |= (unsigned)ad << (8 * c);
        flip |= (dir[c] < 0 ? 0xFFu : 0u) << (8 * c);
        neg += dir[c] < 0 ? ad : 0;
        base = mad24(b, dir[c], base);
    }
    const unsigned len2 = __builtin_amdgcn_udot4(adir, adir, 0u, false);                 // 16 .. 195075
    const unsigned sixth = __umulhi(len2, 0xAAAAAAABu) >> 2;                             // len2 / 6
    pr.adir = adir;
    pr.flip = flip;
    pr.start = (int)sixth - base - 255 * neg;
    pr.top = (int)(len2 + sixth);
    pr.m24 = index_scale(len2);
    return pr;
}

// The clamp the definition states, t to 0 .. top, on four pixels at a time: four dot products, then four v_med3_i32 with
// a register as the upper bound (the compiler forms v_med3 between constants only).  The three dot products behind a
// pixel's own are the three wait states gfx950 wants between a dot product and another VALU reader of its result --
// inside one statement, where the compiler cannot see them, they have to stand there by construction.
#define HAPBC_CLAMPED_DOTS(OP)                                                                                           \
    asm(OP " %0, %4, %8, %9\n\t" OP " %1, %5, %8, %9\n\t" OP " %2, %6, %8, %9\n\t" OP " %3, %7, %8, %9\n\t"              \
        "v_med3_i32 %0, %0, 0, %10\n\tv_med3_i32 %1, %1, 0, %10\n\tv_med3_i32 %2, %2, 0, %10\n\tv_med3_i32 %3, %3, 0, %10" \
        : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])                                                             \
        : "v"(q0), "v"(q1), "v"(q2), "v"(q3), "v"(dir), "v"(start), "v"(top))
// byte pixels . byte direction + start
__device__ __forceinline__ void clamped_dot4(unsigned (&t)[4], unsigned q0, unsigned q1, unsigned q2, unsigned q3, unsigned dir, int start, int top)
{
    HAPBC_CLAMPED_DOTS("v_dot4_u32_u8");
}
// pairs of signed halves . pair of signed halves + start
__device__ __forceinline__ void clamped_dot2(unsigned (&t)[4], unsigned q0, unsigned q1, unsigned q2, unsigned q3, unsigned dir, int start, int top)
{
    HAPBC_CLAMPED_DOTS("v_dot2_i32_i16");
}
#undef HAPBC_CLAMPED_DOTS

// sixteen clamped projections -> sixteen 2-bit indices, pixel 0 in bits 1:0.  m24 * 64 moves the position,
// (t m24) >> 24, to the top two bits of a 32-bit product: top m24 < 3.5 x 2^24, so the product does not wrap, and
// top m24 >= 3 x 2^24, so a pixel clamped to top has position 3 (tests/test_index_selection_identity.py: every len2).
// The funnel shift takes the positions in from below, so the pixels are walked from the last to the first.
template <typename DOTS>
__device__ __forceinline__ unsigned gather_indices(unsigned m24, DOTS dots)
{
    const unsigned m30 = m24 << 6;
    unsigned pos2 = 0;
#pragma unroll
    for (int g = 3; g >= 0; g--) {
        unsigned t[4];
        dots(t, 4 * g);
#pragma unroll
        for (int k = 3; k >= 0; k--)
            pos2 = __builtin_amdgcn_alignbit(pos2, t[k] * m30, 30);          // pos2 << 2 | position
    }
    // positions -> indices {1, 3, 2, 0}, all 16 at once: index high bit = pos.hi ^ pos.lo, low bit = ~pos.hi
    const unsigned hi = pos2 & 0xAAAAAAAAu;
    return (hi ^ ((pos2 << 1) & 0xAAAAAAAAu)) | ((~hi >> 1) & 0x55555555u);
}

template <bool FLIPPED = false>
__device__ __forceinline__ unsigned project4(const unsigned (&px)[16], const projection &pr)
{
    return gather_indices(pr.m24, [&](unsigned (&t)[4], int i) {
        clamped_dot4(t, FLIPPED ? px[i] : px[i] ^ pr.flip, FLIPPED ? px[i + 1] : px[i + 1] ^ pr.flip,
                     FLIPPED ? px[i + 2] : px[i + 2] ^ pr.flip, FLIPPED ? px[i + 3] : px[i + 3] ^ pr.flip, pr.adir, pr.start, pr.top);
    });
}

__device__ __forceinline__ unsigned pack3(int a, int b, int c) { return (unsigned)a | ((unsigned)b << 8) | ((unsigned)c << 16); }

// the two end entries of the palette of a 5:6:5 endpoint pair, packed bytes (the blue field of a scaled YCoCg block
// carries the scale, not a colour: left out there)
__device__ __forceinline__ unsigned expand_565(unsigned c, bool blue)
{
    return pack3(expand5(c >> 11), expand6((c >> 5) & 63), blue ? expand5(c & 31) : 0);
}

// DXT1-style colour block from 16 packed RGB pixels (alpha byte already cleared).
// REFINE (HAPGPU_ENCODE_REFINE_ENDPOINTS): the block below is the start, and two rounds of bc_refine_core.hpp follow.  A
// round makes the least-squares end points for the indices the block has, gives them their indices with the same
// projection, and the pair replaces the block where its error is strictly smaller.  A round that does not win leaves
// the block as it was and the next makes the same candidate again, so two unconditional rounds with selects are the
// definition's "stop at the first failure"; the only branches are the ones around a projection that has no segment
// to project onto, as below.
template <bool REFINE = false>
__device__ __forceinline__ uint2 colour_block(const unsigned (&px)[16])
{
    int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int v = (int)((px[i] >> (8 * c)) & 255u);
            lo[c] = min(lo[c], v);
            hi[c] = max(hi[c], v);
        }
    }
    int cov_rg = 0, cov_bg = 0;
    const int mr = lo[0] + hi[0], mg = lo[1] + hi[1], mb = lo[2] + hi[2];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int dr = 2 * (int)(px[i] & 255u) - mr;
        const int dg = 2 * (int)((px[i] >> 8) & 255u) - mg;
        const int db = 2 * (int)((px[i] >> 16) & 255u) - mb;
        cov_rg = mad24(dr, dg, cov_rg);
        cov_bg = mad24(db, dg, cov_bg);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int inset = (hi[c] - lo[c]) >> 4;
        lo[c] += inset;
        hi[c] -= inset;
    }
    const int ar = cov_rg < 0 ? lo[0] : hi[0], br = cov_rg < 0 ? hi[0] : lo[0];
    const int ab = cov_bg < 0 ? lo[2] : hi[2], bb = cov_bg < 0 ? hi[2] : lo[2];
    const unsigned qa = (unsigned)(quant5(ar) << 11 | quant6(hi[1]) << 5 | quant5(ab));
    const unsigned qb = (unsigned)(quant5(br) << 11 | quant6(lo[1]) << 5 | quant5(bb));
    const unsigned c0 = max(qa, qb), c1 = min(qa, qb);
    unsigned idx = 0;
    if (c0 != c1)
        idx = project4(px, make_projection(expand_565(c0, true), expand_565(c1, true)));
    if constexpr (REFINE) {
        unsigned best0 = c0, best1 = c1, best_idx = idx;
        int best_rank = refine_rank(px, refine_make_palette(c0, c1), idx);
        const refine_sums plain = refine_plain_sums(px);
#pragma unroll
        for (int round = 0; round < 2; round++) {
            unsigned n0, n1, nidx = 0;
            const bool valid = refine_candidate(px, plain, refine_weights(best_idx), n0, n1);
            const refine_palette pal = refine_make_palette(n0, n1);
            if (valid && n0 != n1)
                nidx = project4(px, make_projection(pal.entry[0], pal.entry[1]));
            const int rank = refine_rank(px, pal, nidx);
            const bool win = valid && rank < best_rank;
            best0 = win ? n0 : best0;
            best1 = win ? n1 : best1;
            best_idx = win ? nidx : best_idx;
            best_rank = win ? rank : best_rank;
        }
        return make_uint2(best0 | (best1 << 16), best_idx);
    }
    return make_uint2(c0 | (c1 << 16), idx);
}

// Colour half of a scaled YCoCg-DXT5 block.  Co and Cg stay side by side as a pair of 16-bit halves from the box to the
// index constants, in one of two representations of the pixels:
//   BIASED       cc[i] = Co | Cg << 16, the definition's own values, 1..256 a half (the transform's addend tuple carries
//                the 128, ycocg_addend()): the fused kernel, which is bound by instruction issue;
//   not BIASED   cc[i] = Co - 128 | (Cg - 128) << 16, signed halves -127..128 (the transform with the inline constant):
//                the block-per-lane kernels, which are bound by memory and by their registers -- the tuple's four would
//                cost them a wave -- and keep the box by v_pk_min/max_i16 and the sums by v_pk_add_u16.
// The BIASED pixel loops use what NON-NEGATIVE halves allow:
//   * the box by v_pk_minimum3_f16 / v_pk_maximum3_f16, three pairs an instruction (8 + 8 where the two-input integer
//     forms took 15 + 16): a non-negative 16-bit integer below 0x7C00 read as an IEEE half orders as the integer does, and
//     the instruction returns one of its operands bit for bit -- 1..256 are subnormal halves, which the kernels' float
//     mode keeps (tools/micro/pk_minmax3_probe.hip asks the hardware);
//   * sum Co | sum Cg by 32-bit adds on the words (v_add3_u32): sixteen halves of at most 256 make at most 4096, so
//     nothing carries from Co's half into Cg's;
//   * sum Co Cg by v_mad_i32_i16 as before, products at most 2^16, sixteen of them at most 2^20.
// The covariance's sign is the same number whatever is added to every Co and every Cg, so it is taken from the biased
// values as they stand (mid = lo + hi 2..512, 4 mid - sums -3068..2032).  Once a block the box is RECENTRED, lo and hi
// less 128 | 128 (-127..128), and from there on the per-block work is the same in both representations: the scale (v_pk_lshlrev_b16; the
// scale is what the range leaves room for), the inset, the quantisation (v_pk_mad_u16 by 31 | 63, the constant carries
// the bias, 31 * 128 + 128 | 63 * 128 + 128, and the 16-bit wrap-around of a negative half times 31 or 63 is undone by
// adding it: the true sum lies in 0..16256) and the expansion are packed instructions on both channels at once, the
// 5:6:5 words, len2 and K one 16-bit dot product each (directions +-255, scaled directions +-1020).  The projection
// takes the pixels as they are: for BIASED ones its constant carries the - 128 (s d_o + s d_g), one more dot product a
// block.
// (tests/test_packed_endpoints_identity.py states the per-block form in 16-bit numpy arrays and compares it with the
// definition, tests/test_biased_pairs_identity.py the biased pixel loops and the projection constant.)
// The form of the Hap Q destinations (block_of<kFmtYCoCg, true, BIASED>); Hap Q Alpha keeps ycocg_colour_block_scalar
// below, on centred halves.
template <bool BIASED>
__device__ __forceinline__ uint2 ycocg_colour_block(const unsigned (&cc)[16])
{
    const auto pk_minimum3 = [](unsigned a, unsigned b, unsigned c) {
        unsigned r;
        asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
        return r;
    };
    const auto pk_maximum3 = [](unsigned a, unsigned b, unsigned c) {
        unsigned r;
        asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
        return r;
    };
    pk_i16 lo_b = __builtin_bit_cast(pk_i16, cc[0]), hi_b = lo_b;                                  // the box as cc has it
    if (BIASED) {
        unsigned lo_w = pk_minimum3(cc[0], cc[1], cc[2]), hi_w = pk_maximum3(cc[0], cc[1], cc[2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) {
            lo_w = pk_minimum3(lo_w, cc[i], cc[i + 1]);
            hi_w = pk_maximum3(hi_w, cc[i], cc[i + 1]);
        }
        lo_b = __builtin_bit_cast(pk_i16, pk_minimum3(lo_w, cc[15], cc[15]));                      // 1..256
        hi_b = __builtin_bit_cast(pk_i16, pk_maximum3(hi_w, cc[15], cc[15]));
    } else {
#pragma unroll
        for (int i = 1; i < 16; i++) {
            const pk_i16 v = __builtin_bit_cast(pk_i16, cc[i]);
            lo_b = __builtin_elementwise_min(lo_b, v);
            hi_b = __builtin_elementwise_max(hi_b, v);
        }
    }
    // covariance sign: sum (2 Co - mo)(2 Cg - mg) = 4 sum Co Cg - 2 mg sum Co - 2 mo sum Cg + 16 mo mg with mo = lo + hi
    // of Co, mg of Cg: per pixel one product-accumulate and one add of the pair, 32-bit where no half is negative,
    // packed otherwise.  (The same number whatever is added to every Co and every Cg: centred or biased, the values
    // stand for themselves.)
    int prod = 0;
    unsigned sum_w = 0;                                                                            // <= 4096 a half
    pk_i16 sum_pk = {0, 0};                                                                        // |.| <= 2048
#pragma unroll
    for (int i = 0; i < 16; i++) {
        int r;
        asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[0,1,0,0]" : "=v"(r) : "v"(cc[i]), "v"(prod));   // low half x high half + prod
        prod = r;
        if (BIASED)
            sum_w += cc[i];
        else
            sum_pk += __builtin_bit_cast(pk_i16, cc[i]);
    }
    const pk_i16 sums = BIASED ? __builtin_bit_cast(pk_i16, sum_w) : sum_pk;
    const pk_i16 mid = lo_b + hi_b;                                                                // mo | mg, 2..512 or -254..256
    // half the covariance: cov / 2 = 2 prod + mg (4 mo - sum Co) + mo (4 mg - sum Cg), the two products one dot product
    // of the pair of reduced sums (|.| <= 3072) and mg | mo, with 2 prod as its accumulator
    const pk_i16 rest = mid * (short)4 - sums;
    const int half_cov = __builtin_amdgcn_sdot2(rest, mid.yx, 2 * prod, false);
    // the box recentred, -127..128: what m, the scale, the scaled box and the inset are stated on
    const pk_i16 centre = {128, 128};
    const pk_i16 lo = BIASED ? lo_b - centre : lo_b, hi = BIASED ? hi_b - centre : hi_b;
    // m = max(-lo, hi) over both channels, 0..128; the scale s = 4, 2, 1 for m <= 31, <= 63, above as a shift count
    const pk_i16 mm = __builtin_elementwise_max((pk_i16)-lo, hi);
    const int m = max((int)mm.x, (int)mm.y);
    const unsigned sh = (unsigned)max(2 - (m >> 5), 0);
    const unsigned s1 = (1u << sh) - 1u;                                                           // s - 1: the blue field
    // the box scaled about the centre, (x - 128) s, and inset by a sixteenth of its extent
    pk_u16 ls = pk_shl(__builtin_bit_cast(pk_u16, lo), sh), hs = pk_shl(__builtin_bit_cast(pk_u16, hi), sh);
    const pk_u16 ins = (pk_u16)(hs - ls) >> 4;                                                     // extent 0..255: no sign
    ls += ins;
    hs -= ins;
    // the two ends: Co's upper end with Cg's upper or, under a negative covariance, lower end -- Cg's halves change
    // places under a mask made of the covariance's sign (two v_bfi)
    const unsigned cross = (unsigned)(half_cov >> 31) & 0xFFFF0000u, lsw = __builtin_bit_cast(unsigned, ls), hsw = __builtin_bit_cast(unsigned, hs);
    const pk_u16 end_a = __builtin_bit_cast(pk_u16, (lsw & cross) | (hsw & ~cross));
    const pk_u16 end_b = __builtin_bit_cast(pk_u16, (hsw & cross) | (lsw & ~cross));
    // quant5 | quant6 of the biased values from the centred ones: t = 31 (v + 128) + 128 | 63 (v + 128) + 128
    const pk_u16 q_mul = {31, 63}, q_add = {31 * 128 + 128, 63 * 128 + 128};
    const pk_u16 ta = end_a * q_mul + q_add, tb = end_b * q_mul + q_add;
    const pk_u16 pa = (pk_u16)(ta + (ta >> 8)) >> 8, pb = (pk_u16)(tb + (tb >> 8)) >> 8;           // qo | qg << 16
    // the 5:6:5 words qo << 11 | qg << 5 | s - 1: the two fields do not meet, so the sum of products is the word
    const pk_u16 q_place = {1 << 11, 1 << 5};
    const unsigned qa = __builtin_amdgcn_udot2(pa, q_place, s1, false), qb = __builtin_amdgcn_udot2(pb, q_place, s1, false);
    const unsigned c0 = max(qa, qb), c1 = min(qa, qb);
    unsigned idx = 0;
    if (c0 != c1) {
        // project4 on the scaled pixels v = (c - 128) s + 128 without forming them, and without complementing: with the
        // direction SIGNED per channel (16-bit pair, one v_dot2 on the packed Co | Cg pair) the projection of
        // make_projection(expand_565(c0), expand_565(c1)) is t = s (c . dir) + K: the 255 |dir| of project4's
        // complemented channels and make_projection's - 255 (sum of |dir| over those channels) cancel, which leaves
        // K = len2 / 6 + sum over the channels of dir (128 - 128 s - p1).  The end entries are expanded from the
        // quantised channels at hand, in c0 / c1 order, not unpacked from the 5:6:5 words again.
        // With the centred c' = c - 128, t = (c' . s dir) + K', K' = len2 / 6 + sum of dir (128 - p1): the scale rides in
        // the 16-bit direction (|s dir| <= 1020).  Where the pixels at hand are the biased c, the dot product's
        // accumulator is K = K' - 128 (s d_o + s d_g), |.| below 2^19, one dot product of s dir with -128 | -128 on top
        // of dir . (128 - p1); t is the definition's own, clamped and turned into a position as in project4.
        // On pairs: the quantised pairs in c0 / c1 order, expand5 | expand6 of both, dir and 128 - p1 one packed
        // subtraction each, len2 = dir . dir and K' = dir . (128 - p1) + len2 / 6 one dot product each, s dir one shift.
        const bool sw = qa < qb;                                                             // c0 is qb
        const pk_u16 q0 = sw ? pb : pa, q1 = sw ? pa : pb;
        const pk_u16 up = {3, 2}, down = {2, 4};
        const pk_u16 p0 = (q0 << up) | (q0 >> down), p1 = (q1 << up) | (q1 >> down);
        const pk_i16 dir = __builtin_bit_cast(pk_i16, (pk_u16)(p0 - p1)), back = __builtin_bit_cast(pk_i16, (pk_u16)(128 - p1));
        // The two dot products in one statement, in the three-operand form with the constant 0 (from the builtin the
        // compiler makes the form that accumulates into its destination, and pays a v_mov of the 0 for each), and with
        // their wait states by position: the scaled direction and two idle states behind the second, so that every
        // reader outside the statement, the compiler's or clamped_dot2's, is a safe one.  The BIASED form's third takes
        // the second's result as its accumulator, which a dot product of the same opcode may do without waiting, and
        // three idle states follow it.
        unsigned len2, dir2;                                                                 // len2: 16 .. 130050
        int dot_back;
        if (BIASED)
            asm("v_dot2_i32_i16 %[len2], %[d], %[d], 0\n\tv_dot2_i32_i16 %[k], %[d], %[b], 0\n\t"
                "v_pk_lshlrev_b16 %[d2], %[sh], %[d] op_sel_hi:[0,1]\n\t"
                "v_dot2_i32_i16 %[k], %[d2], %[uncentre], %[k]\n\ts_nop 2"
                : [len2] "=&v"(len2), [k] "=&v"(dot_back), [d2] "=&v"(dir2)
                : [d] "v"(dir), [b] "v"(back), [sh] "v"(sh), [uncentre] "s"(0xFF80FF80u));
        else
            asm("v_dot2_i32_i16 %[len2], %[d], %[d], 0\n\tv_dot2_i32_i16 %[k], %[d], %[b], 0\n\t"
                "v_pk_lshlrev_b16 %[d2], %[sh], %[d] op_sel_hi:[0,1]\n\ts_nop 1"
                : [len2] "=&v"(len2), [k] "=&v"(dot_back), [d2] "=&v"(dir2)
                : [d] "v"(dir), [b] "v"(back), [sh] "v"(sh));
        const int sixth = (int)(__umulhi(len2, 0xAAAAAAABu) >> 2);
        const unsigned m24 = index_scale(len2);
        const int K = dot_back + sixth, top = (int)len2 + sixth;
        idx = gather_indices(m24, [&](unsigned (&t)[4], int i) { clamped_dot2(t, cc[i], cc[i + 1], cc[i + 2], cc[i + 3], dir2, K, top); });
    }
    return make_uint2(c0 | (c1 << 16), idx);
}

// The same colour half with the box taken apart into four ints and every step once per value: the form the Hap Q Alpha
// kernels keep (block_of<kFmtYCoCg, false>).  They run at eight waves and are not bound by instruction issue; with the
// pair form's fewer but longer-chained instructions their block kernel measured 1.3 - 3.6 % SLOWER (LABNOTES, Part R11),
// so their code stays what it was.  The same bytes either way (tests/test_packed_endpoints_identity.py).
__device__ __forceinline__ uint2 ycocg_colour_block_scalar(const unsigned (&cc)[16])
{
    pk_i16 lo = __builtin_bit_cast(pk_i16, cc[0]), hi = lo;
#pragma unroll
    for (int i = 1; i < 16; i++) {
        const pk_i16 v = __builtin_bit_cast(pk_i16, cc[i]);
        lo = __builtin_elementwise_min(lo, v);
        hi = __builtin_elementwise_max(hi, v);
    }
    int lo_o = lo.x, hi_o = hi.x, lo_g = lo.y, hi_g = hi.y;
    const int m = max(max(-lo_o, hi_o), max(-lo_g, hi_g));
    const int s = m <= 31 ? 4 : (m <= 63 ? 2 : 1);
    // covariance sign, as in ycocg_colour_block
    int prod = 0;
    pk_i16 sums = {0, 0};                                                                          // |.| <= 2048
#pragma unroll
    for (int i = 0; i < 16; i++) {
        int r;
        asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[0,1,0,0]" : "=v"(r) : "v"(cc[i]), "v"(prod));   // low half x high half + prod
        prod = r;
        sums += __builtin_bit_cast(pk_i16, cc[i]);
    }
    const int mo = lo_o + hi_o, mg = lo_g + hi_g;
    const int cov = 4 * prod - 2 * mg * (int)sums.x - 2 * mo * (int)sums.y + 16 * mo * mg;
    // the box scaled about the centre and biased: (x - 128) s + 128 from x - 128
    lo_o = lo_o * s + 128; hi_o = hi_o * s + 128;
    lo_g = lo_g * s + 128; hi_g = hi_g * s + 128;
    int ins = (hi_o - lo_o) >> 4; lo_o += ins; hi_o -= ins;
    ins = (hi_g - lo_g) >> 4; lo_g += ins; hi_g -= ins;
    const int ag = cov < 0 ? lo_g : hi_g, bg = cov < 0 ? hi_g : lo_g;
    const int qo_a = quant5(hi_o), qo_b = quant5(lo_o), qg_a = quant6(ag), qg_b = quant6(bg);
    const unsigned qa = (unsigned)(qo_a << 11 | qg_a << 5 | (s - 1));
    const unsigned qb = (unsigned)(qo_b << 11 | qg_b << 5 | (s - 1));
    const unsigned c0 = max(qa, qb), c1 = min(qa, qb);
    unsigned idx = 0;
    if (c0 != c1) {
        // t = (c' . s dir) + K', K' = len2 / 6 + sum of dir (128 - p1), as in ycocg_colour_block, per channel
        const bool sw = qa < qb;                                                             // c0 is qb
        const int eo_a = expand5(qo_a), eo_b = expand5(qo_b), eg_a = expand6(qg_a), eg_b = expand6(qg_b);
        const int d_o = sw ? eo_b - eo_a : eo_a - eo_b, d_g = sw ? eg_b - eg_a : eg_a - eg_b;
        const int p1_o = sw ? eo_a : eo_b, p1_g = sw ? eg_a : eg_b;
        const unsigned len2 = (unsigned)mad24(d_o, d_o, __mul24(d_g, d_g));                  // 16 .. 130050
        const int sixth = (int)(__umulhi(len2, 0xAAAAAAABu) >> 2);
        const unsigned m24 = index_scale(len2);
        const int K = mad24(d_o, 128 - p1_o, mad24(d_g, 128 - p1_g, sixth));
        const unsigned dir2 = ((unsigned)(d_o * s) & 0xFFFFu) | ((unsigned)(d_g * s) << 16);
        const int top = (int)len2 + sixth;
        idx = gather_indices(m24, [&](unsigned (&t)[4], int i) { clamped_dot2(t, cc[i], cc[i + 1], cc[i + 2], cc[i + 3], dir2, K, top); });
    }
    return make_uint2(c0 | (c1 << 16), idx);
}

// ---- the YCoCg transform as one 4x4x4 signed-byte matrix product a pixel (v_mfma_i32_4x4x4_16b_i8) ----
// The instruction makes sixteen independent products D = A B + C, one per group of four lanes: lane l supplies row l & 3
// of A and column l & 3 of B (four signed bytes each, k = byte index) and gets column l & 3 of D in four registers
// (tools/micro/mfma_beside_valu.hip prints the layout).  B's column is the lane's own pixel less 128 a channel
// (p ^ 0x80808080 as signed bytes R', G', B', A'), the rows of A are weights, C is the inline constant 2:
//     row 0:  1,  2,  1, 0  ->  R + 2G + B + 2 - 512          >> 2 = Y - 128   (512 is a whole multiple of the divisor)
//     row 1:  2,  0, -2, 0  ->  2 (R - B + 1)                 >> 2 = (R - B + 1) >> 1 = Co - 128
//     row 2: -1,  2, -1, 0  ->  -R + 2G - B + 2               >> 2 = Cg - 128
//     row 3:  0                                                    (spare)
// (the 128s of rows 1 and 2 cancel: their weights sum to zero; Co's row is doubled so that one constant serves all
// three).  Per pixel: v_xor, the matrix instruction, v_ashrrev (Y), v_perm_b32 + v_pk_ashrrev_i16 (Co | Cg << 16, signed
// halves) -- four vector instructions and one on the matrix pipe, where the dot-product form has seven.
// BIASED: C is a register tuple instead, one addend a row (ycocg_addend(): 32576, 2 + 512, 2 + 512, 0 in every lane), so
// rows 1 and 2 come out 512 higher and the same v_perm_b32 + v_pk_ashrrev_i16 deliver Co | Cg << 16 as the definition's
// own values, 1..256 a half, which is what ycocg_colour_block<true>'s pixel loops want; row 0 has weights of its own
// (ycocg_weight_rows_biased()) and delivers 256 (255 - Y) + junk below 256, one v_and_b32 where the v_ashrrev_i32 stands,
// which is what luma_block_negated() takes.  The same instructions a pixel; the tuple's four registers are the price.
//
// The matrix instruction READS all 64 lanes whatever EXEC says (it writes the active ones only): a lane's result needs
// the weight dwords of lanes 0..2 of its group whether or not those run.  So the weight register is made ONCE, at the
// kernel's entry with every lane active, by ycocg_weight_rows(), and handed down to block_of: its value is opaque to
// the optimiser (a volatile asm move), which therefore cannot make it again inside a divergent region.
typedef int mfma_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned ycocg_weight_rows()
{
    const unsigned row = threadIdx.x & 3u;
    const unsigned w = row == 0u ? 0x00010201u : (row == 1u ? 0x00FE0002u : (row == 2u ? 0x00FF02FFu : 0u));
    unsigned r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(w));
    return r;
}

// The BIASED form's weights: rows 1 and 2 as above, row 0 NEGATED and scaled by 64, -64, -128, -64, 0 (+128 is no signed
// byte; -128 is).  With S = R + 2G + B + 2 = 4 Y + f the row makes -64 (S - 2 - 512), and its addend 32576 brings that to
//     65472 - 64 S  =  256 (255 - Y) + 64 (3 - f):
// a non-negative 16-bit number whose byte 1 is 255 - Y exactly and whose byte 0 (0, 64, 128 or 192) is dropped by one
// v_and_b32 where the centred form has its v_ashrrev_i32 -- luma in the form luma_block_negated() takes.
__device__ __forceinline__ unsigned ycocg_weight_rows_biased()
{
    const unsigned row = threadIdx.x & 3u;
    const unsigned w = row == 0u ? 0x00C080C0u : (row == 1u ? 0x00FE0002u : (row == 2u ? 0x00FF02FFu : 0u));
    unsigned r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(w));
    return r;
}

// The BIASED form's addend tuple, made beside the weights at the kernel's entry and handed down with them: a value the
// optimiser cannot see through is one it cannot make again, register by register, between two matrix instructions.
__device__ __forceinline__ mfma_i32x4 ycocg_addend()
{
    mfma_i32x4 c = {32576, 2 + 512, 2 + 512, 0};
    asm volatile("" : "+v"(c));
    return c;
}

// Two pixels a statement, software-pipelined by one statement: the statement reads the results of the two pixels
// BEFORE its own, then issues its own two matrix instructions.  The compiler sees neither the instruction nor its
// hazards, so both stand here by position: two wait states between the v_xor that writes B and the matrix instruction
// that reads it, five between a matrix instruction and the first reader of its result (the ISA's MAI hazard table for
// a two-pass instruction; what the compiler pads the builtin with).  Every statement ENDS five states behind its last
// matrix instruction, so whatever the compiler puts between two statements (a copy of a result included) is safe too.
// Every reader of the old results stands IN FRONT of the new matrix instructions, and the new results are tied to the
// old ones' registers: two tuples live instead of four.  Every other output is early-clobber: the matrix
// instructions read the weights last, and an output that may share a register with an input could take THEIRS where
// the statement is their last use.  (BIASED: the addend tuple in place of the inline constant, nothing else.)
#define HAPBC_YCOCG_MFMA "v_mfma_i32_4x4x4_16b_i8 "
#define HAPBC_YCOCG_SHIFT(CC) "v_pk_ashrrev_i16 " CC ", 2, " CC " op_sel_hi:[0,1]\n\t"
// first statement of a block: nothing to read yet
template <bool BIASED>
__device__ __forceinline__ void ycocg_pair_first(mfma_i32x4 &ta, mfma_i32x4 &tb, unsigned pa, unsigned pb, unsigned rows, const mfma_i32x4 &addend)
{
    unsigned qa, qb;
    if (BIASED)
        asm("v_xor_b32 %[qa], %[k80], %[pa]\n\tv_xor_b32 %[qb], %[k80], %[pb]\n\ts_nop 0\n\t"
            HAPBC_YCOCG_MFMA "%[ta], %[w], %[qa], %[c]\n\t" HAPBC_YCOCG_MFMA "%[tb], %[w], %[qb], %[c]\n\ts_nop 4"
            : [ta] "=&v"(ta), [tb] "=&v"(tb), [qa] "=&v"(qa), [qb] "=&v"(qb)
            : [pa] "v"(pa), [pb] "v"(pb), [w] "v"(rows), [c] "v"(addend), [k80] "s"(0x80808080u));
    else
        asm("v_xor_b32 %[qa], %[k80], %[pa]\n\tv_xor_b32 %[qb], %[k80], %[pb]\n\ts_nop 0\n\t"
            HAPBC_YCOCG_MFMA "%[ta], %[w], %[qa], 2\n\t" HAPBC_YCOCG_MFMA "%[tb], %[w], %[qb], 2\n\ts_nop 4"
            : [ta] "=&v"(ta), [tb] "=&v"(tb), [qa] "=&v"(qa), [qb] "=&v"(qb)
            : [pa] "v"(pa), [pb] "v"(pb), [w] "v"(rows), [k80] "s"(0x80808080u));
}
// pixels pa, pb in, their results to ta, tb; Y - 128 (BIASED: 256 (255 - Y)) and Co | Cg << 16 (centred or BIASED) of
// the two pixels whose results ta, tb held before out
template <bool BIASED>
__device__ __forceinline__ void ycocg_pair(mfma_i32x4 &ta, mfma_i32x4 &tb, int &ya, int &yb, unsigned &cca, unsigned &ccb,
                                           unsigned pa, unsigned pb, unsigned rows, const mfma_i32x4 &addend)
{
    const mfma_i32x4 oa = ta, ob = tb;
    unsigned qa, qb;
    if (BIASED)
        asm("v_xor_b32 %[qa], %[k80], %[pa]\n\tv_xor_b32 %[qb], %[k80], %[pb]\n\t"
            "v_and_b32 %[ya], %[kff], %[oax]\n\tv_and_b32 %[yb], %[kff], %[obx]\n\t"
            "v_perm_b32 %[ca], %[oaz], %[oay], %[sel]\n\tv_perm_b32 %[cb], %[obz], %[oby], %[sel]\n\t"
            HAPBC_YCOCG_SHIFT("%[ca]")
            HAPBC_YCOCG_MFMA "%[ta], %[w], %[qa], %[c]\n\t" HAPBC_YCOCG_MFMA "%[tb], %[w], %[qb], %[c]\n\t"
            HAPBC_YCOCG_SHIFT("%[cb]") "s_nop 3"
            : [ta] "+v"(ta), [tb] "+v"(tb), [ya] "=&v"(ya), [yb] "=&v"(yb), [ca] "=&v"(cca), [cb] "=&v"(ccb), [qa] "=&v"(qa), [qb] "=&v"(qb)
            : [pa] "v"(pa), [pb] "v"(pb), [w] "v"(rows), [c] "v"(addend), [k80] "s"(0x80808080u), [kff] "s"(0xFF00u), [sel] "s"(0x05040100),
              [oax] "v"(oa.x), [oay] "v"(oa.y), [oaz] "v"(oa.z), [obx] "v"(ob.x), [oby] "v"(ob.y), [obz] "v"(ob.z));
    else
        asm("v_xor_b32 %[qa], %[k80], %[pa]\n\tv_xor_b32 %[qb], %[k80], %[pb]\n\t"
            "v_ashrrev_i32 %[ya], 2, %[oax]\n\tv_ashrrev_i32 %[yb], 2, %[obx]\n\t"
            "v_perm_b32 %[ca], %[oaz], %[oay], %[sel]\n\tv_perm_b32 %[cb], %[obz], %[oby], %[sel]\n\t"
            HAPBC_YCOCG_SHIFT("%[ca]")
            HAPBC_YCOCG_MFMA "%[ta], %[w], %[qa], 2\n\t" HAPBC_YCOCG_MFMA "%[tb], %[w], %[qb], 2\n\t"
            HAPBC_YCOCG_SHIFT("%[cb]") "s_nop 3"
            : [ta] "+v"(ta), [tb] "+v"(tb), [ya] "=&v"(ya), [yb] "=&v"(yb), [ca] "=&v"(cca), [cb] "=&v"(ccb), [qa] "=&v"(qa), [qb] "=&v"(qb)
            : [pa] "v"(pa), [pb] "v"(pb), [w] "v"(rows), [k80] "s"(0x80808080u), [sel] "s"(0x05040100),
              [oax] "v"(oa.x), [oay] "v"(oa.y), [oaz] "v"(oa.z), [obx] "v"(ob.x), [oby] "v"(ob.y), [obz] "v"(ob.z));
}
// last statement of a block: the readers alone
template <bool BIASED>
__device__ __forceinline__ void ycocg_pair_last(int &ya, int &yb, unsigned &cca, unsigned &ccb, mfma_i32x4 oa, mfma_i32x4 ob)
{
    if (BIASED)
        asm("v_and_b32 %[ya], %[kff], %[oax]\n\tv_and_b32 %[yb], %[kff], %[obx]\n\t"
            "v_perm_b32 %[ca], %[oaz], %[oay], %[sel]\n\tv_perm_b32 %[cb], %[obz], %[oby], %[sel]\n\t"
            HAPBC_YCOCG_SHIFT("%[ca]") "v_pk_ashrrev_i16 %[cb], 2, %[cb] op_sel_hi:[0,1]"
            : [ya] "=&v"(ya), [yb] "=&v"(yb), [ca] "=&v"(cca), [cb] "=&v"(ccb)
            : [sel] "s"(0x05040100), [kff] "s"(0xFF00u), [oax] "v"(oa.x), [oay] "v"(oa.y), [oaz] "v"(oa.z), [obx] "v"(ob.x), [oby] "v"(ob.y), [obz] "v"(ob.z));
    else
    asm("v_ashrrev_i32 %[ya], 2, %[oax]\n\tv_ashrrev_i32 %[yb], 2, %[obx]\n\t"
        "v_perm_b32 %[ca], %[oaz], %[oay], %[sel]\n\tv_perm_b32 %[cb], %[obz], %[oby], %[sel]\n\t"
        HAPBC_YCOCG_SHIFT("%[ca]") "v_pk_ashrrev_i16 %[cb], 2, %[cb] op_sel_hi:[0,1]"
        : [ya] "=&v"(ya), [yb] "=&v"(yb), [ca] "=&v"(cca), [cb] "=&v"(ccb)
        : [sel] "s"(0x05040100), [oax] "v"(oa.x), [oay] "v"(oa.y), [oaz] "v"(oa.z), [obx] "v"(ob.x), [oby] "v"(ob.y), [obz] "v"(ob.z));
}
#undef HAPBC_YCOCG_SHIFT
#undef HAPBC_YCOCG_MFMA

// The dot-product form of the transform (block_of<FMT, false>: the kernels that would lose a wave to the matrix form's
// result tuples, the Hap Q Alpha ones).  2 (Co - 128) | 4 (Cg - 128) << 16 of four pixels, signed halves, from the
// pixels' bytes less 128 (q ^ 0x80808080, signed bytes): R - B + 1 and -R + 2G - B + 2 are SIGNED byte dot products, the 128s cancel since each set of weights sums to
// zero, and one v_perm_b32 puts the low halves side by side.  In one statement because the compiler makes v_dot4c of
// the builtin -- it accumulates into its destination and pays a v_mov of the constant per dot product -- and, not
// seeing into a statement, would not keep a dot product's three wait states in front of the v_perm: here at least
// three instructions stand between every dot product and the reader of its result.
__device__ __forceinline__ void chroma4(unsigned (&raw)[4], int q0, int q1, int q2, int q3)
{
    unsigned co[4];
    asm("v_dot4_i32_i8 %4, %8, %12, 1\n\tv_dot4_i32_i8 %0, %8, %13, 2\n\t"
        "v_dot4_i32_i8 %5, %9, %12, 1\n\tv_dot4_i32_i8 %1, %9, %13, 2\n\t"
        "v_dot4_i32_i8 %6, %10, %12, 1\n\tv_dot4_i32_i8 %2, %10, %13, 2\n\t"
        "v_dot4_i32_i8 %7, %11, %12, 1\n\tv_dot4_i32_i8 %3, %11, %13, 2\n\t"
        "v_perm_b32 %0, %0, %4, %14\n\tv_perm_b32 %1, %1, %5, %14\n\tv_perm_b32 %2, %2, %6, %14\n\tv_perm_b32 %3, %3, %7, %14"
        : "=&v"(raw[0]), "=&v"(raw[1]), "=&v"(raw[2]), "=&v"(raw[3]), "=&v"(co[0]), "=&v"(co[1]), "=&v"(co[2]), "=&v"(co[3])
        : "v"(q0), "v"(q1), "v"(q2), "v"(q3), "s"(0x00FF0001), "s"(0x00FF02FF), "s"(0x05040100));
}

// the 8 or 16 bytes of a block from its sixteen RGBA8 pixels (row-major); 8-byte formats leave z, w zero
// (MATRIX: the Hap Q destinations -- the YCoCg transform on the matrix pipe, `rows` the kernel's ycocg_weight_rows(),
// and the colour half on Co | Cg pairs -- BIASED: non-negative pairs, `addend` the kernel's ycocg_addend(); without MATRIX, Hap Q Alpha, the dot-product transform and the scalar colour half.  The
// same bytes either way.  REFINE, DXT1 and DXT5 only: the colour block with refined end points, colour_block<true>)
template <int FMT, bool MATRIX = false, bool BIASED = false, bool REFINE = false>
__device__ __forceinline__ uint4 block_of(const unsigned (&p)[16], unsigned rows = 0u, const mfma_i32x4 &addend = mfma_i32x4{})
{
    static_assert(!REFINE || FMT == kFmtDXT1 || FMT == kFmtDXT5, "refined end points: the S3TC colour block only");
    if (FMT == kFmtRGTC1) {
        int a[16];
#pragma unroll
        for (int i = 0; i < 16; i++)
            a[i] = (int)(p[i] >> 24);
        const uint2 ab = alpha_block(a);
        return make_uint4(ab.x, ab.y, 0u, 0u);
    } else if (FMT == kFmtDXT1) {
        unsigned px[16];
#pragma unroll
        for (int i = 0; i < 16; i++)
            px[i] = p[i] & 0x00FFFFFFu;
        const uint2 cb = colour_block<REFINE>(px);
        return make_uint4(cb.x, cb.y, 0u, 0u);
    } else if (FMT == kFmtDXT5) {
        int a[16];
        unsigned px[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            a[i] = (int)(p[i] >> 24);
            px[i] = p[i] & 0x00FFFFFFu;
        }
        const uint2 ab = alpha_block(a), cb = colour_block<REFINE>(px);
        return make_uint4(ab.x, ab.y, cb.x, cb.y);
    } else {
        // Y = (R+2G+B+2)>>2 ; Co = ((R-B+1)>>1)+128 ; Cg = ((-R+2G-B+2)>>2)+128 ; no clamp (oracle/bc_oracle.c).  Y
        // leaves here less 128 (from the BIASED matrix form as 256 (255 - Y)); Co and Cg as they are from the BIASED
        // matrix form, less 128 otherwise.
        int y[16];
        unsigned cc[16];
        if (MATRIX) {
            mfma_i32x4 ta, tb;
            ycocg_pair_first<BIASED>(ta, tb, p[0], p[1], rows, addend);
#pragma unroll
            for (int i = 2; i < 16; i += 2)
                ycocg_pair<BIASED>(ta, tb, y[i - 2], y[i - 1], cc[i - 2], cc[i - 1], p[i], p[i + 1], rows, addend);
            ycocg_pair_last<BIASED>(y[14], y[15], cc[14], cc[15], ta, tb);
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                // Y's dot product starts at 2 - 512 (wrap-around; a whole multiple of the divisor, so the arithmetic shift
                // gives exactly Y - 128), the other two are the definitions' own numerators, halved / quartered as a pair
                // of signed halves.
                y[i] = (int)__builtin_amdgcn_udot4(p[i], 0x00010201u, (unsigned)(2 - 512), false) >> 2;                   // -128 .. 127
            }
#pragma unroll
            for (int i = 0; i < 16; i += 4) {
                unsigned raw[4];
                chroma4(raw, (int)(p[i] ^ 0x80808080u), (int)(p[i + 1] ^ 0x80808080u), (int)(p[i + 2] ^ 0x80808080u), (int)(p[i + 3] ^ 0x80808080u));
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const pk_i16 sh = {1, 2};
                    cc[i + k] = __builtin_bit_cast(unsigned, (pk_i16)(__builtin_bit_cast(pk_i16, raw[k]) >> sh));         // -127 .. 128 each
                }
            }
        }
        // (BIASED: y holds 256 (255 - Y), non-negative, and the luma half takes it as that)
        const uint2 ab = (MATRIX && BIASED) ? luma_block_negated(reinterpret_cast<const unsigned (&)[16]>(y)) : alpha_block<128>(y);
        const uint2 cb = MATRIX ? ycocg_colour_block<BIASED>(cc) : ycocg_colour_block_scalar(cc);
        return make_uint4(ab.x, ab.y, cb.x, cb.y);
    }
}

} // namespace hapbc
