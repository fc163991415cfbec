// bc_refine_core.hpp -- the per-block arithmetic of HAPGPU_ENCODE_REFINE_ENDPOINTS (include/hap_gpu.h states the
// definition, tests/_refined_endpoints.py restates it in numpy): least-squares refinement of the two end points of an
// S3TC colour block for the indices the block has.  A round takes the block's indices and pixels and makes a
// candidate pair of 5:6:5 words; the caller (bc_encode_core.hpp, colour_block<true>) gives the candidate its indices
// with the encoder's own projection and keeps it where its squared error is strictly smaller.
//
// Everything here is __host__ __device__ and free of inline assembly: tests/c/refine_endpoints_host.hip compiles this
// file for the host and tests/test_refined_endpoints.py holds it against the numpy definition.  Where the device has
// a faster form of the same integers (24-bit multiplies, the byte dot product, v_rcp_f32) it stands behind
// __HIP_DEVICE_COMPILE__ in one of the four small helpers below and nowhere else.
//
// Pixels are packed bytes R | G << 8 | B << 16 with the top byte zero, indices sixteen 2-bit fields, pixel 0 lowest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hapbc {

#define HAPBC_HD __host__ __device__ __forceinline__

// a * b, both below 2^24 (v_mul_u32_u24: full rate, the 32-bit multiplier is quarter rate)
HAPBC_HD unsigned refine_mul(unsigned a, unsigned b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// sum of the products of the four bytes of a and of b, + acc (v_dot4_u32_u8; its result is read by the compiler's own
// instructions only, which the compiler separates from it as gfx950 wants -- never by an inline-asm statement)
HAPBC_HD unsigned refine_dot4(unsigned a, unsigned b, unsigned acc)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int k = 0; k < 4; k++)
        acc += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
    return acc;
#endif
}

HAPBC_HD int refine_popcount(unsigned v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// an approximation of 1 / d, good to a few units in the last place: refine_quotient corrects what it makes of it
HAPBC_HD float refine_reciprocal(float d)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_rcpf(d);
#else
    return 1.0f / d;
#endif
}

HAPBC_HD int refine_quant5(int v) { const int t = v * 31 + 128; return (t + (t >> 8)) >> 8; }
HAPBC_HD int refine_quant6(int v) { const int t = v * 63 + 128; return (t + (t >> 8)) >> 8; }

// the palette entry of a 5:6:5 word, packed bytes
HAPBC_HD unsigned refine_expand_565(unsigned c)
{
    const unsigned r = c >> 11, g = (c >> 5) & 63u, b = c & 31u;
    return ((r << 3) | (r >> 2)) | (((g << 2) | (g >> 4)) << 8) | (((b << 3) | (b >> 2)) << 16);
}

// The four palette entries by index, as oracle/bc_oracle.c:decode_colour builds them with c0 > c1: expand(c0),
// expand(c1), (2 p0 + p1) / 3, (p0 + 2 p1) / 3, floor.  (x * 683 >> 11 is x / 3 for x < 2048; here x <= 765.)
struct refine_palette {
    unsigned entry[4];
};

HAPBC_HD refine_palette refine_make_palette(unsigned c0, unsigned c1)
{
    refine_palette p;
    p.entry[0] = refine_expand_565(c0);
    p.entry[1] = refine_expand_565(c1);
    p.entry[2] = p.entry[3] = 0u;
    for (int c = 0; c < 3; c++) {
        const unsigned a = (p.entry[0] >> (8 * c)) & 255u, b = (p.entry[1] >> (8 * c)) & 255u;
        p.entry[2] |= (refine_mul(2u * a + b, 683u) >> 11) << (8 * c);
        p.entry[3] |= (refine_mul(a + 2u * b, 683u) >> 11) << (8 * c);
    }
    return p;
}

// The weights of sixteen indices, again sixteen 2-bit fields: w = {3, 0, 2, 1}[index], the thirds of entry 0 in the
// entry.  High bit = ~index.low, low bit = ~(index.high ^ index.low).
HAPBC_HD unsigned refine_weights(unsigned idx)
{
    return ((~idx << 1) & 0xAAAAAAAAu) | (~(idx ^ (idx >> 1)) & 0x55555555u);
}

// A = sum w^2, B = sum w v, C = sum v^2 (v = 3 - w), det = A C - B^2: from how many pixels hold each weight
struct refine_moments {
    int A, B, C, det;
};

HAPBC_HD refine_moments refine_make_moments(unsigned weights)
{
    const unsigned hi = (weights >> 1) & 0x55555555u, lo = weights & 0x55555555u;
    const int m3 = refine_popcount(hi & lo), m2 = refine_popcount(hi & ~lo), m1 = refine_popcount(~hi & lo);
    const int sum_w = m1 + 2 * m2 + 3 * m3;                        // <= 48
    refine_moments m;
    m.A = m1 + 4 * m2 + 9 * m3;                                    // <= 144
    m.B = 3 * sum_w - m.A;                                         // sum w (3 - w) <= 32
    m.C = 144 - 6 * sum_w + m.A;                                   // sum (3 - w)^2 <= 144
    m.det = m.A * m.C - m.B * m.B;                                 // 0 .. 20736
    return m;
}

// Per-channel sums of the pixels times per-pixel factors: R and B side by side in the two 16-bit halves of one word
// (px & 0x00FF00FF; sixteen bytes times at most 3 stay below 12241 a half), G in a word of its own.
struct refine_sums {
    unsigned rb, g;
};

HAPBC_HD refine_sums refine_plain_sums(const unsigned (&px)[16])
{
    refine_sums s = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        s.rb += px[i] & 0x00FF00FFu;
        s.g += (px[i] >> 8) & 255u;
    }
    return s;
}

// P = sum w x: one 24-bit multiply-add on the R | B halves and one on G a pixel
HAPBC_HD refine_sums refine_weighted_sums(const unsigned (&px)[16], unsigned weights)
{
    refine_sums s = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const unsigned w = (weights >> (2 * i)) & 3u;
        s.rb = refine_mul(w, px[i] & 0x00FF00FFu) + s.rb;
        s.g = refine_mul(w, (px[i] >> 8) & 255u) + s.g;
    }
    return s;
}

// clamp((2 * 3 * num + det) div (2 det), 0, 255), det > 0: the least-squares end point 3 num / det rounded to nearest.
// |6 num + det| < 2^24 (C <= 144, P <= 12240, det <= 20736), so the numerator is exact as a float; the product with
// the reciprocal is within one of the quotient wherever the quotient is small enough to matter (an estimate of 256 or
// more stands for a quotient of at least 255), and the integer remainder puts that one right.
HAPBC_HD int refine_quotient(int num, int det)
{
    const int n = 6 * num + det, d = 2 * det;
    if (n <= 0)
        return 0;
    unsigned q = (unsigned)((float)n * refine_reciprocal((float)d));          // < 2^24
    q = q < 256u ? q : 256u;
    const int rem = n - (int)refine_mul(q, (unsigned)d);                       // d <= 41472, q <= 256
    q += (rem >= d ? 1u : 0u) - (rem < 0 ? 1u : 0u);
    return (int)(q < 255u ? q : 255u);
}

// A round's candidate: the 5:6:5 words of the least-squares end points for these weights.  False where det == 0 (every
// pixel on one entry): the round then has no candidate.  plain: refine_plain_sums of the block, the same in every round.
HAPBC_HD bool refine_candidate(const unsigned (&px)[16], const refine_sums &plain, unsigned weights, unsigned &c0, unsigned &c1)
{
    const refine_moments m = refine_make_moments(weights);
    const refine_sums p = refine_weighted_sums(px, weights);
    const bool valid = m.det != 0;
    const int det = valid ? m.det : 1;
    int a[3], b[3];
    for (int c = 0; c < 3; c++) {
        // c = 0, 2: the halves of the R | B word; c = 1: G
        const unsigned P = c == 1 ? p.g : (p.rb >> (8 * c)) & 0xFFFFu;
        const unsigned S = c == 1 ? plain.g : (plain.rb >> (8 * c)) & 0xFFFFu;
        const unsigned Q = 3u * S - P;                                                    // sum v x
        a[c] = refine_quotient((int)refine_mul((unsigned)m.C, P) - (int)refine_mul((unsigned)m.B, Q), det);
        b[c] = refine_quotient((int)refine_mul((unsigned)m.A, Q) - (int)refine_mul((unsigned)m.B, P), det);
    }
    const unsigned qa = (unsigned)(refine_quant5(a[0]) << 11 | refine_quant6(a[1]) << 5 | refine_quant5(a[2]));
    const unsigned qb = (unsigned)(refine_quant5(b[0]) << 11 | refine_quant6(b[1]) << 5 | refine_quant5(b[2]));
    c0 = qa > qb ? qa : qb;
    c1 = qa > qb ? qb : qa;
    return valid;
}

// What blocks are ranked by: sum over the pixels of |pal[index]|^2 - 2 px . pal[index], the block's squared error less
// the block's constant sum |px|^2.  The squares from how many pixels hold each index, the products one byte dot product
// of pixel and chosen entry a pixel, chained through the accumulator; the entry is chosen by the index's two bits, three
// selects a pixel (written as masks and bitwise selects the compiler turns them back into compares).  |.| < 2^23.
HAPBC_HD int refine_rank(const unsigned (&px)[16], const refine_palette &pal, unsigned idx)
{
    const unsigned hi = (idx >> 1) & 0x55555555u, lo = idx & 0x55555555u;
    const int n3 = refine_popcount(hi & lo), n2 = refine_popcount(hi & ~lo), n1 = refine_popcount(~hi & lo);
    const unsigned count[4] = {(unsigned)(16 - n1 - n2 - n3), (unsigned)n1, (unsigned)n2, (unsigned)n3};
    unsigned squares = 0u, products = 0u;
    for (int k = 0; k < 4; k++)
        squares += refine_mul(count[k], refine_dot4(pal.entry[k], pal.entry[k], 0u));
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const bool low = (idx >> (2 * i)) & 1u, high = (idx >> (2 * i + 1)) & 1u;
        const unsigned even = high ? pal.entry[2] : pal.entry[0], odd = high ? pal.entry[3] : pal.entry[1];
        products = refine_dot4(px[i], low ? odd : even, products);
    }
    return (int)squares - 2 * (int)products;
}

} // namespace hapbc
