// bc_decode_texels.hpp -- the texels of DXT1 / DXT5 / scaled YCoCg-DXT5 blocks (+ RGTC1 alpha plane): the per-lane
// bodies of the decode kernels, at full size (bc_decode_body) and as the rounded box means of 2x2 / 4x4 texels
// (bc_decode_scaled_body).  bc_decode.hip runs them from memory to pictures; bc_transcode.hip runs the same bodies from
// registers to registers (IN_REGISTERS) and hands the texels to the block encoder.  Arithmetic follows
// oracle/bc_oracle.c (obc_decode_*) exactly; results are bit-identical.
// (One level below hapbc: bc_encode_core.hpp has an expand5 / expand6 of its own there, and bc_transcode.hip sees both.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_core.hpp"

namespace hapbc {
namespace texels {

__device__ __forceinline__ int expand5(int q) { return (q << 3) | (q >> 2); }
__device__ __forceinline__ int expand6(int q) { return (q << 2) | (q >> 4); }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

typedef short pk_i16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pk_i16 as_pk(unsigned v) { return __builtin_bit_cast(pk_i16, v); }
__device__ __forceinline__ unsigned as_u32(pk_i16 v) { return __builtin_bit_cast(unsigned, v); }

// per-channel palettes, one byte per entry: pal[c] = entry0 | entry1<<8 | entry2<<16 | entry3<<24
__device__ __forceinline__ void decode_palette(uint2 blk, bool dxt1_modes, unsigned (&pal)[3])
{
    const unsigned c0 = blk.x & 0xFFFFu, c1 = blk.x >> 16;
    const int e0[3] = {expand5(c0 >> 11), expand6((c0 >> 5) & 63), expand5(c0 & 31)};
    const int e1[3] = {expand5(c1 >> 11), expand6((c1 >> 5) & 63), expand5(c1 & 31)};
    const bool four = !dxt1_modes || c0 > c1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // (/ 3 as one full-rate 24-bit multiply: exact below 32768)
        const int e2 = four ? (int)(__umul24((unsigned)(2 * e0[c] + e1[c]), 21846u) >> 16) : (e0[c] + e1[c]) / 2;
        const int e3 = four ? (int)(__umul24((unsigned)(e0[c] + 2 * e1[c]), 21846u) >> 16) : 0;
        pal[c] = (unsigned)e0[c] | ((unsigned)e1[c] << 8) | ((unsigned)e2 << 16) | ((unsigned)e3 << 24);
    }
}

// Hap Q: undo the per-block chroma scaling once per palette entry (4x) instead of once per pixel:
// pal[0]/pal[1] become (Co/s)+128 and (Cg/s)+128 (division truncating toward zero)
__device__ __forceinline__ void ycocg_unscale(unsigned (&pal)[3])
{
    unsigned co4 = 0, cg4 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = (int)(((pal[2] >> (8 * k)) & 255u) >> 3) + 1;               // 1..32
        int co = (int)((pal[0] >> (8 * k)) & 255u) - 128, cg = (int)((pal[1] >> (8 * k)) & 255u) - 128;
        // |x| / s for |x| <= 128 by a 16-bit reciprocal: floor(65536 / s) + 1 from v_rcp_f32 is exact here (the
        // quotient is an integer for powers of two, else at least 1/31 away from one), and so is the product's
        // top half for |x| < 516
        const unsigned m = (unsigned)(65536.0f * __builtin_amdgcn_rcpf((float)s)) + 1u;
        const int qo = (int)(__umul24((unsigned)abs(co), m) >> 16), qg = (int)(__umul24((unsigned)abs(cg), m) >> 16);
        co = co >= 0 ? qo : -qo;
        cg = cg >= 0 ? qg : -qg;
        co4 |= (unsigned)(co + 128) << (8 * k);
        cg4 |= (unsigned)(cg + 128) << (8 * k);
    }
    pal[0] = co4;
    pal[1] = cg4;
}

// Hap Q, two pixels per instruction (packed 16-bit): R = Y + (Co - Cg), G = Y + Cg, B = Y - Co - Cg with the three
// offsets worked out once per palette entry (4) instead of once per pixel (16), as tables of four 16-bit values
struct ycocg_offsets {
    unsigned tr01, tr23, tg01, tg23, tb01, tb23;
};

__device__ __forceinline__ ycocg_offsets ycocg_offsets_of(const unsigned (&pal)[3])
{
    const pk_i16 k128 = {128, 128}, zero = {0, 0};
    const pk_i16 co01 = as_pk(__builtin_amdgcn_perm(0u, pal[0], 0x0c010c00u)) - k128, co23 = as_pk(__builtin_amdgcn_perm(0u, pal[0], 0x0c030c02u)) - k128;
    const pk_i16 cg01 = as_pk(__builtin_amdgcn_perm(0u, pal[1], 0x0c010c00u)) - k128, cg23 = as_pk(__builtin_amdgcn_perm(0u, pal[1], 0x0c030c02u)) - k128;
    ycocg_offsets o;
    o.tr01 = as_u32(co01 - cg01), o.tr23 = as_u32(co23 - cg23);
    o.tg01 = as_u32(cg01), o.tg23 = as_u32(cg23);
    o.tb01 = as_u32(zero - co01 - cg01), o.tb23 = as_u32(zero - co23 - cg23);
    return o;
}

// pixel pair m (texels 2m and 2m + 1) of a Hap Q block: a pair fetches its two entries' offsets with one v_perm_b32 per
// channel, adds the luma pair and clamps
__device__ __forceinline__ void ycocg_pair(const ycocg_offsets &o, unsigned indices, int m, unsigned ypair, pk_i16 &r2,
                                           pk_i16 &g2, pk_i16 &b2)
{
    const pk_i16 zero = {0, 0}, top = {255, 255};
    const unsigned kk = (indices >> (4 * m)) & 15u;                        // two 2-bit palette indices
    // byte selectors of entries k0 (low half) and k1 (high half) of a table of four 16-bit values
    const unsigned sel = __umul24((kk | (kk << 14)) & 0x00030003u, 0x0202u) + 0x01000100u;
    const pk_i16 y2 = as_pk(ypair);
    r2 = y2 + as_pk(__builtin_amdgcn_perm(o.tr23, o.tr01, sel));
    g2 = y2 + as_pk(__builtin_amdgcn_perm(o.tg23, o.tg01, sel));
    b2 = y2 + as_pk(__builtin_amdgcn_perm(o.tb23, o.tb01, sel));
    r2 = __builtin_elementwise_min(__builtin_elementwise_max(r2, zero), top);
    g2 = __builtin_elementwise_min(__builtin_elementwise_max(g2, zero), top);
    b2 = __builtin_elementwise_min(__builtin_elementwise_max(b2, zero), top);
}

// A block that its lane holds in registers already, and where the body is to leave its texels (IN_REGISTERS below)
struct block_in_registers {
    uint4 block;            // the block's 16 bytes (DXT1: x, y)
    uint2 plane;            // HAS_ALPHA: the RGTC1 plane's block
    unsigned *texels;       // packed R | G << 8 | B << 16 | A << 24, as the pictures hold them
};

// FMT: 0 DXT1, 1 DXT5, 2 YCoCg-DXT5; HAS_ALPHA: separate RGTC1 plane supplies A (Hap Q Alpha)
// REGION: the grid covers a rectangle of the texture instead of all of it (hapgpu_k_block_decode_region) -- blocks_x and
// blocks_total are then the rectangle's, lane (bx, by) of it reads texture (and alpha plane) block first + by *
// texture_blocks_x + bx, and the picture is the rectangle's size.  Everything else is the same code: the texels cannot
// differ, and without REGION the two extra arguments are not looked at.
// IN_REGISTERS: no picture and no grid -- the lane's block is `reg`'s and its sixteen texels go to reg->texels, row-major,
// for a caller that has another use for them (bc_transcode.hip); every argument but `reg` is then not looked at.  Again
// the same code, so the texels are the picture's bit for bit.
template <int FMT, bool HAS_ALPHA, bool REGION = false, bool IN_REGISTERS = false>
__device__ __forceinline__ void bc_decode_body(const uint8_t *__restrict__ blocks,
                                               const uint8_t *__restrict__ alpha_blocks,
                                               unsigned blocks_x, unsigned blocks_total,
                                               uint8_t *__restrict__ rgba, size_t row_bytes,
                                               unsigned first = 0u, unsigned texture_blocks_x = 0u,
                                               const block_in_registers *reg = nullptr)
{
    const unsigned lane_id = blockIdx.x * 256u + threadIdx.x;
    if (!IN_REGISTERS && lane_id >= blocks_total)
        return;
    const unsigned by = lane_id / blocks_x, bx = lane_id - by * blocks_x;
    const unsigned id = REGION ? first + by * texture_blocks_x + bx : lane_id;
    int a[16];
    uint2 colour, luma_block = make_uint2(0u, 0u);
    if (FMT == 0) {
        colour = IN_REGISTERS ? make_uint2(reg->block.x, reg->block.y) : *reinterpret_cast<const uint2 *>(blocks + (size_t)id * 8u);
#pragma unroll
        for (int i = 0; i < 16; i++)
            a[i] = 255;
    } else {
        const uint4 v = IN_REGISTERS ? reg->block : *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);
        if (FMT == 2)
            luma_block = make_uint2(v.x, v.y);          // YCoCg: luma, decoded in pairs below
        else
            decode_alpha(make_uint2(v.x, v.y), a);      // DXT5: alpha
        colour = make_uint2(v.z, v.w);
    }
    unsigned pal[3];
    decode_palette(colour, FMT == 0, pal);
    if (FMT == 2)
        ycocg_unscale(pal);
    uint8_t *dst = rgba + (size_t)(4u * by) * row_bytes + 16u * (size_t)bx;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    if (FMT == 2) {
        // pixel pairs (ycocg_pair), then four v_perm_b32 interleave R, G, B, A into two pixels.  (r04: 544 -> ~400
        // instructions per 64 blocks.)
        const ycocg_offsets offsets = ycocg_offsets_of(pal);
        unsigned ypair[8], apair[8];
        decode_alpha_pairs(make_uint2(luma_block.x, luma_block.y), ypair);
        if (HAS_ALPHA)
            decode_alpha_pairs(IN_REGISTERS ? reg->plane : *reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)id * 8u), apair);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            unsigned px[4];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int m = 2 * r + h;
                pk_i16 r2, g2, b2;
                ycocg_pair(offsets, colour.y, m, ypair[m], r2, g2, b2);
                const unsigned rg = __builtin_amdgcn_perm(as_u32(g2), as_u32(r2), 0x06020400u);      // R0 G0 R1 G1
                const unsigned ba = __builtin_amdgcn_perm(HAS_ALPHA ? apair[m] : 0x00FF00FFu, as_u32(b2), 0x06020400u);   // B0 A0 B1 A1
                px[2 * h] = __builtin_amdgcn_perm(ba, rg, 0x05040100u);
                px[2 * h + 1] = __builtin_amdgcn_perm(ba, rg, 0x07060302u);
            }
            if constexpr (IN_REGISTERS) {
#pragma unroll
                for (int c = 0; c < 4; c++)
                    reg->texels[4 * r + c] = px[c];
                continue;
            }
            const v4u v = {px[0], px[1], px[2], px[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
        }
        return;
    }
    int plane[16];
    if (HAS_ALPHA)
        decode_alpha(IN_REGISTERS ? reg->plane : *reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)id * 8u), plane);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        unsigned px[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = 4 * r + c;
            const unsigned k = (colour.y >> (2 * i)) & 3u;
            const int cr = (int)(__builtin_amdgcn_perm(0u, pal[0], k) & 0xFFu);
            const int cg = (int)(__builtin_amdgcn_perm(0u, pal[1], k) & 0xFFu);
            int R, G, B, A;
            if (FMT == 2) {
                const int co = cr - 128, cgg = cg - 128, y = a[i];
                R = clamp255(y + co - cgg);
                G = clamp255(y + cgg);
                B = clamp255(y - co - cgg);
                A = HAS_ALPHA ? plane[i] : 255;
            } else {
                R = cr;
                G = cg;
                B = (int)(__builtin_amdgcn_perm(0u, pal[2], k) & 0xFFu);
                A = HAS_ALPHA ? plane[i] : a[i];
            }
            px[c] = (unsigned)R | ((unsigned)G << 8) | ((unsigned)B << 16) | ((unsigned)A << 24);
        }
        if constexpr (IN_REGISTERS) {
#pragma unroll
            for (int c = 0; c < 4; c++)
                reg->texels[4 * r + c] = px[c];
        } else {
            // streaming stores: the picture is written once and not read back by this kernel -- without the hint the
            // 16-byte stores of DXT1 / DXT5 run at 0.58 / 0.62 of HBM peak, with it at 0.76 (r04, 8K pictures)
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            const v4u v = {px[0], px[1], px[2], px[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
        }
    }
}

// ---- half- and quarter-size pictures: the rounded box mean of 2^S x 2^S full-size texels per output texel, taken
// inside the lane that holds the block (S = 1: the block's four quadrants, region 2 * qy + qx; S = 2: the whole block)
template <int S>
struct regions {
    static constexpr int count = S == 2 ? 1 : 4;
    static constexpr unsigned texels = 1u << (2 * S);
};

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned acc)
{
    return __builtin_amdgcn_udot4(a, b, acc, false);     // v_dot4_u32_u8
}

typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned dot2(unsigned a, unsigned b, unsigned acc)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(pk_u16, a), __builtin_bit_cast(pk_u16, b), acc, false);   // v_dot2_u32_u16
}

// How often each of the four palette entries is picked in every region, byte-packed like the palettes (count of entry k
// in byte k, at most 16): a region's channel sum is then ONE dot product with pal[c], DXT colour being linear in the
// palette.  indices: 16 x 2 bits, texel 4r + c at bit 8r + 2c.
template <int S>
__device__ __forceinline__ void index_counts(unsigned indices, unsigned (&counts)[regions<S>::count])
{
    const unsigned b0 = indices & 0x55555555u, b1 = (indices >> 1) & 0x55555555u;
    const unsigned is1 = b0 & ~b1, is2 = b1 & ~b0, is3 = b0 & b1;
#pragma unroll
    for (int q = 0; q < regions<S>::count; q++) {
        // (one bit per texel of the region, at the low bit of its index)
        const unsigned mask = S == 2 ? 0x55555555u : (q & 1 ? 0x00005050u : 0x00000505u) << (q & 2 ? 16 : 0);
        const unsigned n1 = (unsigned)__builtin_popcount(is1 & mask), n2 = (unsigned)__builtin_popcount(is2 & mask),
                       n3 = (unsigned)__builtin_popcount(is3 & mask);
        counts[q] = (regions<S>::texels - n1 - n2 - n3) | (n1 << 8) | (n2 << 16) | (n3 << 24);
    }
}

// The region sums of an alpha-style block (DXT5 alpha, an RGTC1 plane) on top of `seed` (the rounding term): its four
// rows of four bytes against byte masks, accumulated by the dot product.  (Counting the eight 3-bit codes per region
// for two dot products with the ramp takes about twice the instructions of fetching the rows: the codes need three bit
// planes and eight matches each.)
template <int S>
__device__ __forceinline__ void alpha_sums(uint2 blk, unsigned seed, unsigned (&sums)[regions<S>::count])
{
    unsigned rows[4];
    decode_alpha_rows(blk, rows);
    if (S == 2) {
        sums[0] = dot4(rows[0], 0x01010101u, dot4(rows[1], 0x01010101u, dot4(rows[2], 0x01010101u, dot4(rows[3], 0x01010101u, seed))));
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned mask = q & 1 ? 0x01010000u : 0x00000101u;
            sums[q] = dot4(rows[q & 2], mask, dot4(rows[(q & 2) + 1], mask, seed));
        }
    }
}

// One block per lane as bc_decode_body; a lane stores one texel (S = 2) or two rows of two (S = 1).  Every full-size
// texel is what bc_decode_body makes of it, Hap Q's per-texel clamp included: there the clamped pairs are summed.
// IN_REGISTERS: as for bc_decode_body -- reg->texels gets the one texel, or the four as [2 * qy + qx].
template <int FMT, bool HAS_ALPHA, int S, bool IN_REGISTERS = false>
__device__ __forceinline__ void bc_decode_scaled_body(const uint8_t *__restrict__ blocks,
                                                      const uint8_t *__restrict__ alpha_blocks,
                                                      unsigned blocks_x, unsigned blocks_total,
                                                      uint8_t *__restrict__ rgba, size_t row_bytes,
                                                      const block_in_registers *reg = nullptr)
{
    constexpr int Q = regions<S>::count;
    constexpr unsigned texels = regions<S>::texels, half = texels / 2u;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (!IN_REGISTERS && id >= blocks_total)
        return;
    const unsigned by = id / blocks_x, bx = id - by * blocks_x;
    uint2 colour, first = make_uint2(0u, 0u);
    if (FMT == 0) {
        colour = IN_REGISTERS ? make_uint2(reg->block.x, reg->block.y) : *reinterpret_cast<const uint2 *>(blocks + (size_t)id * 8u);
    } else {
        const uint4 v = IN_REGISTERS ? reg->block : *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);
        first = make_uint2(v.x, v.y);                   // DXT5: alpha; YCoCg: luma
        colour = make_uint2(v.z, v.w);
    }
    unsigned pal[3];
    decode_palette(colour, FMT == 0, pal);
    // [R, G, B, A][region]: the sums with the rounding term `half` already in them -- it is the accumulator the dot
    // products start from
    unsigned sum[4][Q];
    if (FMT == 2) {
        ycocg_unscale(pal);
        const ycocg_offsets offsets = ycocg_offsets_of(pal);
        unsigned ypair[8];
        decode_alpha_pairs(first, ypair);
        // pair m = 2r + h holds texels (r, 2h) and (r, 2h + 1): both of region 2 * (r / 2) + h.  At most 8 x 255 a half.
        pk_i16 acc[3][Q] = {};
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const int q = S == 2 ? 0 : ((m >> 2) << 1) | (m & 1);
            pk_i16 r2, g2, b2;
            ycocg_pair(offsets, colour.y, m, ypair[m], r2, g2, b2);
            acc[0][q] += r2;
            acc[1][q] += g2;
            acc[2][q] += b2;
        }
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < Q; q++)
                sum[c][q] = dot2(as_u32(acc[c][q]), 0x00010001u, half);      // low half + high half + rounding term
    } else {
        unsigned counts[Q];
        index_counts<S>(colour.y, counts);
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < Q; q++)
                sum[c][q] = dot4(pal[c], counts[q], half);
    }
    if (HAS_ALPHA) {
        alpha_sums<S>(IN_REGISTERS ? reg->plane : *reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)id * 8u), half, sum[3]);
    } else if (FMT == 1) {
        alpha_sums<S>(first, half, sum[3]);
    } else {
#pragma unroll
        for (int q = 0; q < Q; q++)
            sum[3][q] = 255u * texels + half;
    }
    unsigned px[Q];
#pragma unroll
    for (int q = 0; q < Q; q++)
        px[q] = (sum[0][q] >> (2 * S)) | ((sum[1][q] >> (2 * S)) << 8) | ((sum[2][q] >> (2 * S)) << 16) |
                ((sum[3][q] >> (2 * S)) << 24);
    // streaming stores, as at full size: 4 bytes a lane (256 B contiguous per wave-instruction) or two rows of 8
    if constexpr (IN_REGISTERS) {
#pragma unroll
        for (int q = 0; q < Q; q++)
            reg->texels[q] = px[q];
    } else if constexpr (S == 2) {
        __builtin_nontemporal_store(px[0], reinterpret_cast<unsigned *>(rgba + (size_t)by * row_bytes + 4u * (size_t)bx));
    } else {
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        uint8_t *dst = rgba + (size_t)(2u * by) * row_bytes + 8u * (size_t)bx;
        const v2u upper = {px[0], px[1]}, lower = {px[2], px[3]};
        __builtin_nontemporal_store(upper, reinterpret_cast<v2u *>(dst));
        __builtin_nontemporal_store(lower, reinterpret_cast<v2u *>(dst + row_bytes));
    }
}

} // namespace texels
} // namespace hapbc
