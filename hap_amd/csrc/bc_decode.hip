// bc_decode.hip -- DXT1 / DXT5 / scaled YCoCg-DXT5 (+ RGTC1 alpha plane) -> RGBA8 for gfx950.
//
// The reference stops at block-compressed texture bytes because its clients hand them to GPU
// texture units (README.md:4); CDNA has none, so a pipeline that wants pixels needs this kernel
// (SURVEY.md section 8f, rank 1).  Mirror image of bc_encode.hip: one 4x4 block per lane, 8/16-byte
// block load per lane (512 B / 1 KiB contiguous per wave), four 16-byte row stores per lane
// (1 KiB contiguous per wave-instruction).  Bounded by HBM: b read + 64 B written per block.
// Arithmetic follows oracle/bc_oracle.c (obc_decode_*) exactly; results are bit-identical.
// Half- and quarter-size pictures (the rounded box mean of every 2x2 / 4x4 texels, exact) come from the scaled kernels
// further down: the same block per lane, 16 or 4 bytes written per block instead of 64.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_core.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using namespace hapbc;      // decode_alpha, decode_alpha_pairs: the alpha-style half of DXT5 / Hap Q blocks, RGTC1 planes

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

// FMT: 0 DXT1, 1 DXT5, 2 YCoCg-DXT5; HAS_ALPHA: separate RGTC1 plane supplies A (Hap Q Alpha)
// REGION: the grid covers a rectangle of the texture instead of all of it (hapgpu_k_block_decode_region) -- blocks_x and
// blocks_total are then the rectangle's, lane (bx, by) of it reads texture (and alpha plane) block first + by *
// texture_blocks_x + bx, and the picture is the rectangle's size.  Everything else is the same code: the texels cannot
// differ, and without REGION the two extra arguments are not looked at.
template <int FMT, bool HAS_ALPHA, bool REGION = false>
__device__ __forceinline__ void bc_decode_body(const uint8_t *__restrict__ blocks,
                                               const uint8_t *__restrict__ alpha_blocks,
                                               unsigned blocks_x, unsigned blocks_total,
                                               uint8_t *__restrict__ rgba, size_t row_bytes,
                                               unsigned first = 0u, unsigned texture_blocks_x = 0u)
{
    const unsigned lane_id = blockIdx.x * 256u + threadIdx.x;
    if (lane_id >= blocks_total)
        return;
    const unsigned by = lane_id / blocks_x, bx = lane_id - by * blocks_x;
    const unsigned id = REGION ? first + by * texture_blocks_x + bx : lane_id;
    int a[16];
    uint2 colour, luma_block = make_uint2(0u, 0u);
    if (FMT == 0) {
        colour = *reinterpret_cast<const uint2 *>(blocks + (size_t)id * 8u);
#pragma unroll
        for (int i = 0; i < 16; i++)
            a[i] = 255;
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);
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
            decode_alpha_pairs(*reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)id * 8u), apair);
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
            const v4u v = {px[0], px[1], px[2], px[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
        }
        return;
    }
    int plane[16];
    if (HAS_ALPHA)
        decode_alpha(*reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)id * 8u), plane);
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
        {
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
template <int FMT, bool HAS_ALPHA, int S>
__device__ __forceinline__ void bc_decode_scaled_body(const uint8_t *__restrict__ blocks,
                                                      const uint8_t *__restrict__ alpha_blocks,
                                                      unsigned blocks_x, unsigned blocks_total,
                                                      uint8_t *__restrict__ rgba, size_t row_bytes)
{
    constexpr int Q = regions<S>::count;
    constexpr unsigned texels = regions<S>::texels, half = texels / 2u;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= blocks_total)
        return;
    const unsigned by = id / blocks_x, bx = id - by * blocks_x;
    uint2 colour, first = make_uint2(0u, 0u);
    if (FMT == 0) {
        colour = *reinterpret_cast<const uint2 *>(blocks + (size_t)id * 8u);
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);
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
        alpha_sums<S>(*reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)id * 8u), half, sum[3]);
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
    if constexpr (S == 2) {
        __builtin_nontemporal_store(px[0], reinterpret_cast<unsigned *>(rgba + (size_t)by * row_bytes + 4u * (size_t)bx));
    } else {
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        uint8_t *dst = rgba + (size_t)(2u * by) * row_bytes + 8u * (size_t)bx;
        const v2u upper = {px[0], px[1]}, lower = {px[2], px[3]};
        __builtin_nontemporal_store(upper, reinterpret_cast<v2u *>(dst));
        __builtin_nontemporal_store(lower, reinterpret_cast<v2u *>(dst + row_bytes));
    }
}

// pictures of one geometry in one launch: picture blockIdx.z, [textures][alpha planes][pictures] of a
// HapGpuPictureTable; texture address 0 = not this launch's format: skip
template <int FMT, bool HAS_ALPHA>
__global__ __launch_bounds__(256) void bc_decode_kernel(HapGpuPictureTable t, unsigned blocks_x, unsigned blocks_total,
                                                        size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bc_decode_body<FMT, HAS_ALPHA>(blocks, (const uint8_t *)picture_address(t, 1), blocks_x, blocks_total,
                                   (uint8_t *)picture_address(t, 2), row_bytes);
}

template <int FMT>
void launch(const HapGpuPictureTable &t, unsigned pictures, bool alpha, unsigned bx, unsigned by, size_t row_bytes,
            hipStream_t stream)
{
    const unsigned total = bx * by;
    const dim3 grid((total + 255u) / 256u, 1, pictures), block(256);
    if (alpha)
        hipLaunchKernelGGL((bc_decode_kernel<FMT, true>), grid, block, 0, stream, t, bx, total, row_bytes);
    else
        hipLaunchKernelGGL((bc_decode_kernel<FMT, false>), grid, block, 0, stream, t, bx, total, row_bytes);
}

// ... and a rectangle of every texture to pictures of the rectangle's size: the same table
template <int FMT, bool HAS_ALPHA>
__global__ __launch_bounds__(256) void bc_decode_region_kernel(HapGpuPictureTable t, HapGpuRegionBlocks g, size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bc_decode_body<FMT, HAS_ALPHA, true>(blocks, (const uint8_t *)picture_address(t, 1), g.region_x, g.region_total,
                                         (uint8_t *)picture_address(t, 2), row_bytes, g.first, g.blocks_x);
}

template <int FMT>
void launch_region(const HapGpuPictureTable &t, unsigned pictures, bool alpha, const HapGpuRegionBlocks &g, size_t row_bytes,
                   hipStream_t stream)
{
    const dim3 grid((g.region_total + 255u) / 256u, 1, pictures), block(256);
    if (alpha)
        hipLaunchKernelGGL((bc_decode_region_kernel<FMT, true>), grid, block, 0, stream, t, g, row_bytes);
    else
        hipLaunchKernelGGL((bc_decode_region_kernel<FMT, false>), grid, block, 0, stream, t, g, row_bytes);
}

// ... and at half (S = 1) or quarter (S = 2) size: the same table, pictures of (width >> S) x (height >> S)
template <int FMT, bool HAS_ALPHA, int S>
__global__ __launch_bounds__(256) void bc_decode_scaled_kernel(HapGpuPictureTable t, unsigned blocks_x,
                                                               unsigned blocks_total, size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bc_decode_scaled_body<FMT, HAS_ALPHA, S>(blocks, (const uint8_t *)picture_address(t, 1), blocks_x, blocks_total,
                                             (uint8_t *)picture_address(t, 2), row_bytes);
}

template <int FMT, int S>
void launch_scaled(const HapGpuPictureTable &t, unsigned pictures, bool alpha, unsigned bx, unsigned by, size_t row_bytes,
                   hipStream_t stream)
{
    const unsigned total = bx * by;
    const dim3 grid((total + 255u) / 256u, 1, pictures), block(256);
    if (alpha)
        hipLaunchKernelGGL((bc_decode_scaled_kernel<FMT, true, S>), grid, block, 0, stream, t, bx, total, row_bytes);
    else
        hipLaunchKernelGGL((bc_decode_scaled_kernel<FMT, false, S>), grid, block, 0, stream, t, bx, total, row_bytes);
}

template <int FMT>
void launch_scaled(const HapGpuPictureTable &t, unsigned pictures, bool alpha, unsigned bx, unsigned by, size_t row_bytes,
                   unsigned scale_log2, hipStream_t stream)
{
    if (scale_log2 == 1u)
        launch_scaled<FMT, 1>(t, pictures, alpha, bx, by, row_bytes, stream);
    else
        launch_scaled<FMT, 2>(t, pictures, alpha, bx, by, row_bytes, stream);
}

} // namespace

// hapgpu_abi.h: DXT1, DXT5, YCoCg-DXT5 (with_alpha: + RGTC1 plane) here, BC7 in bptc_decode.hip (no alpha plane), BC6H
// in bc6h_decode.hip (no alpha plane, 8-byte texels), lone RGTC1 textures to A8 pictures in alpha_plane.hip.  Returns 0
// launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_decode(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                     unsigned width, unsigned height, unsigned format, size_t row_bytes, int wide,
                                     unsigned picture_kind)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    const bool half = picture_kind == HAPGPU_PICTURE_RGBA16F, plane = picture_kind == HAPGPU_PICTURE_A8;
    if (picture_kind > HAPGPU_PICTURE_A8 || half != (format == 0x8E8F || format == 0x8E8E) ||
        plane != (format == 0x8DBB) || (plane && (with_alpha || height / 4u > 65535u)))
        return 1;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || (width & 3u) || (height & 3u) || row_bytes < (size_t)width * HAPGPU_PICTURE_TEXEL_BYTES(picture_kind) ||
        (row_bytes & (plane ? 3u : 15u)))
        return 1;
    const HapGpuPictureTable &t = *table;
    const unsigned bx = width / 4u, by = height / 4u;
    if (with_alpha && (format == 0x8E8C || half))
        return 1;
    switch (format) {
    case 0x83F0: launch<0>(t, pictures, with_alpha != 0, bx, by, row_bytes, stream); break;
    case 0x83F3: launch<1>(t, pictures, with_alpha != 0, bx, by, row_bytes, stream); break;
    case 0x01: launch<2>(t, pictures, with_alpha != 0, bx, by, row_bytes, stream); break;
    case 0x8DBB: hapgpu_launch_alpha_decode(t, pictures, bx, by, row_bytes, wide != 0, stream); break;
    case 0x8E8C: hapgpu_launch_bptc_decode(t, pictures, bx, by, row_bytes, stream); break;
    case 0x8E8F: hapgpu_launch_bc6h_decode(t, pictures, false, bx, by, row_bytes, stream); break;
    case 0x8E8E: hapgpu_launch_bc6h_decode(t, pictures, true, bx, by, row_bytes, stream); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

// hapgpu_abi.h: the same blocks to RGBA8 pictures of (width >> scale_log2) x (height >> scale_log2), scale_log2 1 or 2:
// DXT1, DXT5, YCoCg-DXT5 (with_alpha: + RGTC1 plane) here, BC7 in bptc_decode.hip.  A lane stores 16 >> scale_log2
// bytes per output row: pictures and row_bytes aligned to that.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_decode_scaled(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                            int with_alpha, unsigned width, unsigned height, unsigned format,
                                            unsigned scale_log2, size_t row_bytes)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (scale_log2 < 1u || scale_log2 > 2u)
        return 1;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || (width & 3u) || (height & 3u) || row_bytes < (size_t)(width >> scale_log2) * 4u ||
        (row_bytes & ((16u >> scale_log2) - 1u)))
        return 1;
    const HapGpuPictureTable &t = *table;
    const unsigned bx = width / 4u, by = height / 4u;
    if (with_alpha && format == 0x8E8C)
        return 1;
    switch (format) {
    case 0x83F0: launch_scaled<0>(t, pictures, with_alpha != 0, bx, by, row_bytes, scale_log2, stream); break;
    case 0x83F3: launch_scaled<1>(t, pictures, with_alpha != 0, bx, by, row_bytes, scale_log2, stream); break;
    case 0x01: launch_scaled<2>(t, pictures, with_alpha != 0, bx, by, row_bytes, scale_log2, stream); break;
    case 0x8E8C: hapgpu_launch_bptc_decode_scaled(t, pictures, bx, by, row_bytes, scale_log2, stream); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

// hapgpu_abi.h: the rectangle (x, y, region_width, region_height) of every texture to an RGBA8 picture of
// region_width x region_height: DXT1, DXT5, YCoCg-DXT5 (with_alpha: + RGTC1 plane) here, BC7 in bptc_decode.hip.  The
// per-block bodies are hapgpu_k_block_decode's; only the block a lane takes differs.  Returns 0 launched, 1 bad arguments,
// 4 launch failure.
extern "C" int hapgpu_k_block_decode_region(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                            int with_alpha, unsigned width, unsigned height, unsigned format, unsigned x,
                                            unsigned y, unsigned region_width, unsigned region_height, size_t row_bytes)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || ((width | height | x | y | region_width | region_height) & 3u) || region_width == 0 ||
        region_height == 0 || x > width || region_width > width - x || y > height || region_height > height - y ||
        row_bytes < (size_t)region_width * 4u || (row_bytes & 15u) ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)
        return 1;
    const HapGpuPictureTable &t = *table;
    HapGpuRegionBlocks g;
    g.blocks_x = width / 4u;
    g.first = (y / 4u) * g.blocks_x + x / 4u;
    g.region_x = region_width / 4u;
    g.region_total = g.region_x * (region_height / 4u);
    if (with_alpha && format == 0x8E8C)
        return 1;
    switch (format) {
    case 0x83F0: launch_region<0>(t, pictures, with_alpha != 0, g, row_bytes, stream); break;
    case 0x83F3: launch_region<1>(t, pictures, with_alpha != 0, g, row_bytes, stream); break;
    case 0x01: launch_region<2>(t, pictures, with_alpha != 0, g, row_bytes, stream); break;
    case 0x8E8C: hapgpu_launch_bptc_decode_region(t, pictures, g, row_bytes, stream); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
