// bptc_decode.hip -- BC7 (RGBA_BPTC_UNORM, Hap R) -> RGBA8 for gfx950.
//
// Same shape as bc_decode.hip: one 4x4 block per lane, one 16-byte block load per lane, four 16-byte streaming row
// stores per lane; 16 B read + 64 B written per block.  Semantics: the BPTC definition the Hap spec cites
// (ARB_texture_compression_bptc / the BC7 section of the Khronos Data Format Specification); reserved blocks (no mode
// bit in the first byte) decode to (0, 0, 0, 0).
//
// Real BC7 content mixes modes inside every wavefront, so there is no switch on the mode: every lane runs the same
// straight-line code, driven by its mode's descriptor.  Each descriptor field is a nibble of a 32-bit constant (one
// v_bfe_u32 per field), every field of the block is read at a lane-varying bit offset with v_alignbit_b32 on a dword
// pair picked by selects, a texel's subset comes from one partition dword (2 bits per texel) and its index position is
// worked out from the anchors.  Per-lane arrays are only ever indexed by unrolled constants (endpoints, weight tables
// picked with v_perm_b32), so nothing goes to scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapgpu_runtime.hpp"
#include "bptc_tables.hpp"

namespace {

// descriptor fields of modes 0..7, mode m in nibble m
constexpr unsigned D_SUBSETS = 0x21112323u;   // 3 2 3 2 1 1 1 2
constexpr unsigned D_PART_BITS = 0x60006664u; // 4 6 6 6 0 0 0 6
constexpr unsigned D_COLOUR_BITS = 0x57757564u; // 4 6 5 7 5 7 7 5
constexpr unsigned D_ALPHA_BITS = 0x57860000u;  // 0 0 0 0 6 8 7 5
constexpr unsigned D_EPB = 0x11001001u;         // endpoint p-bits: modes 0, 3, 6, 7
constexpr unsigned D_SPB = 0x00000010u;         // shared p-bits: mode 1
constexpr unsigned D_INDEX_BITS = 0x24222233u;  // 3 3 2 2 2 2 4 2
constexpr unsigned D_INDEX2_BITS = 0x00230000u; // 0 0 0 0 3 2 0 0

__device__ __forceinline__ unsigned field(unsigned desc, unsigned mode) { return __builtin_amdgcn_ubfe(desc, 4u * mode, 4u); }

// 32 bits of the 128-bit block q0..q3 starting at bit `off` (0..127; bits past the block read as zero)
__device__ __forceinline__ unsigned bits_at(uint4 q, unsigned off)
{
    const unsigned d = off >> 5;
    const unsigned lo = d == 0u ? q.x : d == 1u ? q.y : d == 2u ? q.z : d == 3u ? q.w : 0u;
    const unsigned hi = d == 0u ? q.y : d == 1u ? q.z : d == 2u ? q.w : 0u;
    return __builtin_amdgcn_alignbit(hi, lo, off & 31u);
}

// the 8-bit endpoint of a `bits`-bit value (p-bit already appended): MSB to bit 7, top bits copied into the low bits
__device__ __forceinline__ unsigned unquantize(unsigned v, unsigned bits)
{
    v <<= 8u - bits;
    return v | (v >> bits);
}

// weight of index `i` from a 16-byte table t0..t3
__device__ __forceinline__ unsigned weight(uint4 t, unsigned i)
{
    const unsigned lo = __builtin_amdgcn_perm(t.y, t.x, i & 7u), hi = __builtin_amdgcn_perm(t.w, t.z, i & 7u);
    return (i & 8u ? hi : lo) & 0xFFu;
}

// weight tables of 2, 3 and 4 index bits, one byte per entry
__device__ __forceinline__ uint4 weight_table(unsigned bits)
{
    const uint4 w2 = make_uint4(0x402B1500u, 0u, 0u, 0u);
    const uint4 w3 = make_uint4(0x1B120900u, 0x40372E25u, 0u, 0u);
    const uint4 w4 = make_uint4(0x0D090400u, 0x1E1A1511u, 0x2F2B2622u, 0x403C3733u);
    return bits == 2u ? w2 : bits == 3u ? w3 : w4;
}

typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pk_u16 as_pk(unsigned v) { return __builtin_bit_cast(pk_u16, v); }
__device__ __forceinline__ unsigned as_u32(pk_u16 v) { return __builtin_bit_cast(unsigned, v); }

// S = 0: the full-size picture.  S = 1 / 2: the half- / quarter-size one -- the rounded box mean of 2^S x 2^S texels
// per output texel (bc_decode.hip's scaled kernels): the decoded texels are summed per channel as they come, still
// packed as 16-bit pairs (at most 16 x 255 a half), in the block's four quadrants (region 2 * qy + qx) or in one; the
// rotation's byte order is applied once per output texel.  A lane stores two rows of 8 bytes or one texel.
// REGION (S = 0): the grid covers a rectangle of the texture (bc_decode.hip's bc_decode_body): blocks_x and blocks_total
// are the rectangle's, lane (bx, by) reads texture block first + by * texture_blocks_x + bx.
template <int S, bool REGION = false>
__device__ __forceinline__ void bptc_decode_body(const uint8_t *__restrict__ blocks, unsigned blocks_x,
                                                 unsigned blocks_total, uint8_t *__restrict__ rgba, size_t row_bytes,
                                                 unsigned first = 0u, unsigned texture_blocks_x = 0u)
{
    const unsigned lane_id = blockIdx.x * 256u + threadIdx.x;
    if (lane_id >= blocks_total)
        return;
    const unsigned by = lane_id / blocks_x, bx = lane_id - by * blocks_x;
    const unsigned id = REGION ? first + by * texture_blocks_x + bx : lane_id;
    const uint4 q = *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);

    // ---- the mode and its descriptor
    const unsigned mode_raw = __builtin_ctz(q.x | 0x100u);          // 8: reserved block
    const bool reserved = mode_raw == 8u;
    const unsigned mode = reserved ? 0u : mode_raw;
    const unsigned ns = field(D_SUBSETS, mode);
    const unsigned pb = field(D_PART_BITS, mode);
    const unsigned cb = field(D_COLOUR_BITS, mode);
    const unsigned ab = field(D_ALPHA_BITS, mode);
    const unsigned epb = field(D_EPB, mode), spb = field(D_SPB, mode);
    const unsigned ib = field(D_INDEX_BITS, mode), ib2 = field(D_INDEX2_BITS, mode);
    const unsigned rb = ib2 ? 2u : 0u;                               // rotation bits: modes 4 and 5
    const unsigned isb = ib2 == 3u ? 1u : 0u;                        // index-selection bit: mode 4
    const unsigned after_mode = __builtin_amdgcn_ubfe(q.x, mode + 1u, 8u);
    const unsigned partition = after_mode & ((1u << pb) - 1u);
    const unsigned rotation = __builtin_amdgcn_ubfe(after_mode, 0u, rb);
    const unsigned selection = __builtin_amdgcn_ubfe(after_mode, 2u, isb);

    // ---- endpoints: per channel all 2 * ns values in one window (at most 30 bits), then the p-bits
    const unsigned ne = 2u * ns;
    const unsigned ends_at = mode + 1u + pb + rb + isb;
    const unsigned cwin = ne * cb;
    const unsigned win_r = bits_at(q, ends_at), win_g = bits_at(q, ends_at + cwin), win_b = bits_at(q, ends_at + 2u * cwin);
    const unsigned win_a = bits_at(q, ends_at + 3u * cwin);
    const unsigned pbits_at = ends_at + ne * (3u * cb + ab);
    const unsigned win_p = bits_at(q, pbits_at);
    const unsigned has_p = epb | spb;
    const unsigned cbits = cb + has_p, abits = ab + (ab ? has_p : 0u);
    // endpoint e of subset s is endpoint 2s + e; packed as 16-bit pairs (R | G << 16, B | A << 16)
    unsigned e_rg[6], e_ba[6];
#pragma unroll
    for (unsigned j = 0; j < 6u; j++) {
        const unsigned p = (win_p >> (spb ? (j >> 1) : j)) & has_p;
        const unsigned r = unquantize((__builtin_amdgcn_ubfe(win_r, j * cb, cb) << has_p) | p, cbits);
        const unsigned g = unquantize((__builtin_amdgcn_ubfe(win_g, j * cb, cb) << has_p) | p, cbits);
        const unsigned b = unquantize((__builtin_amdgcn_ubfe(win_b, j * cb, cb) << has_p) | p, cbits);
        const unsigned a = ab ? unquantize((__builtin_amdgcn_ubfe(win_a, j * ab, ab) << has_p) | p, abits) : 255u;
        e_rg[j] = r | (g << 16);
        e_ba[j] = b | (a << 16);
    }

    // ---- partition map and anchors
    const unsigned table_index = ((ns == 3u ? 64u : 0u) + partition) & 127u;
    const unsigned map = ns == 1u ? 0u : k_partitions[table_index];
    const unsigned anchors = ns == 1u ? 0u : (unsigned)k_anchors[table_index];
    const unsigned anchor_mask = 1u | (1u << (anchors & 15u)) | (1u << (anchors >> 4));   // bit t: texel t is an anchor

    // ---- index windows: 64 bits from the first index bit of each index set
    const unsigned idx1_at = 128u - (16u * ib - ns) - (ib2 ? 16u * ib2 - 1u : 0u);
    const unsigned idx2_at = idx1_at + 16u * ib - ns;
    const uint64_t x1 = (uint64_t)bits_at(q, idx1_at) | ((uint64_t)bits_at(q, idx1_at + 32u) << 32);
    const uint64_t x2 = (uint64_t)bits_at(q, idx2_at) | ((uint64_t)bits_at(q, idx2_at + 32u) << 32);
    const unsigned m1 = (1u << ib) - 1u, m2 = (1u << ib2) - 1u;
    // colour and alpha: which index set and which weight table (mode 4's selection bit swaps the two sets)
    const unsigned c_bits = selection ? ib2 : ib, a_bits = ib2 ? (selection ? ib : ib2) : ib;
    const uint4 wc_table = weight_table(c_bits), wa_table = weight_table(a_bits);
    // final byte order: R G B A gathered from (R | G << 16, B | A << 16) and the rotation's swap; zeros if reserved
    const unsigned base_sel = rotation == 0u ? 0x06040200u : rotation == 1u ? 0x00040206u : rotation == 2u ? 0x02040600u : 0x04060200u;
    const unsigned out_sel = reserved ? 0x0C0C0C0Cu : base_sel;

    uint8_t *dst = rgba + (size_t)((4u >> S) * by) * row_bytes + (size_t)(16u >> S) * bx;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    constexpr int Q = S == 1 ? 4 : 1;
    pk_u16 sum_rg[Q] = {}, sum_ba[Q] = {};
#pragma unroll
    for (unsigned r = 0; r < 4u; r++) {
        unsigned px[4];
#pragma unroll
        for (unsigned c = 0; c < 4u; c++) {
            const unsigned t = 4u * r + c;
            const unsigned before = (unsigned)__builtin_popcount(anchor_mask & ((1u << t) - 1u));
            const unsigned anchor = (anchor_mask >> t) & 1u;
            const unsigned i1 = (unsigned)(x1 >> (t * ib - before)) & (m1 >> anchor);
            const unsigned i2 = (unsigned)(x2 >> ((t * ib2 - (t ? 1u : 0u)) & 63u)) & (m2 >> (t ? 0u : 1u));   // (unused without ib2)
            const unsigned ic = selection ? i2 : i1, ia = ib2 ? (selection ? i1 : i2) : i1;
            const unsigned wc = weight(wc_table, ic), wa = weight(wa_table, ia);
            const unsigned s = (map >> (2u * t)) & 3u;
            const unsigned e0rg = s == 0u ? e_rg[0] : s == 1u ? e_rg[2] : e_rg[4];
            const unsigned e1rg = s == 0u ? e_rg[1] : s == 1u ? e_rg[3] : e_rg[5];
            const unsigned e0ba = s == 0u ? e_ba[0] : s == 1u ? e_ba[2] : e_ba[4];
            const unsigned e1ba = s == 0u ? e_ba[1] : s == 1u ? e_ba[3] : e_ba[5];
            // ((64 - w) * e0 + w * e1 + 32) >> 6 on two channels at once (at most 16352: no 16-bit overflow)
            const pk_u16 w_rg = as_pk(wc * 0x10001u), w_ba = as_pk(wc | (wa << 16));
            const pk_u16 k64 = {64, 64}, k32 = {32, 32}, k6 = {6, 6};
            const pk_u16 rg = ((k64 - w_rg) * as_pk(e0rg) + w_rg * as_pk(e1rg) + k32) >> k6;
            const pk_u16 ba = ((k64 - w_ba) * as_pk(e0ba) + w_ba * as_pk(e1ba) + k32) >> k6;
            if constexpr (S == 0) {
                px[c] = __builtin_amdgcn_perm(as_u32(ba), as_u32(rg), out_sel);
            } else {
                const unsigned q = S == 1 ? ((r >> 1) << 1) | (c >> 1) : 0u;
                sum_rg[q] += rg;
                sum_ba[q] += ba;
            }
        }
        if constexpr (S == 0) {
            const v4u v = {px[0], px[1], px[2], px[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
        }
    }
    if constexpr (S != 0) {
        constexpr unsigned short half = 1u << (2 * S - 1);
        const pk_u16 khalf = {half, half}, kshift = {2 * S, 2 * S};
        unsigned out[Q];
#pragma unroll
        for (int q = 0; q < Q; q++)
            out[q] = __builtin_amdgcn_perm(as_u32((sum_ba[q] + khalf) >> kshift), as_u32((sum_rg[q] + khalf) >> kshift), out_sel);
        if constexpr (S == 2) {
            __builtin_nontemporal_store(out[0], reinterpret_cast<unsigned *>(dst));
        } else {
            typedef unsigned v2u __attribute__((ext_vector_type(2)));
            const v2u upper = {out[0], out[1]}, lower = {out[2], out[3]};
            __builtin_nontemporal_store(upper, reinterpret_cast<v2u *>(dst));
            __builtin_nontemporal_store(lower, reinterpret_cast<v2u *>(dst + row_bytes));
        }
    }
}

// pictures of one geometry in one launch: picture blockIdx.z, [textures][unused][pictures] of a HapGpuPictureTable;
// texture address 0 = not this launch's format: skip
__global__ __launch_bounds__(256) void bptc_decode_kernel(HapGpuPictureTable t, unsigned blocks_x, unsigned blocks_total,
                                                          size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bptc_decode_body<0>(blocks, blocks_x, blocks_total, (uint8_t *)picture_address(t, 2), row_bytes);
}

// ... and pictures of (width >> S) x (height >> S), S = 1 or 2
template <int S>
__global__ __launch_bounds__(256) void bptc_decode_scaled_kernel(HapGpuPictureTable t, unsigned blocks_x,
                                                                 unsigned blocks_total, size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bptc_decode_body<S>(blocks, blocks_x, blocks_total, (uint8_t *)picture_address(t, 2), row_bytes);
}

// ... and a rectangle of every texture (bc_decode.hip's bc_decode_region_kernel): lane id is block (bx, by) of the rectangle
__global__ __launch_bounds__(256) void bptc_decode_region_kernel(HapGpuPictureTable t, HapGpuRegionBlocks g, size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bptc_decode_body<0, true>(blocks, g.region_x, g.region_total, (uint8_t *)picture_address(t, 2), row_bytes, g.first, g.blocks_x);
}

} // namespace

// RGBA_BPTC_UNORM of hapgpu_k_block_decode_region (bc_decode.hip)
void hapgpu_launch_bptc_decode_region(const HapGpuPictureTable &t, unsigned pictures, const HapGpuRegionBlocks &g,
                                      size_t row_bytes, hipStream_t stream)
{
    hipLaunchKernelGGL(bptc_decode_region_kernel, dim3((g.region_total + 255u) / 256u, 1, pictures), dim3(256), 0, stream, t, g,
                       row_bytes);
}

// RGBA_BPTC_UNORM of hapgpu_k_block_decode (bc_decode.hip)
void hapgpu_launch_bptc_decode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                               size_t row_bytes, hipStream_t stream)
{
    const unsigned total = bx * by;
    hipLaunchKernelGGL(bptc_decode_kernel, dim3((total + 255u) / 256u, 1, pictures), dim3(256), 0, stream, t, bx, total,
                       row_bytes);
}

// RGBA_BPTC_UNORM of hapgpu_k_block_decode_scaled (bc_decode.hip): scale_log2 1 or 2
void hapgpu_launch_bptc_decode_scaled(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                                      size_t row_bytes, unsigned scale_log2, hipStream_t stream)
{
    const unsigned total = bx * by;
    const dim3 grid((total + 255u) / 256u, 1, pictures), block(256);
    if (scale_log2 == 1u)
        hipLaunchKernelGGL(bptc_decode_scaled_kernel<1>, grid, block, 0, stream, t, bx, total, row_bytes);
    else
        hipLaunchKernelGGL(bptc_decode_scaled_kernel<2>, grid, block, 0, stream, t, bx, total, row_bytes);
}
