// bc6h_decode.hip -- BC6H (RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT, Hap HDR) -> RGBA16F for gfx950.
//
// Same shape as bptc_decode.hip: one 4x4 block per lane, one 16-byte block load per lane, eight 16-byte streaming
// stores per lane (4 rows x 32 B); 16 B read + 128 B written per block.  Semantics: the BC6H section of
// ARB_texture_compression_bptc / the Khronos Data Format Specification, bit for bit: endpoints (base + delta, masked
// and, signed, sign-extended in transformed modes), unquantised to 16 bits, interpolated with the 3- or 4-bit BPTC
// weights and finished (x 31/64 unsigned, x 31/32 with the sign in bit 15 signed; -1 finishes to 0x8000 and stays
// so).  The finish yields the half-float bit pattern directly.  Alpha is 1.0 (0x3C00); reserved modes (0x13, 0x17,
// 0x1B, 0x1F) give RGB 0.
//
// Real BC6H content mixes modes inside every wavefront, so there is no branch on the mode: every lane runs the same
// straight-line code, driven by its mode's row of k_modes.  A row holds the mode's parameters and K = 25 runs of
// header bits, each {source bit, length, destination bit, reversed}; every run lands in one of six packed endpoint
// dwords (rw|gw, bw|rx, gx|bx, ry|gy, by|rz, gz|bz, 16 bits a field).  The runs are grouped by destination dword --
// 4, 3, 2, 4, 4 and 8 slots, the most any mode needs for that dword (the busiest modes, 0x01 and 0x1E, have 20 and
// 21 runs) -- so a slot's destination dword is a constant and a run costs an alignbit on a selected dword pair, two
// bit-field extracts (one of the bit-reversed window) and a shift-or.  Unused slots have length 0.  Per-lane arrays
// are only indexed by unrolled constants, so nothing goes to scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapgpu_runtime.hpp"
#include "bptc_tables.hpp"

namespace {

// the endpoint fields: w, x of region 0, y, z of region 1; field f is bits 16 (f & 1) .. of packed dword f >> 1
enum : unsigned { RW, GW, BW, RX, GX, BX, RY, GY, BY, RZ, GZ, BZ };

// a run of `len` header bits from block bit `src` into field `f` from its bit `bit` (R: stored bit-reversed, the
// first block bit being the field's highest); Z: an unused slot; P: the mode's endpoint and delta precisions
#define S(src, len, f, bit) ((src) | ((len) << 8) | ((16u * ((f) & 1u) + (bit)) << 16) | (((f) >> 1) << 28))
#define R(src, len, f, bit) (S(src, len, f, bit) | (1u << 24))
#define Z 0u
#define P(prec, dr, dg, db, regions, transformed) \
    ((prec) | ((dr) << 8) | ((dg) << 12) | ((db) << 16) | (((regions) - 1u) << 24) | ((transformed) << 25))

constexpr unsigned ROW = 28;                               // parameters, 25 slots, 2 of padding: 7 x 16 bytes
constexpr unsigned SLOTS[6] = {4, 3, 2, 4, 4, 8};          // slots per packed endpoint dword

struct mode_table {
    uint32_t w[14][ROW];
};

// modes in the specification's order; mode index 0..13 from the mode field (mode_index)
constexpr mode_table kModes = {{
    // 0x00: 2 regions, transformed, 10-bit endpoints, deltas 5/5/5
    {P(10, 5, 5, 5, 2, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), Z, Z,
     S(25, 10, BW, 0), S(35, 5, RX, 0), Z,
     S(45, 5, GX, 0), S(55, 5, BX, 0),
     S(2, 1, GY, 4), S(41, 4, GY, 0), S(65, 5, RY, 0), Z,
     S(3, 1, BY, 4), S(61, 4, BY, 0), S(71, 5, RZ, 0), Z,
     S(4, 1, BZ, 4), S(40, 1, GZ, 4), S(50, 1, BZ, 0), S(51, 4, GZ, 0),
     S(60, 1, BZ, 1), S(70, 1, BZ, 2), S(76, 1, BZ, 3), Z, Z, Z},
    // 0x01: 2 regions, transformed, 7-bit endpoints, deltas 6/6/6
    {P(7, 6, 6, 6, 2, 1),
     S(5, 7, RW, 0), S(15, 7, GW, 0), Z, Z,
     S(25, 7, BW, 0), S(35, 6, RX, 0), Z,
     S(45, 6, GX, 0), S(55, 6, BX, 0),
     S(2, 1, GY, 5), S(24, 1, GY, 4), S(41, 4, GY, 0), S(65, 6, RY, 0),
     S(14, 1, BY, 4), S(22, 1, BY, 5), S(61, 4, BY, 0), S(71, 6, RZ, 0),
     S(3, 2, GZ, 4), S(12, 2, BZ, 0), S(23, 1, BZ, 2), S(32, 1, BZ, 3), R(33, 2, BZ, 4), S(51, 4, GZ, 0), Z, Z, Z, Z},
    // 0x02: 2 regions, transformed, 11-bit endpoints, deltas 5/4/4
    {P(11, 5, 4, 4, 2, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), S(40, 1, RW, 10), S(49, 1, GW, 10),
     S(25, 10, BW, 0), S(35, 5, RX, 0), S(59, 1, BW, 10),
     S(45, 4, GX, 0), S(55, 4, BX, 0),
     S(41, 4, GY, 0), S(65, 5, RY, 0), Z, Z,
     S(61, 4, BY, 0), S(71, 5, RZ, 0), Z, Z,
     S(50, 1, BZ, 0), S(51, 4, GZ, 0), S(60, 1, BZ, 1), S(70, 1, BZ, 2), S(76, 1, BZ, 3), Z, Z, Z, Z, Z},
    // 0x06: 2 regions, transformed, 11-bit endpoints, deltas 4/5/4
    {P(11, 4, 5, 4, 2, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), S(39, 1, RW, 10), S(50, 1, GW, 10),
     S(25, 10, BW, 0), S(35, 4, RX, 0), S(59, 1, BW, 10),
     S(45, 5, GX, 0), S(55, 4, BX, 0),
     S(41, 4, GY, 0), S(65, 4, RY, 0), S(75, 1, GY, 4), Z,
     S(61, 4, BY, 0), S(71, 4, RZ, 0), Z, Z,
     S(40, 1, GZ, 4), S(51, 4, GZ, 0), S(60, 1, BZ, 1), S(69, 1, BZ, 0),
     S(70, 1, BZ, 2), S(76, 1, BZ, 3), Z, Z, Z, Z},
    // 0x0A: 2 regions, transformed, 11-bit endpoints, deltas 4/4/5
    {P(11, 4, 4, 5, 2, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), S(39, 1, RW, 10), S(49, 1, GW, 10),
     S(25, 10, BW, 0), S(35, 4, RX, 0), S(60, 1, BW, 10),
     S(45, 4, GX, 0), S(55, 5, BX, 0),
     S(41, 4, GY, 0), S(65, 4, RY, 0), Z, Z,
     S(40, 1, BY, 4), S(61, 4, BY, 0), S(71, 4, RZ, 0), Z,
     S(50, 1, BZ, 0), S(51, 4, GZ, 0), S(69, 2, BZ, 1), R(75, 2, BZ, 3), Z, Z, Z, Z, Z, Z},
    // 0x0E: 2 regions, transformed, 9-bit endpoints, deltas 5/5/5
    {P(9, 5, 5, 5, 2, 1),
     S(5, 9, RW, 0), S(15, 9, GW, 0), Z, Z,
     S(25, 9, BW, 0), S(35, 5, RX, 0), Z,
     S(45, 5, GX, 0), S(55, 5, BX, 0),
     S(24, 1, GY, 4), S(41, 4, GY, 0), S(65, 5, RY, 0), Z,
     S(14, 1, BY, 4), S(61, 4, BY, 0), S(71, 5, RZ, 0), Z,
     S(34, 1, BZ, 4), S(40, 1, GZ, 4), S(50, 1, BZ, 0), S(51, 4, GZ, 0),
     S(60, 1, BZ, 1), S(70, 1, BZ, 2), S(76, 1, BZ, 3), Z, Z, Z},
    // 0x12: 2 regions, transformed, 8-bit endpoints, deltas 6/5/5
    {P(8, 6, 5, 5, 2, 1),
     S(5, 8, RW, 0), S(15, 8, GW, 0), Z, Z,
     S(25, 8, BW, 0), S(35, 6, RX, 0), Z,
     S(45, 5, GX, 0), S(55, 5, BX, 0),
     S(24, 1, GY, 4), S(41, 4, GY, 0), S(65, 6, RY, 0), Z,
     S(14, 1, BY, 4), S(61, 4, BY, 0), S(71, 6, RZ, 0), Z,
     S(13, 1, GZ, 4), S(23, 1, BZ, 2), S(33, 2, BZ, 3), S(50, 1, BZ, 0),
     S(51, 4, GZ, 0), S(60, 1, BZ, 1), Z, Z, Z, Z},
    // 0x16: 2 regions, transformed, 8-bit endpoints, deltas 5/6/5
    {P(8, 5, 6, 5, 2, 1),
     S(5, 8, RW, 0), S(15, 8, GW, 0), Z, Z,
     S(25, 8, BW, 0), S(35, 5, RX, 0), Z,
     S(45, 6, GX, 0), S(55, 5, BX, 0),
     R(23, 2, GY, 4), S(41, 4, GY, 0), S(65, 5, RY, 0), Z,
     S(14, 1, BY, 4), S(61, 4, BY, 0), S(71, 5, RZ, 0), Z,
     S(13, 1, BZ, 0), S(33, 1, GZ, 5), S(34, 1, BZ, 4), S(40, 1, GZ, 4),
     S(51, 4, GZ, 0), S(60, 1, BZ, 1), S(70, 1, BZ, 2), S(76, 1, BZ, 3), Z, Z},
    // 0x1A: 2 regions, transformed, 8-bit endpoints, deltas 5/5/6
    {P(8, 5, 5, 6, 2, 1),
     S(5, 8, RW, 0), S(15, 8, GW, 0), Z, Z,
     S(25, 8, BW, 0), S(35, 5, RX, 0), Z,
     S(45, 5, GX, 0), S(55, 6, BX, 0),
     S(24, 1, GY, 4), S(41, 4, GY, 0), S(65, 5, RY, 0), Z,
     S(14, 1, BY, 4), S(23, 1, BY, 5), S(61, 4, BY, 0), S(71, 5, RZ, 0),
     S(13, 1, BZ, 1), R(33, 2, BZ, 4), S(40, 1, GZ, 4), S(50, 1, BZ, 0),
     S(51, 4, GZ, 0), S(70, 1, BZ, 2), S(76, 1, BZ, 3), Z, Z, Z},
    // 0x1E: 2 regions, raw, 6-bit endpoints
    {P(6, 6, 6, 6, 2, 0),
     S(5, 6, RW, 0), S(15, 6, GW, 0), Z, Z,
     S(25, 6, BW, 0), S(35, 6, RX, 0), Z,
     S(45, 6, GX, 0), S(55, 6, BX, 0),
     S(21, 1, GY, 5), S(24, 1, GY, 4), S(41, 4, GY, 0), S(65, 6, RY, 0),
     S(14, 1, BY, 4), S(22, 1, BY, 5), S(61, 4, BY, 0), S(71, 6, RZ, 0),
     S(11, 1, GZ, 4), S(12, 2, BZ, 0), S(23, 1, BZ, 2), S(31, 1, GZ, 5),
     S(32, 1, BZ, 3), R(33, 2, BZ, 4), S(51, 4, GZ, 0), Z, Z, Z},
    // 0x03: 1 region, raw, 10-bit endpoints
    {P(10, 10, 10, 10, 1, 0),
     S(5, 10, RW, 0), S(15, 10, GW, 0), Z, Z,
     S(25, 10, BW, 0), S(35, 10, RX, 0), Z,
     S(45, 10, GX, 0), S(55, 10, BX, 0),
     Z, Z, Z, Z,
     Z, Z, Z, Z,
     Z, Z, Z, Z, Z, Z, Z, Z, Z, Z},
    // 0x07: 1 region, transformed, 11-bit endpoints, deltas 9/9/9
    {P(11, 9, 9, 9, 1, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), S(44, 1, RW, 10), S(54, 1, GW, 10),
     S(25, 10, BW, 0), S(35, 9, RX, 0), S(64, 1, BW, 10),
     S(45, 9, GX, 0), S(55, 9, BX, 0),
     Z, Z, Z, Z,
     Z, Z, Z, Z,
     Z, Z, Z, Z, Z, Z, Z, Z, Z, Z},
    // 0x0B: 1 region, transformed, 12-bit endpoints, deltas 8/8/8
    {P(12, 8, 8, 8, 1, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), R(43, 2, RW, 10), R(53, 2, GW, 10),
     S(25, 10, BW, 0), S(35, 8, RX, 0), R(63, 2, BW, 10),
     S(45, 8, GX, 0), S(55, 8, BX, 0),
     Z, Z, Z, Z,
     Z, Z, Z, Z,
     Z, Z, Z, Z, Z, Z, Z, Z, Z, Z},
    // 0x0F: 1 region, transformed, 16-bit endpoints, deltas 4/4/4
    {P(16, 4, 4, 4, 1, 1),
     S(5, 10, RW, 0), S(15, 10, GW, 0), R(39, 6, RW, 10), R(49, 6, GW, 10),
     S(25, 10, BW, 0), S(35, 4, RX, 0), R(59, 6, BW, 10),
     S(45, 4, GX, 0), S(55, 4, BX, 0),
     Z, Z, Z, Z,
     Z, Z, Z, Z,
     Z, Z, Z, Z, Z, Z, Z, Z, Z, Z},
}};

#undef S
#undef R
#undef Z
#undef P

// every run of a row sits in its destination dword's slots
constexpr bool slots_match(const mode_table &t)
{
    for (unsigned m = 0; m < 14u; m++) {
        unsigned s = 1;
        for (unsigned k = 0; k < 6u; k++)
            for (unsigned j = 0; j < SLOTS[k]; j++, s++)
                if (t.w[m][s] && (t.w[m][s] >> 28) != k)
                    return false;
    }
    return true;
}
static_assert(slots_match(kModes), "a run is in another dword's slot");

__constant__ mode_table k_modes __attribute__((aligned(16))) = kModes;

// 32 bits of the block from bit `off` (0..95)
__device__ __forceinline__ unsigned bits_at(uint4 q, unsigned off)
{
    const unsigned d = off >> 5;
    const unsigned lo = d == 0u ? q.x : d == 1u ? q.y : q.z;
    const unsigned hi = d == 0u ? q.y : d == 1u ? q.z : q.w;
    return __builtin_amdgcn_alignbit(hi, lo, off & 31u);
}

// the bits of one run, shifted to their place in the packed endpoint dword
__device__ __forceinline__ unsigned run(uint4 q, unsigned s)
{
    const unsigned len = __builtin_amdgcn_ubfe(s, 8u, 5u);
    const unsigned win = bits_at(q, s & 127u);
    const unsigned fwd = __builtin_amdgcn_ubfe(win, 0u, len);
    const unsigned rev = __builtin_amdgcn_ubfe(__builtin_bitreverse32(win), 32u - len, len);
    return (s & (1u << 24) ? rev : fwd) << __builtin_amdgcn_ubfe(s, 16u, 5u);
}

// an endpoint of `prec` bits (sign-extended if SIGNED) -> 16 bits
template <bool SIGNED>
__device__ __forceinline__ int unquantize(int v, unsigned prec)
{
    if (!SIGNED) {
        const unsigned u = (((unsigned)v << 16) + 0x8000u) >> prec;
        return prec >= 15u ? v : v == 0 ? 0 : v == (int)((1u << prec) - 1u) ? 0xFFFF : (int)u;
    }
    const int mag = v < 0 ? -v : v;
    const int u = ((mag << 15) + 0x4000) >> (prec - 1u);
    const int r = mag == 0 ? 0 : mag >= (1 << (prec - 1u)) - 1 ? 0x7FFF : u;
    return prec >= 16u ? v : v < 0 ? -r : r;
}

// an interpolated value -> half-float bit pattern
template <bool SIGNED>
__device__ __forceinline__ unsigned finish(int v)
{
    if (!SIGNED)
        return ((unsigned)v * 31u) >> 6;
    return (v < 0 ? 0x8000u : 0u) | (((unsigned)(v < 0 ? -v : v) * 31u) >> 5);
}

// weight of index `i` from a 16-byte table t0..t3
__device__ __forceinline__ int weight(uint4 t, unsigned i)
{
    const unsigned lo = __builtin_amdgcn_perm(t.y, t.x, i & 7u), hi = __builtin_amdgcn_perm(t.w, t.z, i & 7u);
    return (int)((i & 8u ? hi : lo) & 0xFFu);
}

template <bool SIGNED>
__device__ __forceinline__ void bc6h_decode_body(const uint8_t *__restrict__ blocks, unsigned blocks_x,
                                                 unsigned blocks_total, uint8_t *__restrict__ rgbah, size_t row_bytes)
{
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= blocks_total)
        return;
    const unsigned by = id / blocks_x, bx = id - by * blocks_x;
    const uint4 q = *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);

    // ---- the mode: 2 bits (00, 01) or 5 (xxx10: 0x02..0x1A; xxx11: 0x03..0x0F, then the reserved 0x13..0x1F)
    const unsigned low2 = q.x & 3u, high3 = __builtin_amdgcn_ubfe(q.x, 2u, 3u);
    const unsigned mode = low2 < 2u ? low2 : low2 == 2u ? 2u + high3 : 10u + high3;
    const bool reserved = mode >= 14u;
    const uint4 *row = reinterpret_cast<const uint4 *>(k_modes.w[reserved ? 0u : mode]);
    uint4 d4[ROW / 4u];
#pragma unroll
    for (unsigned j = 0; j < ROW / 4u; j++)
        d4[j] = row[j];
    const unsigned *desc = reinterpret_cast<const unsigned *>(d4);

    // ---- the endpoint fields: the runs of each packed dword's slots
    unsigned e[6];
#pragma unroll
    for (unsigned k = 0, s = 1; k < 6u; k++) {
        e[k] = 0u;
#pragma unroll
        for (unsigned j = 0; j < SLOTS[k]; j++, s++)
            e[k] |= run(q, desc[s]);
    }
    const unsigned par = desc[0];
    const unsigned prec = par & 31u, mask = (1u << prec) - 1u;
    const bool two = (par >> 24) & 1u, transformed = (par >> 25) & 1u;

    // ---- resolve (base + delta), unquantise; per region and channel: 64 * e0 + 32 and e1 - e0 (zeros if reserved)
    int base[2][3], diff[2][3];
#pragma unroll
    for (unsigned c = 0; c < 3u; c++) {
        const unsigned dbits = __builtin_amdgcn_ubfe(par, 8u + 4u * c, 4u);
        const int w = (int)__builtin_amdgcn_ubfe(e[c >> 1], 16u * (c & 1u), 16u);   // rw, gw, bw: fields 0..2
        int ep[4];
#pragma unroll
        for (unsigned k = 0; k < 4u; k++) {
            const unsigned f = 3u * k + c;
            const int raw = (int)__builtin_amdgcn_ubfe(e[f >> 1], 16u * (f & 1u), 16u);
            const int delta = __builtin_amdgcn_sbfe(raw, 0u, dbits);
            int v = k == 0u || !transformed ? raw : (int)(((unsigned)w + (unsigned)delta) & mask);
            if (SIGNED)
                v = __builtin_amdgcn_sbfe(v, 0u, prec);
            ep[k] = reserved ? 0 : unquantize<SIGNED>(v, prec);
        }
#pragma unroll
        for (unsigned r = 0; r < 2u; r++) {
            base[r][c] = 64 * ep[2u * r] + 32;
            diff[r][c] = ep[2u * r + 1u] - ep[2u * r];
        }
    }

    // ---- partition, anchor and the index bits: two regions 46 bits from bit 82 (3 a texel), one region 63 bits from
    // bit 65 (4 a texel); one bit fewer at texel 0 and at the second region's anchor
    const unsigned partition = __builtin_amdgcn_ubfe(q.z, 13u, 5u);
    const unsigned map = two ? k_partitions[partition] : 0u;
    const unsigned anchor = two ? (unsigned)k_anchors[partition] : 16u;
    const unsigned ib = two ? 3u : 4u;
    const unsigned at = two ? 18u : 1u;                              // bit 82 / 65 of the block in q.z
    const uint64_t x = (uint64_t)__builtin_amdgcn_alignbit(q.w, q.z, at) | ((uint64_t)(q.w >> at) << 32);
    const uint4 w3 = make_uint4(0x1B120900u, 0x40372E25u, 0u, 0u);
    const uint4 w4 = make_uint4(0x0D090400u, 0x1E1A1511u, 0x2F2B2622u, 0x403C3733u);
    const uint4 wt = two ? w3 : w4;

    uint8_t *dst = rgbah + (size_t)(4u * by) * row_bytes + 32u * (size_t)bx;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
#pragma unroll
    for (unsigned r = 0; r < 4u; r++) {
        unsigned px[8];
#pragma unroll
        for (unsigned c = 0; c < 4u; c++) {
            const unsigned t = 4u * r + c;
            const unsigned pos = t * ib - (t ? 1u : 0u) - (t > anchor ? 1u : 0u);
            const unsigned bits = ib - (t ? 0u : 1u) - (t == anchor ? 1u : 0u);
            const unsigned i = (unsigned)(x >> pos) & ((1u << bits) - 1u);
            const int w = weight(wt, i);
            const unsigned s = (map >> (2u * t)) & 1u;
            unsigned h[3];
#pragma unroll
            for (unsigned ch = 0; ch < 3u; ch++)
                h[ch] = finish<SIGNED>(((s ? base[1][ch] : base[0][ch]) + w * (s ? diff[1][ch] : diff[0][ch])) >> 6);
            px[2u * c] = h[0] | (h[1] << 16);
            px[2u * c + 1u] = h[2] | (0x3C00u << 16);
        }
        const v4u lo = {px[0], px[1], px[2], px[3]}, hi = {px[4], px[5], px[6], px[7]};
        __builtin_nontemporal_store(lo, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
        __builtin_nontemporal_store(hi, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes + 16u));
    }
}

// pictures of one geometry in one launch: picture blockIdx.z, [textures][unused][pictures] of a HapGpuPictureTable;
// texture address 0 = not this launch's format: skip
template <bool SIGNED>
__global__ __launch_bounds__(256) void bc6h_decode_kernel(HapGpuPictureTable t, unsigned blocks_x, unsigned blocks_total,
                                                          size_t row_bytes)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    bc6h_decode_body<SIGNED>(blocks, blocks_x, blocks_total, (uint8_t *)picture_address(t, 2), row_bytes);
}

} // namespace

// RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT of hapgpu_k_block_decode (bc_decode.hip): RGBA16F pictures
void hapgpu_launch_bc6h_decode(const HapGpuPictureTable &t, unsigned pictures, bool is_signed, unsigned bx, unsigned by,
                               size_t row_bytes, hipStream_t stream)
{
    const unsigned total = bx * by;
    const dim3 grid((total + 255u) / 256u, 1, pictures), block(256);
    if (is_signed)
        hipLaunchKernelGGL(bc6h_decode_kernel<true>, grid, block, 0, stream, t, bx, total, row_bytes);
    else
        hipLaunchKernelGGL(bc6h_decode_kernel<false>, grid, block, 0, stream, t, bx, total, row_bytes);
}
