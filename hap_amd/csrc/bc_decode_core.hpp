// bc_decode_core.hpp -- the decoder of 8-byte alpha-style blocks (S3TC alpha / RGTC1: two endpoints, 16 x 3-bit codes):
// one palette and code-word routine, and the three shapes its 16 values are wanted in.  Shared by bc_decode.hip (DXT5
// alpha, Hap Q luma, Hap Q Alpha's plane) and alpha_plane.hip (RGTC1 -> A8 pictures).  Arithmetic follows
// oracle/bc_oracle.c (obc_decode_rgtc1) exactly; results are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hapbc {

// the 8-entry palette of a block packed into two dwords (entry e = byte e of hi:lo) and its 48 code bits: texels 0..7
// in lo24, 8..15 in hi24, three bits each
struct alpha_table {
    unsigned lo, hi, lo24, hi24;
};

__device__ __forceinline__ alpha_table alpha_table_of(uint2 blk)
{
    const int a0 = (int)(blk.x & 255u), a1 = (int)((blk.x >> 8) & 255u);
    int v[8];
    v[0] = a0;
    v[1] = a1;
    if (a0 > a1) {
#pragma unroll
        for (int i = 1; i < 7; i++)
            v[i + 1] = (int)(__umul24((unsigned)((7 - i) * a0 + i * a1), 9363u) >> 16);     // / 7, exact below 13107
    } else {
#pragma unroll
        for (int i = 1; i < 5; i++)
            v[i + 1] = (int)(__umul24((unsigned)((5 - i) * a0 + i * a1), 13108u) >> 16);    // / 5, exact below 3277
        v[6] = 0;
        v[7] = 255;
    }
    alpha_table t;
    t.lo = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    t.hi = (unsigned)v[4] | ((unsigned)v[5] << 8) | ((unsigned)v[6] << 16) | ((unsigned)v[7] << 24);
    // 48 index bits = blk.x[16..31] | blk.y << 16
    t.lo24 = (blk.x >> 16) | ((blk.y & 0xFFu) << 16);
    t.hi24 = blk.y >> 8;
    return t;
}

// 16 values, one per int: every texel picks its byte of the table with one v_perm_b32
__device__ __forceinline__ void decode_alpha(uint2 blk, int (&out)[16])
{
    const alpha_table t = alpha_table_of(blk);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        out[i] = (int)(__builtin_amdgcn_perm(t.hi, t.lo, (t.lo24 >> (3 * i)) & 7u) & 0xFFu);
        out[8 + i] = (int)(__builtin_amdgcn_perm(t.hi, t.lo, (t.hi24 >> (3 * i)) & 7u) & 0xFFu);
    }
}

// The same 16 values as packed pairs (texel 2m in the low half, 2m + 1 in the high half of pairs[m]): one v_perm_b32
// fetches two palette bytes, the second selector byte of each half (0x0c) reads as zero
__device__ __forceinline__ void decode_alpha_pairs(uint2 blk, unsigned (&pairs)[8])
{
    const alpha_table t = alpha_table_of(blk);
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const unsigned c_lo = (t.lo24 >> (6 * m)) & 63u, c_hi = (t.hi24 >> (6 * m)) & 63u;     // two 3-bit codes each
        pairs[m] = __builtin_amdgcn_perm(t.hi, t.lo, ((c_lo | (c_lo << 13)) & 0x00070007u) | 0x0c000c00u);
        pairs[4 + m] = __builtin_amdgcn_perm(t.hi, t.lo, ((c_hi | (c_hi << 13)) & 0x00070007u) | 0x0c000c00u);
    }
}

// ... and as the block's four rows of four bytes (texel 4r + c in byte c of rows[r]): the four codes of a row, spread
// to the four selector bytes, fetch the whole row with one v_perm_b32
__device__ __forceinline__ void decode_alpha_rows(uint2 blk, unsigned (&rows)[4])
{
    const alpha_table t = alpha_table_of(blk);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const unsigned c = ((r < 2 ? t.lo24 : t.hi24) >> (12 * (r & 1))) & 0xFFFu;            // four 3-bit codes
        const unsigned even = (c | (c << 10)) & 0x00070007u;                                     // texels 0 and 2
        const unsigned odd = ((c >> 3) | (c << 7)) & 0x00070007u;                                // texels 1 and 3
        rows[r] = __builtin_amdgcn_perm(t.hi, t.lo, even | (odd << 8));
    }
}

} // namespace hapbc
