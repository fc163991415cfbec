// bc_source_texels.hpp -- the sixteen texels of one destination block, gathered in registers from the 1, 2 x 2 or 4 x 4
// DXT1 / DXT5 / scaled YCoCg-DXT5 source blocks (+ RGTC1 alpha plane) that cover it, by the bodies of the picture decoders
// (bc_decode_texels.hpp): bit for bit what hapgpu_k_block_decode (S = 0) or hapgpu_k_block_decode_scaled (S = 1, 2) would
// have stored there.  For the kernels that go on from texels without a picture: bc_transcode.hip hands them to the block
// encoder, bc_decode_video.hip converts them to the samples of a video picture.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_decode_texels.hpp"

namespace hapbc {
namespace texels {

// WORDS dwords from a 4 * WORDS-byte aligned (at most 16) address: 16-byte loads where there are that many bytes
template <int WORDS>
__device__ __forceinline__ void load_words(const uint8_t *__restrict__ at, unsigned (&w)[WORDS])
{
    if constexpr (WORDS == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(at);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int k = 0; k < WORDS / 4; k++) {
            const uint4 v = *reinterpret_cast<const uint4 *>(at + 16 * k);
            w[4 * k + 0] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    }
}

// What one block row of the 2^S x 2^S source blocks under a destination block gives: the texels of its 2^S blocks, block
// after block -- sixteen of the one block at S = 0, 2 x 2 ([2 * qy + qx]) of each of two at S = 1, one of each of four at
// S = 2.  first: the row's first block; the blocks (and their plane's) are contiguous and loaded together.
template <int S>
struct source_row {
    static constexpr int blocks = 1 << S, texels_per_block = 16 >> (2 * S);
};

template <int SRC, bool HAS_ALPHA, int S>
__device__ __forceinline__ void source_row_texels(const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ planes,
                                                  size_t first, unsigned (&q)[source_row<S>::blocks][source_row<S>::texels_per_block])
{
    constexpr int N = source_row<S>::blocks, BLOCK_WORDS = SRC == 0 ? 2 : 4;
    unsigned w[N * BLOCK_WORDS], a[N * 2];
    load_words<N * BLOCK_WORDS>(blocks + first * (4u * BLOCK_WORDS), w);
    if (HAS_ALPHA)
        load_words<N * 2>(planes + first * 8u, a);
#pragma unroll
    for (int i = 0; i < N; i++) {
        block_in_registers reg;
        reg.block = SRC == 0 ? make_uint4(w[2 * i], w[2 * i + 1], 0u, 0u)
                             : make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
        reg.plane = HAS_ALPHA ? make_uint2(a[2 * i], a[2 * i + 1]) : make_uint2(0u, 0u);
        reg.texels = q[i];
        // (the bodies of the picture decoders, from registers to registers: no grid, no picture)
        if constexpr (S == 0)
            bc_decode_body<SRC, HAS_ALPHA, false, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, 0u, 0u, &reg);
        else
            bc_decode_scaled_body<SRC, HAS_ALPHA, S, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, &reg);
    }
}

// The sixteen texels of destination block (bx, by), row-major: those of source block (bx, by) at S = 0, else the box
// means of the 2^S x 2^S source blocks from (bx << S, by << S) on.
template <int SRC, bool HAS_ALPHA, int S>
__device__ __forceinline__ void source_texels(const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ planes,
                                              unsigned source_blocks_x, unsigned by, unsigned bx, unsigned (&p)[16])
{
    const size_t first = (size_t)(by << S) * source_blocks_x + ((size_t)bx << S);
    unsigned q[source_row<S>::blocks][source_row<S>::texels_per_block];
    if constexpr (S == 0) {
        source_row_texels<SRC, HAS_ALPHA, 0>(blocks, planes, first, q);
#pragma unroll
        for (int k = 0; k < 16; k++)
            p[k] = q[0][k];
    } else if constexpr (S == 1) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            source_row_texels<SRC, HAS_ALPHA, 1>(blocks, planes, first + (size_t)j * source_blocks_x, q);
#pragma unroll
            for (int k = 0; k < 8; k++)       // texel (2j + qy, 2i + qx) = q[i][2 * qy + qx]
                p[8 * j + k] = q[(k & 3) >> 1][2 * (k >> 2) + (k & 1)];
        }
    } else {
        // The sixteen source blocks one block row after another, in a loop that stays one: unrolled, the compiler
        // decodes all sixteen at once (378 registers for Hap Q Alpha sources -- one wave a SIMD -- and four times the
        // code).  Row j's four texels are destination row j; which registers those are is a uniform choice.
#pragma unroll
        for (int k = 0; k < 16; k++)
            p[k] = 0u;
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            source_row_texels<SRC, HAS_ALPHA, 2>(blocks, planes, first + (size_t)j * source_blocks_x, q);
#pragma unroll
            for (int k = 0; k < 16; k++)
                p[k] = (k >> 2) == j ? q[k & 3][0] : p[k];
        }
    }
}

} // namespace texels
} // namespace hapbc
