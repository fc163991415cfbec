// alpha_plane.hip -- A8 pictures (one byte a texel: mattes, masks) <-> RGTC1 textures, Hap Alpha-Only, for gfx950.
//
// The block code is alpha_block() of bc_encode_core.hpp and the alpha-style decoder of bc_decode_core.hpp, the ones
// the RGBA roads run; only the picture layout is new.  Plain streaming, no LDS: 16 B of picture + 8 B of texture per
// block.  One block per lane gives a lane 4 bytes of each picture row, so a wave-instruction moves 256 B.  Hence two
// roads in one kernel per direction:
//   wide    picture address and row pitch 16-byte aligned: a lane takes four horizontally adjacent blocks -- four
//           16-byte row accesses (1 KiB per wave-instruction) and 32 contiguous bytes of blocks; the last
//           blocks_x mod 4 blocks of a block row are taken by the lanes behind, one block each, in the same launch
//   narrow  any 4-byte aligned picture and pitch: one block per lane, dword row accesses
// A workgroup is 256 lanes of one block row (the row's address is scalar, no division per lane).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_decode_core.hpp"
#include "bc_encode_core.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using namespace hapbc;

constexpr unsigned kLanes = 256;

// 32 bytes of blocks at an 8-byte aligned address (a block row of an odd number of blocks starts 8 off 16)
struct __attribute__((aligned(8))) four_blocks {
    uint2 b[4];
};

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// lanes a block row takes: one per four blocks and one per block of the rest (WIDE), or one per block
template <bool WIDE>
__host__ __device__ __forceinline__ unsigned row_lanes(unsigned blocks_x)
{
    return WIDE ? blocks_x / 4u + (blocks_x & 3u) : blocks_x;
}

__device__ __forceinline__ uint2 encode_row_dwords(unsigned r0, unsigned r1, unsigned r2, unsigned r3)
{
    const unsigned rows[4] = {r0, r1, r2, r3};
    int a[16];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++)
            a[4 * r + c] = (int)((rows[r] >> (8 * c)) & 255u);
    return alpha_block(a);
}

template <bool WIDE>
__global__ __launch_bounds__(kLanes) void alpha_encode_kernel(HapGpuPictureTable t, size_t row_bytes, unsigned blocks_x)
{
    const uint8_t *plane = (const uint8_t *)picture_address(t, 0);
    uint8_t *out = (uint8_t *)picture_address(t, 1);
    if (!plane || !out)
        return;
    const unsigned by = blockIdx.y, lane = blockIdx.x * kLanes + threadIdx.x;
    if (lane >= row_lanes<WIDE>(blocks_x))
        return;
    const uint8_t *row = plane + (size_t)(4u * by) * row_bytes;
    uint8_t *dst = out + (size_t)by * blocks_x * 8u;
    const unsigned quads = WIDE ? blocks_x / 4u : 0u;
    if (WIDE && lane < quads) {
        uint4 v[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
            v[r] = *reinterpret_cast<const uint4 *>(row + (size_t)r * row_bytes + 16u * (size_t)lane);
        four_blocks f;
        f.b[0] = encode_row_dwords(v[0].x, v[1].x, v[2].x, v[3].x);
        f.b[1] = encode_row_dwords(v[0].y, v[1].y, v[2].y, v[3].y);
        f.b[2] = encode_row_dwords(v[0].z, v[1].z, v[2].z, v[3].z);
        f.b[3] = encode_row_dwords(v[0].w, v[1].w, v[2].w, v[3].w);
        *reinterpret_cast<four_blocks *>(dst + 32u * (size_t)lane) = f;
        return;
    }
    const unsigned bx = 4u * quads + (lane - quads);
    unsigned d[4];
#pragma unroll
    for (int r = 0; r < 4; r++)
        d[r] = *reinterpret_cast<const unsigned *>(row + (size_t)r * row_bytes + 4u * (size_t)bx);
    *reinterpret_cast<uint2 *>(dst + 8u * (size_t)bx) = encode_row_dwords(d[0], d[1], d[2], d[3]);
}

// [textures][-][pictures] of a HapGpuPictureTable; texture address 0 = not this launch's: skip
template <bool WIDE>
__global__ __launch_bounds__(kLanes) void alpha_decode_kernel(HapGpuPictureTable t, size_t row_bytes, unsigned blocks_x)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    uint8_t *plane = (uint8_t *)picture_address(t, 2);
    if (!blocks || !plane)
        return;
    const unsigned by = blockIdx.y, lane = blockIdx.x * kLanes + threadIdx.x;
    if (lane >= row_lanes<WIDE>(blocks_x))
        return;
    const uint8_t *src = blocks + (size_t)by * blocks_x * 8u;
    uint8_t *row = plane + (size_t)(4u * by) * row_bytes;
    const unsigned quads = WIDE ? blocks_x / 4u : 0u;
    if (WIDE && lane < quads) {
        const four_blocks f = *reinterpret_cast<const four_blocks *>(src + 32u * (size_t)lane);
        unsigned rows[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            decode_alpha_rows(f.b[j], rows[j]);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // streaming stores, as in bc_decode.hip: the picture is written once and not read back here
            const v4u v = {rows[0][r], rows[1][r], rows[2][r], rows[3][r]};
            __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(row + (size_t)r * row_bytes + 16u * (size_t)lane));
        }
        return;
    }
    const unsigned bx = 4u * quads + (lane - quads);
    unsigned rows[4];
    decode_alpha_rows(*reinterpret_cast<const uint2 *>(src + 8u * (size_t)bx), rows);
#pragma unroll
    for (int r = 0; r < 4; r++)
        __builtin_nontemporal_store(rows[r], reinterpret_cast<unsigned *>(row + (size_t)r * row_bytes + 4u * (size_t)bx));
}

template <bool WIDE>
dim3 grid_of(unsigned pictures, unsigned bx, unsigned by)
{
    return dim3((row_lanes<WIDE>(bx) + kLanes - 1u) / kLanes, by, pictures);
}

} // namespace

// A8 pictures of hapgpu_k_block_encode (bc_encode.hip): sources and row_bytes 4-byte aligned (wide: 16), outputs 8
void hapgpu_launch_alpha_encode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                                size_t row_bytes, bool wide, hipStream_t stream)
{
    if (wide)
        hipLaunchKernelGGL(alpha_encode_kernel<true>, grid_of<true>(pictures, bx, by), dim3(kLanes), 0, stream, t, row_bytes, bx);
    else
        hipLaunchKernelGGL(alpha_encode_kernel<false>, grid_of<false>(pictures, bx, by), dim3(kLanes), 0, stream, t, row_bytes, bx);
}

// A8 pictures of hapgpu_k_block_decode (bc_decode.hip): textures 8-byte, pictures and row_bytes 4-byte aligned (wide: 16)
void hapgpu_launch_alpha_decode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                                size_t row_bytes, bool wide, hipStream_t stream)
{
    if (wide)
        hipLaunchKernelGGL(alpha_decode_kernel<true>, grid_of<true>(pictures, bx, by), dim3(kLanes), 0, stream, t, row_bytes, bx);
    else
        hipLaunchKernelGGL(alpha_decode_kernel<false>, grid_of<false>(pictures, bx, by), dim3(kLanes), 0, stream, t, row_bytes, bx);
}
