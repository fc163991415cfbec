// bc_decode_video.hip -- DXT1 / DXT5 / scaled YCoCg-DXT5 textures -> NV12 video pictures (a Y plane and a half-size plane
// of interleaved Cb, Cr pairs: what a video encoder or a network sender takes) of the same, half or quarter size for
// gfx950, without an RGBA8 picture in between.  The way back of bc_encode_video.hip.
//
// The sixteen texels of a destination block are source_texels' (bc_source_texels.hpp): bit for bit what
// hapgpu_k_block_decode (S = 0) or hapgpu_k_block_decode_scaled (S = 1, 2) would have stored there.  rgb_ycbcr.hpp makes
// sixteen Y samples and 2 x 2 Cb, Cr pairs of them -- integers, one rounding each, every pair from the sums of its 2 x 2
// texels: nothing outside the block is looked at.  Alpha is never read: no instantiation takes the RGTC1 plane.
//
// Mapping: bc_transcode.hip's -- one destination block per lane, one wavefront per 64 destination blocks of a block row
// (the rows' addresses are scalar, no division per lane), blockIdx.y the destination block row, blockIdx.z the picture of
// a HapGpuPictureTable whose columns are [textures][CbCr planes][Y planes].  A lane stores one dword to each of its four
// Y rows and one dword (two pairs) to each of its two chroma rows: a wave instruction covers 256 B of one row.  The planes
// are written once and not read back: the stores are non-temporal.
// Traffic per destination block: 4^S source blocks read, 24 bytes written -- 16 + 24 for Hap Q at S = 0, where the road
// over a picture moves 16 + 64 + 64 + 24.  The matrix and the range are the launch's: nine integers are kernel
// arguments, and nothing branches on them.
//
// Instantiated per source format and size: 3 x 3.  No atomics, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_source_texels.hpp"
#include "hapgpu_runtime.hpp"
#include "rgb_ycbcr.hpp"

namespace {

using namespace hapbc;
using hapbc::texels::source_texels;

// where the rows of the two planes lie and what becomes of a texel on its way to a sample
struct video_layout {
    size_t luma_row_bytes, chroma_row_bytes;
    video::sample_coefficients k;
};

// SRC: 0 DXT1, 1 DXT5, 2 YCoCg-DXT5.  Pictures of one geometry in one launch: picture blockIdx.z, [textures][CbCr
// planes][Y planes] of a HapGpuPictureTable (address 0: skip).  blocks_x: of the destination.
template <int SRC, int S>
__global__ __launch_bounds__(64) void bc_decode_video_kernel(HapGpuPictureTable t, unsigned blocks_x, video_layout l)
{
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    uint8_t *chroma = (uint8_t *)picture_address(t, 1);
    uint8_t *luma = (uint8_t *)picture_address(t, 2);
    if (!blocks || !chroma || !luma)
        return;
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    unsigned p[16], y[4], c[2];
    source_texels<SRC, false, S>(blocks, nullptr, blocks_x << S, by, bx, p);
    video::samples_of_block(p, l.k, y, c);
    uint8_t *ya = luma + (size_t)(4u * by) * l.luma_row_bytes + (size_t)bx * 4u;
    uint8_t *ca = chroma + (size_t)(2u * by) * l.chroma_row_bytes + (size_t)bx * 4u;
#pragma unroll
    for (int r = 0; r < 4; r++)
        __builtin_nontemporal_store(y[r], reinterpret_cast<unsigned *>(ya + (size_t)r * l.luma_row_bytes));
#pragma unroll
    for (int r = 0; r < 2; r++)
        __builtin_nontemporal_store(c[r], reinterpret_cast<unsigned *>(ca + (size_t)r * l.chroma_row_bytes));
}

template <int SRC, int S>
void launch(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by, const video_layout &l,
            hipStream_t stream)
{
    const dim3 grid((bx + 63u) / 64u, by, pictures), block(64);
    hipLaunchKernelGGL((bc_decode_video_kernel<SRC, S>), grid, block, 0, stream, t, bx, l);
}

template <int SRC>
void launch(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by, const video_layout &l,
            hipStream_t stream, unsigned scale_log2)
{
    if (scale_log2 == 0u)
        launch<SRC, 0>(t, pictures, bx, by, l, stream);
    else if (scale_log2 == 1u)
        launch<SRC, 1>(t, pictures, bx, by, l, stream);
    else
        launch<SRC, 2>(t, pictures, bx, by, l, stream);
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_decode_video(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                           unsigned width, unsigned height, unsigned format, unsigned scale_log2,
                                           size_t luma_row_bytes, size_t chroma_row_bytes, unsigned matrix,
                                           unsigned range)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (scale_log2 > 2u || matrix > 1u || range > 1u)
        return 1;
    const unsigned step = 4u << scale_log2;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[1] || table->one[1]) ||
        !(table->column[2] || table->one[2]) || pictures == 0 || pictures > 65535u || width == 0 || height == 0 ||
        width % step || height % step || height / step > 65535u)
        return 1;
    // (width / 2 pairs of two bytes: a chroma row is as long as a luma row)
    const unsigned out_width = width >> scale_log2;
    if (luma_row_bytes < out_width || chroma_row_bytes < out_width || (luma_row_bytes & 3u) || (chroma_row_bytes & 3u))
        return 1;
    video_layout l;
    l.luma_row_bytes = luma_row_bytes;
    l.chroma_row_bytes = chroma_row_bytes;
    l.k = video::sample_coefficients_of(matrix, range);
    const unsigned bx = width / step, by = height / step;
    switch (format) {
    case 0x83F0: launch<0>(*table, pictures, bx, by, l, stream, scale_log2); break;
    case 0x83F3: launch<1>(*table, pictures, bx, by, l, stream, scale_log2); break;
    case 0x01: launch<2>(*table, pictures, bx, by, l, stream, scale_log2); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
