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
// The per-lane bodies of all of them are in bc_decode_texels.hpp, which bc_transcode.hip shares; here are the kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_texels.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using namespace hapbc::texels;      // bc_decode_body, bc_decode_scaled_body: a block's texels, shared with bc_transcode.hip

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
