// bc_composite_encode.hip -- layers of DXT1 / DXT5 / scaled YCoCg-DXT5 (+ RGTC1 alpha plane) textures of sizes of their
// own, placed and clipped on a canvas and composited "over" a background colour, to DXT1 / DXT5 / scaled YCoCg-DXT5
// (+ RGTC1 alpha plane) textures of the canvas for gfx950, without the canvas's picture in between.
//
// bc_composite_canvas.hpp leaves the finished canvas block in registers, bit for bit what hapgpu_k_block_composite_placed
// stores; the encoder starts from sixteen packed texels in registers (block_of, bc_encode_core.hpp).  This kernel joins
// the two as bc_transcode.hip joins decoder and encoder: the canvas is packed once, to R | G << 8 | B << 16 | A << 24,
// and handed over, so the textures are byte for byte what hapgpu_k_block_encode makes of those pictures.  The canvas
// bytes go to the encoder as they are: a premultiplied canvas, opaque where the background is.
//
// Mapping: bc_transcode.hip's -- one destination block per lane, one wavefront per 64 canvas blocks of a block row,
// blockIdx.y the block row, blockIdx.z the picture.  Traffic per canvas block: per layer that covers it 8 / 16 (+ 8)
// bytes of texture read, and one block written -- where the road over a picture writes 64 bytes and reads them again.
// The canvas (32 registers), one layer's texels and the encoder are live one after another, never together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_composite_canvas.hpp"
#include "bc_encode_core.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using namespace hapbc;
using namespace hapbc::canvas;

// DST: kFmtDXT1, kFmtDXT5, kFmtYCoCg or kFmtYCoCgAlpha, the last with the RGTC1 plane to the second outputs
// (bc_transcode.hip's).  One launch for `gridDim.z` canvases of one geometry.  layers: [pictures][layer_count];
// outputs, outputs2: the destination textures' and planes' addresses.  A destination address of 0, or a texture address
// of 0 in any layer, skips the picture.  background: R | G << 8 | B << 16 | A << 24, taken as it is.
// Ordinary stores: the second stage reads the textures again at once.
template <int DST>
__global__ __launch_bounds__(64) void bc_composite_encode_kernel(const HapGpuPlacedLayer *__restrict__ layers,
                                                                 unsigned layer_count, const uint64_t *__restrict__ outputs,
                                                                 const uint64_t *__restrict__ outputs2, unsigned background,
                                                                 unsigned blocks_x)
{
    // (before any return: every lane of the wave must hold its weight row, bc_encode_core.hpp; Hap Q Alpha keeps the
    // dot-product form, as in bc_transcode.hip)
    const unsigned ycocg_rows = DST == kFmtYCoCg ? ycocg_weight_rows() : 0u;
    const HapGpuPlacedLayer *mine = layers + (size_t)blockIdx.z * layer_count;
    uint8_t *out = (uint8_t *)outputs[blockIdx.z];
    uint8_t *out2 = DST == kFmtYCoCgAlpha ? (uint8_t *)outputs2[blockIdx.z] : nullptr;
    if (!out || (DST == kFmtYCoCgAlpha && !out2))
        return;                     // (the whole workgroup: blockIdx.z is its picture)
    for (unsigned l = 0; l < layer_count; l++)
        if (!mine[l].texture)
            return;
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    unsigned p[16];
    {
        canvas_block c;
        placed_canvas_block(mine, layer_count, background, bx, by, c);
#pragma unroll
        for (int i = 0; i < 16; i++)
            p[i] = canvas_texel(c, i);
    }
    const size_t id = (size_t)by * blocks_x + bx;
    if (DST == kFmtDXT1) {
        const uint4 b = block_of<kFmtDXT1>(p);
        *reinterpret_cast<uint2 *>(out + id * 8u) = make_uint2(b.x, b.y);
    } else {
        *reinterpret_cast<uint4 *>(out + id * 16u) = block_of<DST == kFmtYCoCgAlpha ? kFmtYCoCg : DST, DST == kFmtYCoCg>(p, ycocg_rows);
        if (DST == kFmtYCoCgAlpha) {
            const uint4 a = block_of<kFmtRGTC1>(p);
            *reinterpret_cast<uint2 *>(out2 + id * 8u) = make_uint2(a.x, a.y);
        }
    }
}

template <int DST>
void launch(hipStream_t stream, const HapGpuPlacedLayer *layers, unsigned layer_count, const uint64_t *outputs,
            const uint64_t *outputs2, unsigned pictures, unsigned colour, unsigned blocks_x, unsigned blocks_y)
{
    const dim3 grid((blocks_x + 63u) / 64u, blocks_y, pictures), block(64);
    hipLaunchKernelGGL(bc_composite_encode_kernel<DST>, grid, block, 0, stream, layers, layer_count, outputs, outputs2,
                       colour, blocks_x);
}

} // namespace

// hapgpu_abi.h.  Timed with the block encoder's class, as hapgpu_k_block_transcode.  Returns 0 launched, 1 bad
// arguments, 4 launch failure.
extern "C" int hapgpu_k_block_composite_encode(hapgpu_rt *rt, const HapGpuPlacedLayer *layers, unsigned layer_count,
                                               const uint64_t *outputs, const uint64_t *outputs2, unsigned pictures,
                                               const unsigned char *background, unsigned width, unsigned height,
                                               unsigned dst_format, int dst_with_alpha)
{
    scoped_timing st(rt, 0);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!layers || !outputs || !background || layer_count == 0 || layer_count > HAPGPU_COMPOSITE_LAYERS_MAX ||
        pictures == 0 || pictures > 65535u || width == 0 || height == 0 || (width & 3u) || (height & 3u) ||
        height / 4u > 65535u || (dst_with_alpha && (dst_format != 0x01 || !outputs2)))
        return 1;
    const unsigned blocks_x = width / 4u, blocks_y = height / 4u;
    const unsigned colour = (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16) |
                            ((unsigned)background[3] << 24);
    switch (dst_format) {
    case 0x83F0: launch<kFmtDXT1>(stream, layers, layer_count, outputs, outputs2, pictures, colour, blocks_x, blocks_y); break;
    case 0x83F3: launch<kFmtDXT5>(stream, layers, layer_count, outputs, outputs2, pictures, colour, blocks_x, blocks_y); break;
    case 0x01:
        if (dst_with_alpha)
            launch<kFmtYCoCgAlpha>(stream, layers, layer_count, outputs, outputs2, pictures, colour, blocks_x, blocks_y);
        else
            launch<kFmtYCoCg>(stream, layers, layer_count, outputs, outputs2, pictures, colour, blocks_x, blocks_y);
        break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
