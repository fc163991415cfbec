// bc_composite.hip -- layers of DXT1 / DXT5 / scaled YCoCg-DXT5 (+ RGTC1 alpha plane) textures composited "over" a
// background colour to one RGBA8 picture per output frame, for gfx950, without the layers' decoded pictures in between.
//
// The decoder's body (bc_decode_texels.hpp, IN_REGISTERS) leaves a block's sixteen texels in registers, bit for bit what
// hapgpu_k_block_decode would have stored; this kernel blends them into a canvas block it keeps in registers
// (composite_blend.hpp: the definition) and stores the canvas after the last layer.  Mapping: bc_decode.hip's -- one
// block per lane, consecutive lanes consecutive blocks of a block row, output picture blockIdx.z, 256 lanes per
// workgroup, four 16-byte row stores per lane (1 KiB contiguous per wave-instruction).  Traffic per block and layer:
// 8 / 16 (+ 8) bytes of texture read; per block 64 bytes written, once.
//
// A picture's layers are HapGpuCompositeLayer descriptors [pictures][layers] in device memory.  Their address depends
// on blockIdx.z alone, so a descriptor is scalar loads and the choice among the six decoder bodies a uniform branch;
// layers of one picture may differ in format.  The canvas is held as two registers per texel, R | B << 16 and
// G | A << 16, the packed 16-bit lanes the blend works in: it is unpacked once, from the background, and packed once,
// for the stores.  Per texel and layer: two v_perm_b32 spread the layer's texel the same way (with 255 in A's lane --
// composite_blend.hpp), a shift and a 24-bit multiply-add make a = rdiv255(As * o), a v_perm_b32 doubles it, a
// subtraction makes 255 - a, and each of the two pairs costs a packed multiply-add, a second one, and shift, add,
// shift for rdiv255 -- sixteen instructions.  Wave-uniform shortcuts, exact: a layer of opacity 0 is not loaded; a
// layer without alpha (DXT1, YCoCg-DXT5 without a plane: As = 255, so a = o) skips the four instructions of a per
// texel, and at opacity 255 replaces the canvas.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_composite_canvas.hpp"
#include "hapgpu_runtime.hpp"

namespace {

// (the canvas block, a layer's texels and the blend: bc_composite_canvas.hpp, shared with bc_composite_encode.hip)
using namespace hapbc::canvas;

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// One launch for `gridDim.z` output pictures of one geometry.  layers: [pictures][layer_count]; outputs: the pictures'
// addresses.  An output address of 0, or a texture address of 0 in any layer, skips the picture.
// background: R | G << 8 | B << 16 | A << 24, taken as it is.
__global__ __launch_bounds__(256) void bc_composite_kernel(const HapGpuCompositeLayer *__restrict__ layers,
                                                           unsigned layer_count, const uint64_t *__restrict__ outputs,
                                                           unsigned background, unsigned blocks_x, unsigned blocks_total,
                                                           size_t row_bytes)
{
    const HapGpuCompositeLayer *mine = layers + (size_t)blockIdx.z * layer_count;
    uint8_t *rgba = (uint8_t *)outputs[blockIdx.z];
    if (!rgba)
        return;                     // (the whole workgroup: blockIdx.z is its picture)
    for (unsigned l = 0; l < layer_count; l++)
        if (!mine[l].texture)
            return;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= blocks_total)
        return;
    const unsigned by = id / blocks_x, bx = id - by * blocks_x;
    canvas_block c;
    canvas_background(c, background);
#pragma unroll 1
    for (unsigned l = 0; l < layer_count; l++) {
        // (wave-uniform: the descriptor's address is; readfirstlane says so to the branches below)
        const unsigned opacity = __builtin_amdgcn_readfirstlane(mine[l].opacity);
        if (opacity == 0u)
            continue;               // a = 0 keeps every texel: the layer is not loaded
        const unsigned format = __builtin_amdgcn_readfirstlane(mine[l].format);
        const uint8_t *blocks = (const uint8_t *)mine[l].texture, *plane = (const uint8_t *)mine[l].alpha;
        unsigned px[16];
        bool source_alpha = plane != nullptr;
        if (format == 0x83F0u) {
            if (plane)
                layer_texels<0, true>(blocks, plane, id, px);
            else
                layer_texels<0, false>(blocks, plane, id, px);
        } else if (format == 0x83F3u) {
            source_alpha = true;
            if (plane)
                layer_texels<1, true>(blocks, plane, id, px);
            else
                layer_texels<1, false>(blocks, plane, id, px);
        } else {
            if (plane)
                layer_texels<2, true>(blocks, plane, id, px);
            else
                layer_texels<2, false>(blocks, plane, id, px);
        }
        if (source_alpha)
            blend_block<true>(px, opacity, c);
        else
            blend_block<false>(px, opacity, c);
    }
    uint8_t *dst = rgba + (size_t)(4u * by) * row_bytes + 16u * (size_t)bx;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        v4u v;
#pragma unroll
        for (int k = 0; k < 4; k++)
            v[k] = canvas_texel(c, 4 * r + k);
        // (streaming stores, as the picture decoder's: written once, not read back)
        __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
    }
}

// The same for layers of sizes of their own, placed and clipped on the canvas (hap_place.h).  A layer's descriptor adds
// its clip in blocks; a lane is inside when its canvas block (bx, by) has bx - cx0 < cw and by - cy0 < ch, unsigned, and
// then the layer's block under it is first + (by - cy0) * layer_blocks_x + (bx - cx0).  Only lanes inside load, decode
// and blend: the whole of a layer's work is under that one divergent branch, so lanes outside keep their canvas
// registers -- on the "opaque at opacity 255 replaces the canvas" shortcut too, wave-uniform in its condition and
// lane-masked in its effect -- and a wave with no lane inside skips the layer's loads.  A layer of opacity 0 or with an
// empty clip is not loaded.  (The canvas and that loop are placed_canvas_block, bc_composite_canvas.hpp: the kernel that
// encodes the canvas calls it too.)
__global__ __launch_bounds__(256) void bc_composite_placed_kernel(const HapGpuPlacedLayer *__restrict__ layers,
                                                                  unsigned layer_count, const uint64_t *__restrict__ outputs,
                                                                  unsigned background, unsigned blocks_x,
                                                                  unsigned blocks_total, size_t row_bytes)
{
    const HapGpuPlacedLayer *mine = layers + (size_t)blockIdx.z * layer_count;
    uint8_t *rgba = (uint8_t *)outputs[blockIdx.z];
    if (!rgba)
        return;                     // (the whole workgroup: blockIdx.z is its picture)
    for (unsigned l = 0; l < layer_count; l++)
        if (!mine[l].texture)
            return;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= blocks_total)
        return;
    const unsigned by = id / blocks_x, bx = id - by * blocks_x;
    canvas_block c;
    placed_canvas_block(mine, layer_count, background, bx, by, c);
    uint8_t *dst = rgba + (size_t)(4u * by) * row_bytes + 16u * (size_t)bx;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        v4u v;
#pragma unroll
        for (int k = 0; k < 4; k++)
            v[k] = canvas_texel(c, 4 * r + k);
        __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + (size_t)r * row_bytes));
    }
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_composite(hapgpu_rt *rt, const HapGpuCompositeLayer *layers, unsigned layer_count,
                                        const uint64_t *outputs, unsigned pictures, const unsigned char *background,
                                        unsigned width, unsigned height, size_t row_bytes)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!layers || !outputs || !background || layer_count == 0 || layer_count > HAPGPU_COMPOSITE_LAYERS_MAX ||
        pictures == 0 || pictures > 65535u || width == 0 || height == 0 || (width & 3u) || (height & 3u) ||
        row_bytes < (size_t)width * 4u || (row_bytes & 15u) ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)
        return 1;
    const unsigned blocks_x = width / 4u, blocks_total = blocks_x * (height / 4u);
    const unsigned colour = (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16) |
                            ((unsigned)background[3] << 24);
    const dim3 grid((blocks_total + 255u) / 256u, 1, pictures);
    hipLaunchKernelGGL(bc_composite_kernel, grid, dim3(256), 0, stream, layers, layer_count, outputs, colour, blocks_x,
                       blocks_total, row_bytes);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_composite_placed(hapgpu_rt *rt, const HapGpuPlacedLayer *layers, unsigned layer_count,
                                               const uint64_t *outputs, unsigned pictures, const unsigned char *background,
                                               unsigned width, unsigned height, size_t row_bytes)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!layers || !outputs || !background || layer_count == 0 || layer_count > HAPGPU_COMPOSITE_LAYERS_MAX ||
        pictures == 0 || pictures > 65535u || width == 0 || height == 0 || (width & 3u) || (height & 3u) ||
        row_bytes < (size_t)width * 4u || (row_bytes & 15u) ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)
        return 1;
    const unsigned blocks_x = width / 4u, blocks_total = blocks_x * (height / 4u);
    const unsigned colour = (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16) |
                            ((unsigned)background[3] << 24);
    const dim3 grid((blocks_total + 255u) / 256u, 1, pictures);
    hipLaunchKernelGGL(bc_composite_placed_kernel, grid, dim3(256), 0, stream, layers, layer_count, outputs, colour,
                       blocks_x, blocks_total, row_bytes);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
