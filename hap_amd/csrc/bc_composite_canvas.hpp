// bc_composite_canvas.hpp -- the canvas block of a compositing kernel, in registers: what bc_composite.hip stores as an
// RGBA8 picture and bc_composite_encode.hip hands to the block encoder.  One definition of the canvas for both, so the
// two cannot differ in a bit.
//
// The decoder's body (bc_decode_texels.hpp, IN_REGISTERS) leaves a layer's block as sixteen texels in registers;
// blend_block takes them into the canvas block by composite_blend.hpp's formulas.  The canvas is held as two registers
// per texel, R | B << 16 and G | A << 16, the packed 16-bit lanes the blend works in: it is unpacked once, from the
// background (canvas_background), and packed once, by the caller (canvas_texel).  placed_canvas_block is what the
// placed kernels share: the canvas block (bx, by) of a picture after all its placed layers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_texels.hpp"
#include "composite_blend.hpp"
#include "hapgpu_abi.h"

namespace hapbc {
namespace canvas {

using hapbc::texels::bc_decode_body;
using hapbc::texels::block_in_registers;
using namespace hapbc::composite;

// the canvas block: texel i as R | B << 16 and G | A << 16
struct canvas_block {
    unsigned rb[16], ga[16];
};

// layer `d`'s block `id` as sixteen texels R | G << 8 | B << 16 | A << 24: the body of the picture decoder, from
// registers to registers
template <int FMT, bool HAS_ALPHA>
__device__ __forceinline__ void layer_texels(const uint8_t *blocks, const uint8_t *plane, unsigned id, unsigned (&px)[16])
{
    block_in_registers reg;
    if (FMT == 0) {
        const uint2 v = *reinterpret_cast<const uint2 *>(blocks + (size_t)id * 8u);
        reg.block = make_uint4(v.x, v.y, 0u, 0u);
    } else {
        reg.block = *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);
    }
    reg.plane = HAS_ALPHA ? *reinterpret_cast<const uint2 *>(plane + (size_t)id * 8u) : make_uint2(0u, 0u);
    reg.texels = px;
    bc_decode_body<FMT, HAS_ALPHA, false, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, 0u, 0u, &reg);
}

// SOURCE_ALPHA: the layer's texels carry an alpha of their own (DXT5, an RGTC1 plane); else As = 255 and a = o
template <bool SOURCE_ALPHA>
__device__ __forceinline__ void blend_block(const unsigned (&px)[16], unsigned opacity, canvas_block &c)
{
    const unsigned o257 = opacity_scaled(opacity);
    if (!SOURCE_ALPHA && opacity == 255u) {
        // a = 255 replaces the texel
#pragma unroll
        for (int i = 0; i < 16; i++) {
            c.rb[i] = __builtin_amdgcn_perm(0u, px[i], 0x0c020c00u);          // R . B .
            c.ga[i] = __builtin_amdgcn_perm(0u, px[i], 0x0c0d0c01u);          // G . 255 .
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const unsigned rb = __builtin_amdgcn_perm(0u, px[i], 0x0c020c00u);    // Rs . Bs .
        const unsigned ga = __builtin_amdgcn_perm(0u, px[i], 0x0c0d0c01u);    // Gs . 255 .: the canvas's alpha as a colour
        // (As * o257 + 32896 < 2^24: a 24-bit multiply-add, a in byte 2; without source alpha a scalar)
        const unsigned m = layer_alpha_in_byte_2(SOURCE_ALPHA ? px[i] >> 24 : 255u, o257);
        const unsigned a2 = __builtin_amdgcn_perm(0u, m, 0x0c020c02u);        // a . a .
        const unsigned inv2 = 0x00FF00FFu - a2;
        c.rb[i] = as_dword(blend_pair(as_pk_u16(rb), as_pk_u16(c.rb[i]), as_pk_u16(a2), as_pk_u16(inv2)));
        c.ga[i] = as_dword(blend_pair(as_pk_u16(ga), as_pk_u16(c.ga[i]), as_pk_u16(a2), as_pk_u16(inv2)));
    }
}

// every texel of the canvas block as the background, R | G << 8 | B << 16 | A << 24 taken as it is
__device__ __forceinline__ void canvas_background(canvas_block &c, unsigned background)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        c.rb[i] = (background & 0xFFu) | ((background & 0x00FF0000u));
        c.ga[i] = ((background >> 8) & 0xFFu) | ((background >> 8) & 0x00FF0000u);
    }
}

// texel i of the canvas block, packed for a store or for the encoder: R | G << 8 | B << 16 | A << 24
__device__ __forceinline__ unsigned canvas_texel(const canvas_block &c, int i)
{
    return __builtin_amdgcn_perm(c.ga[i], c.rb[i], 0x06020400u);             // R G B A
}

// The canvas block (bx, by) of the picture whose placed layers are mine[0 .. layer_count), bottom to top, after all of
// them have gone over `background` (hap_place.h).  A lane is inside a layer when bx - cx0 < cw and by - cy0 < ch,
// unsigned, and then the layer's block under it is first + (by - cy0) * layer_blocks_x + (bx - cx0).  Only lanes inside
// load, decode and blend: the whole of a layer's work is under that one divergent branch, so lanes outside keep their
// canvas registers -- on the "opaque at opacity 255 replaces the canvas" shortcut too, wave-uniform in its condition and
// lane-masked in its effect -- and a wave with no lane inside skips the layer's loads.  A layer of opacity 0 or with an
// empty clip is not loaded.  `mine` is wave-uniform: its address depends on the picture alone.
__device__ __forceinline__ void placed_canvas_block(const HapGpuPlacedLayer *mine, unsigned layer_count, unsigned background,
                                                    unsigned bx, unsigned by, canvas_block &c)
{
    canvas_background(c, background);
#pragma unroll 1
    for (unsigned l = 0; l < layer_count; l++) {
        // (wave-uniform: the descriptor's address is; readfirstlane says so to the branches below)
        const unsigned opacity = __builtin_amdgcn_readfirstlane(mine[l].opacity);
        const unsigned cw = __builtin_amdgcn_readfirstlane(mine[l].cw);
        if (opacity == 0u || cw == 0u)
            continue;               // a = 0 keeps every texel, an empty clip covers none: the layer is not loaded
        const unsigned format = __builtin_amdgcn_readfirstlane(mine[l].format);
        const unsigned ux = bx - __builtin_amdgcn_readfirstlane(mine[l].cx0);
        const unsigned uy = by - __builtin_amdgcn_readfirstlane(mine[l].cy0);
        const uint8_t *blocks = (const uint8_t *)mine[l].texture, *plane = (const uint8_t *)mine[l].alpha;
        if (ux < cw && uy < __builtin_amdgcn_readfirstlane(mine[l].ch)) {
            const unsigned lid = __builtin_amdgcn_readfirstlane(mine[l].first) +
                                 uy * __builtin_amdgcn_readfirstlane(mine[l].layer_blocks_x) + ux;
            unsigned px[16];
            bool source_alpha = plane != nullptr;
            if (format == 0x83F0u) {
                if (plane)
                    layer_texels<0, true>(blocks, plane, lid, px);
                else
                    layer_texels<0, false>(blocks, plane, lid, px);
            } else if (format == 0x83F3u) {
                source_alpha = true;
                if (plane)
                    layer_texels<1, true>(blocks, plane, lid, px);
                else
                    layer_texels<1, false>(blocks, plane, lid, px);
            } else {
                if (plane)
                    layer_texels<2, true>(blocks, plane, lid, px);
                else
                    layer_texels<2, false>(blocks, plane, lid, px);
            }
            if (source_alpha)
                blend_block<true>(px, opacity, c);
            else
                blend_block<false>(px, opacity, c);
        }
    }
}

} // namespace canvas
} // namespace hapbc
