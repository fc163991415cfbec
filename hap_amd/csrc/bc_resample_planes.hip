// bc_resample_planes.hip -- a crop per picture of DXT1 / DXT5 / scaled YCoCg-DXT5 textures (+ RGTC1 alpha plane), at any
// texel position and size of the full-, half- or quarter-size picture, resized to one output size -> planar half /
// bfloat16 / float tensors for gfx950, without an RGBA8 picture in between (include/hap_gpu.h:
// HapGpuDecodeFramesPlanesResized).
//
// One workgroup of 256 lanes per 64 x 4 output tile of one picture (blockIdx.z), in two phases:
//   A  the tile's footprint -- from its first element's first tap to its last element's second tap, in texels of the
//      level (resample_taps.hpp), widened to the texture blocks that cover it -- is decoded into LDS: one block per lane,
//      256 blocks per pass, by the bodies of the picture decoders from registers to registers (bc_decode_texels.hpp,
//      IN_REGISTERS), so a texel is bit for bit what hapgpu_k_block_decode / hapgpu_k_block_decode_scaled store.  A lane
//      writes its block's rows as they are (16, 8 or 4 bytes each), consecutive lanes consecutive blocks of a block row.
//   B  after a barrier a lane takes one output element: two unsigned divisions per axis give its taps, four ds_read_b32
//      its texels, resample::blend_texel its four bytes; the conversion and the streaming stores are
//      bc_decode_planes.hip's, one element per lane and plane -- a wave is one row of the tile, 64 consecutive elements.
// No block outside the crop's blocks is read: taps never leave the crop.
//
// LDS: the footprint, row-major at a pitch of its own width (a multiple of the block's 4 >> S texels, so every phase A
// write is aligned).  With a crop of at most 4 x the output per axis, 64 elements span at most 255 texels -- 65 blocks
// at full size -- and 4 rows at most 15 texels -- 5 block rows; the tile holds 66 x 6 blocks, 264 x 24 dwords.  Phase B
// reads are ds_read_b32 (bank = dword index mod 32, conflicts inside a half wave), a half wave reading one LDS row at a
// stride of the ratio: conflict-free at ratio 1, 2-way at 2, 4-way at 4; the pitch plays no part since a wave reads one
// row per instruction.
//
// Instantiated per source format, alpha plane and level (18 kernels, as bc_decode_planes.hip); the element kind and the
// number of planes are wave-uniform branches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_texels.hpp"
#include "hapgpu_runtime.hpp"
#include "resample_taps.hpp"

namespace {

using hapbc::resample::blend_texel;
using hapbc::resample::tap;
using hapbc::resample::tap_of;
using hapbc::texels::bc_decode_body;
using hapbc::texels::bc_decode_scaled_body;
using hapbc::texels::block_in_registers;

enum { kF16 = 0, kBF16 = 1, kF32 = 2 };     // HapGpuPlaneElement
enum { kTileX = 64, kTileY = 4, kTileDwords = 264 * 24, kMaxOut = 16384, kMaxRatio = 4 };

struct plane_layout {
    size_t plane_bytes, row_bytes;
    unsigned channels, element;
    float scale[4], bias[4];
};

struct crop_rect {
    unsigned x, y, w, h;        // in texels of the level
};

// (bc_decode_planes.hip's: the definition's two roundings, the multiply and the add stay apart)
__device__ __forceinline__ float element_of(unsigned v, float scale, float bias)
{
#pragma clang fp contract(off)
    const float t = (float)v * scale;
    const float r = t + bias;
    return r;
}

template <int KIND>
__device__ __forceinline__ void store_texel(const plane_layout &l, uint8_t *planes, unsigned ox, unsigned oy, unsigned v)
{
    constexpr size_t e = KIND == kF32 ? 4u : 2u;
    uint8_t *at = planes + (size_t)oy * l.row_bytes + (size_t)ox * e;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= (int)l.channels)
            break;
        const float r = element_of((v >> (8 * c)) & 255u, l.scale[c], l.bias[c]);
        uint8_t *to = at + (size_t)c * l.plane_bytes;
        if constexpr (KIND == kF32)
            __builtin_nontemporal_store(r, reinterpret_cast<float *>(to));
        else if constexpr (KIND == kF16)
            __builtin_nontemporal_store(__builtin_bit_cast(unsigned short, (_Float16)r), reinterpret_cast<unsigned short *>(to));
        else
            __builtin_nontemporal_store(__builtin_bit_cast(unsigned short, (__bf16)r), reinterpret_cast<unsigned short *>(to));
    }
}

// FMT, HAS_ALPHA, S: bc_decode_planes.hip's.  crops: four words (x, y, w, h) per picture, or, without an array, `one` for
// all; level_w x level_h: the level's size in texels; blocks_x: blocks in a row of the texture
template <int FMT, bool HAS_ALPHA, int S>
__global__ __launch_bounds__(256) void bc_resample_planes_kernel(HapGpuPictureTable t, const uint32_t *crops, crop_rect one,
                                                                 unsigned blocks_x, unsigned level_w, unsigned level_h,
                                                                 unsigned out_w, unsigned out_h, plane_layout l)
{
    constexpr unsigned N = 4u >> S, LOG = 2u - S;
    __shared__ __attribute__((aligned(16))) unsigned tile[kTileDwords];
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    crop_rect c = one;
    if (crops) {
        const uint32_t *mine = crops + 4u * (size_t)blockIdx.z;
        c.x = mine[0], c.y = mine[1], c.w = mine[2], c.h = mine[3];
    }
    // (what the host has checked already: nothing outside the texture is read whatever the array holds)
    if (c.w == 0u || c.h == 0u || c.x > level_w || c.w > level_w - c.x || c.y > level_h || c.h > level_h - c.y ||
        c.w > (unsigned)kMaxRatio * out_w || c.h > (unsigned)kMaxRatio * out_h)
        return;
    // ---- A: the footprint's blocks to LDS
    const unsigned ox0 = blockIdx.x * (unsigned)kTileX, oy0 = blockIdx.y * (unsigned)kTileY;
    const unsigned ox1 = min(ox0 + (unsigned)kTileX, out_w) - 1u, oy1 = min(oy0 + (unsigned)kTileY, out_h) - 1u;
    const unsigned bx0 = (c.x + tap_of(ox0, out_w, c.w).i0) >> LOG, by0 = (c.y + tap_of(oy0, out_h, c.h).i0) >> LOG;
    const unsigned fbw = ((c.x + tap_of(ox1, out_w, c.w).i1) >> LOG) - bx0 + 1u;
    const unsigned fbh = ((c.y + tap_of(oy1, out_h, c.h).i1) >> LOG) - by0 + 1u;
    const unsigned pitch = fbw * N, count = fbw * fbh;
    if (pitch * fbh * N > (unsigned)kTileDwords)
        return;
    const uint8_t *alpha_blocks = HAS_ALPHA ? (const uint8_t *)picture_address(t, 1) : nullptr;
    for (unsigned first = 0; first < count; first += 256u) {
        const unsigned id = first + threadIdx.x;
        if (id >= count)
            continue;
        const unsigned fby = id / fbw, fbx = id - fby * fbw;
        const unsigned src = (by0 + fby) * blocks_x + bx0 + fbx;
        unsigned px[N * N];
        block_in_registers reg;
        if (FMT == 0) {
            const uint2 v = *reinterpret_cast<const uint2 *>(blocks + (size_t)src * 8u);
            reg.block = make_uint4(v.x, v.y, 0u, 0u);
        } else {
            reg.block = *reinterpret_cast<const uint4 *>(blocks + (size_t)src * 16u);
        }
        reg.plane = HAS_ALPHA ? *reinterpret_cast<const uint2 *>(alpha_blocks + (size_t)src * 8u) : make_uint2(0u, 0u);
        reg.texels = px;
        if constexpr (S == 0)
            bc_decode_body<FMT, HAS_ALPHA, false, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, 0u, 0u, &reg);
        else
            bc_decode_scaled_body<FMT, HAS_ALPHA, S, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, &reg);
        unsigned *at = tile + fby * N * pitch + fbx * N;
        if constexpr (S == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                *reinterpret_cast<uint4 *>(at + r * pitch) = make_uint4(px[4 * r], px[4 * r + 1], px[4 * r + 2], px[4 * r + 3]);
        } else if constexpr (S == 1) {
            *reinterpret_cast<uint2 *>(at) = make_uint2(px[0], px[1]);
            *reinterpret_cast<uint2 *>(at + pitch) = make_uint2(px[2], px[3]);
        } else {
            at[0] = px[0];
        }
    }
    __syncthreads();
    // ---- B: an output element per lane, a row of the tile per wave
    const unsigned ox = ox0 + (threadIdx.x & 63u), oy = oy0 + (threadIdx.x >> 6);
    if (ox >= out_w || oy >= out_h)
        return;
    const tap tx = tap_of(ox, out_w, c.w), ty = tap_of(oy, out_h, c.h);
    // (tile coordinates of the taps: the level's, less the footprint's first block's)
    const unsigned col0 = c.x + tx.i0 - (bx0 << LOG), col1 = c.x + tx.i1 - (bx0 << LOG);
    const unsigned *row0 = tile + (c.y + ty.i0 - (by0 << LOG)) * pitch, *row1 = tile + (c.y + ty.i1 - (by0 << LOG)) * pitch;
    const unsigned v = blend_texel(row0[col0], row0[col1], row1[col0], row1[col1], tx.w, ty.w);
    uint8_t *planes = (uint8_t *)picture_address(t, 2);
    if (l.element == kF16)
        store_texel<kF16>(l, planes, ox, oy, v);
    else if (l.element == kBF16)
        store_texel<kBF16>(l, planes, ox, oy, v);
    else
        store_texel<kF32>(l, planes, ox, oy, v);
}

struct launch_geometry {
    unsigned pictures, blocks_x, level_w, level_h, out_w, out_h;
    const uint32_t *crops;
    crop_rect one;
    hipStream_t stream;
};

template <int FMT, bool HAS_ALPHA, int S>
void launch(const HapGpuPictureTable &t, const launch_geometry &g, const plane_layout &l)
{
    const dim3 grid((g.out_w + kTileX - 1u) / kTileX, (g.out_h + kTileY - 1u) / kTileY, g.pictures);
    hipLaunchKernelGGL((bc_resample_planes_kernel<FMT, HAS_ALPHA, S>), grid, dim3(256), 0, g.stream, t, g.crops, g.one,
                       g.blocks_x, g.level_w, g.level_h, g.out_w, g.out_h, l);
}

template <int FMT, bool HAS_ALPHA>
void launch(const HapGpuPictureTable &t, const launch_geometry &g, const plane_layout &l, unsigned scale_log2)
{
    if (scale_log2 == 0u)
        launch<FMT, HAS_ALPHA, 0>(t, g, l);
    else if (scale_log2 == 1u)
        launch<FMT, HAS_ALPHA, 1>(t, g, l);
    else
        launch<FMT, HAS_ALPHA, 2>(t, g, l);
}

template <int FMT>
void launch(const HapGpuPictureTable &t, const launch_geometry &g, const plane_layout &l, unsigned scale_log2, bool alpha)
{
    if (alpha)
        launch<FMT, true>(t, g, l, scale_log2);
    else
        launch<FMT, false>(t, g, l, scale_log2);
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_decode_planes_resized(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                                    int with_alpha, unsigned width, unsigned height, unsigned format,
                                                    const uint32_t *crops, const unsigned *crop, unsigned out_width,
                                                    unsigned out_height, unsigned scale_log2, unsigned channels,
                                                    unsigned element_kind, size_t plane_bytes, size_t row_bytes,
                                                    const float *scale, const float *bias)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || (width & 3u) || (height & 3u) ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u || scale_log2 > 2u ||
        out_width == 0 || out_width > (unsigned)kMaxOut || out_height == 0 || out_height > (unsigned)kMaxOut ||
        element_kind > (unsigned)kF32 || channels < 3u || channels > 4u || !scale || !bias || (!crops && !crop))
        return 1;
    const unsigned level_w = width >> scale_log2, level_h = height >> scale_log2;
    crop_rect one = {0u, 0u, 0u, 0u};
    if (!crops) {
        one = crop_rect{crop[0], crop[1], crop[2], crop[3]};
        // (one crop without an array: the host can check it; an array is the caller's promise, and the kernel looks again)
        if (one.w == 0u || one.h == 0u || one.x > level_w || one.w > level_w - one.x || one.y > level_h ||
            one.h > level_h - one.y || one.w > (unsigned)kMaxRatio * out_width || one.h > (unsigned)kMaxRatio * out_height)
            return 1;
    }
    const size_t e = element_kind == (unsigned)kF32 ? 4u : 2u, pixel_row = (size_t)out_width * e;
    if (row_bytes < pixel_row || row_bytes % e || plane_bytes % e || plane_bytes < row_bytes * ((size_t)out_height - 1u) + pixel_row)
        return 1;
    plane_layout l;
    l.plane_bytes = plane_bytes;
    l.row_bytes = row_bytes;
    l.channels = channels;
    l.element = element_kind;
    for (unsigned c = 0; c < 4u; c++) {
        l.scale[c] = c < channels ? scale[c] : 0.0f;
        l.bias[c] = c < channels ? bias[c] : 0.0f;
    }
    const launch_geometry g = {pictures, width / 4u, level_w, level_h, out_width, out_height, crops, one, stream};
    switch (format) {
    case 0x83F0: launch<0>(*table, g, l, scale_log2, with_alpha != 0); break;
    case 0x83F3: launch<1>(*table, g, l, scale_log2, with_alpha != 0); break;
    case 0x01: launch<2>(*table, g, l, scale_log2, with_alpha != 0); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
