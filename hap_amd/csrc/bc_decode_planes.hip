// bc_decode_planes.hip -- DXT1 / DXT5 / scaled YCoCg-DXT5 (+ RGTC1 alpha plane) -> planar half / bfloat16 / float
// tensors for gfx950, at full, half or quarter size, scaled and shifted per channel, without an RGBA8 picture in between.
//
// The decoder's bodies (bc_decode_texels.hpp, IN_REGISTERS) leave a block's 16, 4 or 1 texels in registers, bit for bit
// what hapgpu_k_block_decode (S = 0) or hapgpu_k_block_decode_scaled (S = 1, 2) would have stored; this kernel adds the
// conversion and the stores.  Element of channel c for a texel byte v:
//     t = (float)v * scale[c]    one binary32 multiply, round to nearest even
//     r = t + bias[c]            one binary32 add, round to nearest even -- NOT a fused multiply-add
//     r, or r rounded to nearest even to half (subnormal halves kept) or to bfloat16.
//
// Mapping: bc_decode.hip's -- one block per lane, consecutive lanes consecutive blocks of a block row, picture
// blockIdx.z of a HapGpuPictureTable.  A lane stores n = 4 >> S elements per output row and plane: a wave-instruction
// covers 64 * n * e contiguous bytes of one plane row (512 B for half elements at full size, 1 KiB for floats).
// Traffic per block at full size: 8 / 16 (+ 8) bytes read, 16 * channels * e written -- 16 + 96 for three half planes of
// Hap Q, where the road over a picture and torch moves 16 + 64 + 64 + 96 or more.
//
// Instantiated per source format, alpha plane and size (18 kernels: what the decode bodies are templates of, and what
// fixes the registers a lane holds), and once more for a rectangle of every texture with an origin per picture
// (hapgpu_k_block_decode_planes_region: 18 more, the same body behind another block index).  The element kind and the number of planes are wave-uniform branches around the
// conversion and the stores: as template parameters they would make 108 kernels of the same decode code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_texels.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using hapbc::texels::bc_decode_body;
using hapbc::texels::bc_decode_scaled_body;
using hapbc::texels::block_in_registers;

enum { kF16 = 0, kBF16 = 1, kF32 = 2 };     // HapGpuPlaneElement

// where the planes of a picture lie and what becomes of a texel byte on its way there
struct plane_layout {
    size_t plane_bytes, row_bytes;
    unsigned channels, element;
    float scale[4], bias[4];
};

// the definition's two roundings: the multiply and the add stay apart
__device__ __forceinline__ float element_of(unsigned v, float scale, float bias)
{
#pragma clang fp contract(off)
    const float t = (float)v * scale;
    const float r = t + bias;
    return r;
}

__device__ __forceinline__ unsigned short half_bits(float r)
{
    return __builtin_bit_cast(unsigned short, (_Float16)r);      // v_cvt_f16_f32: nearest even, subnormal halves kept
}

__device__ __forceinline__ unsigned short bfloat_bits(float r)
{
    return __builtin_bit_cast(unsigned short, (__bf16)r);        // nearest even
}

// N consecutive elements of kind KIND to `at` (N * e-byte aligned), as one streaming store: the planes are written once
// and not read back by this kernel
template <int KIND, int N>
__device__ __forceinline__ void store_elements(uint8_t *at, const float (&r)[N])
{
    if constexpr (KIND == kF32) {
        typedef float vf __attribute__((ext_vector_type(N)));
        if constexpr (N == 1) {
            __builtin_nontemporal_store(r[0], reinterpret_cast<float *>(at));
        } else {
            vf v;
#pragma unroll
            for (int i = 0; i < N; i++)
                v[i] = r[i];
            __builtin_nontemporal_store(v, reinterpret_cast<vf *>(at));
        }
    } else {
        unsigned short h[N];
#pragma unroll
        for (int i = 0; i < N; i++)
            h[i] = KIND == kF16 ? half_bits(r[i]) : bfloat_bits(r[i]);
        if constexpr (N == 1) {
            __builtin_nontemporal_store(h[0], reinterpret_cast<unsigned short *>(at));
        } else if constexpr (N == 2) {
            __builtin_nontemporal_store((unsigned)h[0] | ((unsigned)h[1] << 16), reinterpret_cast<unsigned *>(at));
        } else {
            typedef unsigned v2u __attribute__((ext_vector_type(2)));
            const v2u v = {(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
            __builtin_nontemporal_store(v, reinterpret_cast<v2u *>(at));
        }
    }
}

// The N x N texels of block (bx, by) -- packed R | G << 8 | B << 16 | A << 24, row-major -- to the planes
template <int KIND, int N>
__device__ __forceinline__ void store_planes(const plane_layout &l, uint8_t *planes, unsigned bx, unsigned by,
                                             const unsigned (&px)[N * N])
{
    constexpr size_t e = KIND == kF32 ? 4u : 2u;
    uint8_t *at = planes + (size_t)(by * (unsigned)N) * l.row_bytes + (size_t)bx * (N * e);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= (int)l.channels)
            break;
#pragma unroll
        for (int y = 0; y < N; y++) {
            float r[N];
#pragma unroll
            for (int x = 0; x < N; x++)
                r[x] = element_of((px[N * y + x] >> (8 * c)) & 255u, l.scale[c], l.bias[c]);
            store_elements<KIND, N>(at + (size_t)c * l.plane_bytes + (size_t)y * l.row_bytes, r);
        }
    }
}

// FMT: 0 DXT1, 1 DXT5, 2 YCoCg-DXT5; HAS_ALPHA: an RGTC1 plane supplies A (bc_decode.hip's); S: 0 full, 1 half, 2 quarter
// size.  Pictures of one geometry in one launch: picture blockIdx.z, [textures][alpha planes][tensors] of a
// HapGpuPictureTable; texture address 0 = not this launch's format: skip
template <int FMT, bool HAS_ALPHA, int S>
__global__ __launch_bounds__(256) void bc_decode_planes_kernel(HapGpuPictureTable t, unsigned blocks_x, unsigned blocks_total,
                                                               plane_layout l)
{
    constexpr int N = 4 >> S;
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= blocks_total)
        return;
    const unsigned by = id / blocks_x, bx = id - by * blocks_x;
    unsigned px[N * N];
    block_in_registers reg;
    if (FMT == 0) {
        const uint2 v = *reinterpret_cast<const uint2 *>(blocks + (size_t)id * 8u);
        reg.block = make_uint4(v.x, v.y, 0u, 0u);
    } else {
        reg.block = *reinterpret_cast<const uint4 *>(blocks + (size_t)id * 16u);
    }
    reg.plane = HAS_ALPHA ? *reinterpret_cast<const uint2 *>((const uint8_t *)picture_address(t, 1) + (size_t)id * 8u)
                          : make_uint2(0u, 0u);
    reg.texels = px;
    // (the bodies of the picture decoders, from registers to registers: no grid, no picture)
    if constexpr (S == 0)
        bc_decode_body<FMT, HAS_ALPHA, false, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, 0u, 0u, &reg);
    else
        bc_decode_scaled_body<FMT, HAS_ALPHA, S, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, &reg);
    uint8_t *planes = (uint8_t *)picture_address(t, 2);
    if (l.element == kF16)
        store_planes<kF16, N>(l, planes, bx, by, px);
    else if (l.element == kBF16)
        store_planes<kBF16, N>(l, planes, bx, by, px);
    else
        store_planes<kF32, N>(l, planes, bx, by, px);
}

// ... and a rectangle of every texture, a different one per picture (bc_decode.hip's bc_decode_region_kernel with an
// origin per picture): the grid covers the rectangle, lane id is block (bx, by) = (id % region_x, id / region_x) of it
// and of the rectangle's tensor, and reads texture (and alpha plane) block first + by * blocks_x + bx -- first: the
// texture block of the rectangle's upper left corner, origins[blockIdx.z] or, without an array, `origin`.  No block
// outside a picture's rectangle is read.  The body is the kernel's above behind another block index, written out again:
// routed through a shared function, the whole-frame kernels come out with the operands of their commutative adds in
// another order, and they are to stay instruction for instruction what they were.
template <int FMT, bool HAS_ALPHA, int S>
__global__ __launch_bounds__(256) void bc_decode_planes_region_kernel(HapGpuPictureTable t, const uint32_t *origins,
                                                                      unsigned origin, HapGpuRegionBlocks g, plane_layout l)
{
    constexpr int N = 4 >> S;
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= g.region_total)
        return;
    const unsigned by = id / g.region_x, bx = id - by * g.region_x;
    const unsigned src = (origins ? origins[blockIdx.z] : origin) + by * g.blocks_x + bx;
    unsigned px[N * N];
    block_in_registers reg;
    if (FMT == 0) {
        const uint2 v = *reinterpret_cast<const uint2 *>(blocks + (size_t)src * 8u);
        reg.block = make_uint4(v.x, v.y, 0u, 0u);
    } else {
        reg.block = *reinterpret_cast<const uint4 *>(blocks + (size_t)src * 16u);
    }
    reg.plane = HAS_ALPHA ? *reinterpret_cast<const uint2 *>((const uint8_t *)picture_address(t, 1) + (size_t)src * 8u)
                          : make_uint2(0u, 0u);
    reg.texels = px;
    if constexpr (S == 0)
        bc_decode_body<FMT, HAS_ALPHA, false, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, 0u, 0u, &reg);
    else
        bc_decode_scaled_body<FMT, HAS_ALPHA, S, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, &reg);
    uint8_t *planes = (uint8_t *)picture_address(t, 2);
    if (l.element == kF16)
        store_planes<kF16, N>(l, planes, bx, by, px);
    else if (l.element == kBF16)
        store_planes<kBF16, N>(l, planes, bx, by, px);
    else
        store_planes<kF32, N>(l, planes, bx, by, px);
}

struct launch_geometry {
    unsigned pictures, blocks_x, blocks_total;
    hipStream_t stream;
    bool region;                // the grid covers a rectangle: region_x, region_total, and where it begins
    unsigned region_x, region_total, origin;
    const uint32_t *origins;
};

template <int FMT, bool HAS_ALPHA, int S>
void launch(const HapGpuPictureTable &t, const launch_geometry &g, const plane_layout &l)
{
    const dim3 block(256);
    if (g.region) {
        const HapGpuRegionBlocks r = {g.blocks_x, 0u, g.region_x, g.region_total};
        hipLaunchKernelGGL((bc_decode_planes_region_kernel<FMT, HAS_ALPHA, S>), dim3((g.region_total + 255u) / 256u, 1, g.pictures),
                           block, 0, g.stream, t, g.origins, g.origin, r, l);
        return;
    }
    const dim3 grid((g.blocks_total + 255u) / 256u, 1, g.pictures);
    hipLaunchKernelGGL((bc_decode_planes_kernel<FMT, HAS_ALPHA, S>), grid, block, 0, g.stream, t, g.blocks_x, g.blocks_total, l);
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

// what both entries ask of the tensors' layout, for tensors of picture_width x picture_height elements; fills `l`
bool layout_of(plane_layout &l, unsigned picture_width, unsigned picture_height, unsigned scale_log2, unsigned channels,
               unsigned element_kind, size_t plane_bytes, size_t row_bytes, const float *scale, const float *bias)
{
    if (scale_log2 > 2u || element_kind > (unsigned)kF32 || channels < 3u || channels > 4u || !scale || !bias ||
        picture_width == 0 || picture_height == 0)
        return false;
    const size_t e = element_kind == (unsigned)kF32 ? 4u : 2u, unit = (4u >> scale_log2) * e;
    const size_t pixel_row = (size_t)picture_width * e;
    if (row_bytes < pixel_row || row_bytes % unit || plane_bytes % unit ||
        plane_bytes < row_bytes * ((size_t)picture_height - 1u) + pixel_row)
        return false;
    l.plane_bytes = plane_bytes;
    l.row_bytes = row_bytes;
    l.channels = channels;
    l.element = element_kind;
    for (unsigned c = 0; c < 4u; c++) {
        l.scale[c] = c < channels ? scale[c] : 0.0f;
        l.bias[c] = c < channels ? bias[c] : 0.0f;
    }
    return true;
}

bool launch_format(unsigned format, const HapGpuPictureTable &t, const launch_geometry &g, const plane_layout &l,
                   unsigned scale_log2, bool alpha)
{
    switch (format) {
    case 0x83F0: launch<0>(t, g, l, scale_log2, alpha); break;
    case 0x83F3: launch<1>(t, g, l, scale_log2, alpha); break;
    case 0x01: launch<2>(t, g, l, scale_log2, alpha); break;
    default: return false;
    }
    return true;
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_decode_planes(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                            int with_alpha, unsigned width, unsigned height, unsigned format,
                                            unsigned scale_log2, unsigned channels, unsigned element_kind,
                                            size_t plane_bytes, size_t row_bytes, const float *scale, const float *bias)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || (width & 3u) || (height & 3u) ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)
        return 1;
    plane_layout l;
    if (!layout_of(l, scale_log2 > 2u ? 0u : width >> scale_log2, scale_log2 > 2u ? 0u : height >> scale_log2, scale_log2,
                   channels, element_kind, plane_bytes, row_bytes, scale, bias))
        return 1;
    const launch_geometry g = {pictures, width / 4u, (width / 4u) * (height / 4u), stream, false, 0u, 0u, 0u, nullptr};
    if (!launch_format(format, *table, g, l, scale_log2, with_alpha != 0))
        return 1;
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

// hapgpu_abi.h: a rectangle of region_width x region_height of every texture, where origins[z] (or origin) says.  The same
// return codes.
extern "C" int hapgpu_k_block_decode_planes_region(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                                   int with_alpha, unsigned width, unsigned height, unsigned format,
                                                   const uint32_t *origins, unsigned origin, unsigned region_width,
                                                   unsigned region_height, unsigned scale_log2, unsigned channels,
                                                   unsigned element_kind, size_t plane_bytes, size_t row_bytes,
                                                   const float *scale, const float *bias)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || ((width | height | region_width | region_height) & 3u) || region_width == 0 || region_height == 0 ||
        region_width > width || region_height > height ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)
        return 1;
    // (one origin without an array: the host can check that the rectangle lies inside the texture; an array is the
    // caller's promise, like the table's addresses)
    if (!origins && (origin % (width / 4u) > (width - region_width) / 4u || origin / (width / 4u) > (height - region_height) / 4u))
        return 1;
    plane_layout l;
    if (!layout_of(l, scale_log2 > 2u ? 0u : region_width >> scale_log2, scale_log2 > 2u ? 0u : region_height >> scale_log2,
                   scale_log2, channels, element_kind, plane_bytes, row_bytes, scale, bias))
        return 1;
    const launch_geometry g = {pictures, width / 4u, (width / 4u) * (height / 4u), stream, true, region_width / 4u,
                               (region_width / 4u) * (region_height / 4u), origin, origins};
    if (!launch_format(format, *table, g, l, scale_log2, with_alpha != 0))
        return 1;
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
