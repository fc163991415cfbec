// bc_encode_planes.hip -- planar half / bfloat16 / float tensors -> DXT1 / DXT5 / scaled YCoCg-DXT5 / RGTC1 blocks for
// gfx950, scaled and shifted per channel on the way, without an RGBA8 picture in between: bc_decode_planes.hip's way back.
//
// An element of plane c becomes the texel byte quantise(x, scale[c], bias[c]) of plane_quantise.hpp -- one binary32
// multiply, one binary32 add (not fused), then 0 for a NaN and anything not above 0, 255 from 255 up, else rounded to
// nearest, halves to even.  The sixteen packed texels R | G << 8 | B << 16 | A << 24 go to bc_encode_core.hpp's block_of:
// the blocks are byte for byte what hapgpu_k_block_encode makes of the RGBA8 picture of those bytes.
//
// Mapping: bc_encode.hip's -- one block per lane, a wavefront 64 consecutive blocks of one block row (the row's address
// is scalar, no division per lane), picture blockIdx.z of a HapGpuPictureTable.  Per plane and row a lane loads its four
// elements at once, 8 bytes (half, bfloat16) or 16 (float): a wave instruction covers 512 B or 1 KiB of one plane row.
// The tensors are read once: the loads are non-temporal.  Every plane is quantised and ORed into the sixteen texel
// registers as it arrives, so beyond those only the loads in flight are live.  Only the planes the format looks at are
// read: R, G, B for DXT1 and YCoCg-DXT5, A alone for RGTC1.  Traffic per Hap Q block from three half planes: 96 bytes
// read, 16 written, where the road over a picture reads 96, writes 64 and reads 64 again.
//
// Instantiated per destination format (5 kernels: what block_of is a template of, and what fixes the registers a lane
// holds), and once more for DXT1 and DXT5 with refined end points (HAPGPU_ENCODE_REFINE_ENDPOINTS: colour_block<true>).  The element kind is a wave-uniform branch around the loads and the quantiser, the number of planes one around
// the fourth plane: as template parameters they would make 30 kernels of the same encoder code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_encode_core.hpp"
#include "hapgpu_runtime.hpp"
#include "plane_quantise.hpp"

namespace {

using namespace hapbc;
using planes::kBF16;
using planes::kF16;
using planes::kF32;

// where the planes of a tensor lie and what becomes of an element on its way to a byte
struct plane_layout {
    size_t plane_bytes, row_bytes;
    unsigned channels, element;
    float scale[4], bias[4];
};

// the four elements of one plane row of a block, as one streaming load
template <int KIND>
__device__ __forceinline__ void load_elements(const uint8_t *at, float (&x)[4])
{
    if constexpr (KIND == kF32) {
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(at));
#pragma unroll
        for (int i = 0; i < 4; i++)
            x[i] = planes::value_of_float(v[i]);
    } else {
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        const v2u v = __builtin_nontemporal_load(reinterpret_cast<const v2u *>(at));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned short h = (unsigned short)(v[i >> 1] >> (16 * (i & 1)));
            x[i] = KIND == kF16 ? planes::value_of_half(h) : planes::value_of_bfloat(h);
        }
    }
}

// plane C of the block at `at` (its first element in plane 0), quantised into byte C of the sixteen texels
template <int KIND, int C>
__device__ __forceinline__ void gather_plane(const plane_layout &l, const uint8_t *at, unsigned (&p)[16])
{
    const float s = l.scale[C], b = l.bias[C];
    at += (size_t)C * l.plane_bytes;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float x[4];
        load_elements<KIND>(at + (size_t)r * l.row_bytes, x);
#pragma unroll
        for (int i = 0; i < 4; i++)
            p[4 * r + i] |= planes::quantise(x[i], s, b) << (8 * C);
    }
}

// the texels of block (bx, by) of a tensor from the planes FMT looks at; alpha 255 where the tensor has three planes
template <int FMT, int KIND>
__device__ __forceinline__ void gather_block(const plane_layout &l, const uint8_t *tensor, unsigned bx, unsigned by,
                                             unsigned (&p)[16])
{
    constexpr size_t e = KIND == kF32 ? 4u : 2u;
    constexpr bool colour = FMT != kFmtRGTC1, alpha = FMT != kFmtDXT1 && FMT != kFmtYCoCg;
    const uint8_t *at = tensor + (size_t)(4u * by) * l.row_bytes + (size_t)bx * (4u * e);
#pragma unroll
    for (int i = 0; i < 16; i++)
        p[i] = 0u;
    if (colour) {
        gather_plane<KIND, 0>(l, at, p);
        gather_plane<KIND, 1>(l, at, p);
        gather_plane<KIND, 2>(l, at, p);
    }
    if (alpha) {
        if (l.channels == 4u) {
            gather_plane<KIND, 3>(l, at, p);
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++)
                p[i] |= 0xFF000000u;
        }
    }
}

// Tensors of one geometry in one launch: tensor blockIdx.z, [tensors][outputs][second outputs] of a HapGpuPictureTable
// (address 0: skip).  kFmtYCoCgAlpha is Hap Q Alpha: both textures from one pass over the planes.
template <int FMT, bool REFINE = false>
__global__ __launch_bounds__(64) void bc_encode_planes_kernel(HapGpuPictureTable t, unsigned blocks_x, plane_layout l)
{
    // (before any return: every lane of the wave must hold its weight row, bc_encode_core.hpp; Hap Q Alpha keeps the
    // dot-product form -- its kernels hold the pixels for the alpha plane and would lose a wave to the result tuples)
    const unsigned ycocg_rows = FMT == kFmtYCoCg ? ycocg_weight_rows() : 0u;
    const uint8_t *tensor = (const uint8_t *)picture_address(t, 0);
    uint8_t *out = (uint8_t *)picture_address(t, 1);
    uint8_t *out2 = FMT == kFmtYCoCgAlpha ? (uint8_t *)picture_address(t, 2) : nullptr;
    if (!tensor || !out || (FMT == kFmtYCoCgAlpha && !out2))
        return;
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    const size_t id = (size_t)by * blocks_x + bx;
    unsigned p[16];
    if (l.element == (unsigned)kF16)
        gather_block<FMT, kF16>(l, tensor, bx, by, p);
    else if (l.element == (unsigned)kBF16)
        gather_block<FMT, kBF16>(l, tensor, bx, by, p);
    else
        gather_block<FMT, kF32>(l, tensor, bx, by, p);
    if (FMT == kFmtRGTC1 || FMT == kFmtDXT1) {
        const uint4 b = block_of<FMT, false, false, REFINE>(p);
        *reinterpret_cast<uint2 *>(out + id * 8u) = make_uint2(b.x, b.y);
    } else {
        *reinterpret_cast<uint4 *>(out + id * 16u) = block_of<FMT == kFmtYCoCgAlpha ? kFmtYCoCg : FMT, FMT == kFmtYCoCg, false, REFINE>(p, ycocg_rows);
        if (FMT == kFmtYCoCgAlpha) {
            const uint4 a = block_of<kFmtRGTC1>(p);
            *reinterpret_cast<uint2 *>(out2 + id * 8u) = make_uint2(a.x, a.y);
        }
    }
}

template <int FMT, bool REFINE = false>
void launch(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by, const plane_layout &l,
            hipStream_t stream)
{
    const dim3 grid((bx + 63u) / 64u, by, pictures), block(64);
    hipLaunchKernelGGL((bc_encode_planes_kernel<FMT, REFINE>), grid, block, 0, stream, t, bx, l);
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_encode_planes(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                            unsigned width, unsigned height, unsigned format, unsigned flags,
                                            unsigned channels, unsigned element_kind, size_t plane_bytes,
                                            size_t row_bytes, const float *scale, const float *bias)
{
    scoped_timing st(rt, 0);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    const int with_alpha = (flags & HAPGPU_BLOCK_ENCODE_WITH_ALPHA) != 0;
    const bool refine = (flags & HAPGPU_BLOCK_ENCODE_REFINE) != 0;      // looked at for DXT1 and DXT5, ignored otherwise
    if (element_kind > (unsigned)kF32 || channels < 3u || channels > 4u || !scale || !bias)
        return 1;
    const size_t e = element_kind == (unsigned)kF32 ? 4u : 2u, unit = 4u * e;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[1] || table->one[1]) ||
        (with_alpha && (format != 0x01 || !(table->column[2] || table->one[2]))) || pictures == 0 || pictures > 65535u ||
        width == 0 || height == 0 || (width & 3u) || (height & 3u) || height / 4u > 65535u)
        return 1;
    const size_t pixel_row = (size_t)width * e;
    if (row_bytes < pixel_row || row_bytes % unit || plane_bytes % unit ||
        plane_bytes < row_bytes * ((size_t)height - 1u) + pixel_row)
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
    const unsigned bx = width / 4u, by = height / 4u;
    switch (format) {
    case 0x83F0:
        if (refine)
            launch<kFmtDXT1, true>(*table, pictures, bx, by, l, stream);
        else
            launch<kFmtDXT1>(*table, pictures, bx, by, l, stream);
        break;
    case 0x83F3:
        if (refine)
            launch<kFmtDXT5, true>(*table, pictures, bx, by, l, stream);
        else
            launch<kFmtDXT5>(*table, pictures, bx, by, l, stream);
        break;
    case 0x01:
        if (with_alpha)
            launch<kFmtYCoCgAlpha>(*table, pictures, bx, by, l, stream);
        else
            launch<kFmtYCoCg>(*table, pictures, bx, by, l, stream);
        break;
    case 0x8DBB: launch<kFmtRGTC1>(*table, pictures, bx, by, l, stream); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
