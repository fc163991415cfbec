// bc_encode.hip -- RGBA8 -> DXT1 / DXT5 / scaled YCoCg-DXT5 / RGTC1 block compression for gfx950.
//
// Replaces the "external squish/DXT encoder" stage that clients of the reference run in front
// of HapEncode (the reference itself has none: hap.h:82-104 takes compressed texture bytes).
// The integer algorithm is the one defined by oracle/bc_oracle.c; results are bit-identical.
//
// Mapping: one 4x4 block per lane.  Lane l of a wavefront loads the 16-byte pixel row segment
// of block bx = base + l for each of the block's 4 rows, so every load instruction of a wave
// covers 1 KiB of contiguous RGBA and every store 512 B / 1 KiB of contiguous blocks: fully
// coalesced without an LDS stage.  Bounded by HBM: 64 B read + 8/16 B written per block.
// Endpoint fitting uses per-lane min/max; index selection uses v_dot4_u32_u8 to get the
// |p-c|^2 ordering of four palette entries in four instructions per pixel.
// With HAPGPU_ENCODE_REFINE_ENDPOINTS the DXT1 and DXT5 kernels are instantiations of their own (REFINE): two rounds of
// bc_refine_core.hpp behind the default colour block, about 1900 vector instructions a block instead of 480 -- those are
// bound by instruction issue, not by HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_encode_core.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using namespace hapbc;

template <int FMT, bool WIDE, bool REFINE>
__device__ __forceinline__ void encode_block(const uint8_t *__restrict__ rgba, size_t row_bytes, unsigned blocks_x,
                                             uint8_t *__restrict__ out, uint8_t *__restrict__ out2, unsigned ycocg_rows)
{
    // one wavefront per 64 blocks of one block row: the row's address is scalar, no division per lane
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    const size_t id = (size_t)by * blocks_x + bx;
    const uint8_t *src = rgba + (size_t)(4u * by) * row_bytes + 16u * bx;
    unsigned p[16];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (WIDE) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)r * row_bytes);
            p[4 * r + 0] = v.x; p[4 * r + 1] = v.y; p[4 * r + 2] = v.z; p[4 * r + 3] = v.w;
        } else {
            const unsigned *q = reinterpret_cast<const unsigned *>(src + (size_t)r * row_bytes);
            p[4 * r + 0] = q[0]; p[4 * r + 1] = q[1]; p[4 * r + 2] = q[2]; p[4 * r + 3] = q[3];
        }
    }
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

// pictures of one geometry in one launch: picture blockIdx.z, addresses from a HapGpuPictureTable (0: skip the picture).
// kFmtYCoCgAlpha is Hap Q Alpha: both textures of a picture in one pass over its RGBA (64 + 16 + 8 bytes per
// block), the RGTC1 plane to the second outputs.  REFINE (kFmtDXT1 and kFmtDXT5 only): the colour blocks with refined
// end points, HAPGPU_ENCODE_REFINE_ENDPOINTS -- kernels of their own, the others are what they were.
template <int FMT, bool WIDE, bool REFINE = false>
__global__ __launch_bounds__(64) void bc_encode_kernel(HapGpuPictureTable t, size_t row_bytes, unsigned blocks_x)
{
    // (before any return: every lane of the wave must hold its weight row, bc_encode_core.hpp; Hap Q Alpha keeps the
    // dot-product form -- its kernels hold the pixels for the alpha plane and would lose a wave to the result tuples)
    const unsigned ycocg_rows = FMT == kFmtYCoCg ? ycocg_weight_rows() : 0u;
    const uint8_t *rgba = (const uint8_t *)picture_address(t, 0);
    uint8_t *out = (uint8_t *)picture_address(t, 1);
    uint8_t *out2 = FMT == kFmtYCoCgAlpha ? (uint8_t *)picture_address(t, 2) : nullptr;
    if (!rgba || !out || (FMT == kFmtYCoCgAlpha && !out2))
        return;
    encode_block<FMT, WIDE, REFINE>(rgba, row_bytes, blocks_x, out, out2, ycocg_rows);
}

template <int FMT, bool REFINE = false>
void launch(const HapGpuPictureTable &t, unsigned pictures, size_t row_bytes, unsigned bx, unsigned by, bool wide,
            hipStream_t stream)
{
    const dim3 grid((bx + 63u) / 64u, by, pictures), block(64);
    if (wide)
        hipLaunchKernelGGL((bc_encode_kernel<FMT, true, REFINE>), grid, block, 0, stream, t, row_bytes, bx);
    else
        hipLaunchKernelGGL((bc_encode_kernel<FMT, false, REFINE>), grid, block, 0, stream, t, row_bytes, bx);
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_encode(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, unsigned width,
                                     unsigned height, size_t row_bytes, unsigned format, unsigned flags, int wide,
                                     unsigned picture_kind)
{
    const int with_alpha = (flags & HAPGPU_BLOCK_ENCODE_WITH_ALPHA) != 0;
    const bool refine = (flags & HAPGPU_BLOCK_ENCODE_REFINE) != 0;      // looked at for DXT1 and DXT5, ignored otherwise
    scoped_timing st(rt, 0);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    // BC6H is made from RGBA16F pictures and nothing else is: 8 bytes a texel, rows a multiple of 16 bytes; A8
    // pictures (alpha_plane.hip) make RGTC1 alone
    const bool half = picture_kind == HAPGPU_PICTURE_RGBA16F, plane = picture_kind == HAPGPU_PICTURE_A8;
    if (picture_kind > HAPGPU_PICTURE_A8 || half != (format == 0x8E8F || format == 0x8E8E) ||
        (plane && (format != 0x8DBB || with_alpha || height / 4u > 65535u)))
        return 1;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[1] || table->one[1]) ||
        (with_alpha && (format != 0x01 || !(table->column[2] || table->one[2]))) || pictures == 0 || pictures > 65535u ||
        width == 0 || height == 0 || (width & 3u) || (height & 3u) || row_bytes < (size_t)width * HAPGPU_PICTURE_TEXEL_BYTES(picture_kind) ||
        (row_bytes & (half ? 15u : 3u)))
        return 1;
    const HapGpuPictureTable &t = *table;
    const unsigned bx = width / 4u, by = height / 4u;
    switch (format) {
    case 0x83F0:
        if (refine)
            launch<kFmtDXT1, true>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        else
            launch<kFmtDXT1>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        break;
    case 0x83F3:
        if (refine)
            launch<kFmtDXT5, true>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        else
            launch<kFmtDXT5>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        break;
    case 0x01:
        if (with_alpha)
            launch<kFmtYCoCgAlpha>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        else
            launch<kFmtYCoCg>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        break;
    case 0x8DBB:
        if (plane)
            hapgpu_launch_alpha_encode(t, pictures, bx, by, row_bytes, wide != 0, stream);
        else
            launch<kFmtRGTC1>(t, pictures, row_bytes, bx, by, wide != 0, stream);
        break;
    case 0x8E8C: hapgpu_launch_bptc_encode(t, pictures, bx, by, row_bytes, wide != 0, stream); break;
    case 0x8E8F:
    case 0x8E8E: hapgpu_launch_bc6h_encode(t, pictures, format == 0x8E8E, bx, by, row_bytes, stream); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
