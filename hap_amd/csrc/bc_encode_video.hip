// bc_encode_video.hip -- NV12 video pictures (a full-size 8-bit Y plane and a half-size plane of interleaved Cb, Cr
// pairs: what a hardware video decoder leaves in device memory) -> DXT1 / scaled YCoCg-DXT5 blocks for gfx950, converted
// to RGB on the way, without an RGBA8 picture in between.
//
// Texel (x, y) takes Y[y][x] and the pair UV[y >> 1][2 * (x >> 1)], UV[y >> 1][2 * (x >> 1) + 1]: chroma is replicated
// over its 2 x 2 luma samples, so a 4 x 4 block is exactly 4 x 4 Y samples and 2 x 2 pairs and nothing outside the block
// is looked at.  The sample becomes the texel of ycbcr_rgb.hpp -- integers, one rounding, a clamp -- and the sixteen
// packed texels R | G << 8 | B << 16 | 0xFF000000 go to bc_encode_core.hpp's block_of: the blocks are byte for byte what
// hapgpu_k_block_encode makes of the RGBA8 picture of those bytes.  Hap Q goes YCbCr -> RGB bytes -> YCoCg: a direct
// YCbCr -> YCoCg form would make other bytes.
//
// Mapping: bc_encode_planes.hip's -- one block per lane, a wavefront 64 consecutive blocks of one block row (the row's
// address is scalar, no division per lane), picture blockIdx.z of a HapGpuPictureTable whose columns are [Y planes]
// [outputs][CbCr planes].  A lane loads one dword of each of its four Y rows and one dword (two pairs) of each of its two
// chroma rows: a wave instruction covers 256 B of one row.  The planes are read once: the loads are non-temporal.
// Traffic per block: 24 bytes read, 8 (DXT1) or 16 (YCoCg-DXT5) written, where the road over a picture writes 64 and
// reads 64 again.  The matrix and the range are the launch's: five coefficients and the luma offset are kernel
// arguments, and nothing branches on them.
//
// Instantiated per destination (what block_of is a template of): DXT1, DXT1 with refined end points
// (HAPGPU_ENCODE_REFINE_ENDPOINTS: colour_block<true>), scaled YCoCg-DXT5.  No atomics, and no LDS but what the refined
// colour block keeps for itself (bc_refine_core.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_encode_core.hpp"
#include "hapgpu_runtime.hpp"
#include "ycbcr_rgb.hpp"

namespace {

using namespace hapbc;

// where the rows of the two planes lie and what becomes of a sample on its way to a texel
struct video_layout {
    size_t luma_row_bytes, chroma_row_bytes;
    video::coefficients k;
};

// the texels of block (bx, by): six streaming dword loads, then the four pairs' terms and the sixteen samples
__device__ __forceinline__ void gather_block(const video_layout &l, const uint8_t *luma, const uint8_t *chroma,
                                             unsigned bx, unsigned by, unsigned (&p)[16])
{
    const uint8_t *ya = luma + (size_t)(4u * by) * l.luma_row_bytes + (size_t)bx * 4u;
    const uint8_t *ca = chroma + (size_t)(2u * by) * l.chroma_row_bytes + (size_t)bx * 4u;
    unsigned y[4], c[2];
#pragma unroll
    for (int r = 0; r < 4; r++)
        y[r] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(ya + (size_t)r * l.luma_row_bytes));
#pragma unroll
    for (int r = 0; r < 2; r++)
        c[r] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(ca + (size_t)r * l.chroma_row_bytes));
#pragma unroll
    for (int cy = 0; cy < 2; cy++) {
#pragma unroll
        for (int cx = 0; cx < 2; cx++) {
            const video::chroma_terms t = video::chroma_of((c[cy] >> (16 * cx)) & 0xFFu, (c[cy] >> (16 * cx + 8)) & 0xFFu, l.k);
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int r = 2 * cy + dy, i = 2 * cx + dx;
                    p[4 * r + i] = video::rgba_of_luma((y[r] >> (8 * i)) & 0xFFu, t, l.k);
                }
            }
        }
    }
}

// Pictures of one geometry in one launch: picture blockIdx.z, [Y planes][outputs][CbCr planes] of a HapGpuPictureTable
// (address 0: skip).
template <int FMT, bool REFINE = false>
__global__ __launch_bounds__(64) void bc_encode_video_kernel(HapGpuPictureTable t, unsigned blocks_x, video_layout l)
{
    static_assert(FMT == kFmtDXT1 || FMT == kFmtYCoCg, "opaque pictures: Hap and Hap Q");
    // (before any return: every lane of the wave must hold its weight row, bc_encode_core.hpp)
    const unsigned ycocg_rows = FMT == kFmtYCoCg ? ycocg_weight_rows() : 0u;
    const uint8_t *luma = (const uint8_t *)picture_address(t, 0);
    uint8_t *out = (uint8_t *)picture_address(t, 1);
    const uint8_t *chroma = (const uint8_t *)picture_address(t, 2);
    if (!luma || !out || !chroma)
        return;
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    const size_t id = (size_t)by * blocks_x + bx;
    unsigned p[16];
    gather_block(l, luma, chroma, bx, by, p);
    if (FMT == kFmtDXT1) {
        const uint4 b = block_of<FMT, false, false, REFINE>(p);
        *reinterpret_cast<uint2 *>(out + id * 8u) = make_uint2(b.x, b.y);
    } else {
        *reinterpret_cast<uint4 *>(out + id * 16u) = block_of<FMT, true, false, REFINE>(p, ycocg_rows);
    }
}

template <int FMT, bool REFINE = false>
void launch(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by, const video_layout &l,
            hipStream_t stream)
{
    const dim3 grid((bx + 63u) / 64u, by, pictures), block(64);
    hipLaunchKernelGGL((bc_encode_video_kernel<FMT, REFINE>), grid, block, 0, stream, t, bx, l);
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_encode_video(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures,
                                           unsigned width, unsigned height, unsigned format, unsigned flags,
                                           size_t luma_row_bytes, size_t chroma_row_bytes, unsigned matrix,
                                           unsigned range)
{
    scoped_timing st(rt, 0);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    const bool refine = (flags & HAPGPU_BLOCK_ENCODE_REFINE) != 0;      // looked at for DXT1, ignored otherwise
    if (matrix > (unsigned)video::kBT709 || range > (unsigned)video::kFull || (flags & HAPGPU_BLOCK_ENCODE_WITH_ALPHA))
        return 1;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[1] || table->one[1]) ||
        !(table->column[2] || table->one[2]) || pictures == 0 || pictures > 65535u || width == 0 || height == 0 ||
        (width & 3u) || (height & 3u) || height / 4u > 65535u)
        return 1;
    // (width / 2 pairs of two bytes: a chroma row is as long as a luma row)
    if (luma_row_bytes < width || chroma_row_bytes < width || (luma_row_bytes & 3u) || (chroma_row_bytes & 3u))
        return 1;
    video_layout l;
    l.luma_row_bytes = luma_row_bytes;
    l.chroma_row_bytes = chroma_row_bytes;
    l.k = video::coefficients_of(matrix, range);
    const unsigned bx = width / 4u, by = height / 4u;
    switch (format) {
    case 0x83F0:
        if (refine)
            launch<kFmtDXT1, true>(*table, pictures, bx, by, l, stream);
        else
            launch<kFmtDXT1>(*table, pictures, bx, by, l, stream);
        break;
    case 0x01: launch<kFmtYCoCg>(*table, pictures, bx, by, l, stream); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
