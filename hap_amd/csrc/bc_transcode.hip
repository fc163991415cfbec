// bc_transcode.hip -- DXT1 / DXT5 / scaled YCoCg-DXT5 (+ RGTC1 alpha plane) textures -> DXT1 / DXT5 / scaled YCoCg-DXT5
// (+ RGTC1 alpha plane) textures of the same, half or quarter size for gfx950, without a picture in between.
//
// The decoder's bodies (bc_decode_texels.hpp) leave a block's texels in registers; the encoder starts from sixteen
// packed texels in registers (block_of, bc_encode_core.hpp).  This kernel joins the two (source_texels,
// bc_source_texels.hpp, gathers the 1, 2 x 2 or 4 x 4 source blocks under a destination block): what reaches the encoder is
// bit for bit what hapgpu_k_block_decode (S = 0) or hapgpu_k_block_decode_scaled (S = 1, 2) would have stored, so the
// textures are byte for byte what hapgpu_k_block_encode makes of those pictures.
//
// Mapping: bc_encode.hip's -- one destination block per lane, one wavefront per 64 destination blocks of a block row,
// blockIdx.y the destination block row, blockIdx.z the picture.  A lane reads the 1, 2x2 or 4x4 source blocks that cover
// its block: per source block row 16 / 32 / 64 contiguous bytes (DXT1 and the planes: half that), so that a
// wave-instruction covers 1 KiB or more of contiguous memory (DXT1 and planes at S = 0: 512 B, as in bc_decode.hip).
// Traffic per destination block: 4^S source blocks read, one block written -- 16 + 16 bytes for Hap Q to Hap Q at S = 0,
// where the road over a picture moves 16 + 64 + 64 + 16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_source_texels.hpp"
#include "bc_encode_core.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using namespace hapbc;
using hapbc::texels::source_texels;

__device__ __forceinline__ uint64_t transcode_address(const HapGpuTranscodeTable &t, unsigned c)
{
    return t.column[c] ? t.column[c][blockIdx.z] : t.one[c];
}

// SRC: 0 DXT1, 1 DXT5, 2 YCoCg-DXT5, HAS_ALPHA: an RGTC1 plane supplies A (bc_decode.hip's); DST: kFmtDXT1, kFmtDXT5,
// kFmtYCoCg or kFmtYCoCgAlpha, the last with the RGTC1 plane to the second outputs (bc_encode.hip's).  Pictures of one
// geometry in one launch: picture blockIdx.z, [source textures][source planes][destination textures][destination
// planes] of a HapGpuTranscodeTable; a source or destination address of 0: skip the picture.
// Ordinary stores: the second stage reads the textures again at once.  (The texels of S > 0 come out of dot products;
// what block_of's inline-asm helpers read are the bytes shifted and packed from them, never a dot product itself.)
template <int SRC, bool HAS_ALPHA, int DST, int S>
__global__ __launch_bounds__(64) void bc_transcode_kernel(HapGpuTranscodeTable t, unsigned blocks_x)
{
    // (before any return: every lane of the wave must hold its weight row, bc_encode_core.hpp; Hap Q Alpha keeps the
    // dot-product form -- its kernels hold the pixels for the alpha plane and would lose a wave to the result tuples)
    const unsigned ycocg_rows = DST == kFmtYCoCg ? ycocg_weight_rows() : 0u;
    const uint8_t *blocks = (const uint8_t *)transcode_address(t, 0);
    const uint8_t *planes = HAS_ALPHA ? (const uint8_t *)transcode_address(t, 1) : nullptr;
    uint8_t *out = (uint8_t *)transcode_address(t, 2);
    uint8_t *out2 = DST == kFmtYCoCgAlpha ? (uint8_t *)transcode_address(t, 3) : nullptr;
    if (!blocks || !out || (HAS_ALPHA && !planes) || (DST == kFmtYCoCgAlpha && !out2))
        return;
    // one wavefront per 64 destination blocks of one block row, as in bc_encode.hip
    const unsigned by = blockIdx.y, bx = blockIdx.x * 64u + threadIdx.x;
    if (bx >= blocks_x)
        return;
    unsigned p[16];
    source_texels<SRC, HAS_ALPHA, S>(blocks, planes, blocks_x << S, by, bx, p);
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

struct launch_geometry {
    unsigned pictures, blocks_x, blocks_y;      // of the destination
    hipStream_t stream;
};

template <int SRC, bool HAS_ALPHA, int DST, int S>
void launch(const HapGpuTranscodeTable &t, const launch_geometry &g)
{
    const dim3 grid((g.blocks_x + 63u) / 64u, g.blocks_y, g.pictures), block(64);
    hipLaunchKernelGGL((bc_transcode_kernel<SRC, HAS_ALPHA, DST, S>), grid, block, 0, g.stream, t, g.blocks_x);
}

template <int SRC, bool HAS_ALPHA, int DST>
void launch(const HapGpuTranscodeTable &t, const launch_geometry &g, unsigned scale_log2)
{
    if (scale_log2 == 0u)
        launch<SRC, HAS_ALPHA, DST, 0>(t, g);
    else if (scale_log2 == 1u)
        launch<SRC, HAS_ALPHA, DST, 1>(t, g);
    else
        launch<SRC, HAS_ALPHA, DST, 2>(t, g);
}

// (a destination that keeps no alpha -- DXT1, YCoCg alone -- never reads the source's plane)
template <int SRC>
void launch(const HapGpuTranscodeTable &t, const launch_geometry &g, bool alpha, unsigned scale_log2, int dst)
{
    switch (dst) {
    case kFmtDXT1: launch<SRC, false, kFmtDXT1>(t, g, scale_log2); break;
    case kFmtYCoCg: launch<SRC, false, kFmtYCoCg>(t, g, scale_log2); break;
    case kFmtDXT5:
        if (alpha)
            launch<SRC, true, kFmtDXT5>(t, g, scale_log2);
        else
            launch<SRC, false, kFmtDXT5>(t, g, scale_log2);
        break;
    default:
        if (alpha)
            launch<SRC, true, kFmtYCoCgAlpha>(t, g, scale_log2);
        else
            launch<SRC, false, kFmtYCoCgAlpha>(t, g, scale_log2);
        break;
    }
}

} // namespace

// hapgpu_abi.h.  Timed with the block encoder's class: most of its instructions are the encoder's.  Returns 0 launched,
// 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_transcode(hapgpu_rt *rt, const HapGpuTranscodeTable *table, unsigned pictures,
                                        unsigned src_format, int with_alpha, unsigned width, unsigned height,
                                        unsigned scale_log2, unsigned dst_format, int dst_with_alpha)
{
    scoped_timing st(rt, 0);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (scale_log2 > 2u)
        return 1;
    const unsigned step = 4u << scale_log2;
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) ||
        (dst_with_alpha && (dst_format != 0x01 || !(table->column[3] || table->one[3]))) || pictures == 0 ||
        pictures > 65535u || width == 0 || height == 0 || width % step || height % step || height / step > 65535u)
        return 1;
    int dst;
    switch (dst_format) {
    case 0x83F0: dst = kFmtDXT1; break;
    case 0x83F3: dst = kFmtDXT5; break;
    case 0x01: dst = dst_with_alpha ? kFmtYCoCgAlpha : kFmtYCoCg; break;
    default: return 1;
    }
    const launch_geometry g = {pictures, width / step, height / step, stream};
    switch (src_format) {
    case 0x83F0: launch<0>(*table, g, with_alpha != 0, scale_log2, dst); break;
    case 0x83F3: launch<1>(*table, g, with_alpha != 0, scale_log2, dst); break;
    case 0x01: launch<2>(*table, g, with_alpha != 0, scale_log2, dst); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 4;
}
