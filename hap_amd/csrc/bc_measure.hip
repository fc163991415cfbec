// bc_measure.hip -- DXT1 / DXT5 / scaled YCoCg-DXT5 (+ RGTC1 alpha plane) textures against RGBA8 reference pictures for
// gfx950: per picture and channel the exact sums of (d - p)^2 and |d - p| over every texel, d the byte
// hapgpu_k_block_decode writes there and p the reference picture's, without the decoded picture in between.
//
// The decoder's body (bc_decode_texels.hpp, IN_REGISTERS) leaves a block's sixteen texels in registers, bit for bit what
// hapgpu_k_block_decode would have stored; this kernel loads the same 4 x 16 bytes of the reference picture and adds up.
// Mapping: bc_decode_planes.hip's -- one block per lane, consecutive lanes consecutive blocks of a block row, picture
// blockIdx.z of a HapGpuPictureTable ([textures][alpha planes][reference pictures]).  A lane loads 16 bytes of each of
// its four picture rows: a wave-instruction covers 1 KiB contiguous.  A workgroup takes kTiles = 4 consecutive tiles of
// 256 blocks, a lane one block of each, so that the adding-up across lanes is paid once per four blocks.  Traffic per
// block: 8 / 16 (+ 8) bytes of texture and 64 of the picture read, 32 bytes per 1024 blocks written.
//
// Per lane and picture row, two rounds of v_perm_b32 turn four texels into one dword per channel, for both sides; then
//     sum (d - p)^2 = dot4(d, d) + dot4(p, p) - 2 dot4(d, p)       (v_dot4_u32_u8, accumulating)
//     sum |d - p|   = sad(d, p)                                    (v_sad_u8, accumulating)
// in 32-bit registers: a block's sixteen texels give at most 16 * 255^2 = 1040400 per channel, a lane's four blocks under
// 2^22, a wave's 64 lanes under 2^28, a workgroup's 256 under 2^30.  The eight sums are added across the wave with DPP,
// across the four waves through LDS, and the workgroup stores its eight partials with one plain store:
// partials[picture][workgroup][8].  No atomics: an 8K picture has 2025 workgroups, and atomics on one address are served
// one after the other.  A second kernel, one workgroup per picture, adds a picture's partials in 64 bits in a fixed
// order: the totals depend on nothing but the texture and the picture.
//
// Instantiated per source format and alpha plane (6 kernels: what bc_decode_body is a template of).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc_decode_texels.hpp"
#include "hapgpu_runtime.hpp"

namespace {

using hapbc::texels::bc_decode_body;
using hapbc::texels::block_in_registers;

typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr unsigned kTiles = 4u;         // tiles of 256 blocks a workgroup takes: 4 * 256 * 16 * 255^2 < 2^30

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned acc)
{
    return __builtin_amdgcn_udot4(a, b, acc, false);     // v_dot4_u32_u8
}

// four texels R | G << 8 | B << 16 | A << 24 -> one dword per channel, texel i in byte i
__device__ __forceinline__ void channels_of(const unsigned (&px)[4], unsigned (&ch)[4])
{
    const unsigned rg01 = __builtin_amdgcn_perm(px[1], px[0], 0x05010400u);      // R0 R1 G0 G1
    const unsigned rg23 = __builtin_amdgcn_perm(px[3], px[2], 0x05010400u);
    const unsigned ba01 = __builtin_amdgcn_perm(px[1], px[0], 0x07030602u);      // B0 B1 A0 A1
    const unsigned ba23 = __builtin_amdgcn_perm(px[3], px[2], 0x07030602u);
    ch[0] = __builtin_amdgcn_perm(rg23, rg01, 0x05040100u);
    ch[1] = __builtin_amdgcn_perm(rg23, rg01, 0x07060302u);
    ch[2] = __builtin_amdgcn_perm(ba23, ba01, 0x05040100u);
    ch[3] = __builtin_amdgcn_perm(ba23, ba01, 0x07060302u);
}

// the sum of v over the wave's 64 lanes, in lane 63 (every lane active): within quads, rows of 16, then across the rows
__device__ __forceinline__ unsigned wave_sum_in_lane_63(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);      // quad_perm [1, 0, 3, 2]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);      // quad_perm [2, 3, 0, 1]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);     // row_half_mirror
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);     // row_mirror: every lane its row's sum
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return v;
}

// FMT: 0 DXT1, 1 DXT5, 2 YCoCg-DXT5; HAS_ALPHA: an RGTC1 plane supplies A (bc_decode.hip's).  Pictures of one geometry in
// one launch: picture blockIdx.z, [textures][alpha planes][reference pictures] of a HapGpuPictureTable; texture address
// 0 = not this launch's format: skip (its partials are not written, and the reduction does not read them).
// partials: [pictures][gridDim.x][8] -- sse R, G, B, A, then sad R, G, B, A
template <int FMT, bool HAS_ALPHA>
__global__ __launch_bounds__(256) void bc_measure_kernel(HapGpuPictureTable t, unsigned blocks_x, unsigned blocks_total,
                                                         size_t row_bytes, uint32_t *__restrict__ partials)
{
    __shared__ unsigned wave_sums[4][8];
    const uint8_t *blocks = (const uint8_t *)picture_address(t, 0);
    if (!blocks)
        return;                     // (the whole workgroup: blockIdx.z is its picture)
    unsigned dd[4] = {0u, 0u, 0u, 0u}, pp[4] = {0u, 0u, 0u, 0u}, dp[4] = {0u, 0u, 0u, 0u}, sad[4] = {0u, 0u, 0u, 0u};
    // (a lane past the last block adds nothing more and stays for the reduction)
#pragma unroll 1
    for (unsigned tile = 0; tile < kTiles; tile++) {
        const unsigned id = (blockIdx.x * kTiles + tile) * 256u + threadIdx.x;
        if (id >= blocks_total)
            break;
        const unsigned by = id / blocks_x, bx = id - by * blocks_x;
        const uint8_t *reference = (const uint8_t *)picture_address(t, 2) + (size_t)(4u * by) * row_bytes + 16u * (size_t)bx;
        v4u p[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
            p[r] = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(reference + (size_t)r * row_bytes));
        unsigned px[16];
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
        // (the body of the picture decoder, from registers to registers: no grid, no picture)
        bc_decode_body<FMT, HAS_ALPHA, false, true>(nullptr, nullptr, 1u, 0u, nullptr, 0u, 0u, 0u, &reg);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned drow[4] = {px[4 * r], px[4 * r + 1], px[4 * r + 2], px[4 * r + 3]};
            const unsigned prow[4] = {p[r][0], p[r][1], p[r][2], p[r][3]};
            unsigned d[4], q[4];
            channels_of(drow, d);
            channels_of(prow, q);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                dd[c] = dot4(d[c], d[c], dd[c]);
                pp[c] = dot4(q[c], q[c], pp[c]);
                dp[c] = dot4(d[c], q[c], dp[c]);
                sad[c] = __builtin_amdgcn_sad_u8(d[c], q[c], sad[c]);
            }
        }
    }
    unsigned sums[8];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        sums[c] = dd[c] + pp[c] - 2u * dp[c];           // (exact: sum (d - p)^2, at most 4 * 16 * 255^2)
        sums[4 + c] = sad[c];
    }
    const unsigned wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const unsigned total = wave_sum_in_lane_63(sums[i]);
        if ((threadIdx.x & 63u) == 63u)
            wave_sums[wave][i] = total;
    }
    __syncthreads();
    if (threadIdx.x < 8u)
        partials[((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 8u + threadIdx.x] =
            wave_sums[0][threadIdx.x] + wave_sums[1][threadIdx.x] + wave_sums[2][threadIdx.x] + wave_sums[3][threadIdx.x];
}

// One workgroup per picture: totals[picture][8] = the 64-bit sums of its `workgroups` partials.  Lane i adds entries
// i, i + 1024, ... and the lanes are added in a fixed tree, so a picture's totals are the same in every call (they would
// be anyway: integer addition).  A picture whose texture address is 0 is not this launch's and is left alone.
__global__ __launch_bounds__(1024) void bc_measure_reduce_kernel(HapGpuPictureTable t, const uint32_t *__restrict__ partials,
                                                                 unsigned workgroups, unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long wave_sums[16][8];
    const unsigned z = blockIdx.x;
    if (!(t.column[0] ? t.column[0][z] : t.one[0]))
        return;
    const v4u *mine = reinterpret_cast<const v4u *>(partials + (size_t)z * workgroups * 8u);
    unsigned long long sums[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (unsigned w = threadIdx.x; w < workgroups; w += 1024u) {
        const v4u a = mine[2u * (size_t)w], b = mine[2u * (size_t)w + 1u];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sums[i] += a[i];
            sums[4 + i] += b[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            sums[i] += __shfl_down(sums[i], step, 64);
        if ((threadIdx.x & 63u) == 0u)
            wave_sums[threadIdx.x >> 6][i] = sums[i];
    }
    __syncthreads();
    if (threadIdx.x < 8u) {
        unsigned long long total = 0ull;
#pragma unroll
        for (int w = 0; w < 16; w++)
            total += wave_sums[w][threadIdx.x];
        totals[(size_t)z * 8u + threadIdx.x] = total;
    }
}

template <int FMT>
void launch(const HapGpuPictureTable &t, const dim3 &grid, unsigned blocks_x, unsigned blocks_total, size_t row_bytes,
            bool alpha, uint32_t *partials, hipStream_t stream)
{
    if (alpha)
        hipLaunchKernelGGL((bc_measure_kernel<FMT, true>), grid, dim3(256), 0, stream, t, blocks_x, blocks_total, row_bytes, partials);
    else
        hipLaunchKernelGGL((bc_measure_kernel<FMT, false>), grid, dim3(256), 0, stream, t, blocks_x, blocks_total, row_bytes, partials);
}

} // namespace

// hapgpu_abi.h.  Returns 0 launched, 1 bad arguments, 4 launch failure.
extern "C" int hapgpu_k_block_measure(hapgpu_rt *rt, const HapGpuPictureTable *table, unsigned pictures, int with_alpha,
                                      unsigned width, unsigned height, unsigned format, size_t row_bytes, uint32_t *partials,
                                      unsigned long long *totals)
{
    scoped_timing st(rt, 6);
    const hipStream_t stream = hapgpu_rt_stream(rt);
    if (!table || !(table->column[0] || table->one[0]) || !(table->column[2] || table->one[2]) ||
        (with_alpha && !(table->column[1] || table->one[1])) || pictures == 0 || pictures > 65535u || width == 0 ||
        height == 0 || (width & 3u) || (height & 3u) || row_bytes < (size_t)width * 4u || (row_bytes & 15u) || !partials ||
        !totals || ((uintptr_t)partials & 15u) || ((uintptr_t)totals & 7u) ||
        (unsigned long long)(width / 4u) * (height / 4u) > 0xFFFFFFFFull / 256u * 255u)
        return 1;
    const unsigned blocks_x = width / 4u, blocks_total = blocks_x * (height / 4u);
    const dim3 grid((blocks_total + 256u * kTiles - 1u) / (256u * kTiles), 1, pictures);
    switch (format) {
    case 0x83F0: launch<0>(*table, grid, blocks_x, blocks_total, row_bytes, with_alpha != 0, partials, stream); break;
    case 0x83F3: launch<1>(*table, grid, blocks_x, blocks_total, row_bytes, with_alpha != 0, partials, stream); break;
    case 0x01: launch<2>(*table, grid, blocks_x, blocks_total, row_bytes, with_alpha != 0, partials, stream); break;
    default: return 1;
    }
    if (hipGetLastError() != hipSuccess)
        return 4;
    hipLaunchKernelGGL(bc_measure_reduce_kernel, dim3(pictures), dim3(1024), 0, stream, *table, partials, grid.x, totals);
    return hipGetLastError() == hipSuccess ? 0 : 4;
}

// hapgpu_abi.h: the scratch hapgpu_k_block_measure asks for
extern "C" size_t hapgpu_block_measure_partial_bytes(unsigned width, unsigned height)
{
    return (((size_t)(width / 4u) * (height / 4u) + 256u * kTiles - 1u) / (256u * kTiles)) * 8u * sizeof(uint32_t);
}
