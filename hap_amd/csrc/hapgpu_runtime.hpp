// hapgpu_runtime.hpp -- what the kernel files see of the runtime (HIP translation units only; to the host C code
// hapgpu_rt stays opaque).  Each kernel file defines the hapgpu_k_* entries of hapgpu_abi.h for its own kernels: an
// entry opens a scoped_timing of its profile class and launches on the runtime's stream.  Helpers one kernel file
// calls in another are declared here, with C++ linkage, so that a signature that drifts fails to link.
#ifndef HAPGPU_RUNTIME_HPP
#define HAPGPU_RUNTIME_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapgpu_abi.h"

// Launch settings of one runtime, fixed by hapgpu_rt_create while its device is current (HAP_AB_ENV switches are read
// there, function attributes set there: they are the device's)
struct hapgpu_launch_settings {
    unsigned cus;                 // compute units of the device (0: unknown)
    int block_resolve;            // snappy_decode_block_resolve_kernel in use (off for this runtime after a refusal)
    unsigned resolve_workgroups;  // its grid: a workgroup per CU
    unsigned resolve_max_units;   // the largest block hint it is launched for
    unsigned ring_log2_forced;    // HAP_AMD_STREAM_RING_LOG2 (0: the ring is chosen per call)
    unsigned guess_lds_bytes;     // dynamic LDS of guess_group_tables_kernel
    int compress_big_lds;         // snappy_compress_wg_kernel may be launched with more than 64 KiB of LDS
    int copy_kernels;             // small copies of the pinned scratch as kernels (else hipMemcpyAsync)
};

hipStream_t hapgpu_rt_stream(hapgpu_rt *rt);
hapgpu_launch_settings *hapgpu_rt_settings(hapgpu_rt *rt);
uint32_t *hapgpu_rt_resolved_counter(hapgpu_rt *rt);     // device counter of hapgpu_rt_resolved_blocks, or null
unsigned long long *hapgpu_rt_skipped_counter(hapgpu_rt *rt);   // device counter of hapgpu_rt_skipped_bytes, or null

struct timed_launch {
    int cls;
    hipEvent_t start, stop;
};

// HIP events around the launches of its scope while profiling is on, collected as class `cls` (hapgpu_rt_collect_profile)
struct scoped_timing {
    hapgpu_rt *rt;
    timed_launch t;
    bool on;
    scoped_timing(hapgpu_rt *r, int cls);
    ~scoped_timing();
};

// the kernel files' parts of hapgpu_rt_create
void hapgpu_prepare_snappy_compress(hapgpu_launch_settings *s);
void hapgpu_prepare_snappy_decode(hapgpu_launch_settings *s);
void hapgpu_prepare_snappy_decode_fields(hapgpu_launch_settings *s);

// snappy_compress_blocks.hip
int hapgpu_snappy_compress_blocks(const HapGpuFrameEnc *frames, unsigned frame_count, unsigned max_frags_per_texture,
                                  unsigned textures, void *slots, unsigned slot_stride, uint32_t *frag_sizes,
                                  uint8_t *group_tables, unsigned layouts, unsigned fused, hipStream_t stream);
// snappy_decode_fields.hip
int hapgpu_snappy_decode_fields(const HapGpuDecodeUnit *units, unsigned unit_count, HapGpuDecodeJob *jobs,
                                unsigned fields_kinds, hipStream_t stream);
// address column c of picture blockIdx.z of a block-codec launch: one scalar choice, no table for a single picture
__device__ __forceinline__ uint64_t picture_address(const HapGpuPictureTable &t, unsigned c)
{
    return t.column[c] ? t.column[c][blockIdx.z] : t.one[c];
}
// the BC7 and BC6H launches of hapgpu_k_block_encode / hapgpu_k_block_decode (arguments checked there)
void hapgpu_launch_bptc_encode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                               size_t row_bytes, bool wide, hipStream_t stream);      // bptc_encode.hip
void hapgpu_launch_bc6h_encode(const HapGpuPictureTable &t, unsigned pictures, bool is_signed, unsigned bx,
                               unsigned by, size_t row_bytes, hipStream_t stream);    // bc6h_encode.hip
void hapgpu_launch_bptc_decode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                               size_t row_bytes, hipStream_t stream);                 // bptc_decode.hip
void hapgpu_launch_bptc_decode_scaled(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                                      size_t row_bytes, unsigned scale_log2, hipStream_t stream);   // bptc_decode.hip
void hapgpu_launch_bc6h_decode(const HapGpuPictureTable &t, unsigned pictures, bool is_signed, unsigned bx,
                               unsigned by, size_t row_bytes, hipStream_t stream);    // bc6h_decode.hip
// A rectangle of a texture in blocks, for the kernels of hapgpu_k_block_decode_region: the grid is region_total lanes,
// lane id block (id % region_x, id / region_x) of the rectangle -- texture block first + (id / region_x) * blocks_x +
// id % region_x
struct HapGpuRegionBlocks {
    unsigned blocks_x;        // blocks in a row of the texture
    unsigned first;           // the texture block of the rectangle's upper left corner
    unsigned region_x;        // blocks in a row of the rectangle
    unsigned region_total;    // blocks of the rectangle
};
void hapgpu_launch_bptc_decode_region(const HapGpuPictureTable &t, unsigned pictures, const HapGpuRegionBlocks &g,
                                      size_t row_bytes, hipStream_t stream);          // bptc_decode.hip
// ... and the A8 pictures of both (RGTC1 only; wide: 16-byte aligned pictures and pitch)
void hapgpu_launch_alpha_encode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                                size_t row_bytes, bool wide, hipStream_t stream);     // alpha_plane.hip
void hapgpu_launch_alpha_decode(const HapGpuPictureTable &t, unsigned pictures, unsigned bx, unsigned by,
                                size_t row_bytes, bool wide, hipStream_t stream);     // alpha_plane.hip
// snappy_decode.hip
int hapgpu_group_tables_from_records(HapGpuDecodeUnit *units, unsigned unit_count, const HapGpuDecodeJob *jobs,
                                     const uint32_t *work, unsigned work_slots, const void *recs, const void *joins,
                                     hipStream_t stream);
#ifdef BRK_TIMING
void hapgpu_debug_merge_counters(unsigned *out);
#endif

#endif
