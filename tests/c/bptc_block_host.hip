// The block functions of bc6h_encode.hip and bptc_encode.hip compiled for the host (they are __host__ __device__): plain
// C loops over blocks for tests/test_bptc_value_space.py.  Each file keeps its code in a namespace of its own (hapbc6h,
// hapbc7) and both share bptc_encode_core.hpp, so they are included as they are; the launchers stay out (the HOST_ONLY
// guards).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "hapgpu_runtime.hpp"

#define HAPGPU_BC6H_ENCODE_HOST_ONLY
#define HAPGPU_BPTC_ENCODE_HOST_ONLY

#include "bc6h_encode.hip"
#include "bptc_encode.hip"

// texels: n blocks of 16 RGBA16F texels (128 bytes a block, row-major) -> n * 16 bytes
extern "C" void bc6h_encode_blocks(const uint16_t *texels, size_t n, int is_signed, uint8_t *out)
{
    for (size_t i = 0; i < n; i++) {
        unsigned px[32];
        memcpy(px, texels + 64 * i, sizeof px);
        const uint4 w = is_signed ? hapbc6h::hapgpu_bc6h_encode_block<true>(px) : hapbc6h::hapgpu_bc6h_encode_block<false>(px);
        memcpy(out + 16 * i, &w, 16);
    }
}

// texels: n blocks of 16 RGBA8 texels (64 bytes a block, row-major) -> n * 16 bytes
extern "C" void bc7_encode_blocks(const uint8_t *texels, size_t n, uint8_t *out)
{
    for (size_t i = 0; i < n; i++) {
        unsigned px[16];
        memcpy(px, texels + 64 * i, sizeof px);
        const uint4 w = hapbc7::hapgpu_bc7_encode_block(px);
        memcpy(out + 16 * i, &w, 16);
    }
}
