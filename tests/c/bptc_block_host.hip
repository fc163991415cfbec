// The block functions of bc6h_encode.hip and bptc_encode.hip compiled for the host (they are __host__ __device__): plain
// C loops over blocks for tests/test_bptc_value_space.py.  Both files keep their code in unnamed namespaces with the same
// helper names, so each is included into a namespace of its own; the launchers stay out (the HOST_ONLY guards).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "hapgpu_runtime.hpp"
#include "bptc_tables.hpp"

#define HAPGPU_BC6H_ENCODE_HOST_ONLY
#define HAPGPU_BPTC_ENCODE_HOST_ONLY

namespace host_bc6h {
#include "bc6h_encode.hip"
}
#undef HD
namespace host_bc7 {
#include "bptc_encode.hip"
}

// texels: n blocks of 16 RGBA16F texels (128 bytes a block, row-major) -> n * 16 bytes
extern "C" void bc6h_encode_blocks(const uint16_t *texels, size_t n, int is_signed, uint8_t *out)
{
    for (size_t i = 0; i < n; i++) {
        unsigned px[32];
        memcpy(px, texels + 64 * i, sizeof px);
        const uint4 w = is_signed ? host_bc6h::hapgpu_bc6h_encode_block<true>(px) : host_bc6h::hapgpu_bc6h_encode_block<false>(px);
        memcpy(out + 16 * i, &w, 16);
    }
}

// texels: n blocks of 16 RGBA8 texels (64 bytes a block, row-major) -> n * 16 bytes
extern "C" void bc7_encode_blocks(const uint8_t *texels, size_t n, uint8_t *out)
{
    for (size_t i = 0; i < n; i++) {
        unsigned px[16];
        memcpy(px, texels + 64 * i, sizeof px);
        const uint4 w = host_bc7::hapgpu_bc7_encode_block(px);
        memcpy(out + 16 * i, &w, 16);
    }
}
