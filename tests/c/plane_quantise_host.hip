// plane_quantise_host.hip -- hap_amd/csrc/plane_quantise.hpp compiled for the host (hipcc --offload-host-only -shared):
// the kernel's quantiser and its three element loads, over arrays, for tests/test_plane_quantise_host.py.
#include <stddef.h>
#include <stdint.h>

#include "plane_quantise.hpp"

using namespace hapbc::planes;

// kind: HapGpuPlaneElement; bits: n elements' bit patterns, 16 bits each (half, bfloat16) or 32 (float)
extern "C" int plane_quantise(unsigned kind, const void *bits, size_t n, float scale, float bias, uint8_t *out)
{
    if (kind > (unsigned)kF32)
        return 1;
    for (size_t i = 0; i < n; i++) {
        const float x = kind == (unsigned)kF32   ? value_of_float(((const uint32_t *)bits)[i])
                        : kind == (unsigned)kF16 ? value_of_half(((const uint16_t *)bits)[i])
                                                 : value_of_bfloat(((const uint16_t *)bits)[i]);
        out[i] = (uint8_t)quantise(x, scale, bias);
    }
    return 0;
}

// the elements' values as binary32 bit patterns: the loads alone
extern "C" int plane_values(unsigned kind, const void *bits, size_t n, uint32_t *out)
{
    if (kind > (unsigned)kF32)
        return 1;
    for (size_t i = 0; i < n; i++) {
        const float x = kind == (unsigned)kF32   ? value_of_float(((const uint32_t *)bits)[i])
                        : kind == (unsigned)kF16 ? value_of_half(((const uint16_t *)bits)[i])
                                                 : value_of_bfloat(((const uint16_t *)bits)[i]);
        out[i] = __builtin_bit_cast(uint32_t, x);
    }
    return 0;
}
