// ycbcr_rgb_host.hip -- hap_amd/csrc/ycbcr_rgb.hpp compiled for the host (hipcc --offload-host-only -shared): the
// kernel's conversion over all 2^24 (Y, Cb, Cr) triples, for tests/test_ycbcr_rgb_host.py.
#include <stddef.h>
#include <stdint.h>

#include "ycbcr_rgb.hpp"

using namespace hapbc::video;

// out[(y << 16) | (cb << 8) | cr] = the packed texel of (y, cb, cr), through the (matrix, range) form
extern "C" int ycbcr_rgb_all(unsigned matrix, unsigned range, uint32_t *out)
{
    if (matrix > (unsigned)kBT709 || range > (unsigned)kFull)
        return 1;
    for (unsigned y = 0; y < 256u; y++)
        for (unsigned cb = 0; cb < 256u; cb++)
            for (unsigned cr = 0; cr < 256u; cr++)
                out[(y << 16) | (cb << 8) | cr] = rgba_of(y, cb, cr, matrix, range);
    return 0;
}

// ... the way the kernel goes: a pair's terms once, then a luma sample under them
extern "C" int ycbcr_rgb_all_by_pair(unsigned matrix, unsigned range, uint32_t *out)
{
    if (matrix > (unsigned)kBT709 || range > (unsigned)kFull)
        return 1;
    const coefficients k = coefficients_of(matrix, range);
    for (unsigned cb = 0; cb < 256u; cb++)
        for (unsigned cr = 0; cr < 256u; cr++) {
            const chroma_terms t = chroma_of(cb, cr, k);
            for (unsigned y = 0; y < 256u; y++)
                out[(y << 16) | (cb << 8) | cr] = rgba_of_luma(y, t, k);
        }
    return 0;
}

// the table as the header holds it: cy, crv, cbu, cgu, cgv, luma offset
extern "C" int ycbcr_rgb_coefficients(unsigned matrix, unsigned range, int *out)
{
    if (matrix > (unsigned)kBT709 || range > (unsigned)kFull)
        return 1;
    const coefficients k = coefficients_of(matrix, range);
    out[0] = k.cy, out[1] = k.crv, out[2] = k.cbu, out[3] = k.cgu, out[4] = k.cgv, out[5] = k.luma_offset;
    return 0;
}
