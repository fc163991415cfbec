// rgb_ycbcr_host.hip -- hap_amd/csrc/rgb_ycbcr.hpp compiled for the host (hipcc --offload-host-only -shared): the
// kernel's conversion over all 2^24 colours and over sums of texels, for tests/test_rgb_ycbcr_host.py.
#include <stddef.h>
#include <stdint.h>

#include "rgb_ycbcr.hpp"

using namespace hapbc::video;

static bool inside(unsigned matrix, unsigned range) { return matrix <= 1u && range <= 1u; }

// out[(r << 16) | (g << 8) | b] = Y of the texel (r, g, b), alpha taking every value in turn
extern "C" int rgb_ycbcr_luma_all(unsigned matrix, unsigned range, uint8_t *out)
{
    if (!inside(matrix, range))
        return 1;
    const sample_coefficients k = sample_coefficients_of(matrix, range);
    for (unsigned r = 0; r < 256u; r++)
        for (unsigned g = 0; g < 256u; g++)
            for (unsigned b = 0; b < 256u; b++)
                out[(r << 16) | (g << 8) | b] = (uint8_t)luma_of(r | g << 8 | b << 16 | ((r + g + b) & 0xFFu) << 24, k);
    return 0;
}

// out[(r << 16) | (g << 8) | b] = Cb | Cr << 8 of four texels (r, g, b): through sums_of, the kernel's way
extern "C" int rgb_ycbcr_chroma_all(unsigned matrix, unsigned range, uint16_t *out)
{
    if (!inside(matrix, range))
        return 1;
    const sample_coefficients k = sample_coefficients_of(matrix, range);
    for (unsigned r = 0; r < 256u; r++)
        for (unsigned g = 0; g < 256u; g++)
            for (unsigned b = 0; b < 256u; b++) {
                const unsigned t = r | g << 8 | b << 16 | ((r ^ g ^ b) & 0xFFu) << 24;
                out[(r << 16) | (g << 8) | b] = (uint16_t)pair_of(sums_of(t, t, t, t), k);
            }
    return 0;
}

// out[i] = Cb | Cr << 8 of the sums (rs[i], gs[i], bs[i]), each 0 .. 1020
extern "C" int rgb_ycbcr_chroma_of_sums(unsigned matrix, unsigned range, size_t n, const uint16_t *rs, const uint16_t *gs,
                                        const uint16_t *bs, uint16_t *out)
{
    if (!inside(matrix, range))
        return 1;
    const sample_coefficients k = sample_coefficients_of(matrix, range);
    for (size_t i = 0; i < n; i++)
        out[i] = (uint16_t)pair_of((int)rs[i], (int)gs[i], (int)bs[i], k);
    return 0;
}

// n blocks of sixteen texels -> per block four words of Y and two of pairs, as the kernel stores them
extern "C" int rgb_ycbcr_blocks(unsigned matrix, unsigned range, size_t n, const uint32_t *texels, uint32_t *out)
{
    if (!inside(matrix, range))
        return 1;
    const sample_coefficients k = sample_coefficients_of(matrix, range);
    for (size_t i = 0; i < n; i++) {
        unsigned p[16], y[4], c[2];
        for (int t = 0; t < 16; t++)
            p[t] = texels[16 * i + t];
        samples_of_block(p, k, y, c);
        for (int r = 0; r < 4; r++)
            out[6 * i + r] = y[r];
        out[6 * i + 4] = c[0];
        out[6 * i + 5] = c[1];
    }
    return 0;
}

// the table as the header holds it: yr, yg, yb, cbr, cbg, ch, crg, crb, lo
extern "C" int rgb_ycbcr_coefficients(unsigned matrix, unsigned range, int *out)
{
    if (!inside(matrix, range))
        return 1;
    const sample_coefficients k = sample_coefficients_of(matrix, range);
    out[0] = k.yr, out[1] = k.yg, out[2] = k.yb, out[3] = k.cbr, out[4] = k.cbg, out[5] = k.ch, out[6] = k.crg,
    out[7] = k.crb, out[8] = k.lo;
    return 0;
}
