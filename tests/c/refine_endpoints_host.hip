// bc_refine_core.hpp compiled for the host (its functions are __host__ __device__ and hold no inline assembly): plain C
// loops over blocks for tests/test_refined_endpoints.py.  A block: sixteen packed pixels R | G << 8 | B << 16 and the
// sixteen 2-bit indices it has.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "bc_refine_core.hpp"

// a round's candidate for n blocks: out[3 i] = 1 where the round has one, out[3 i + 1], out[3 i + 2] = c0', c1'
extern "C" void refine_candidates(const uint32_t *px, const uint32_t *idx, size_t n, uint32_t *out)
{
    for (size_t i = 0; i < n; i++) {
        unsigned p[16], c0 = 0, c1 = 0;
        memcpy(p, px + 16 * i, sizeof p);
        const bool valid = hapbc::refine_candidate(p, hapbc::refine_plain_sums(p), hapbc::refine_weights(idx[i]), c0, c1);
        out[3 * i] = valid ? 1u : 0u;
        out[3 * i + 1] = c0;
        out[3 * i + 2] = c1;
    }
}

// what n blocks (c0, c1, indices) are ranked by: the squared error less the sum of the squares of the block's pixels
extern "C" void refine_ranks(const uint32_t *px, const uint32_t *c0, const uint32_t *c1, const uint32_t *idx, size_t n, int32_t *out)
{
    for (size_t i = 0; i < n; i++) {
        unsigned p[16];
        memcpy(p, px + 16 * i, sizeof p);
        out[i] = hapbc::refine_rank(p, hapbc::refine_make_palette(c0[i], c1[i]), idx[i]);
    }
}

// the rounded, clamped quotient of n (numerator, determinant) pairs, determinants above 0
extern "C" void refine_quotients(const int32_t *num, const int32_t *det, size_t n, int32_t *out)
{
    for (size_t i = 0; i < n; i++)
        out[i] = hapbc::refine_quotient(num[i], det[i]);
}
