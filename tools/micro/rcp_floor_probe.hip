// Dev probe (round 11): is floor(N / d) exactly (unsigned)(c * v_rcp_f32((float)d)) for some float constant c near N, over
// the whole domain of d?  Two domains of bc_encode_core.hpp: N = 2^19, d = 1..255 (alpha_block's ramp multiplier) and
// N = 3 * 2^24, d = 1..195075 (index_scale).  For every candidate c = N stepped up by 0..7 units in the last place it
// prints how many d come out wrong and the extremes of (got - floor(N / d)): 0 wrong means no fix-up is needed, an error
// of one sign only means one compare and carry is.  One launch per domain; v_rcp_f32 is deterministic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#define CANDIDATES 8

__global__ void probe(unsigned *out, unsigned n, float c0)
{
    const unsigned d = blockIdx.x * blockDim.x + threadIdx.x + 1u;
    if (d > n)
        return;
    float c = c0;
    for (int k = 0; k < CANDIDATES; k++) {
        out[(size_t)k * n + (d - 1u)] = (unsigned)(c * __builtin_amdgcn_rcpf((float)d));
        c = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, c) + 1u);      // the next float up
    }
}

static int run(const char *what, unsigned N, unsigned n)
{
    unsigned *dev, *host = (unsigned *)malloc(sizeof(unsigned) * CANDIDATES * n);
    if (hipMalloc(&dev, sizeof(unsigned) * CANDIDATES * n) != hipSuccess)
        return 1;
    hipLaunchKernelGGL(probe, dim3((n + 255u) / 256u), dim3(256), 0, 0, dev, n, (float)N);
    if (hipMemcpy(host, dev, sizeof(unsigned) * CANDIDATES * n, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    printf("%s: N = %u, d = 1..%u\n", what, N, n);
    float c = (float)N;
    for (int k = 0; k < CANDIDATES; k++) {
        long wrong = 0, lo = 0, hi = 0;
        unsigned first = 0;
        for (unsigned d = 1; d <= n; d++) {
            const long e = (long)host[(size_t)k * n + d - 1] - (long)(N / d);
            if (e != 0 && !wrong++)
                first = d;
            lo = e < lo ? e : lo;
            hi = e > hi ? e : hi;
        }
        printf("  c = N + %d ulp = %.1f (0x%08x): wrong %ld of %u, error %ld .. %ld, first wrong d %u\n", k, (double)c,
               __builtin_bit_cast(unsigned, c), wrong, n, lo, hi, first);
        c = nextafterf(c, INFINITY);
    }
    hipFree(dev);
    free(host);
    return 0;
}

int main()
{
    return run("ramp multiplier", 1u << 19, 255u) || run("index scale", 3u << 24, 195075u);
}
