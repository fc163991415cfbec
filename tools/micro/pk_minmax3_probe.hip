// Dev probe (round 13): do v_pk_minimum3_f16 / v_pk_maximum3_f16 return the INTEGER minimum / maximum of three pairs of
// non-negative 16-bit halves, bit for bit?  The Hap Q colour box (bc_encode_core.hpp, ycocg_colour_block) holds Co | Cg
// as halves 1..256 -- subnormal IEEE halves, whose order is the integers' order provided the instruction neither flushes
// them nor rewrites the operand it returns.  Two domains, each half of each result compared with the integer answer:
//   * every triple of words whose halves are drawn from {0, 1, 2, 127, 128, 129, 255, 256}, independently per half
//     (64 words, 64^3 triples);
//   * every pair a, b of 0..256 as (a | b << 16, b | a << 16, a | b << 16): the third operand the first again, which is
//     how the box pads its last step.
// The kernel is compiled like the library's (no float-mode option), and prints the wave's MODE register: FP_DENORM is
// bits 7:4, the upper two the half / double field, 3 = subnormals kept both ways.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

__device__ __forceinline__ unsigned minimum3(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm volatile("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned maximum3(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__constant__ unsigned kSet[8] = {0, 1, 2, 127, 128, 129, 255, 256};

__device__ __forceinline__ unsigned word_of(unsigned i) { return kSet[i & 7u] | kSet[(i >> 3) & 7u] << 16; }

// out[2 i], out[2 i + 1]: minimum3, maximum3 of triple i; mode[0]: the MODE register of the first wave
__global__ void probe_triples(unsigned *out, unsigned n, unsigned *mode)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u) {
        unsigned m;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_MODE)" : "=s"(m));
        mode[0] = m;
    }
    if (i >= n)
        return;
    const unsigned a = word_of(i), b = word_of(i >> 6), c = word_of(i >> 12);
    out[2u * i] = minimum3(a, b, c);
    out[2u * i + 1u] = maximum3(a, b, c);
}

__global__ void probe_pairs(unsigned *out, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const unsigned a = i % 257u, b = i / 257u, x = a | b << 16, y = b | a << 16;
    out[2u * i] = minimum3(x, y, x);
    out[2u * i + 1u] = maximum3(x, y, x);
}

static unsigned min3(unsigned a, unsigned b, unsigned c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
static unsigned max3(unsigned a, unsigned b, unsigned c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
static unsigned pk(unsigned (*f)(unsigned, unsigned, unsigned), unsigned a, unsigned b, unsigned c)
{
    return f(a & 0xFFFFu, b & 0xFFFFu, c & 0xFFFFu) | f(a >> 16, b >> 16, c >> 16) << 16;
}

static const unsigned kSetHost[8] = {0, 1, 2, 127, 128, 129, 255, 256};
static unsigned word_of_host(unsigned i) { return kSetHost[i & 7u] | kSetHost[(i >> 3) & 7u] << 16; }

static void report(const char *what, const char *op, long wrong, unsigned n, const unsigned *first)
{
    printf("  %-18s %s: %ld of %u differ from the integer result", op, what, wrong, n);
    if (wrong)
        printf(" (first: %08x %08x %08x -> %08x, integer %08x)", first[0], first[1], first[2], first[3], first[4]);
    printf("\n");
}

int main()
{
    const unsigned n3 = 64u * 64u * 64u, n2 = 257u * 257u;
    unsigned *dev, *mode, *host = (unsigned *)malloc(sizeof(unsigned) * 2u * n3), host_mode = 0;
    if (!host || hipMalloc(&dev, sizeof(unsigned) * 2u * n3) != hipSuccess || hipMalloc(&mode, sizeof(unsigned)) != hipSuccess)
        return 1;
    long bad = 0;

    hipLaunchKernelGGL(probe_triples, dim3((n3 + 255u) / 256u), dim3(256), 0, 0, dev, n3, mode);
    if (hipMemcpy(host, dev, sizeof(unsigned) * 2u * n3, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&host_mode, mode, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    printf("MODE register 0x%08x: FP_DENORM %u (single %u, half / double %u)\n", host_mode, (host_mode >> 4) & 15u,
           (host_mode >> 4) & 3u, (host_mode >> 6) & 3u);
    printf("triples of words with halves from {0, 1, 2, 127, 128, 129, 255, 256}:\n");
    for (int which = 0; which < 2; which++) {
        long wrong = 0;
        unsigned first[5] = {0, 0, 0, 0, 0};
        for (unsigned i = 0; i < n3; i++) {
            const unsigned a = word_of_host(i), b = word_of_host(i >> 6), c = word_of_host(i >> 12);
            const unsigned want = pk(which ? max3 : min3, a, b, c), got = host[2u * i + which];
            if (got != want && !wrong++) {
                first[0] = a; first[1] = b; first[2] = c; first[3] = got; first[4] = want;
            }
        }
        report("", which ? "v_pk_maximum3_f16" : "v_pk_minimum3_f16", wrong, n3, first);
        bad += wrong;
    }

    hipLaunchKernelGGL(probe_pairs, dim3((n2 + 255u) / 256u), dim3(256), 0, 0, dev, n2);
    if (hipMemcpy(host, dev, sizeof(unsigned) * 2u * n2, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    printf("pairs a, b of 0..256, operands a | b << 16, b | a << 16, a | b << 16:\n");
    for (int which = 0; which < 2; which++) {
        long wrong = 0;
        unsigned first[5] = {0, 0, 0, 0, 0};
        for (unsigned i = 0; i < n2; i++) {
            const unsigned a = i % 257u, b = i / 257u, x = a | b << 16, y = b | a << 16;
            const unsigned want = pk(which ? max3 : min3, x, y, x), got = host[2u * i + which];
            if (got != want && !wrong++) {
                first[0] = x; first[1] = y; first[2] = x; first[3] = got; first[4] = want;
            }
        }
        report("", which ? "v_pk_maximum3_f16" : "v_pk_minimum3_f16", wrong, n2, first);
        bad += wrong;
    }
    printf(bad ? "NOT the integer minimum / maximum: the box keeps its two-input integer form\n"
               : "the integer minimum / maximum, bit for bit, subnormal halves included\n");
    hipFree(dev);
    hipFree(mode);
    free(host);
    return 0;
}
