// Dev probe 3: what v_mfma_i32_4x4x4_16b_i8 costs beside vector work (waves per SIMD = argv[1], default 5: the fused Hap Q
// encode kernel's).  Build: hipcc -O3 --offload-arch=gfx950 -o mfma_beside_valu mfma_beside_valu.hip
//   (a) the D tuple of every lane for known A and B, against the layout bc_encode_core.hpp relies on: lane l supplies
//       row l & 3 of A and column l & 3 of B of block l >> 2 (k = byte index), register r of lane l holds D[r][l & 3];
//       and the same instruction issued with one lane active (what inactive lanes supply, and whether they are written);
//   (b) cycles per instruction back to back (eight independent destinations);
//   (c) cycles per step of 4 cheap-class + 4 dear-class VALU with 0 / 1 / 2 MFMAs or 3 / 6 v_dot4_i32_i8 in between.  The
//       MFMAs' results are read by one of the eight VALU a step later (seven instructions behind the MFMA; five are
//       required), so every variant issues the same vector instructions and the difference is the MFMA's price.
// Fixed registers v40.. hold the MFMA results: an inline-assembly operand cannot name one register of a tuple.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#define ITER 4096
#define MFMA "v_mfma_i32_4x4x4_16b_i8 "
#define CLOBBERS "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", \
                 "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71"

// ---- (a) layout ----
__global__ __launch_bounds__(64) void k_layout(const unsigned *a, const unsigned *b, int *d, int only_lane)
{
    const unsigned lane = threadIdx.x;
    const unsigned va = a[lane], vb = b[lane];
    int r0, r1, r2, r3;
    asm volatile("v_mov_b32 v40, -1\n\tv_mov_b32 v41, -1\n\tv_mov_b32 v42, -1\n\tv_mov_b32 v43, -1" ::: "v40", "v41", "v42", "v43");
    if (only_lane < 0 || (int)lane == only_lane)
        asm volatile("s_nop 1\n\t" MFMA "v[40:43], %0, %1, 2\n\ts_nop 4" ::"v"(va), "v"(vb) : "v40", "v41", "v42", "v43");
    asm volatile("v_mov_b32 %0, v40\n\tv_mov_b32 %1, v41\n\tv_mov_b32 %2, v42\n\tv_mov_b32 %3, v43"
                 : "=v"(r0), "=v"(r1), "=v"(r2), "=v"(r3)::"v40", "v41", "v42", "v43");
    d[4 * lane] = r0; d[4 * lane + 1] = r1; d[4 * lane + 2] = r2; d[4 * lane + 3] = r3;
}

// ---- (b), (c) rates ----
#define V_CHEAP(x, src) "v_xor_b32 " #x ", " #x ", " src "\n"
#define V_PERM(x) "v_perm_b32 " #x ", " #x ", %8, " #x "\n"
#define V_MAD(x) "v_mad_i32_i24 " #x ", " #x ", %8, " #x "\n"
#define BODY(SRC0, SRC1, M0, M1, D0, D1)                                                                         \
    V_CHEAP(%0, SRC0) M0 V_PERM(%1) D0 V_CHEAP(%2, SRC1) M1 V_MAD(%3) V_CHEAP(%4, "%8") D1 V_PERM(%5) V_CHEAP(%6, "%8") V_MAD(%7)
#define M_0 MFMA "v[40:43], %8, %6, 2\n"
#define M_1 MFMA "v[44:47], %8, %4, 2\n"
#define DOT3A "v_dot4_i32_i8 v48, %6, %8, 1\nv_dot4_i32_i8 v49, %6, %8, 2\nv_dot4_i32_i8 v50, %6, %8, 2\n"
#define DOT3B "v_dot4_i32_i8 v51, %2, %8, 1\nv_dot4_i32_i8 v52, %2, %8, 2\nv_dot4_i32_i8 v53, %2, %8, 2\n"
#define B_BASE BODY("%8", "%8", "", "", "", "")
#define B_MFMA1 BODY("v40", "%8", M_0, "", "", "")
#define B_MFMA2 BODY("v40", "v44", M_0, M_1, "", "")
#define B_DOT3 BODY("%8", "%8", "", "", DOT3A, "")
#define B_DOT6 BODY("%8", "%8", "", "", DOT3A, DOT3B)
#define B_MFMA8                                                                                                  \
    MFMA "v[40:43], %8, %0, 2\n" MFMA "v[44:47], %8, %1, 2\n" MFMA "v[48:51], %8, %2, 2\n" MFMA "v[52:55], %8, %3, 2\n" \
    MFMA "v[56:59], %8, %4, 2\n" MFMA "v[60:63], %8, %5, 2\n" MFMA "v[64:67], %8, %6, 2\n" MFMA "v[68:71], %8, %7, 2\n"
#define B_DOT8                                                                                                   \
    "v_dot4_i32_i8 %0, %0, %8, 1\nv_dot4_i32_i8 %1, %1, %8, 1\nv_dot4_i32_i8 %2, %2, %8, 1\nv_dot4_i32_i8 %3, %3, %8, 1\n" \
    "v_dot4_i32_i8 %4, %4, %8, 1\nv_dot4_i32_i8 %5, %5, %8, 1\nv_dot4_i32_i8 %6, %6, %8, 1\nv_dot4_i32_i8 %7, %7, %8, 1\n"
#define B_PKASHR8                                                                                                \
    "v_pk_ashrrev_i16 %0, 2, %0 op_sel_hi:[0,1]\nv_pk_ashrrev_i16 %1, 2, %1 op_sel_hi:[0,1]\nv_pk_ashrrev_i16 %2, 2, %2 op_sel_hi:[0,1]\n" \
    "v_pk_ashrrev_i16 %3, 2, %3 op_sel_hi:[0,1]\nv_pk_ashrrev_i16 %4, 2, %4 op_sel_hi:[0,1]\nv_pk_ashrrev_i16 %5, 2, %5 op_sel_hi:[0,1]\n" \
    "v_pk_ashrrev_i16 %6, 2, %6 op_sel_hi:[0,1]\nv_pk_ashrrev_i16 %7, 2, %7 op_sel_hi:[0,1]\n"
#define KERNEL(NAME, ASM)                                                                                        \
    __global__ __launch_bounds__(256) void NAME(unsigned *out, unsigned long long *ticks, unsigned seed)         \
    {                                                                                                            \
        unsigned a0 = threadIdx.x + seed, a1 = a0 * 3 + 1, a2 = a0 ^ 0x55, a3 = a0 + 7, a4 = a0 * 5, a5 = a0 + 11, \
                 a6 = a0 ^ 99, a7 = a0 + 13;                                                                     \
        unsigned b = seed | 1u;                                                                                  \
        asm volatile("v_mov_b32 v40, 0\n\tv_mov_b32 v44, 0" ::: "v40", "v44");                                   \
        const unsigned long long t0 = __builtin_readcyclecounter();                                              \
        for (int i = 0; i < ITER; i++) {                                                                         \
            asm volatile(ASM : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)     \
                         : "v"(b) : CLOBBERS);                                                                   \
        }                                                                                                        \
        asm volatile("s_nop 7" ::: CLOBBERS);                                                                    \
        const unsigned long long t1 = __builtin_readcyclecounter();                                              \
        out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;                             \
        if ((threadIdx.x & 63u) == 0u)                                                                           \
            ticks[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;                                                \
    }
KERNEL(k_base, B_BASE) KERNEL(k_mfma1, B_MFMA1) KERNEL(k_mfma2, B_MFMA2) KERNEL(k_dot3, B_DOT3) KERNEL(k_dot6, B_DOT6)
KERNEL(k_mfma8, B_MFMA8) KERNEL(k_dot8, B_DOT8) KERNEL(k_pkashr8, B_PKASHR8)

static int g_waves = 5;      // waves per SIMD: workgroups of 4 waves, g_waves of them per CU
template <typename K> double run(const char *name, K kern, unsigned *d, unsigned long long *ticks, double per_step)
{
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int blocks = 256 * g_waves;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d, ticks, 1u);
    hipEventRecord(e0);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d, ticks, 3u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    static unsigned long long host[256 * 8 * 4];
    hipMemcpy(host, ticks, sizeof(unsigned long long) * blocks * 4, hipMemcpyDeviceToHost);
    double sum = 0;
    for (int i = 0; i < blocks * 4; i++)
        sum += (double)host[i];
    // a wave's own loop time in counter ticks (s_memtime: 100 MHz on this part), and the wall time of the launch; per
    // SIMD, a step of every resident wave takes wall / ITER / (waves per SIMD)
    const double steps_per_simd = (double)ITER * g_waves;
    const double ns_step = ms * 1e6 / steps_per_simd;
    printf("%-10s %8.3f ms  %7.2f ns/step/SIMD  %7.2f cyc @2.4GHz  (%5.2f per %s)  wave ticks/step %.4f\n", name, ms, ns_step,
           ns_step * 2.4, ns_step * 2.4 / per_step, per_step == 8 ? "instr" : "VALU", sum / (blocks * 4) / ITER);
    return ns_step * 2.4;
}

static int layout(int only_lane)
{
    unsigned ha[64], hb[64], *da, *db; int hd[256], *dd;
    for (int l = 0; l < 64; l++) {
        signed char ab[4], bb[4];
        for (int k = 0; k < 4; k++) {
            ab[k] = (signed char)((l * 7 + k * 3) % 11 - 5);          // -5 .. 5, differs by lane and by k
            bb[k] = (signed char)((l * 5 + k * 13) % 255 - 127);
        }
        ha[l] = (unsigned char)ab[0] | (unsigned char)ab[1] << 8 | (unsigned char)ab[2] << 16 | (unsigned)(unsigned char)ab[3] << 24;
        hb[l] = (unsigned char)bb[0] | (unsigned char)bb[1] << 8 | (unsigned char)bb[2] << 16 | (unsigned)(unsigned char)bb[3] << 24;
    }
    hipMalloc(&da, 256); hipMalloc(&db, 256); hipMalloc(&dd, 1024);
    hipMemcpy(da, ha, 256, hipMemcpyHostToDevice); hipMemcpy(db, hb, 256, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, da, db, dd, only_lane);
    if (hipMemcpy(hd, dd, 1024, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    int good = 0, written = 0;
    for (int l = 0; l < 64; l++) {
        int want[4];
        for (int r = 0; r < 4; r++) {
            want[r] = 2;
            for (int k = 0; k < 4; k++)
                want[r] += (int)(signed char)(ha[(l & ~3) + r] >> (8 * k)) * (int)(signed char)(hb[l] >> (8 * k));
        }
        const bool ok = hd[4 * l] == want[0] && hd[4 * l + 1] == want[1] && hd[4 * l + 2] == want[2] && hd[4 * l + 3] == want[3];
        const bool untouched = hd[4 * l] == -1 && hd[4 * l + 1] == -1 && hd[4 * l + 2] == -1 && hd[4 * l + 3] == -1;
        good += ok; written += !untouched;
        if (only_lane < 0 || l == only_lane || (l & 15) == 0)
            printf("  lane %2d  A %08x B %08x  D %6d %6d %6d %6d  want %6d %6d %6d %6d %s\n", l, ha[l], hb[l], hd[4 * l], hd[4 * l + 1],
                   hd[4 * l + 2], hd[4 * l + 3], want[0], want[1], want[2], want[3], ok ? "ok" : (untouched ? "not written" : "DIFFERENT"));
    }
    printf("  lanes with the expected tuple: %d of 64; lanes whose registers were written: %d\n", good, written);
    hipFree(da); hipFree(db); hipFree(dd);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1)
        g_waves = atoi(argv[1]);
    if (g_waves < 1 || g_waves > 8)
        return 2;
    printf("(a) layout, every lane active: D[r] of lane l = 2 + sum_k A[lane (l & ~3) + r][k] * B[lane l][k]\n");
    if (layout(-1))
        return 1;
    printf("(a) the same with lane 61 alone active (EXEC = 1 << 61)\n");
    if (layout(61))
        return 1;
    printf("waves per SIMD: %d\n", g_waves);
    unsigned *d; hipMalloc(&d, 256 * 8 * 256 * 4);
    unsigned long long *ticks; hipMalloc(&ticks, 256 * 8 * 4 * 8);
    printf("(b) back to back, 8 independent destinations a step\n");
    run("mfma x8", k_mfma8, d, ticks, 8);
    run("dot4_i8 x8", k_dot8, d, ticks, 8);
    run("pkashr x8", k_pkashr8, d, ticks, 8);
    printf("(c) 4 v_xor + 2 v_perm + 2 v_mad_i32_i24 a step, and between them:\n");
    const double base = run("nothing", k_base, d, ticks, 8);
    const double m1 = run("1 mfma", k_mfma1, d, ticks, 8);
    const double m2 = run("2 mfma", k_mfma2, d, ticks, 8);
    const double d3 = run("3 dot4_i8", k_dot3, d, ticks, 8);
    const double d6 = run("6 dot4_i8", k_dot6, d, ticks, 8);
    const double base2 = run("nothing", k_base, d, ticks, 8);
    printf("price beside VALU, cycles @2.4GHz: one mfma %.2f (from 1), %.2f (from 2); three dot4_i8 %.2f (from 3), %.2f (from 6); base drift %.2f\n",
           m1 - base, (m2 - base) / 2, d3 - base, (d6 - base) / 2, base2 - base);
    return 0;
}
