// Dev probe 2: one opcode per kernel via inline asm (8 independent chains; v20 is kept free as a third, constant source;
// waves per SIMD = argv[1], default 8:
// the fused Hap Q encode kernel runs at 5).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#define ITER 4096
#define KERNEL(NAME, ASM)                                                                          \
    __global__ __launch_bounds__(256) void NAME(unsigned *out, unsigned seed)                      \
    {                                                                                              \
        unsigned a0 = threadIdx.x + seed, a1 = a0 * 3 + 1, a2 = a0 ^ 0x55, a3 = a0 + 7, a4 = a0 * 5, a5 = a0 + 11, \
                 a6 = a0 ^ 99, a7 = a0 + 13;                                                       \
        unsigned b = seed | 1u;                                                                    \
        for (int i = 0; i < ITER; i++) {                                                           \
            asm volatile(ASM(%0) ASM(%1) ASM(%2) ASM(%3) ASM(%4) ASM(%5) ASM(%6) ASM(%7)            \
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b) : "vcc", "s20", "s21", "v20"); \
        }                                                                                          \
        out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;               \
    }
#define A_ADD(x) "v_add_u32 " #x ", " #x ", %8\n"
#define A_AND(x) "v_and_b32 " #x ", " #x ", %8\n"
#define A_LSHL(x) "v_lshlrev_b32 " #x ", 1, " #x "\n"
#define A_BFE(x) "v_bfe_u32 " #x ", " #x ", 3, 8\n"
#define A_LSHLOR(x) "v_lshl_or_b32 " #x ", " #x ", 2, %8\n"
#define A_MINU(x) "v_min_u32 " #x ", " #x ", %8\n"
#define A_MINI(x) "v_min_i32 " #x ", " #x ", %8\n"
#define A_MINF(x) "v_min_f32 " #x ", " #x ", %8\n"
#define A_ADDF(x) "v_add_f32 " #x ", " #x ", %8\n"
#define A_FMA(x) "v_fma_f32 " #x ", " #x ", %8, " #x "\n"
#define A_CVTUB(x) "v_cvt_f32_ubyte0 " #x ", " #x "\n"
#define A_CVTU(x) "v_cvt_u32_f32 " #x ", " #x "\n"
#define A_MAD24(x) "v_mad_u32_u24 " #x ", " #x ", %8, " #x "\n"
#define A_MADI24(x) "v_mad_i32_i24 " #x ", " #x ", %8, " #x "\n"
#define A_CND(x) "v_cndmask_b32 " #x ", " #x ", %8, vcc\n"
#define A_CND64(x) "v_cndmask_b32_e64 " #x ", " #x ", %8, s[20:21]\n"
#define A_CMPCND(x) "v_cmp_lt_u32 vcc, " #x ", %8\nv_cndmask_b32 " #x ", " #x ", %8, vcc\n"
#define A_CMPCND64(x) "v_cmp_lt_u32_e64 s[20:21], " #x ", %8\nv_cndmask_b32_e64 " #x ", " #x ", %8, s[20:21]\n"
#define A_CMP(x) "v_cmp_lt_u32 vcc, " #x ", %8\n"
#define A_CMPF(x) "v_cmp_lt_f32 vcc, " #x ", %8\n"
#define A_MOV(x) "v_mov_b32 " #x ", %8\n"
#define A_XOR(x) "v_xor_b32 " #x ", " #x ", %8\n"
#define A_MIN3(x) "v_min3_u32 " #x ", " #x ", %8, " #x "\n"
#define A_MED3F(x) "v_med3_f32 " #x ", " #x ", %8, " #x "\n"
#define A_SAD(x) "v_sad_u32 " #x ", " #x ", %8, " #x "\n"
#define A_PKMIN(x) "v_pk_min_u16 " #x ", " #x ", %8\n"
#define A_PKFMA(x) "v_pk_fma_f32 " #x ", " #x ", " #x ", " #x "\n"
#define A_DOT4(x) "v_dot4_u32_u8 " #x ", " #x ", %8, " #x "\n"
#define A_FFBL(x) "v_ffbl_b32 " #x ", " #x "\n"
#define A_MBCNT(x) "v_mbcnt_lo_u32_b32 " #x ", " #x ", %8\n"
#define A_ADD3(x) "v_add3_u32 " #x ", " #x ", %8, " #x "\n"
#define A_OR(x) "v_or_b32 " #x ", " #x ", %8\n"
#define A_SUB(x) "v_sub_u32 " #x ", " #x ", %8\n"
#define A_LSHR(x) "v_lshrrev_b32 " #x ", 1, " #x "\n"
#define A_ASHR(x) "v_ashrrev_i32 " #x ", 1, " #x "\n"
#define A_LSHLADD(x) "v_lshl_add_u32 " #x ", " #x ", 2, %8\n"
#define A_ADDLSHL(x) "v_add_lshl_u32 " #x ", " #x ", %8, 2\n"
#define A_ANDOR(x) "v_and_or_b32 " #x ", " #x ", %8, " #x "\n"
#define A_OR3(x) "v_or3_b32 " #x ", " #x ", %8, " #x "\n"
#define A_BFI(x) "v_bfi_b32 " #x ", %8, " #x ", " #x "\n"
#define A_XAD(x) "v_xad_u32 " #x ", " #x ", %8, " #x "\n"
#define A_MADU16(x) "v_mad_u32_u16 " #x ", " #x ", %8, " #x "\n"
#define A_MADI16(x) "v_mad_i32_i16 " #x ", " #x ", %8, " #x "\n"
#define A_MUL24(x) "v_mul_u32_u24 " #x ", " #x ", %8\n"
#define A_PKADD(x) "v_pk_add_u16 " #x ", " #x ", %8\n"
#define A_PKLSHR(x) "v_pk_lshrrev_b16 " #x ", 1, " #x "\n"
#define A_PKMAD(x) "v_pk_mad_u16 " #x ", " #x ", %8, " #x "\n"
#define A_PKMAX(x) "v_pk_max_u16 " #x ", " #x ", %8\n"
#define A_ALIGNBIT(x) "v_alignbit_b32 " #x ", %8, " #x ", 2\n"
#define A_PERM(x) "v_perm_b32 " #x ", " #x ", %8, " #x "\n"
#define A_MED3I(x) "v_med3_i32 " #x ", " #x ", 0, 3\n"
#define A_MAX3(x) "v_max3_u32 " #x ", " #x ", %8, " #x "\n"
#define A_DOT2(x) "v_dot2_i32_i16 " #x ", " #x ", %8, " #x "\n"
#define A_BCNT(x) "v_bcnt_u32_b32 " #x ", " #x ", %8\n"
#define A_ADDDPP(x) "v_add_u32_dpp " #x ", " #x ", " #x " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
#define A_MOVDPP(x) "v_mov_b32_dpp " #x ", " #x " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
#define A_READLANE(x) "v_readlane_b32 s20, " #x ", 5\n"
#define A_MULLO(x) "v_mul_lo_u32 " #x ", " #x ", %8\n"
#define A_MULHI(x) "v_mul_hi_u32 " #x ", " #x ", %8\n"
#define A_BITOP3(x) "v_bitop3_b32 " #x ", " #x ", %8, " #x " bitop3:0x48\n"
#define A_CMPSDWA(x) "v_cmp_ne_u32_sdwa s[20:21], " #x ", %8 src0_sel:WORD_0 src1_sel:WORD_0\n"
#define A_ADDC64(x) "v_addc_co_u32_e64 " #x ", s[20:21], " #x ", " #x ", s[20:21]\n"
#define A_CMPADDC64(x) "v_cmp_ne_u32_e64 s[20:21], " #x ", %8\nv_addc_co_u32_e64 " #x ", s[20:21], " #x ", " #x ", s[20:21]\n"
#define A_PKSUBI(x) "v_pk_sub_i16 " #x ", " #x ", %8\n"
#define A_PKLSHL(x) "v_pk_lshlrev_b16 " #x ", 1, " #x " op_sel_hi:[0,1]\n"
#define A_PKMAXI(x) "v_pk_max_i16 " #x ", " #x ", %8\n"
#define A_PKMINI(x) "v_pk_min_i16 " #x ", " #x ", %8\n"
#define A_UDOT2(x) "v_dot2_u32_u16 " #x ", " #x ", %8, " #x "\n"
#define A_DOT2C(x) "v_dot2c_i32_i16 " #x ", " #x ", %8\n"
#define A_MAXI16(x) "v_max_i16 " #x ", " #x ", %8\n"
#define A_ASHRI16(x) "v_ashrrev_i16 " #x ", 1, " #x "\n"
#define A_SUBU16(x) "v_sub_u16 " #x ", " #x ", %8\n"
// round 12: the Co | Cg pack -- a 32-bit arithmetic shift straight into a half of its destination (SDWA), the second
// one keeping the first one's half, and the two back to back on one register as the kernel would issue them; beside
// it the packed shift and the v_perm_b32 + packed shift pair they would replace
#define A_ASHRSDWA0(x) "v_ashrrev_i32_sdwa " #x ", 2, " #x " dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n"
#define A_ASHRSDWA1(x) "v_ashrrev_i32_sdwa " #x ", 2, %8 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n"
#define A_ASHRSDWA01(x) "v_ashrrev_i32_sdwa " #x ", 2, " #x " dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n" \
                        "s_nop 0\n"                                                                                                  \
                        "v_ashrrev_i32_sdwa " #x ", 2, %8 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n"
#define A_PKASHRI(x) "v_pk_ashrrev_i16 " #x ", 2, " #x " op_sel_hi:[0,1]\n"
#define A_PERMPKASHR(x) "v_perm_b32 " #x ", %8, " #x ", s22\nv_pk_ashrrev_i16 " #x ", 2, " #x " op_sel_hi:[0,1]\n"
// round 13: the colour box on non-negative Co | Cg pairs -- the three-input packed half minimum / maximum (two and three
// distinct sources, as the box's steps and its padded last step have them) and v_add3_u32 on words holding pairs
#define A_PKMINIMUM3(x) "v_pk_minimum3_f16 " #x ", " #x ", %8, " #x "\n"
#define A_PKMAXIMUM3(x) "v_pk_maximum3_f16 " #x ", " #x ", %8, " #x "\n"
#define A_PKMINIMUM3V(x) "v_pk_minimum3_f16 " #x ", " #x ", %8, v20\n"
#define A_ADD3PAIRS(x) "v_add3_u32 " #x ", " #x ", %8, v20\n"
KERNEL(k_pkminimum3, A_PKMINIMUM3) KERNEL(k_pkmaximum3, A_PKMAXIMUM3) KERNEL(k_pkminimum3v, A_PKMINIMUM3V) KERNEL(k_add3pairs, A_ADD3PAIRS)
KERNEL(k_ashrsdwa0, A_ASHRSDWA0) KERNEL(k_ashrsdwa1, A_ASHRSDWA1) KERNEL(k_ashrsdwa01, A_ASHRSDWA01) KERNEL(k_pkashri, A_PKASHRI)
KERNEL(k_permpkashr, A_PERMPKASHR)
KERNEL(k_add, A_ADD) KERNEL(k_and, A_AND) KERNEL(k_lshl, A_LSHL) KERNEL(k_bfe, A_BFE) KERNEL(k_lshlor, A_LSHLOR)
KERNEL(k_minu, A_MINU) KERNEL(k_mini, A_MINI) KERNEL(k_minf, A_MINF) KERNEL(k_addf, A_ADDF) KERNEL(k_fma, A_FMA)
KERNEL(k_cvtub, A_CVTUB) KERNEL(k_cvtu, A_CVTU) KERNEL(k_mad24, A_MAD24) KERNEL(k_madi24, A_MADI24) KERNEL(k_cnd, A_CND)
KERNEL(k_cmp, A_CMP) KERNEL(k_cmpf, A_CMPF) KERNEL(k_mov, A_MOV) KERNEL(k_xor, A_XOR) KERNEL(k_min3, A_MIN3)
KERNEL(k_med3f, A_MED3F) KERNEL(k_sad, A_SAD) KERNEL(k_pkmin, A_PKMIN) KERNEL(k_dot4, A_DOT4) KERNEL(k_ffbl, A_FFBL)
KERNEL(k_mbcnt, A_MBCNT) KERNEL(k_add3, A_ADD3) KERNEL(k_cnd64, A_CND64) KERNEL(k_cmpcnd, A_CMPCND) KERNEL(k_cmpcnd64, A_CMPCND64)
KERNEL(k_or, A_OR) KERNEL(k_sub, A_SUB) KERNEL(k_lshr, A_LSHR) KERNEL(k_ashr, A_ASHR) KERNEL(k_lshladd, A_LSHLADD)
KERNEL(k_addlshl, A_ADDLSHL) KERNEL(k_andor, A_ANDOR) KERNEL(k_or3, A_OR3) KERNEL(k_bfi, A_BFI) KERNEL(k_xad, A_XAD)
KERNEL(k_madu16, A_MADU16) KERNEL(k_madi16, A_MADI16) KERNEL(k_mul24, A_MUL24) KERNEL(k_pkadd, A_PKADD) KERNEL(k_pklshr, A_PKLSHR)
KERNEL(k_pkmad, A_PKMAD) KERNEL(k_pkmax, A_PKMAX) KERNEL(k_alignbit, A_ALIGNBIT) KERNEL(k_perm, A_PERM) KERNEL(k_med3i, A_MED3I)
KERNEL(k_max3, A_MAX3) KERNEL(k_dot2, A_DOT2) KERNEL(k_bcnt, A_BCNT) KERNEL(k_adddpp, A_ADDDPP) KERNEL(k_movdpp, A_MOVDPP)
KERNEL(k_readlane, A_READLANE) KERNEL(k_mullo, A_MULLO) KERNEL(k_mulhi, A_MULHI) KERNEL(k_bitop3, A_BITOP3)
KERNEL(k_cmpsdwa, A_CMPSDWA) KERNEL(k_addc64, A_ADDC64) KERNEL(k_cmpaddc64, A_CMPADDC64)
KERNEL(k_pksubi, A_PKSUBI) KERNEL(k_pklshl, A_PKLSHL) KERNEL(k_pkmaxi, A_PKMAXI) KERNEL(k_pkmini, A_PKMINI) KERNEL(k_udot2, A_UDOT2)
KERNEL(k_dot2c, A_DOT2C) KERNEL(k_maxi16, A_MAXI16) KERNEL(k_ashri16, A_ASHRI16) KERNEL(k_subu16, A_SUBU16)
static int g_waves = 8;      // waves per SIMD: workgroups of 4 waves, g_waves of them per CU
template <typename K> void run(const char *name, K kern, unsigned *d)
{
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int blocks = 256 * g_waves;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d, 1u);
    hipEventRecord(e0);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d, 3u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double instr_per_simd = blocks * 4.0 / 1024.0 * ITER * 8;
    printf("%-22s %7.3f ms  %.2f ns/instr/SIMD (%.2f cyc @2.4GHz)\n", name, ms, ms * 1e6 / instr_per_simd, ms * 1e6 / instr_per_simd * 2.4);
}
int main(int argc, char **argv)
{
    if (argc > 1)
        g_waves = atoi(argv[1]);
    if (g_waves < 1 || g_waves > 8)
        return 2;
    printf("waves per SIMD: %d\n", g_waves);
    unsigned *d; hipMalloc(&d, 256 * 8 * 256 * 4);
#define RUN(n) run(#n, n, d);
    RUN(k_add) RUN(k_and) RUN(k_xor) RUN(k_lshl) RUN(k_bfe) RUN(k_lshlor) RUN(k_add3) RUN(k_minu) RUN(k_mini) RUN(k_min3) RUN(k_sad) RUN(k_mad24) RUN(k_madi24)
    RUN(k_dot4) RUN(k_pkmin) RUN(k_ffbl) RUN(k_mbcnt) RUN(k_mov) RUN(k_cnd) RUN(k_cnd64) RUN(k_cmpcnd) RUN(k_cmpcnd64) RUN(k_cmp) RUN(k_cmpf) RUN(k_minf) RUN(k_addf) RUN(k_fma) RUN(k_med3f) RUN(k_cvtub) RUN(k_cvtu)
    RUN(k_or) RUN(k_sub) RUN(k_lshr) RUN(k_ashr) RUN(k_lshladd) RUN(k_addlshl) RUN(k_andor) RUN(k_or3) RUN(k_bfi) RUN(k_xad) RUN(k_madu16) RUN(k_madi16)
    RUN(k_mul24) RUN(k_pkadd) RUN(k_pklshr) RUN(k_pkmad) RUN(k_pkmax) RUN(k_alignbit) RUN(k_perm) RUN(k_med3i) RUN(k_max3) RUN(k_dot2) RUN(k_bcnt)
    RUN(k_adddpp) RUN(k_movdpp) RUN(k_readlane)
    RUN(k_mullo) RUN(k_mulhi) RUN(k_bitop3) RUN(k_cmpsdwa) RUN(k_addc64) RUN(k_cmpaddc64)       // (two-instruction kernels: cycles per PAIR)
    RUN(k_pksubi) RUN(k_pklshl) RUN(k_pkmaxi) RUN(k_pkmini) RUN(k_udot2) RUN(k_dot2c) RUN(k_maxi16) RUN(k_ashri16) RUN(k_subu16)      // round 11: the pair form
    RUN(k_ashrsdwa0) RUN(k_ashrsdwa1) RUN(k_pkashri) RUN(k_ashrsdwa01) RUN(k_permpkashr)      // round 12: the Co | Cg pack (the last two: cycles per PAIR)
    RUN(k_pkminimum3) RUN(k_pkmaximum3) RUN(k_pkminimum3v) RUN(k_add3pairs)      // round 13: the box and the sums on non-negative pairs
    return 0;
}
