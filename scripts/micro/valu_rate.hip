// Microbenchmark (development aid): issue rate of integer vector instructions on gfx950 as a function of the
// number of waves per SIMD.  Question it answers: which wave64 integer instructions take 2 and which 4 cycles of a
// SIMD when several waves share it (SQ_ACTIVE_INST_VALU counts 4 per instruction either way)?
//   hipcc -O3 --offload-arch=gfx950 -o scripts/micro/valu_rate.bin scripts/micro/valu_rate.hip
// (eight independent accumulators per op; `valu_rate.bin selects` runs the select modes and their yardsticks only)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define REP8(x) x x x x x x x x
#define REP4(x) x x x x
template <int MODE>
__global__ __launch_bounds__(64) void k(uint32_t *out, int iters)
{
    extern __shared__ uint8_t pad[];
    uint32_t a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    const uint32_t b = blockIdx.x | 1u;
    const uint32_t m = 0u - (threadIdx.x & 1u);                   // a 0 / -1 lane mask in a VGPR (modes 36..39 and 50)
    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0, t7 = 0;
    for (int i = 0; i < iters; i++) {
        if (MODE == 0) { REP8(asm volatile("v_add_u32 %0, %0, %8\n\tv_add_u32 %1, %1, %8\n\tv_add_u32 %2, %2, %8\n\tv_add_u32 %3, %3, %8\n\tv_add_u32 %4, %4, %8\n\tv_add_u32 %5, %5, %8\n\tv_add_u32 %6, %6, %8\n\tv_add_u32 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 1) { REP8(asm volatile("v_and_b32 %0, %0, %8\n\tv_and_b32 %1, %1, %8\n\tv_and_b32 %2, %2, %8\n\tv_and_b32 %3, %3, %8\n\tv_and_b32 %4, %4, %8\n\tv_and_b32 %5, %5, %8\n\tv_and_b32 %6, %6, %8\n\tv_and_b32 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 2) { REP8(asm volatile("v_or_b32 %0, %0, %8\n\tv_or_b32 %1, %1, %8\n\tv_or_b32 %2, %2, %8\n\tv_or_b32 %3, %3, %8\n\tv_or_b32 %4, %4, %8\n\tv_or_b32 %5, %5, %8\n\tv_or_b32 %6, %6, %8\n\tv_or_b32 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 3) { REP8(asm volatile("v_lshlrev_b32 %0, 1, %0\n\tv_lshlrev_b32 %1, 1, %1\n\tv_lshlrev_b32 %2, 1, %2\n\tv_lshlrev_b32 %3, 1, %3\n\tv_lshlrev_b32 %4, 1, %4\n\tv_lshlrev_b32 %5, 1, %5\n\tv_lshlrev_b32 %6, 1, %6\n\tv_lshlrev_b32 %7, 1, %7" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 4) { REP8(asm volatile("v_lshrrev_b32 %0, %8, %0\n\tv_lshrrev_b32 %1, %8, %1\n\tv_lshrrev_b32 %2, %8, %2\n\tv_lshrrev_b32 %3, %8, %3\n\tv_lshrrev_b32 %4, %8, %4\n\tv_lshrrev_b32 %5, %8, %5\n\tv_lshrrev_b32 %6, %8, %6\n\tv_lshrrev_b32 %7, %8, %7" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 5) { REP8(asm volatile("v_min_u32 %0, %0, %8\n\tv_min_u32 %1, %1, %8\n\tv_min_u32 %2, %2, %8\n\tv_min_u32 %3, %3, %8\n\tv_min_u32 %4, %4, %8\n\tv_min_u32 %5, %5, %8\n\tv_min_u32 %6, %6, %8\n\tv_min_u32 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 6) { REP8(asm volatile("v_mov_b32 %0, %8\n\tv_mov_b32 %1, %8\n\tv_mov_b32 %2, %8\n\tv_mov_b32 %3, %8\n\tv_mov_b32 %4, %8\n\tv_mov_b32 %5, %8\n\tv_mov_b32 %6, %8\n\tv_mov_b32 %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 7) { REP8(asm volatile("v_cndmask_b32 %0, %0, %8, vcc\n\tv_cndmask_b32 %1, %1, %8, vcc\n\tv_cndmask_b32 %2, %2, %8, vcc\n\tv_cndmask_b32 %3, %3, %8, vcc\n\tv_cndmask_b32 %4, %4, %8, vcc\n\tv_cndmask_b32 %5, %5, %8, vcc\n\tv_cndmask_b32 %6, %6, %8, vcc\n\tv_cndmask_b32 %7, %7, %8, vcc" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 8) { REP8(asm volatile("v_cmp_lt_u32 vcc, %0, %8\n\tv_cmp_lt_u32 vcc, %1, %8\n\tv_cmp_lt_u32 vcc, %2, %8\n\tv_cmp_lt_u32 vcc, %3, %8\n\tv_cmp_lt_u32 vcc, %4, %8\n\tv_cmp_lt_u32 vcc, %5, %8\n\tv_cmp_lt_u32 vcc, %6, %8\n\tv_cmp_lt_u32 vcc, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b) : "vcc");) }
        if (MODE == 9) { REP8(asm volatile("v_cmp_lt_u32 s[20:21], %0, %8\n\tv_cmp_lt_u32 s[20:21], %1, %8\n\tv_cmp_lt_u32 s[20:21], %2, %8\n\tv_cmp_lt_u32 s[20:21], %3, %8\n\tv_cmp_lt_u32 s[20:21], %4, %8\n\tv_cmp_lt_u32 s[20:21], %5, %8\n\tv_cmp_lt_u32 s[20:21], %6, %8\n\tv_cmp_lt_u32 s[20:21], %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b) : "s20", "s21");) }
        if (MODE == 10) { REP8(asm volatile("v_bfe_u32 %0, %0, 1, 30\n\tv_bfe_u32 %1, %1, 1, 30\n\tv_bfe_u32 %2, %2, 1, 30\n\tv_bfe_u32 %3, %3, 1, 30\n\tv_bfe_u32 %4, %4, 1, 30\n\tv_bfe_u32 %5, %5, 1, 30\n\tv_bfe_u32 %6, %6, 1, 30\n\tv_bfe_u32 %7, %7, 1, 30" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 11) { REP8(asm volatile("v_and_or_b32 %0, %0, %8, %8\n\tv_and_or_b32 %1, %1, %8, %8\n\tv_and_or_b32 %2, %2, %8, %8\n\tv_and_or_b32 %3, %3, %8, %8\n\tv_and_or_b32 %4, %4, %8, %8\n\tv_and_or_b32 %5, %5, %8, %8\n\tv_and_or_b32 %6, %6, %8, %8\n\tv_and_or_b32 %7, %7, %8, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 12) { REP8(asm volatile("v_lshl_add_u32 %0, %0, 1, %8\n\tv_lshl_add_u32 %1, %1, 1, %8\n\tv_lshl_add_u32 %2, %2, 1, %8\n\tv_lshl_add_u32 %3, %3, 1, %8\n\tv_lshl_add_u32 %4, %4, 1, %8\n\tv_lshl_add_u32 %5, %5, 1, %8\n\tv_lshl_add_u32 %6, %6, 1, %8\n\tv_lshl_add_u32 %7, %7, 1, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 13) { REP8(asm volatile("v_lshl_or_b32 %0, %0, 1, %8\n\tv_lshl_or_b32 %1, %1, 1, %8\n\tv_lshl_or_b32 %2, %2, 1, %8\n\tv_lshl_or_b32 %3, %3, 1, %8\n\tv_lshl_or_b32 %4, %4, 1, %8\n\tv_lshl_or_b32 %5, %5, 1, %8\n\tv_lshl_or_b32 %6, %6, 1, %8\n\tv_lshl_or_b32 %7, %7, 1, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 14) { REP8(asm volatile("v_add3_u32 %0, %0, %8, %8\n\tv_add3_u32 %1, %1, %8, %8\n\tv_add3_u32 %2, %2, %8, %8\n\tv_add3_u32 %3, %3, %8, %8\n\tv_add3_u32 %4, %4, %8, %8\n\tv_add3_u32 %5, %5, %8, %8\n\tv_add3_u32 %6, %6, %8, %8\n\tv_add3_u32 %7, %7, %8, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 15) { REP8(asm volatile("v_alignbyte_b32 %0, %0, %8, %8\n\tv_alignbyte_b32 %1, %1, %8, %8\n\tv_alignbyte_b32 %2, %2, %8, %8\n\tv_alignbyte_b32 %3, %3, %8, %8\n\tv_alignbyte_b32 %4, %4, %8, %8\n\tv_alignbyte_b32 %5, %5, %8, %8\n\tv_alignbyte_b32 %6, %6, %8, %8\n\tv_alignbyte_b32 %7, %7, %8, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 16) { REP8(asm volatile("v_perm_b32 %0, %0, %8, %8\n\tv_perm_b32 %1, %1, %8, %8\n\tv_perm_b32 %2, %2, %8, %8\n\tv_perm_b32 %3, %3, %8, %8\n\tv_perm_b32 %4, %4, %8, %8\n\tv_perm_b32 %5, %5, %8, %8\n\tv_perm_b32 %6, %6, %8, %8\n\tv_perm_b32 %7, %7, %8, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 17) { REP8(asm volatile("v_mov_b32_dpp %0, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %2, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %3, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %4, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %5, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %6, %8 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %7, %8 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 18) { REP8(asm volatile("v_add_u32_dpp %0, %8, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %1, %8, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %2, %8, %2 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %3, %8, %3 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %4, %8, %4 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %5, %8, %5 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %6, %8, %6 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_add_u32_dpp %7, %8, %7 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 19) { REP8(asm volatile("v_add_u32_sdwa %0, %0, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %1, %1, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %2, %2, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %3, %3, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %4, %4, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %5, %5, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %6, %6, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\tv_add_u32_sdwa %7, %7, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 20) { REP8(asm volatile("v_pk_add_u16 %0, %0, %8\n\tv_pk_add_u16 %1, %1, %8\n\tv_pk_add_u16 %2, %2, %8\n\tv_pk_add_u16 %3, %3, %8\n\tv_pk_add_u16 %4, %4, %8\n\tv_pk_add_u16 %5, %5, %8\n\tv_pk_add_u16 %6, %6, %8\n\tv_pk_add_u16 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 21) { REP8(asm volatile("v_pk_min_u16 %0, %0, %8\n\tv_pk_min_u16 %1, %1, %8\n\tv_pk_min_u16 %2, %2, %8\n\tv_pk_min_u16 %3, %3, %8\n\tv_pk_min_u16 %4, %4, %8\n\tv_pk_min_u16 %5, %5, %8\n\tv_pk_min_u16 %6, %6, %8\n\tv_pk_min_u16 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 22) { REP8(asm volatile("v_mul_u32_u24 %0, %0, %8\n\tv_mul_u32_u24 %1, %1, %8\n\tv_mul_u32_u24 %2, %2, %8\n\tv_mul_u32_u24 %3, %3, %8\n\tv_mul_u32_u24 %4, %4, %8\n\tv_mul_u32_u24 %5, %5, %8\n\tv_mul_u32_u24 %6, %6, %8\n\tv_mul_u32_u24 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 23) { REP8(asm volatile("v_mad_u32_u24 %0, %0, %8, %8\n\tv_mad_u32_u24 %1, %1, %8, %8\n\tv_mad_u32_u24 %2, %2, %8, %8\n\tv_mad_u32_u24 %3, %3, %8, %8\n\tv_mad_u32_u24 %4, %4, %8, %8\n\tv_mad_u32_u24 %5, %5, %8, %8\n\tv_mad_u32_u24 %6, %6, %8, %8\n\tv_mad_u32_u24 %7, %7, %8, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 24) { REP8(asm volatile("v_mul_lo_u32 %0, %0, %8\n\tv_mul_lo_u32 %1, %1, %8\n\tv_mul_lo_u32 %2, %2, %8\n\tv_mul_lo_u32 %3, %3, %8\n\tv_mul_lo_u32 %4, %4, %8\n\tv_mul_lo_u32 %5, %5, %8\n\tv_mul_lo_u32 %6, %6, %8\n\tv_mul_lo_u32 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 25) { REP8(asm volatile("v_mbcnt_lo_u32_b32 %0, %8, %0\n\tv_mbcnt_lo_u32_b32 %1, %8, %1\n\tv_mbcnt_lo_u32_b32 %2, %8, %2\n\tv_mbcnt_lo_u32_b32 %3, %8, %3\n\tv_mbcnt_lo_u32_b32 %4, %8, %4\n\tv_mbcnt_lo_u32_b32 %5, %8, %5\n\tv_mbcnt_lo_u32_b32 %6, %8, %6\n\tv_mbcnt_lo_u32_b32 %7, %8, %7" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (MODE == 26) { REP8(asm volatile("v_readlane_b32 s20, %0, 3\n\tv_readlane_b32 s20, %1, 3\n\tv_readlane_b32 s20, %2, 3\n\tv_readlane_b32 s20, %3, 3\n\tv_readlane_b32 s20, %4, 3\n\tv_readlane_b32 s20, %5, 3\n\tv_readlane_b32 s20, %6, 3\n\tv_readlane_b32 s20, %7, 3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b) : "s20");) }
        if (MODE == 27) { REP8(asm volatile("v_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %2\n\tv_permlane32_swap_b32 %2, %3\n\tv_permlane32_swap_b32 %3, %4\n\tv_permlane32_swap_b32 %4, %5\n\tv_permlane32_swap_b32 %5, %6\n\tv_permlane32_swap_b32 %6, %7\n\tv_permlane32_swap_b32 %7, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        // Select forms and their replacements (modes 28..42; runs of selects: modes 43..51 below).  A8 is the eight-chain operand list; the selects' condition
        // registers are written by two s_mov per 64 vector instructions so that no mode reads an unwritten mask.
#define A8 "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
#define T8 "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3), "+v"(t4), "+v"(t5), "+v"(t6), "+v"(t7)
#define SETVCC "s_mov_b32 vcc_lo, 0x55555555\n\ts_mov_b32 vcc_hi, 0x33333333\n\t"
#define SETS20 "s_mov_b32 s20, 0x55555555\n\ts_mov_b32 s21, 0x33333333\n\t"
#define ADD7 "v_add_u32 %1, %1, %8\n\tv_add_u32 %2, %2, %8\n\tv_add_u32 %3, %3, %8\n\tv_add_u32 %4, %4, %8\n\tv_add_u32 %5, %5, %8\n\tv_add_u32 %6, %6, %8\n\tv_add_u32 %7, %7, %8\n\t"
#define ADD6 "v_add_u32 %2, %2, %8\n\tv_add_u32 %3, %3, %8\n\tv_add_u32 %4, %4, %8\n\tv_add_u32 %5, %5, %8\n\tv_add_u32 %6, %6, %8\n\tv_add_u32 %7, %7, %8\n\t"
#define BFE8 "v_bfe_i32 %0, %0, 4, 1\n\tv_bfe_i32 %1, %1, 4, 1\n\tv_bfe_i32 %2, %2, 4, 1\n\tv_bfe_i32 %3, %3, 4, 1\n\tv_bfe_i32 %4, %4, 4, 1\n\tv_bfe_i32 %5, %5, 4, 1\n\tv_bfe_i32 %6, %6, 4, 1\n\tv_bfe_i32 %7, %7, 4, 1\n\t"
#define ADD6B "v_add_u32 %2, %2, %16\n\tv_add_u32 %3, %3, %16\n\tv_add_u32 %4, %4, %16\n\tv_add_u32 %5, %5, %16\n\tv_add_u32 %6, %6, %16\n\tv_add_u32 %7, %7, %16\n\t"   // ADD6 where T8 stands between A8 and b (mode 42)
#define EACH8(pre, post) pre "%0" post "%0\n\t" pre "%1" post "%1\n\t" pre "%2" post "%2\n\t" pre "%3" post "%3\n\t" pre "%4" post "%4\n\t" pre "%5" post "%5\n\t" pre "%6" post "%6\n\t" pre "%7" post "%7\n\t"
        if (MODE == 28) { asm volatile(SETVCC REP8("v_cndmask_b32 %0, %0, %8, vcc\n\tv_cndmask_b32 %1, %1, %8, vcc\n\tv_cndmask_b32 %2, %2, %8, vcc\n\tv_cndmask_b32 %3, %3, %8, vcc\n\tv_cndmask_b32 %4, %4, %8, vcc\n\tv_cndmask_b32 %5, %5, %8, vcc\n\tv_cndmask_b32 %6, %6, %8, vcc\n\tv_cndmask_b32 %7, %7, %8, vcc\n\t") : A8 : "v"(b) : "vcc"); }
        if (MODE == 29) { asm volatile(SETVCC REP8("v_cndmask_b32 %0, %0, %8, vcc\n\t" ADD7) : A8 : "v"(b) : "vcc"); }
        if (MODE == 30) { asm volatile(REP4("v_cmp_lt_u32 vcc, %0, %8\n\tv_cndmask_b32 %0, %0, %8, vcc\n\tv_cmp_lt_u32 vcc, %1, %8\n\tv_cndmask_b32 %1, %1, %8, vcc\n\tv_cmp_lt_u32 vcc, %2, %8\n\tv_cndmask_b32 %2, %2, %8, vcc\n\tv_cmp_lt_u32 vcc, %3, %8\n\tv_cndmask_b32 %3, %3, %8, vcc\n\tv_cmp_lt_u32 vcc, %4, %8\n\tv_cndmask_b32 %4, %4, %8, vcc\n\tv_cmp_lt_u32 vcc, %5, %8\n\tv_cndmask_b32 %5, %5, %8, vcc\n\tv_cmp_lt_u32 vcc, %6, %8\n\tv_cndmask_b32 %6, %6, %8, vcc\n\tv_cmp_lt_u32 vcc, %7, %8\n\tv_cndmask_b32 %7, %7, %8, vcc\n\t") : A8 : "v"(b) : "vcc"); }
        if (MODE == 31) { asm volatile(REP8("v_cmp_lt_u32 vcc, %0, %8\n\tv_cndmask_b32 %0, %1, %8, vcc\n\t" ADD6) : A8 : "v"(b) : "vcc"); }
        if (MODE == 32) { asm volatile(SETS20 REP8("v_cndmask_b32_e64 %0, %0, %8, s[20:21]\n\tv_cndmask_b32_e64 %1, %1, %8, s[20:21]\n\tv_cndmask_b32_e64 %2, %2, %8, s[20:21]\n\tv_cndmask_b32_e64 %3, %3, %8, s[20:21]\n\tv_cndmask_b32_e64 %4, %4, %8, s[20:21]\n\tv_cndmask_b32_e64 %5, %5, %8, s[20:21]\n\tv_cndmask_b32_e64 %6, %6, %8, s[20:21]\n\tv_cndmask_b32_e64 %7, %7, %8, s[20:21]\n\t") : A8 : "v"(b) : "s20", "s21"); }
        if (MODE == 33) { asm volatile(SETS20 REP8("v_cndmask_b32_e64 %0, %0, %8, s[20:21]\n\t" ADD7) : A8 : "v"(b) : "s20", "s21"); }
        if (MODE == 34) { asm volatile(REP4("v_cmp_lt_u32_e64 s[20:21], %0, %8\n\tv_cndmask_b32_e64 %0, %0, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %1, %8\n\tv_cndmask_b32_e64 %1, %1, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %2, %8\n\tv_cndmask_b32_e64 %2, %2, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %3, %8\n\tv_cndmask_b32_e64 %3, %3, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %4, %8\n\tv_cndmask_b32_e64 %4, %4, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %5, %8\n\tv_cndmask_b32_e64 %5, %5, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %6, %8\n\tv_cndmask_b32_e64 %6, %6, %8, s[20:21]\n\tv_cmp_lt_u32_e64 s[20:21], %7, %8\n\tv_cndmask_b32_e64 %7, %7, %8, s[20:21]\n\t") : A8 : "v"(b) : "s20", "s21"); }
        if (MODE == 35) { asm volatile(REP8("v_cmp_lt_u32_e64 s[20:21], %0, %8\n\tv_cndmask_b32_e64 %0, %1, %8, s[20:21]\n\t" ADD6) : A8 : "v"(b) : "s20", "s21"); }
        if (MODE == 36) { asm volatile(REP8(EACH8("v_bfi_b32 ", ", %9, %8, ")) : A8 : "v"(b), "v"(m)); }
        if (MODE == 37) { asm volatile(REP8("v_bfi_b32 %0, %9, %8, %0\n\t" ADD7) : A8 : "v"(b), "v"(m)); }
        if (MODE == 38) { asm volatile(REP4("v_and_b32 %8, %16, %17\n\tv_and_or_b32 %0, %0, %18, %8\n\tv_and_b32 %9, %16, %17\n\tv_and_or_b32 %1, %1, %18, %9\n\tv_and_b32 %10, %16, %17\n\tv_and_or_b32 %2, %2, %18, %10\n\tv_and_b32 %11, %16, %17\n\tv_and_or_b32 %3, %3, %18, %11\n\tv_and_b32 %12, %16, %17\n\tv_and_or_b32 %4, %4, %18, %12\n\tv_and_b32 %13, %16, %17\n\tv_and_or_b32 %5, %5, %18, %13\n\tv_and_b32 %14, %16, %17\n\tv_and_or_b32 %6, %6, %18, %14\n\tv_and_b32 %15, %16, %17\n\tv_and_or_b32 %7, %7, %18, %15\n\t") : A8, T8 : "v"(b), "v"(m), "v"(~m)); }
        if (MODE == 39) { asm volatile(REP4("v_xor_b32 %8, %0, %16\n\tv_and_b32 %8, %8, %17\n\tv_xor_b32 %0, %0, %8\n\tv_xor_b32 %9, %1, %16\n\tv_and_b32 %9, %9, %17\n\tv_xor_b32 %1, %1, %9\n\tv_xor_b32 %10, %2, %16\n\tv_and_b32 %10, %10, %17\n\tv_xor_b32 %2, %2, %10\n\tv_xor_b32 %11, %3, %16\n\tv_and_b32 %11, %11, %17\n\tv_xor_b32 %3, %3, %11\n\tv_xor_b32 %12, %4, %16\n\tv_and_b32 %12, %12, %17\n\tv_xor_b32 %4, %4, %12\n\tv_xor_b32 %13, %5, %16\n\tv_and_b32 %13, %13, %17\n\tv_xor_b32 %5, %5, %13\n\tv_xor_b32 %14, %6, %16\n\tv_and_b32 %14, %14, %17\n\tv_xor_b32 %6, %6, %14\n\tv_xor_b32 %15, %7, %16\n\tv_and_b32 %15, %15, %17\n\tv_xor_b32 %7, %7, %15\n\t") : A8, T8 : "v"(b), "v"(m)); }
        if (MODE == 40) { asm volatile(REP4(EACH8("v_sub_u32 ", ", %8, ") EACH8("v_ashrrev_i32 ", ", 31, ")) : A8 : "v"(b)); }
        if (MODE == 41) { asm volatile(REP8(BFE8 ) : A8 : "v"(b)); }
        if (MODE == 42) { asm volatile(REP8("v_sub_u32 %8, %0, %16\n\tv_ashrrev_i32 %8, 31, %8\n\tv_bfi_b32 %0, %8, %16, %1\n\t" ADD6B) : A8, T8 : "v"(b)); }
        // Runs of selects on one condition, the shape the compiler emits for several values chosen by one test
        // (modes 43..51): r selects in a row, the rest of each group of eight is v_add_u32.
#define C32(n) "v_cndmask_b32 %" #n ", %" #n ", %8, vcc\n\t"
#define C64(n) "v_cndmask_b32_e64 %" #n ", %" #n ", %8, s[20:21]\n\t"
#define BF(n) "v_bfi_b32 %" #n ", %9, %8, %" #n "\n\t"
#define AD(n) "v_add_u32 %" #n ", %" #n ", %8\n\t"
        if (MODE == 43) { asm volatile(SETVCC REP8(C32(0) C32(1) AD(2) AD(3) AD(4) AD(5) AD(6) AD(7)) : A8 : "v"(b) : "vcc"); }
        if (MODE == 44) { asm volatile(SETVCC REP8(C32(0) C32(1) C32(2) C32(3) AD(4) AD(5) AD(6) AD(7)) : A8 : "v"(b) : "vcc"); }
        if (MODE == 45) { asm volatile(SETVCC REP8(C32(0) C32(1) C32(2) C32(3) C32(4) C32(5) AD(6) AD(7)) : A8 : "v"(b) : "vcc"); }
        if (MODE == 46) { asm volatile(SETVCC REP8(C32(0) AD(1) C32(2) AD(3) C32(4) AD(5) C32(6) AD(7)) : A8 : "v"(b) : "vcc"); }
        if (MODE == 47) { asm volatile(REP8("v_cmp_lt_u32 vcc, %7, %8\n\t" C32(0) C32(1) C32(2) C32(3) AD(4) AD(5) AD(6)) : A8 : "v"(b) : "vcc"); }
        if (MODE == 48) { asm volatile(SETVCC SETS20 REP8(C64(0) C64(1) C64(2) C64(3) C32(4) C32(5) C32(6) C32(7)) : A8 : "v"(b) : "vcc", "s20", "s21"); }
        if (MODE == 49) { asm volatile(SETS20 REP8(C64(0) C64(1) C64(2) C64(3) AD(4) AD(5) AD(6) AD(7)) : A8 : "v"(b) : "s20", "s21"); }
        if (MODE == 50) { asm volatile(REP8(BF(0) BF(1) BF(2) BF(3) AD(4) AD(5) AD(6) AD(7)) : A8 : "v"(b), "v"(m)); }
        if (MODE == 51) { asm volatile(SETVCC REP8(C32(0) "v_and_or_b32 %1, %1, %8, %8\n\t" C32(2) "v_perm_b32 %3, %3, %8, %8\n\t" C32(4) "v_lshl_add_u32 %5, %5, 1, %8\n\t" C32(6) "v_min_u32 %7, %7, %8\n\t") : A8 : "v"(b) : "vcc"); }
    }
    out[blockIdx.x * 64 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + t0 + t1 + t2 + t3 + t4 + t5 + t6 + t7 + pad[0];
}

// instPerIter vector instructions per loop trip, of which `fill` are v_add_u32 fillers around `seqs` sequences under
// test.  With fillers the line also gives what one sequence costs once the fillers are paid at v_add_u32's own rate.
template <int MODE>
static double run(const char *name, int wavesPerSimd, int instPerIter = 64, int seqs = 0, int fill = 0, double addRate = 0)
{
    const int iters = 2000;
    const int NB = 256 * 4 * wavesPerSimd;
    const int lds = (160 * 1024) / (4 * wavesPerSimd) - 256;     // exactly wavesPerSimd * 4 workgroups fit a CU
    static uint32_t *out = nullptr;
    if (!out) (void)hipMalloc(&out, (size_t)256 * 4 * 8 * 64 * 4);
    (void)hipFuncSetAttribute((const void *)k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(NB), dim3(64), lds, 0, out, iters);
    (void)hipEventRecord(e0); hipLaunchKernelGGL(k<MODE>, dim3(NB), dim3(64), lds, 0, out, iters); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    const double perIter = ms * 1e-3 * 2.4e9 / ((double)iters * wavesPerSimd), rate = perIter / instPerIter;
    printf("%-16s waves/SIMD=%d : %.2f SIMD cycles per wave-instruction (2.4 GHz)", name, wavesPerSimd, rate);
    if (seqs) printf("   = %.2f per sequence of %d%s", (perIter - fill * addRate) / seqs, (instPerIter - fill) / seqs, fill ? " beside v_add_u32 fillers at their own rate" : "");
    printf("\n");
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rate;
}

int main(int argc, char **argv)
{
    const bool selectsOnly = argc > 1 && !strcmp(argv[1], "selects");
    for (int w : {1, 4, 8}) {
        const double add = run<0>("v_add_u32", w);
        if (!selectsOnly) {
        run<1>("v_and_b32", w);
        run<2>("v_or_b32", w);
        run<3>("v_lshlrev_b32", w);
        run<4>("v_lshrrev_b32", w);
        run<5>("v_min_u32", w);
        run<6>("v_mov_b32", w);
        }
        run<7>("v_cndmask vcc", w);
        run<8>("v_cmp_lt e32", w);
        run<9>("v_cmp_lt e64", w);
        if (!selectsOnly) {
        run<10>("v_bfe_u32", w);
        run<11>("v_and_or_b32", w);
        run<12>("v_lshl_add_u32", w);
        run<13>("v_lshl_or_b32", w);
        run<14>("v_add3_u32", w);
        run<15>("v_alignbyte", w);
        run<16>("v_perm_b32", w);
        run<17>("v_mov_dpp shr1", w);
        run<18>("v_add_dpp shr1", w);
        run<19>("v_add_sdwa", w);
        run<20>("v_pk_add_u16", w);
        run<21>("v_pk_min_u16", w);
        run<22>("v_mul_u32_u24", w);
        run<23>("v_mad_u32_u24", w);
        run<24>("v_mul_lo_u32", w);
        run<25>("v_mbcnt_lo", w);
        run<26>("v_readlane", w);
        run<27>("v_permlane32sw", w);
        }
        // the selects: back to back, one among seven v_add_u32, and directly behind the v_cmp that writes the condition
        run<28>("cnd e32 b2b", w, 64, 64);
        run<29>("cnd e32 1-in-8", w, 64, 8, 56, add);
        run<30>("cmp+cnd e32 b2b", w, 64, 32);
        run<31>("cmp+cnd e32 +6", w, 64, 8, 48, add);
        run<32>("cnd e64 b2b", w, 64, 64);
        run<33>("cnd e64 1-in-8", w, 64, 8, 56, add);
        run<34>("cmp+cnd e64 b2b", w, 64, 32);
        run<35>("cmp+cnd e64 +6", w, 64, 8, 48, add);
        // replacements on a 0 / -1 lane mask in a VGPR, and two ways to build such a mask
        run<36>("v_bfi_b32 b2b", w, 64, 64);
        run<37>("v_bfi 1-in-8", w, 64, 8, 56, add);
        run<38>("and + and_or", w, 64, 32);
        run<39>("xor + and + xor", w, 96, 32);
        run<40>("sub + ashr 31", w, 64, 32);
        run<41>("v_bfe_i32", w, 64, 64);
        run<42>("sub+ashr+bfi +6", w, 72, 8, 48, add);
        // runs of selects on one condition inside groups of eight (the fillers are v_add_u32)
        run<43>("2 cnd e32 + 6", w, 64, 8, 48, add);
        run<44>("4 cnd e32 + 4", w, 64, 8, 32, add);
        run<45>("6 cnd e32 + 2", w, 64, 8, 16, add);
        run<46>("cnd e32,add x4", w, 64, 32, 32, add);
        run<47>("cmp,4 cnd e32 +3", w, 64, 8, 24, add);
        run<48>("4 e64 + 4 e32", w, 64, 8);
        run<49>("4 cnd e64 + 4", w, 64, 8, 32, add);
        run<50>("4 v_bfi + 4", w, 64, 8, 32, add);
        run<51>("cnd e32,vop3 x4", w, 64, 32);
    }
    return 0;
}
