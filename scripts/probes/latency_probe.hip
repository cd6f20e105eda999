// Probe: per-instruction costs of a single wave's dependent chain on gfx950 (informs the rANS chains).
// Each test runs REP copies of a snippet inside a 256-iteration loop and reports shader cycles per copy.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <string>

#define REP8(S) S S S S S S S S
#define REP32(S) REP8(S) REP8(S) REP8(S) REP8(S)

#define PROBE_KERNEL(NAME, SNIPPET)                                                           \
__global__ __launch_bounds__(64) void NAME(unsigned long long* out, uint32_t seed) {          \
  unsigned long long t0, t1;                                                                  \
  uint32_t cnt;                                                                               \
  asm volatile(                                                                               \
    "s_mov_b32 s40, %[seed]\n\t s_mov_b32 s41, 0x10001\n\t s_mov_b32 s42, 3\n\t s_mov_b32 s43, 0\n\t" \
    "v_mov_b32 v40, %[seed]\n\t v_mov_b32 v41, 0x10001\n\t v_mov_b32 v42, 3\n\t v_mov_b32 v43, 7\n\t" \
    "s_mov_b32 s44, 0x00800000\n\t s_mov_b32 s46, 0\n\t s_mov_b32 s47, 1\n\t"                 \
    "s_mov_b32 s48, 1\n\t s_mov_b32 s49, 0\n\t"                                               \
    "s_set_gpr_idx_on s43, 0x1\n\t"                                                           \
    "s_memtime %[t0]\n\t s_waitcnt lgkmcnt(0)\n\t"                                            \
    "s_mov_b32 %[cnt], 256\n\t"                                                               \
    "1:\n\t" REP32(SNIPPET)                                                                   \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t s_cmp_lg_u32 %[cnt], 0\n\t s_cbranch_scc1 1b\n\t"        \
    "s_memtime %[t1]\n\t s_waitcnt lgkmcnt(0)\n\t"                                            \
    "s_set_gpr_idx_off\n\t"                                                                   \
    : [t0] "=&s"(t0), [t1] "=&s"(t1), [cnt] "=&s"(cnt) : [seed] "s"(seed)                     \
    : "s40","s41","s42","s43","s44","s45","s46","s47","s48","s49","s50","s51","v40","v41","v42","v43","v44","v45","v46","v47","v48","v49","vcc","scc","m0","memory"); \
  if (threadIdx.x == 0) out[0] = t1 - t0;                                                     \
}

PROBE_KERNEL(k_empty, "")
PROBE_KERNEL(k_sadd, "s_add_u32 s40, s40, s41\n\t")
PROBE_KERNEL(k_sadd_indep, "s_add_u32 s45, s41, s42\n\t")
PROBE_KERNEL(k_smul, "s_mul_i32 s40, s40, s41\n\t")
PROBE_KERNEL(k_smulhi, "s_mul_hi_u32 s40, s40, s41\n\t s_or_b32 s40, s40, s41\n\t")
PROBE_KERNEL(k_sbfe, "s_bfe_u32 s40, s40, 0x1f0001\n\t")
PROBE_KERNEL(k_slshl64, "s_lshl_b64 s[40:41], s[40:41], s43\n\t")
PROBE_KERNEL(k_vadd, "v_add_u32 v40, v40, v41\n\t")
PROBE_KERNEL(k_vadd_indep, "v_add_u32 v44, v41, v42\n\t")
PROBE_KERNEL(k_vmulhi, "v_mul_hi_u32 v40, v40, v41\n\t v_or_b32 v40, v40, v41\n\t")
PROBE_KERNEL(k_vmullo, "v_mul_lo_u32 v40, v40, v41\n\t")
PROBE_KERNEL(k_vmad24, "v_mad_u32_u24 v40, v40, v42, v41\n\t")
PROBE_KERNEL(k_vdpp, "v_add_u32_dpp v40, v40, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t s_nop 1\n\t")
PROBE_KERNEL(k_vrowdpp, "v_add_u32_dpp v40, v40, v41 row_shr:1 row_mask:0xf bank_mask:0xf\n\t s_nop 1\n\t")
PROBE_KERNEL(k_vcmp_cnd, "v_cmp_ge_u32_e32 vcc, v40, v41\n\t s_nop 1\n\t v_cndmask_b32_e32 v40, v40, v42, vcc\n\t")
PROBE_KERNEL(k_readlane_salu, "v_readlane_b32 s45, v40, s42\n\t s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_readlane_chain, "v_readlane_b32 s40, v40, s40\n\t")
PROBE_KERNEL(k_readlane_chain2, "v_readlane_b32 s45, v40, s40\n\t s_and_b32 s40, s45, 63\n\t")
PROBE_KERNEL(k_setidx_readlane, "s_set_gpr_idx_idx s43\n\t v_readlane_b32 s45, v40, s40\n\t s_and_b32 s40, s45, 63\n\t")
PROBE_KERNEL(k_writelane, "v_writelane_b32 v44, s40, 5\n\t")
PROBE_KERNEL(k_branch_nt, "s_cmp_lt_u32 s40, s46\n\t s_cbranch_scc1 9f\n\t 9:\n\t")
PROBE_KERNEL(k_branch_t, "s_cmp_lt_u32 s46, s47\n\t s_cbranch_scc1 9f\n\t s_nop 0\n\t 9:\n\t")
PROBE_KERNEL(k_branch_t_far, "s_cmp_lt_u32 s46, s47\n\t s_cbranch_scc1 9f\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t s_nop 0\n\t 9:\n\t")
PROBE_KERNEL(k_snop0, "s_nop 0\n\t")
PROBE_KERNEL(k_snop1, "s_nop 1\n\t")
PROBE_KERNEL(k_cselect, "s_cmp_lt_u32 s40, s44\n\t s_cselect_b32 s40, s41, s42\n\t")
PROBE_KERNEL(k_dec_core, "s_bfe_u32 s45, s40, 0x60006\n\t s_set_gpr_idx_idx s43\n\t s_lshr_b32 s46, s40, 12\n\t v_writelane_b32 v44, s40, 3\n\t v_readlane_b32 s47, v40, s40\n\t s_and_b32 s45, s47, 0xffff\n\t s_lshr_b32 s47, s47, 16\n\t s_mul_i32 s46, s45, s46\n\t s_add_u32 s40, s46, s47\n\t")
PROBE_KERNEL(k_setidx_on, "s_set_gpr_idx_on s43, 0x1\n\t")
PROBE_KERNEL(k_setidx_idx, "s_set_gpr_idx_idx s43\n\t")
PROBE_KERNEL(k_flbit, "s_flbit_i32_b32 s45, s40\n\t")
PROBE_KERNEL(k_flbit_m0_movrels, "s_flbit_i32_b32 m0, s44\n\t s_nop 0\n\t s_movrels_b32 s45, s40\n\t")
PROBE_KERNEL(k_m0_write, "s_mov_b32 m0, s43\n\t")
PROBE_KERNEL(k_dec2_core, "s_bfe_u32 s45, s40, 0x60006\n\t s_set_gpr_idx_on s43, 0x1\n\t v_readlane_b32 s47, v40, s40\n\t v_readlane_b32 s46, v41, s40\n\t s_lshr_b32 s45, s41, 9\n\t s_lshr_b32 s45, s41, 3\n\t s_set_gpr_idx_on s43, 0x1\n\t v_readlane_b32 s45, v42, s41\n\t s_lshr_b32 s45, s40, 12\n\t v_writelane_b32 v44, s40, 3\n\t s_mul_i32 s47, s47, s45\n\t s_add_u32 s40, s47, s46\n\t s_flbit_i32_b32 m0, s44\n\t s_nop 0\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t s_add_u32 s41, s41, s43\n\t")
PROBE_KERNEL(k_dec2_core_idx, "s_bfe_u32 s45, s40, 0x60006\n\t s_set_gpr_idx_idx s43\n\t v_readlane_b32 s47, v40, s40\n\t v_readlane_b32 s46, v41, s40\n\t s_lshr_b32 s45, s41, 9\n\t s_lshr_b32 s45, s41, 3\n\t s_set_gpr_idx_idx s43\n\t v_readlane_b32 s45, v42, s41\n\t s_lshr_b32 s45, s40, 12\n\t v_writelane_b32 v44, s40, 3\n\t s_mul_i32 s47, s47, s45\n\t s_add_u32 s40, s47, s46\n\t s_cmp_lt_u32 s40, s44\n\t s_cselect_b32 s45, 8, 0\n\t s_cmp_lt_u32 s40, s42\n\t s_cselect_b32 s45, 16, s45\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t s_add_u32 s41, s41, s43\n\t")
PROBE_KERNEL(k_dec4_core, "s_lshr_b32 s45, s40, 12\n\t s_bfe_u32 s46, s40, 0x60006\n\t s_set_gpr_idx_on s43, 0x1\n\t v_writelane_b32 v44, s40, 3\n\t v_readlane_b32 s47, v40, s40\n\t v_readlane_b32 s46, v41, s40\n\t s_mul_i32 s47, s47, s45\n\t s_add_u32 s40, s47, s46\n\t s_flbit_i32_b32 m0, s44\n\t s_mov_b32 s46, s41\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t s_lshl_b64 s[46:47], s[46:47], s43\n\t s_sub_u32 s45, s45, s43\n\t")
PROBE_KERNEL(k_dec4_pair, "s_lshr_b32 s45, s40, 12\n\t s_bfe_u32 s46, s40, 0x60006\n\t s_set_gpr_idx_on s43, 0x1\n\t v_writelane_b32 v44, s40, 3\n\t v_readlane_b32 s47, v40, s40\n\t v_readlane_b32 s46, v41, s40\n\t s_mul_i32 s47, s47, s45\n\t s_add_u32 s40, s47, s46\n\t s_flbit_i32_b32 m0, s44\n\t s_mov_b32 s46, s41\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t s_lshl_b64 s[46:47], s[46:47], s43\n\t s_sub_u32 s45, s45, s43\n\ts_lshr_b32 s45, s40, 12\n\t s_bfe_u32 s46, s40, 0x60006\n\t s_set_gpr_idx_on s43, 0x1\n\t v_writelane_b32 v44, s40, 3\n\t v_readlane_b32 s47, v40, s40\n\t v_readlane_b32 s46, v41, s40\n\t s_mul_i32 s47, s47, s45\n\t s_add_u32 s40, s47, s46\n\t s_flbit_i32_b32 m0, s44\n\t s_mov_b32 s46, s41\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t s_lshl_b64 s[46:47], s[46:47], s43\n\t s_sub_u32 s45, s45, s43\n\ts_cmp_lt_u32 s42, s43\n\t s_cbranch_scc1 9f\n\t 9:\n\t")
PROBE_KERNEL(k_enc_core, "v_add_u32_dpp v40, v44, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t v_cmp_ge_u32_e64 s[46:47], v40, v41\n\t v_cmp_ge_u32_e32 vcc, v40, v42\n\t s_nop 0\n\t v_cndmask_b32_e64 v45, 0, 8, s[46:47]\n\t v_cndmask_b32_e64 v45, v45, 16, vcc\n\t v_lshrrev_b32_e32 v45, v45, v40\n\t v_mul_hi_u32 v43, v45, v41\n\t v_lshrrev_b32_e32 v43, v42, v43\n\t v_mad_i32_i24 v44, v43, v42, v45\n\t s_nop 1\n\t")

// the encode steps of clean tiles (csrc/rans.hip): ripple64_clean (9 slots), the complement step with an arithmetic shift and
// an add (8 slots), and with the two as one v_mad_i64_i32 (u * 2^24 + (T'' << 32): the high dword is ashr(u, 8) + T''; 7 slots,
// the one ripple64_comp uses).  Measured: DESIGN.md section 4.3.
PROBE_KERNEL(k_enc_clean9, "v_add_u32_dpp v40, v44, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t v_cmp_ge_u32_e32 vcc, v40, v42\n\t s_nop 1\n\t v_cndmask_b32_e32 v45, v42, v43, vcc\n\t v_lshrrev_b32_e32 v45, v45, v40\n\t v_mul_hi_u32 v43, v45, v41\n\t v_lshrrev_b32_e32 v43, v42, v43\n\t v_mad_i32_i24 v44, v43, v42, v45\n\t s_nop 1\n\t")
PROBE_KERNEL(k_enc_comp8, "v_add_u32_dpp v40, v44, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t v_ashrrev_i32_e32 v46, 8, v40\n\t v_add_u32_e32 v46, v46, v41\n\t v_min_u32_e32 v45, v40, v46\n\t v_mul_hi_u32 v43, v45, v41\n\t v_lshrrev_b32_e32 v43, v42, v43\n\t v_mad_i32_i24 v44, v43, v42, v45\n\t s_nop 1\n\t")
PROBE_KERNEL(k_enc_comp7, "v_add_u32_dpp v40, v44, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t v_mad_i64_i32 v[46:47], s[46:47], v40, v41, v[48:49]\n\t v_min_u32_e32 v45, v40, v47\n\t v_mul_hi_u32 v43, v45, v41\n\t v_lshrrev_b32_e32 v43, v42, v43\n\t v_mad_i32_i24 v44, v43, v42, v45\n\t s_nop 1\n\t")
PROBE_KERNEL(k_vmad_i64_i32, "v_mad_i64_i32 v[46:47], s[46:47], v47, v41, v[48:49]\n\t")

// The decode symbol with the state update on the vector side (csrc/gen/gen_rans_decode_asm.py: vector_tile).  All rows are
// dependent chains on the state (s40, or s41 / s47 in turn for candidate B); the index register s43 is 0 and v40 / v41 stand
// in for the F' / B' rows, so every relative operand stays inside the registers this kernel owns.  M0 = 8 after the s_flbit
// (s44 = 2^23), so s_movrels reads s50.
//   dec: classic   today's even symbol: two table readlanes, the record, s_mul_hi + s_add (11 slots)
//   dec: A         rows as src1 of v_mul_hi / v_add (mode 0x6), record, ONE readlane (10 slots)
//   dec: B pair    A plus the shift on the vector side ((clz - 1, saturated) & 24 per lane, a second readlane by the old
//                  state), no s_flbit / filler / s_movrels; the window copy and the two window shifts take slots of their
//                  own; two symbols, states in s41 and s47 in turn; no compare / branch
// gfx940 and later want one wait state between a VALU write of a VGPR and a v_readlane of it: the record's v_writelane (A)
// and the v_ffbh / v_writelane (B) stand there.
PROBE_KERNEL(k_dec_classic, "s_bfe_u32 s45, s40, 0x60006\n\t s_set_gpr_idx_on s43, 0x1\n\t v_readlane_b32 s47, v40, s40\n\t v_readlane_b32 s46, v41, s40\n\t v_writelane_b32 v44, s40, 3\n\t s_mul_hi_u32 s45, s47, s40\n\t s_add_u32 s40, s45, s46\n\t s_flbit_i32_b32 m0, s44\n\t s_mov_b32 s46, s41\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t")
PROBE_KERNEL(k_dec_vec_a, "s_bfe_u32 s45, s40, 0x60006\n\t s_set_gpr_idx_on s43, 0x6\n\t v_mul_hi_u32 v45, s40, v40\n\t v_add_u32_e64 v45, v45, v41\n\t v_writelane_b32 v44, s40, 3\n\t v_readlane_b32 s40, v45, s40\n\t s_flbit_i32_b32 m0, s44\n\t s_mov_b32 s46, s41\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t")
#define DEC_B_SYM(X, XN, COPY) "s_bfe_u32 s48, " X ", 0x60006\n\t s_set_gpr_idx_on s43, 0x6\n\t v_mul_hi_u32 v45, " X ", v40\n\t v_add_u32_e64 v45, v45, v41\n\t v_ffbh_u32_e32 v46, v45\n\t v_readlane_b32 " XN ", v45, " X "\n\t v_sub_u32_e64 v46, v46, 1 clamp\n\t v_and_b32_e32 v46, 24, v46\n\t v_writelane_b32 v44, " X ", 3\n\t v_readlane_b32 s42, v46, " X "\n\t" COPY
PROBE_KERNEL(k_dec_vec_b, DEC_B_SYM("s41", "s47", "s_mov_b32 s46, s45\n\t s_lshl_b64 s[46:47], s[46:47], s42\n\t s_lshl_b64 s[44:45], s[44:45], s42\n\t")
                          DEC_B_SYM("s47", "s41", "s_mov_b32 s40, s46\n\t s_lshl_b64 s[40:41], s[40:41], s42\n\t s_lshl_b64 s[44:45], s[44:45], s42\n\t"))
// the VALU -> SALU crossing: does the stall count from the first or from the last VALU write of an SGPR, and do VALU
// instructions between the lane read and the first SALU instruction ride in it for nothing?
#define VALU4 "v_add_u32_e32 v44, v41, v42\n\t v_xor_b32_e32 v46, v41, v42\n\t v_add_u32_e32 v47, v41, v42\n\t v_xor_b32_e32 v48, v41, v42\n\t"
#define VALU3 "v_add_u32_e32 v44, v41, v42\n\t v_xor_b32_e32 v46, v41, v42\n\t v_add_u32_e32 v47, v41, v42\n\t"
PROBE_KERNEL(k_cross_0, "v_readlane_b32 s45, v40, s42\n\t s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_cross_4valu, "v_readlane_b32 s45, v40, s42\n\t" VALU4 "s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_cross_3valu_readlane, "v_readlane_b32 s45, v40, s42\n\t" VALU3 "v_readlane_b32 s46, v41, s42\n\t s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_valu4, VALU4)
// the multiply of candidate A (a table row as relative src1, the state as an SGPR) against the 24-bit multiply-add;
// both rows carry an s_set_gpr_idx_on, whose own row is above
PROBE_KERNEL(k_vmulhi_rel, "s_set_gpr_idx_on s43, 0x6\n\t v_mul_hi_u32 v45, s41, v45\n\t")
PROBE_KERNEL(k_vmad24_rel, "s_set_gpr_idx_on s43, 0x6\n\t v_mad_u32_u24 v45, s41, v45, v41\n\t")

// The shadow pair (csrc/gen/gen_rans_decode_asm.py: shadow_tile): the lane read writes the OTHER shift pair's state register,
// so the record's v_writelane can follow it and ride in the VALU -> SALU stall, and the wait state between the v_add and the
// lane read becomes a hole that carries a window shift.  The states are s41 (pair s[40:41]) and s47 (pair s[46:47]) in turn,
// the window stands in s[48:49] = {1 : 0} (shifted by s43 = 0, so "s48 == 0" is never true and the branch is never taken),
// the rest as in the rows above.  Rows, all per copy of the whole snippet:
//   shadow: (a)    today's vector symbol (the kernel of "dec: A symbol")
//   shadow: (a2)   today's pair: two vector symbols with their fillers, then the tail (window shift, compare, untaken branch)
//   shadow: (b)    the shadow pair, compare in front of the lane read and the branch behind lane read and record
//   shadow: (c)    the shadow pair, compare and branch together in front of the lane read
//   shadow: (d0/d1)  v_readlane; SALU   against   v_readlane; v_writelane (reading an SGPR); SALU
//   shadow: (e0/e1/e2)  s_cmp; v_readlane; SALU   against the same with an untaken s_cbranch_scc1 in front of / behind the SALU
#define SH_HEAD(X) "s_bfe_u32 s45, " X ", 0x60006\n\t s_set_gpr_idx_on s43, 0x6\n\t v_mul_hi_u32 v45, " X ", v40\n\t v_add_u32_e64 v45, v45, v41\n\t"
#define SH_SHIFT(PAIR, FILL) "s_flbit_i32_b32 m0, s44\n\t" FILL "s_movrels_b32 s45, s42\n\t s_lshl_b64 " PAIR ", " PAIR ", s43\n\t"
#define SH_WSHIFT "s_lshl_b64 s[48:49], s[48:49], s43\n\t"
#define VEC_SYM(FILL) SH_HEAD("s41") "v_writelane_b32 v44, s41, 3\n\t v_readlane_b32 s41, v45, s41\n\t" SH_SHIFT("s[40:41]", FILL)
PROBE_KERNEL(k_sh_pair_today, VEC_SYM("s_mov_b32 s40, s49\n\t") VEC_SYM(SH_WSHIFT)
                              SH_WSHIFT "s_cmp_eq_u32 s48, 0\n\t s_cbranch_scc1 9f\n\t 9:\n\t")
#define SH_ODD SH_HEAD("s47") SH_WSHIFT "v_readlane_b32 s41, v45, s47\n\t v_writelane_b32 v44, s47, 3\n\t"       \
               SH_SHIFT("s[40:41]", "s_mov_b32 s40, s46\n\t")
PROBE_KERNEL(k_sh_pair_v1, SH_HEAD("s41") SH_WSHIFT "s_cmp_eq_u32 s48, 0\n\t"
                           "v_readlane_b32 s47, v45, s41\n\t v_writelane_b32 v44, s41, 3\n\t s_cbranch_scc1 9f\n\t 9:\n\t"
                           SH_SHIFT("s[46:47]", "s_mov_b32 s46, s49\n\t") SH_ODD)
PROBE_KERNEL(k_sh_pair_v2, SH_HEAD("s41") SH_WSHIFT "s_cmp_eq_u32 s48, 0\n\t s_cbranch_scc1 9f\n\t 9:\n\t"
                           "v_readlane_b32 s47, v45, s41\n\t v_writelane_b32 v44, s41, 3\n\t"
                           SH_SHIFT("s[46:47]", "s_mov_b32 s46, s49\n\t") SH_ODD)
PROBE_KERNEL(k_sh_record, "v_readlane_b32 s45, v40, s42\n\t v_writelane_b32 v44, s40, 5\n\t s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_sh_cmp_salu, "s_cmp_eq_u32 s48, 0\n\t v_readlane_b32 s45, v40, s42\n\t s_flbit_i32_b32 s46, s45\n\t")
PROBE_KERNEL(k_sh_branch_salu, "s_cmp_eq_u32 s48, 0\n\t v_readlane_b32 s45, v40, s42\n\t s_cbranch_scc1 9f\n\t 9:\n\t s_flbit_i32_b32 s46, s45\n\t")
PROBE_KERNEL(k_sh_salu_branch, "s_cmp_eq_u32 s48, 0\n\t v_readlane_b32 s45, v40, s42\n\t s_flbit_i32_b32 s46, s45\n\t s_cbranch_scc1 9f\n\t 9:\n\t")

// The window refill (csrc/gen/gen_rans_decode_asm.py: refill() in the shadow tile, inhand_tile()).  The pairs are the shadow
// pair above with the compare always true ("s43 == 0"), so the even symbol leaves the main line every time; the window's
// content does not matter to the timing (it is shifted by s43 = 0 and only copied).  The out-of-line code of a copy stands
// behind the copy's main line, which ends in an s_branch over it: rows (c), (d) and (d1) all carry that one extra taken
// branch, their differences do not.  Scratch: s45, s50, s51.  Rows, per copy of the snippet:
//   refill: (a0/a1/a2)  v_readlane; taken s_branch; SALU   against   v_readlane; SALU; taken s_branch   and the branch-in:
//                       s_cmp; v_readlane; TAKEN s_cbranch_scc1; SALU (untaken: shadow (e1))
//   refill: (b1/b2)     v_readlane; SALU   against   two v_readlane back to back; SALU
//   refill: (c0)        the shadow pair, branch never taken, with the s_branch over an (empty) path: the base of c, d, d1
//   refill: (c)         the shadow pair whose even symbol takes refill() every time (mode switch, lane read, branch back)
//   refill: (d)         the in-hand pair: five SALU, the pair's rest up to the odd lane read + prefetch + record, branch back
//   refill: (d1)        the same with the odd symbol's s_flbit in the path, in front of the return branch
//   refill: (e)         the staging of the row v227 at a block end, alone
#define RF_EVEN_HEAD SH_HEAD("s41") SH_WSHIFT "s_cmp_eq_u32 s43, 0\n\t v_readlane_b32 s47, v45, s41\n\t v_writelane_b32 v44, s41, 3\n\t"
#define RF_EVEN_TAIL SH_SHIFT("s[46:47]", "s_mov_b32 s46, s49\n\t")
#define RF_ODD_HEAD SH_HEAD("s47") SH_WSHIFT "v_readlane_b32 s41, v45, s47\n\t"
#define RF_ODD_REC "v_writelane_b32 v44, s47, 3\n\t"
#define RF_TODAY "s_lshr_b32 s50, s42, 6\n\t s_set_gpr_idx_on s43, 0x1\n\t s_ff1_i32_b32 s45, s49\n\t s_sub_u32 s45, 31, s45\n\t" \
                 "v_readlane_b32 s51, v40, s42\n\t s_add_u32 s50, s50, 1\n\t s_lshr_b64 s[50:51], s[50:51], s45\n\t"        \
                 "s_xor_b64 s[48:49], s[48:49], s[50:51]\n\t"
#define RF_INHAND "s_ff1_i32_b32 s45, s49\n\t s_sub_u32 s45, 31, s45\n\t s_lshr_b64 s[50:51], s[50:51], s45\n\t"               \
                  "s_xor_b64 s[48:49], s[48:49], s[50:51]\n\t s_add_u32 s45, s45, 1\n\t"
PROBE_KERNEL(k_rf_branch_salu, "v_readlane_b32 s45, v40, s42\n\t s_branch 9f\n\t s_nop 0\n\t 9:\n\t s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_rf_salu_branch, "v_readlane_b32 s45, v40, s42\n\t s_add_u32 s40, s45, s40\n\t s_branch 9f\n\t s_nop 0\n\t 9:\n\t")
PROBE_KERNEL(k_rf_cbranch_taken, "s_cmp_eq_u32 s43, 0\n\t v_readlane_b32 s45, v40, s42\n\t s_cbranch_scc1 9f\n\t s_nop 0\n\t 9:\n\t s_flbit_i32_b32 s46, s45\n\t")
PROBE_KERNEL(k_rf_two_reads, "v_readlane_b32 s45, v40, s42\n\t v_readlane_b32 s46, v41, s42\n\t s_add_u32 s40, s45, s40\n\t")
PROBE_KERNEL(k_rf_pair_base, SH_HEAD("s41") SH_WSHIFT "s_cmp_eq_u32 s48, 0\n\t v_readlane_b32 s47, v45, s41\n\t v_writelane_b32 v44, s41, 3\n\t"
                             "s_cbranch_scc1 3f\n\t 4:\n\t" RF_EVEN_TAIL SH_ODD "s_branch 5f\n\t 3:\n\t s_branch 4b\n\t 5:\n\t")
PROBE_KERNEL(k_rf_pair_today, RF_EVEN_HEAD "s_cbranch_scc1 3f\n\t 4:\n\t" RF_EVEN_TAIL SH_ODD "s_branch 5f\n\t"
                              "3:\n\t" RF_TODAY "s_branch 4b\n\t 5:\n\t")
PROBE_KERNEL(k_rf_pair_inhand, RF_EVEN_HEAD "s_cbranch_scc1 3f\n\t" RF_EVEN_TAIL RF_ODD_HEAD RF_ODD_REC
                               "6:\n\t" SH_SHIFT("s[40:41]", "s_mov_b32 s40, s46\n\t") "s_branch 5f\n\t"
                               "3:\n\t" RF_INHAND RF_EVEN_TAIL RF_ODD_HEAD "v_readlane_b32 s51, v40, s42\n\t" RF_ODD_REC "s_branch 6b\n\t 5:\n\t")
PROBE_KERNEL(k_rf_pair_inhand_flbit, RF_EVEN_HEAD "s_cbranch_scc1 3f\n\t" RF_EVEN_TAIL RF_ODD_HEAD RF_ODD_REC
                               "s_flbit_i32_b32 m0, s44\n\t 6:\n\t s_mov_b32 s40, s46\n\t s_movrels_b32 s45, s42\n\t s_lshl_b64 s[40:41], s[40:41], s43\n\t s_branch 5f\n\t"
                               "3:\n\t" RF_INHAND RF_EVEN_TAIL RF_ODD_HEAD "v_readlane_b32 s51, v40, s42\n\t" RF_ODD_REC
                               "s_flbit_i32_b32 m0, s44\n\t s_branch 6b\n\t 5:\n\t")
PROBE_KERNEL(k_rf_stage, "s_lshr_b32 s45, s42, 6\n\t s_set_gpr_idx_on s43, 0x1\n\t v_mov_b32_e32 v46, v40\n\t s_bfm_b64 exec, s42, 0\n\t"
                         "v_mov_b32_e32 v46, v41\n\t s_mov_b64 exec, -1\n\t")

// What the seventh slot of the complement step (its closing s_nop 1: the two wait states between the VALU write of z
// and the DPP read) can carry for nothing.  The same six chain instructions as k_enc_comp7, then the filler.  These
// kernels own LDS (the ds_read's target; v50 = 16 * lane) and take a byte buffer (the store's target: out + 256 + lane,
// as an SGPR base s[50:51] + the lane offset v51).  The ds_read variant is a 16-step group: one read per step, the
// first into v[52:55] and the others into v[56:59], the wait (lgkmcnt(14): the first read is back) in the slot of step
// 14 and the first read's v53 as the multiplier of step 15 -- a result consumed 16 steps after its read.
#define FILL_CHAIN_M(MUL)                                                                                         \
  "v_add_u32_dpp v40, v44, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"                                          \
  "v_mad_i64_i32 v[46:47], s[46:47], v40, v41, v[48:49]\n\t v_min_u32_e32 v45, v40, v47\n\t"                       \
  "v_mul_hi_u32 v43, v45, " MUL "\n\t v_lshrrev_b32_e32 v43, v42, v43\n\t v_mad_i32_i24 v44, v43, v42, v45\n\t"
#define FILL_CHAIN FILL_CHAIN_M("v41")
#define FILL_KERNEL(NAME, BODY32)                                                                                  \
__global__ __launch_bounds__(64) void NAME(unsigned long long* out, uint32_t seed) {                               \
  __shared__ uint4 lds[64];                                                                                        \
  lds[threadIdx.x] = make_uint4(seed, 0x10001u, 3u, 7u);                                                            \
  __syncthreads();                                                                                                 \
  unsigned long long t0, t1;                                                                                       \
  uint32_t cnt;                                                                                                    \
  asm volatile(                                                                                                    \
    "s_mov_b32 s41, 0x10001\n\t s_mov_b32 s42, 3\n\t"                                                              \
    "v_mov_b32 v40, %[seed]\n\t v_mov_b32 v41, 0x10001\n\t v_mov_b32 v42, 3\n\t v_mov_b32 v44, 7\n\t"              \
    "v_mov_b32 v48, 0\n\t v_mov_b32 v49, 0x1000\n\t v_mov_b32 v50, %[la]\n\t v_mov_b32 v51, %[so]\n\t"             \
    "v_mov_b32 v53, 0x10001\n\t s_mov_b64 s[50:51], %[sb]\n\t"                                                     \
    "s_memtime %[t0]\n\t s_waitcnt lgkmcnt(0)\n\t"                                                                 \
    "s_mov_b32 %[cnt], 256\n\t"                                                                                    \
    "1:\n\t" BODY32                                                                                                \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t s_cmp_lg_u32 %[cnt], 0\n\t s_cbranch_scc1 1b\n\t"                             \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t"                                                                            \
    "s_memtime %[t1]\n\t s_waitcnt lgkmcnt(0)\n\t"                                                                 \
    : [t0] "=&s"(t0), [t1] "=&s"(t1), [cnt] "=&s"(cnt)                                                             \
    : [seed] "s"(seed), [la] "v"((uint32_t)(threadIdx.x * 16u)), [so] "v"((uint32_t)(256u + threadIdx.x)), [sb] "s"(out) \
    : "s41","s42","s45","s46","s47","s50","s51","v40","v41","v42","v43","v44","v45","v46","v47","v48","v49",      \
      "v50","v51","v52","v53","v54","v55","v56","v57","v58","v59","v60","v61","vcc","scc","memory");               \
  if (threadIdx.x == 0) out[0] = t1 - t0;                                                                          \
}
#define FILL_DS_FIRST FILL_CHAIN "ds_read_b128 v[52:55], v50\n\t s_nop 0\n\t"
#define FILL_DS_MID FILL_CHAIN "ds_read_b128 v[56:59], v50\n\t s_nop 0\n\t"
#define FILL_DS_WAIT FILL_CHAIN "ds_read_b128 v[56:59], v50\n\t s_waitcnt lgkmcnt(14)\n\t"
#define FILL_DS_USE FILL_CHAIN_M("v53") "ds_read_b128 v[56:59], v50\n\t s_nop 0\n\t"
#define FILL_DS_GROUP16 FILL_DS_FIRST FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID \
  FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_MID FILL_DS_WAIT FILL_DS_USE
FILL_KERNEL(k_fill_nop1, REP32(FILL_CHAIN "s_nop 1\n\t"))
FILL_KERNEL(k_fill_valu_nop0, REP32(FILL_CHAIN "v_add_u32_e32 v60, v41, v42\n\t s_nop 0\n\t"))
FILL_KERNEL(k_fill_valu2, REP32(FILL_CHAIN "v_add_u32_e32 v60, v41, v42\n\t v_xor_b32_e32 v61, v41, v42\n\t"))
FILL_KERNEL(k_fill_ds_read, FILL_DS_GROUP16 FILL_DS_GROUP16)
FILL_KERNEL(k_fill_store_byte, REP32(FILL_CHAIN "global_store_byte v51, v42, s[50:51]\n\t s_nop 0\n\t"))
FILL_KERNEL(k_fill_salu_nop0, REP32(FILL_CHAIN "s_add_u32 s45, s41, s42\n\t s_nop 0\n\t"))
// further slots a run of blocks would use: a VALU compare into an SGPR pair (the deferred sign test), a DPP move of a
// value that is not on the chain (cc_prev), and a block's whole share of the work spread over its steps (one filler in
// 27 of 32 steps, s_nop 1 in the others)
FILL_KERNEL(k_fill_vcmp_sgpr, REP32(FILL_CHAIN "v_cmp_gt_i32_e64 s[46:47], 0, v41\n\t s_nop 0\n\t"))
FILL_KERNEL(k_fill_dpp_mov, REP32(FILL_CHAIN "v_mov_b32_dpp v60, v41 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t s_nop 0\n\t"))
FILL_KERNEL(k_fill_valu_only, REP32(FILL_CHAIN "v_add_u32_e32 v60, v41, v42\n\t"))
FILL_KERNEL(k_fill_nop0, REP32(FILL_CHAIN "s_nop 0\n\t"))

struct T { const char* name; void (*fn)(unsigned long long*, uint32_t); };
int main(int argc, char** argv) {
  unsigned long long* d; hipMalloc(&d, 4096);
  T tests[] = {{"empty loop", k_empty}, {"s_add dep", k_sadd}, {"s_add indep", k_sadd_indep}, {"s_mul_i32 dep", k_smul},
    {"s_mul_hi+s_or dep", k_smulhi}, {"s_bfe dep", k_sbfe}, {"s_lshl_b64 dep", k_slshl64}, {"v_add dep", k_vadd},
    {"v_add indep", k_vadd_indep}, {"v_mul_hi+v_or dep", k_vmulhi}, {"v_mul_lo dep", k_vmullo}, {"v_mad_u32_u24 dep", k_vmad24},
    {"v_add_dpp wave_shr + s_nop1 dep", k_vdpp}, {"v_add_dpp row_shr + s_nop1 dep", k_vrowdpp},
    {"v_cmp;s_nop1;v_cndmask dep", k_vcmp_cnd}, {"v_readlane;s_add(dep on it)", k_readlane_salu},
    {"v_readlane lane-sel chain", k_readlane_chain}, {"v_readlane;s_and chain", k_readlane_chain2},
    {"set_idx;v_readlane;s_and chain", k_setidx_readlane}, {"v_writelane", k_writelane},
    {"cmp+branch not taken", k_branch_nt}, {"cmp+branch taken (skip 1)", k_branch_t}, {"cmp+branch taken (skip 16)", k_branch_t_far},
    {"s_nop 0", k_snop0}, {"s_nop 1", k_snop1}, {"s_cmp+s_cselect dep", k_cselect},
    {"s_set_gpr_idx_on", k_setidx_on}, {"s_set_gpr_idx_idx", k_setidx_idx}, {"s_flbit", k_flbit}, {"s_flbit m0;nop;s_movrels", k_flbit_m0_movrels}, {"s_mov m0", k_m0_write}, {"decode v3 core (17 instr, idx_on+flbit)", k_dec2_core}, {"decode v3 core (18 instr, idx_idx+cmp/csel)", k_dec2_core_idx}, {"decode v4 symbol (14 instr)", k_dec4_core}, {"decode v4 pair (28 instr + cmp + untaken branch)", k_dec4_pair}, {"decode core (9 instr)", k_dec_core}, {"encode ripple step (11 instr)", k_enc_core},
    {"encode clean step (9 slots)", k_enc_clean9}, {"encode complement step (8 slots)", k_enc_comp8},
    {"encode complement step, v_mad_i64_i32 (7 slots)", k_enc_comp7}, {"v_mad_i64_i32 dep", k_vmad_i64_i32},
    {"comp step + s_nop 1", k_fill_nop1}, {"comp step + VALU + s_nop 0", k_fill_valu_nop0},
    {"comp step + 2 VALU", k_fill_valu2}, {"comp step + ds_read_b128 (used 16 steps on) + s_nop 0", k_fill_ds_read},
    {"comp step + global_store_byte + s_nop 0", k_fill_store_byte}, {"comp step + SALU + s_nop 0", k_fill_salu_nop0},
    {"comp step + v_cmp to SGPR pair + s_nop 0", k_fill_vcmp_sgpr}, {"comp step + v_mov_dpp + s_nop 0", k_fill_dpp_mov},
    {"comp step + VALU alone", k_fill_valu_only}, {"comp step + s_nop 0", k_fill_nop0},
    {"dec: classic symbol (11 slots)", k_dec_classic}, {"dec: A symbol (10 slots)", k_dec_vec_a},
    {"dec: B symbol pair (2 x 13 slots)", k_dec_vec_b},
    {"dec: v_readlane; SALU", k_cross_0}, {"dec: v_readlane; 4 x VALU; SALU", k_cross_4valu},
    {"dec: v_readlane; 3 x VALU; v_readlane; SALU", k_cross_3valu_readlane}, {"dec: 4 x VALU", k_valu4},
    {"dec: s_set_gpr_idx_on 0x6; v_mul_hi_u32 s, v(rel)", k_vmulhi_rel},
    {"dec: s_set_gpr_idx_on 0x6; v_mad_u32_u24 s, v(rel), v(rel)", k_vmad24_rel},
    {"shadow: (a) vector symbol today (10 slots)", k_dec_vec_a},
    {"shadow: (a2) vector pair today with its tail (23 slots)", k_sh_pair_today},
    {"shadow: (b) shadow pair, branch behind lane read and record", k_sh_pair_v1},
    {"shadow: (c) shadow pair, compare and branch in front of the lane read", k_sh_pair_v2},
    {"shadow: (d0) v_readlane; SALU", k_cross_0}, {"shadow: (d1) v_readlane; v_writelane of an SGPR; SALU", k_sh_record},
    {"shadow: (e0) s_cmp; v_readlane; SALU", k_sh_cmp_salu},
    {"shadow: (e1) s_cmp; v_readlane; untaken s_cbranch_scc1; SALU", k_sh_branch_salu},
    {"shadow: (e2) s_cmp; v_readlane; SALU; untaken s_cbranch_scc1", k_sh_salu_branch},
    {"refill: (a0) v_readlane; taken s_branch; SALU", k_rf_branch_salu},
    {"refill: (a1) v_readlane; SALU; taken s_branch", k_rf_salu_branch},
    {"refill: (a2) s_cmp; v_readlane; taken s_cbranch_scc1; SALU", k_rf_cbranch_taken},
    {"refill: (a3) s_cmp; v_readlane; untaken s_cbranch_scc1; SALU", k_sh_branch_salu},
    {"refill: (b1) v_readlane; SALU", k_cross_0}, {"refill: (b2) two v_readlane; SALU", k_rf_two_reads},
    {"refill: (c0) shadow pair, no refill, s_branch over the path", k_rf_pair_base},
    {"refill: (c) shadow pair, refill() in every pair", k_rf_pair_today},
    {"refill: (d) in-hand pair, refill in every pair", k_rf_pair_inhand},
    {"refill: (d1) in-hand pair, s_flbit in front of the return branch", k_rf_pair_inhand_flbit},
    {"refill: (e) staging of the window row at a block end", k_rf_stage}};
  double base = 0;
  FILE* js = argc > 1 ? fopen(argv[1], "w") : nullptr;   // the "comp step + ..." rows as JSON (cycles per step)
  FILE* jd = argc > 2 ? fopen(argv[2], "w") : nullptr;   // the "dec: ..." rows as JSON (cycles per copy)
  FILE* jh = argc > 3 ? fopen(argv[3], "w") : nullptr;   // the "shadow: ..." rows as JSON (cycles per copy)
  FILE* jr = argc > 4 ? fopen(argv[4], "w") : nullptr;   // the "refill: ..." rows as JSON (cycles per copy)
  if (jr) fprintf(jr, "{\n  \"what\": \"scripts/probes/latency_probe.hip: the window refill of the decode tile, today's (mode switch and lane read of its own, branch back at once) against the in-hand one (dword already in an SGPR, the path runs on to the odd symbol's lane read), one wave alone; shader cycles per copy of the row's snippet, best of 5 launches, empty loop subtracted; rows c0, c, d and d1 each contain one taken s_branch over the out-of-line code that the tile does not have\"");
  if (jh) fprintf(jh, "{\n  \"what\": \"scripts/probes/latency_probe.hip: the shadow pair of the decode tile (record behind the lane read, window shifts in the wait-state holes) against today's vector pair, one wave alone; shader cycles per copy of the row's snippet, best of 5 launches, empty loop subtracted\"");
  if (jd) fprintf(jd, "{\n  \"what\": \"scripts/probes/latency_probe.hip: the decode symbol with the state update on the vector side, one wave alone; shader cycles per copy of the row's snippet, best of 5 launches, empty loop subtracted\"");
  if (js) fprintf(js, "{\n  \"what\": \"scripts/probes/latency_probe.hip: the 7-slot complement step on one wave alone, its closing s_nop 1 replaced by fillers; shader cycles per step, best of 5 launches, empty loop subtracted\"");
  for (auto& t : tests) {
    unsigned long long best = ~0ull;
    for (int r = 0; r < 5; ++r) {
      hipLaunchKernelGGL(t.fn, dim3(1), dim3(64), 0, 0, d, 12345u + r);
      unsigned long long h; hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
      if (h < best) best = h;
    }
    double per = (double)best / (256.0 * 32.0);
    if (std::string(t.name) == "empty loop") base = (double)best;
    printf("%-40s %8.2f cycles/copy\n", t.name, ((double)best - base) / (256.0 * 32.0) + (std::string(t.name) == "empty loop" ? per : 0));
    if (js && std::string(t.name).rfind("comp step + ", 0) == 0)
      fprintf(js, ",\n  \"%s\": %.2f", t.name, ((double)best - base) / (256.0 * 32.0));
    if (jd && std::string(t.name).rfind("dec: ", 0) == 0)
      fprintf(jd, ",\n  \"%s\": %.2f", t.name + 5, ((double)best - base) / (256.0 * 32.0));
    if (jh && std::string(t.name).rfind("shadow: ", 0) == 0)
      fprintf(jh, ",\n  \"%s\": %.2f", t.name + 8, ((double)best - base) / (256.0 * 32.0));
    if (jr && std::string(t.name).rfind("refill: ", 0) == 0)
      fprintf(jr, ",\n  \"%s\": %.2f", t.name + 8, ((double)best - base) / (256.0 * 32.0));
  }
  if (jr) { fprintf(jr, "\n}\n"); fclose(jr); }
  if (jh) { fprintf(jh, "\n}\n"); fclose(jh); }
  if (js) { fprintf(js, "\n}\n"); fclose(js); }
  if (jd) { fprintf(jd, "\n}\n"); fclose(jd); }
  return 0;
}
