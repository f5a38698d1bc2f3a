// bsw_pc.hip -- the packed-COLUMN lane kernel for gfx950: one SeqPair per
// lane as in the lane kernel (bsw_kernels.hip), but the pair's DP row is split into an H plane
// and an E plane, each packed TWO COLUMNS per VGPR, so that every column-independent step of
// the ksw_extend2 recurrence is one v_pk_* instruction for two cells.
//
//   HH[k] = {H(i-1, 2k-1), H(i-1, 2k)}   -- "slot" s holds eh[s].h = H(i-1, s-1), the hold of column s
//   EE[k] = {E(i, 2k),     E(i, 2k+1)}   -- eh[s].e
//   Q[g]  = query codes of columns 4g..4g+3 in byte order {c0, c2, c1, c3}
//
// Per 4-column group (two HH and two EE registers), default scoring (match 1, one mismatch
// value, N -1, symmetric gaps; the host's pk_ok contract):
//   scores   : Y = v_perm(profile[t], Q[g]) -> {S0, S2, S1, S3} bytes; {S0, S1} and {S2, S3}
//              sign-extended by packed 16-bit shifts                         (4 instructions)
//   phase 1  : M = hold + min(S, hold) (the A.5 gate), T~ = M - oe, ME = max(M, E),
//              E' = max(E - e, T~) -- 6 packed instructions per 2 columns     (12)
//   F chain  : h = max(F, ME_j), F = max(sat(F - e), T~_j) per column, 32-bit ops with SDWA
//              word selects                                                   (12)
//   pack/key : HH <- {h_{j-1}, h_j} (v_lshl_or), key = max(HH << 8 | j) by v_pk_max_u16 (6)
// = 34 VALU per 4 cells, against 47 for the lane kernel's fast group.  ~200 VGPRs at
// QMAX = 160: two waves per SIMD (the occupancy the packed two-pairs-per-lane kernel lacks).
//
// Eligibility (planner, bsw_dispatch.hip): pk_ok scoring, h0 + min(qlen, tlen) <= 255 (H <= 255:
// the 8-bit key H << 8 | j and the 16-bit lanes), qlen < QMAX (slot qlen inside a group).
//
// Band edges (per lane [beg, end)): a group is FAST when every live lane has all
// four columns in band and 4G > beg (so the entering F / H chain is valid); otherwise it is
// MASKED: the same arithmetic, then per-lane packed masks write slots <= end only (slots
// beyond end keep their stale values, A.7: a later row whose end grows by 2 reads them), put
// E = 0 at slot end, drop slots > end (and < beg) from the key, and pass H(i, end-1) along the
// chain (h1 at row end = H(i, end-1), for gscore and the lazy last-positive scan).  Groups that
// contain some lane's beg (L) also reset F and H to 0 entering column beg, on a per-cell chain;
// the others (R: right edge only) run the FAST packed chain (PC_REDGE).  Slots left of beg may
// take garbage: they are never read again (beg never decreases).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <limits.h>
#include <utility>
#include "bsw_kernels.h"
#include "bsw_wave.h"

namespace bsw {

constexpr int kPcChunkDw = 17;           // dwords per lane per 64-row target chunk (as lane kernel)
#ifndef BSW_PC_EXP_HALFHEAD
#define BSW_PC_EXP_HALFHEAD 0
#endif
#ifdef BSW_PC_STATS
__device__ unsigned long long g_pc_stats[19];
// per-wave schedule record (tools/pc_times.py): start / end (s_memrealtime, 100 MHz), XCC id and
// HW_ID (CU / SIMD / SE), rows run -- the launch's occupancy over time, ramp-up and tail
constexpr int kPcTimesMax = 1 << 16;
__device__ unsigned long long g_pc_times[kPcTimesMax][4];
#endif

struct PcRow {                           // per-row uniform (SGPR) group sets, bit G = group G
    uint64_t enter;                      // groups touching slots [min beg, max end]
    uint64_t fast;                       // FAST groups
    uint64_t left;                       // groups containing some lane's beg (masked-L)
};

// groups lo .. lo + n - 1 as a bit set (uniform; only bits < QMAX / 4 <= 40 are read).  Callers
// pass n >= 0 and lo < 40 whenever n > 0 (lo: a live lane's group; the FAST set's lo may pass 63
// only with n == 0), so a width clamped to 63 and one s_bfm_b64 give every bit that is read --
// no branches in the row's scalar chain
__device__ __forceinline__ uint64_t gbits(int lo, int n)
{
    uint64_t m;
    asm("s_bfm_b64 %0, %1, %2" : "=s"(m)
        : "s"(__builtin_amdgcn_readfirstlane(min(n, 63))), "s"(__builtin_amdgcn_readfirstlane(lo)));
    return m;
}

// {v, v} as two int16 halves
__device__ __forceinline__ uint32_t pack2(int v) { return ((uint32_t)v & 0xffffu) * 0x10001u; }

#define PC_SDWA(op, d, a, b, sel) \
    op "_sdwa " d ", " a ", " b " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" sel "\n\t"

// phase 1 of one packed register X (columns 2k, 2k+1): S in %[sX] -> M -> ME; T~ in %[tX];
// E~' into EOUT (in place for FAST, %[xX] for MASKED).
//
// T and E are kept UNCLAMPED (T~ = M - oe, E~' = max(E~ - e, T~)): only their positive parts
// matter.  Invariant max(E~, 0) = E: E' = max(E - e, T) = max(max(E~, 0) - e, T~, 0) =
// max(E~ - e, T~, 0) (as -e < 0).  The F chain clamps instead (f - e saturates at 0, so
// F >= 0 always) and H = max(ME, F) = max(M, E~, F) equals max(M, E, F) because F >= 0.
// Bounds: M >= -127, oe < 4096 (pk_ok), so T~, E~ stay far inside int16.
#define PC_PH1_(X, EOUT, ESUB)                                                          \
    "v_pk_min_i16 %[s" X "], %[s" X "], %[h" X "]\n\t"                                      \
    "v_pk_add_u16 %[s" X "], %[s" X "], %[h" X "]\n\t"                                      \
    "v_pk_sub_i16 %[t" X "], %[s" X "], %[oe2]\n\t"                                         \
    "v_pk_max_i16 %[s" X "], %[s" X "], %[e" X "]\n\t"                                      \
    ESUB                                                                                     \
    "v_pk_max_i16 " EOUT ", " EOUT ", %[t" X "]\n\t"
#define PC_PH1(X, EOUT) PC_PH1_(X, EOUT, "v_pk_sub_i16 " EOUT ", %[e" X "], %[ed2]\n\t")
// byte planes (BY kernels): E enters >= 0 (a stored byte), so E - e saturating at 0 makes E'
// = max(sat(E - e), T~) = max(E - e, T, 0) clamped for free -- a byte again
#define PC_PH1B(X, EOUT) PC_PH1_(X, EOUT, "v_pk_sub_u16 " EOUT ", %[e" X "], %[ed2] clamp\n\t")

#define PC_SCORES                                                                        \
    "v_perm_b32 %[y], %[phi], %[plo], %[q]\n\t"                                              \
    "v_pk_lshlrev_b16 %[sa], 8, %[y] op_sel_hi:[0,1]\n\t"                                    \
    "v_pk_ashrrev_i16 %[sa], 8, %[sa] op_sel_hi:[0,1]\n\t"                                   \
    "v_pk_ashrrev_i16 %[sb], 8, %[y] op_sel_hi:[0,1]\n\t"

// one F-chain cell: H -> C, F updated.  X = a|b register, W = WORD_0|WORD_1 half
// ME and T~ may be negative now: their word selects must sign-extend (sext)
#define PC_CELL(C, X, W)                                                                 \
    PC_SDWA("v_max_i32", C, "%[f]", "sext(%[s" X "])", W)                                    \
    "v_subrev_u32_e64 %[f], %[ed], %[f] clamp\n\t"                                           \
    PC_SDWA("v_max_i32", "%[f]", "%[f]", "sext(%[t" X "])", W)

// masked cell: optional reset entering column J (J == beg: F = 0, H(i, J-1) = 0), then the
// cell, then C = (J < end) ? H : HP (H(i, end-1) travels on past end)
#define PC_RESET(HP, RJ)                                                                 \
    "v_cmp_ne_u32_e32 vcc, " RJ ", %[begv]\n\t"                                              \
    "v_cndmask_b32_e32 " HP ", 0, " HP ", vcc\n\t"                                           \
    "v_cndmask_b32_e32 %[f], 0, %[f], vcc\n\t"
#define PC_MCELL(C, HP, X, W, J)                                                         \
    PC_CELL(C, X, W)                                                                         \
    "v_cmp_lt_i32_e32 vcc, " J ", %[endv]\n\t"                                               \
    "v_cndmask_b32_e32 " C ", " HP ", " C ", vcc\n\t"

// masked write-back of register X from packed new values in %[pX]:
//   slot <= end : HH <- new (else stale kept);  slot < end : EE <- E';  slot == end : EE <- 0
//   key over slots in [beg, end] (LEFT adds the slot >= beg mask)
#define PC_MWRITE(X, KEYSRC, LEFT)                                                       \
    "v_pk_sub_i16 %[y], %[jj" X "], %[endw]\n\t"                                             \
    "v_pk_ashrrev_i16 %[y], 15, %[y] op_sel_hi:[0,1]\n\t"                                    \
    "v_bfi_b32 %[h" X "], %[y], %[p" X "], %[h" X "]\n\t"                                    \
    "v_bfi_b32 %[e" X "], %[y], 0, %[e" X "]\n\t"                                            \
    KEYSRC                                                                                   \
    "v_and_b32_e32 %[p" X "], %[p" X "], %[y]\n\t"                                           \
    "v_pk_sub_i16 %[y], %[jj" X "], %[endm1w]\n\t"                                           \
    "v_pk_ashrrev_i16 %[y], 15, %[y] op_sel_hi:[0,1]\n\t"                                    \
    "v_bfi_b32 %[e" X "], %[y], %[x" X "], %[e" X "]\n\t"                                    \
    LEFT                                                                                     \
    "v_pk_max_u16 %[key], %[key], %[p" X "]\n\t"
#define PC_LEFTMASK(X)                                                                   \
    "v_pk_sub_i16 %[y], %[begm2w], %[jj" X "]\n\t"                                           \
    "v_pk_ashrrev_i16 %[y], 15, %[y] op_sel_hi:[0,1]\n\t"                                    \
    "v_and_b32_e32 %[p" X "], %[p" X "], %[y]\n\t"

// masked body (chain variant CH), shared by the L (left-reset) and R forms
#define PC_MASKED(CH0, CH1, CH2, CH3, KA, KB, LA, LB) PC_MASKED_(PC_PH1, CH0, CH1, CH2, CH3, KA, KB, LA, LB)
#define PC_MASKED_(PH, CH0, CH1, CH2, CH3, KA, KB, LA, LB)                               \
    PH("a", "%[xa]") PH("b", "%[xb]")                                                        \
    CH0 CH1                                                                                  \
    "v_lshl_or_b32 %[pa], %[c0], 16, %[h1]\n\t"                                              \
    CH2 CH3                                                                                  \
    "v_lshl_or_b32 %[pb], %[c2], 16, %[c1]\n\t"                                              \
    PC_MWRITE("a", KA, LA) PC_MWRITE("b", KB, LB)

#ifdef BSW_PC_STATS          // group-path counters (tools/pc_stats.py; never in the product build)
#define PC_CNT(k) "v_add_u32_e32 %[ct" #k "], 1, %[ct" #k "]\n\t"
#define PC_CNT_OPS , [ct0] "+v"(ctr[0]), [ct1] "+v"(ctr[1]), [ct2] "+v"(ctr[2]), [ct3] "+v"(ctr[3])
#else
#define PC_CNT(k)
#define PC_CNT_OPS
#endif

// FAST F chain, packed (two columns per instruction where the recurrence allows it).
// F(j+1) = max(sat(F(j) - e), T~(j)); H(j) = max(ME(j), F(j)).  Per register X (columns 2k, 2k+1)
// with Fp = {F(2k), sat(F(2k) - e)} entering:
//   Fp <- max(Fp, {T~(2k), T~(2k)})          = {max(F(2k), T~(2k)), F(2k+1)}  (the low half may
//                                              absorb T~(2k): ME >= M > T~, so H(2k) is unchanged)
//   Hp  = max(Fp, ME)                        = {H(2k), H(2k+1)}
//   Fp <- max(sat({F(2k+1) - e, F(2k+1) - 2e}), {T~(2k+1), T~(2k+1) - e})
//                                            = {F(2k+2), sat(F(2k+2) - e)}
// (sat(max(a, b) - e) = max(sat(a - e), sat(b - e)); the second half is >= 0 through its first
// operand, so T~ needs no clamp).  The group enters with a clean f = F(4G) and leaves with a clean
// f = F(4G+4) (32-bit ops for the last step, so masked bodies read it unchanged), and leaves
// h1 = {H(4G+2), H(4G+3)}: h1 travels in its HIGH half between groups, so the new row
// registers are two byte-aligns, HH[2G] = {H(4G-1), H(4G)}, HH[2G+1] = {H(4G+1), H(4G+2)}.
// 10 VALU per 4 cells for the chain (12 before) and 2 for the packing.
#define PC_FAST_CHAIN                                                                    \
    PC_FAST_CHAIN_("v_alignbyte_b32 %[ha], %[pa], %[h1], 2\n\t", "v_alignbyte_b32 %[hb], %[h1], %[pa], 2\n\t")
// A1 reads the entering h1 (H(4G-1) in its high half) and pa = {H(4G), H(4G+1)}; A2 the leaving
// h1 = {H(4G+2), H(4G+3)}: the int16 form builds HH[2G], HH[2G+1]; the byte form (BY) builds
// HB[G] = bytes {H(4G-1), H(4G), H(4G+1), H(4G+2)} by two v_perm (the same instruction count)
#define PC_FAST_CHAIN_(A1, A2) PC_FAST_CHAIN__(A1, A2, "%[h1]")
// H1O: the register the leaving h1 is written to (the right-edge body keeps the entering one)
#define PC_FAST_CHAIN__(A1, A2, H1O)                                                     \
    "v_pk_sub_u16 %[fp], %[f], %[e0e] op_sel_hi:[0,1] clamp\n\t"                            \
    "v_pk_max_i16 %[fp], %[fp], %[ta] op_sel_hi:[1,0]\n\t"                                  \
    "v_pk_max_i16 %[pa], %[fp], %[sa]\n\t"                                                  \
    "v_pk_sub_u16 %[fp], %[fp], %[ee2] op_sel:[1,0] clamp\n\t"                              \
    "v_pk_sub_i16 %[y], %[ta], %[e0e] op_sel:[1,0]\n\t"                                     \
    "v_pk_max_i16 %[fp], %[fp], %[y]\n\t"                                                   \
    A1                                                                                       \
    "v_pk_max_i16 %[fp], %[fp], %[tb] op_sel_hi:[1,0]\n\t"                                  \
    "v_pk_max_i16 " H1O ", %[fp], %[sb]\n\t"                                                \
    "v_sub_u32_sdwa %[f], %[fp], %[ed] clamp dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD\n\t" \
    A2                                                                                       \
    PC_SDWA("v_max_i32", "%[f]", "%[f]", "sext(%[tb])", "WORD_1")

// Right-edge (masked-R) group on the packed chain (BSW_PC_RIGHT_EDGE 0: the
// per-cell PC_MASKED form).  An R group holds no lane's beg, so the entering f / h1 are valid for
// every lane it matters to and the FAST chain gives H(4G..4G+3) for all of them at once; columns
// at or past a lane's end run on stale inputs, bounded like any cell's, and are never written.
// The chain leaves its h1 in c1, the new-row candidates are the FAST byte-aligns (c0 = slots
// {4G, 4G+1}, pb = slots {4G+2, 4G+3}), and per-lane masks from end do the rest:
//   sa = slots {4G, 4G+1} <= end, sb = slots {4G+2, 4G+3} <= end, ta / tb = the same slots < end
//   (ta = {sa.hi, sb.lo}: slot s <= end is slot s - 1 < end)
//   HH <- candidate under sa / sb; EE <- E' & (slot < end) under sa / sb (0 at slot end, stale
//   beyond); key halves & sa / sb
//   h1 carry: v(s) = the value of slot s (v(4G) = the entering h1) sits in the HIGH half of
//   h1, c0, pa, pb, c1 for s = 4G .. 4G+4, and slot s <= end in the high half of sa, ta, sb, tb
//   for s = 4G+1 .. 4G+4: four v_bfi leave h1 = v(clamp(end, 4G, 4G+4)) = H(i, end-1) for a lane
//   whose end lies in or below the group, H(4G+3) for a lane wholly in band.  (f is dead for a
//   lane past its end: every later group is masked out for it.)
// KA / KB build the key halves from c0 / pb into fp / c2.  51 VALU with the scores (60 before).
#ifndef BSW_PC_RIGHT_EDGE
#define BSW_PC_RIGHT_EDGE 1
#endif
#define PC_REDGE(PH, KA, KB)                                                             \
    PH("a", "%[xa]") PH("b", "%[xb]")                                                        \
    PC_FAST_CHAIN__("v_alignbyte_b32 %[c0], %[pa], %[h1], 2\n\t",                            \
                    "v_alignbyte_b32 %[pb], %[c1], %[pa], 2\n\t", "%[c1]")                   \
    KA KB                                                                                    \
    "v_pk_sub_i16 %[sa], %[jja], %[endw]\n\t"                                                \
    "v_pk_sub_i16 %[sb], %[jjb], %[endw]\n\t"                                                \
    "v_pk_sub_i16 %[tb], %[jjb], %[endm1w]\n\t"                                              \
    "v_pk_ashrrev_i16 %[sa], 15, %[sa] op_sel_hi:[0,1]\n\t"                                  \
    "v_pk_ashrrev_i16 %[sb], 15, %[sb] op_sel_hi:[0,1]\n\t"                                  \
    "v_pk_ashrrev_i16 %[tb], 15, %[tb] op_sel_hi:[0,1]\n\t"                                  \
    "v_alignbyte_b32 %[ta], %[sb], %[sa], 2\n\t"                                             \
    "v_bfi_b32 %[h1], %[sa], %[c0], %[h1]\n\t"                                               \
    "v_bfi_b32 %[ha], %[sa], %[c0], %[ha]\n\t"                                               \
    "v_and_b32_e32 %[xa], %[xa], %[ta]\n\t"                                                  \
    "v_bfi_b32 %[h1], %[ta], %[pa], %[h1]\n\t"                                               \
    "v_bfi_b32 %[ea], %[sa], %[xa], %[ea]\n\t"                                               \
    "v_and_b32_e32 %[fp], %[fp], %[sa]\n\t"                                                  \
    "v_bfi_b32 %[h1], %[sb], %[pb], %[h1]\n\t"                                               \
    "v_bfi_b32 %[hb], %[sb], %[pb], %[hb]\n\t"                                               \
    "v_and_b32_e32 %[xb], %[xb], %[tb]\n\t"                                                  \
    "v_bfi_b32 %[h1], %[tb], %[c1], %[h1]\n\t"                                               \
    "v_bfi_b32 %[eb], %[sb], %[xb], %[eb]\n\t"                                               \
    "v_and_b32_e32 %[c2], %[c2], %[sb]\n\t"                                                  \
    "v_pk_max_u16 %[key], %[key], %[fp]\n\t"                                                 \
    "v_pk_max_u16 %[key], %[key], %[c2]\n\t"
// the R body of a group: the packed form above, or the per-cell one (h1 as a clean int inside)
#if BSW_PC_RIGHT_EDGE
#define PC_RBODY(PH, KA_M, KB_M, KA_R, KB_R) PC_REDGE(PH, KA_R, KB_R)
#else
#define PC_RBODY(PH, KA_M, KB_M, KA_R, KB_R)                                             \
    "v_lshrrev_b32_e32 %[h1], 16, %[h1]\n\t"                                                 \
    PC_MASKED_(PH, PC_MCELL("%[c0]", "%[h1]", "a", "WORD_0", "%[j0]"),                       \
                   PC_MCELL("%[c1]", "%[c0]", "a", "WORD_1", "%[j1]"),                       \
                   PC_MCELL("%[c2]", "%[c1]", "b", "WORD_0", "%[j2]"),                       \
                   PC_MCELL("%[h1]", "%[c2]", "b", "WORD_1", "%[j3]"), KA_M, KB_M, "", "")   \
    "v_lshlrev_b32_e32 %[h1], 16, %[h1]\n\t"
#endif
#define PC_LBODY(PH, KA_M, KB_M)                                                         \
    "v_lshrrev_b32_e32 %[h1], 16, %[h1]\n\t"         /* per-cell chain: h1 as a clean int */ \
    PC_MASKED_(PH, PC_RESET("%[h1]", "%[r0]") PC_MCELL("%[c0]", "%[h1]", "a", "WORD_0", "%[j0]"), \
                   PC_RESET("%[c0]", "%[j1]") PC_MCELL("%[c1]", "%[c0]", "a", "WORD_1", "%[j1]"), \
                   PC_RESET("%[c1]", "%[j2]") PC_MCELL("%[c2]", "%[c1]", "b", "WORD_0", "%[j2]"), \
                   PC_RESET("%[c2]", "%[j3]") PC_MCELL("%[h1]", "%[c2]", "b", "WORD_1", "%[j3]"), \
                   KA_M, KB_M, PC_LEFTMASK("a"), PC_LEFTMASK("b"))                           \
    "v_lshlrev_b32_e32 %[h1], 16, %[h1]\n\t"

// the out-of-line part of a group (subsection 1): skip test, then the L or the R body.  PRE: what
// the masked bodies need first (their key constants, the byte planes' unpack); POST: the byte
// planes' pack
#define PC_OUTOFLINE(PRE, PH, KA_M, KB_M, KA_R, KB_R, POST)                              \
    ".subsection 1\n"                                                                        \
    "5:\n\t"                                                                                 \
    "s_bitcmp1_b64 %[men], %[g]\n\t"                 /* outside [min beg, max end]: skip */ \
    "s_cbranch_scc0 3b\n\t"                                                                  \
    "s_setprio 2\n\t"                                /* masked bodies: short per-cell chains */\
    PC_CNT(0)                                                                                \
    PRE                                                                                      \
    PC_SCORES                                                                                \
    "s_bitcmp1_b64 %[mle], %[g]\n\t"                 /* some lane's beg in this group: L */ \
    "s_cbranch_scc1 4f\n\t"                                                                  \
    PC_CNT(2)                                                                                \
    PC_RBODY(PH, KA_M, KB_M, KA_R, KB_R)                                                     \
    POST                                                                                     \
    "s_setprio 0\n\t"                                                                        \
    "s_branch 3b\n"                                                                          \
    "4:\n\t"                                                                                 \
    PC_CNT(3)                                                                                \
    PC_LBODY(PH, KA_M, KB_M)                                                                 \
    POST                                                                                     \
    "s_setprio 0\n\t"                                                                        \
    "s_branch 3b\n"                                                                          \
    ".subsection 0\n"

// Layout: the FAST body is the fall-through path (one bit test, a not-taken branch, no taken
// branch); skipped and masked groups branch to code in subsection 1 of the kernel's section
// (out of line, after the kernel's main body) and back.  Branch targets stay inside the
// kernel's own section (built with -ffunction-sections), well within s_cbranch's +-128 KB.
#define PC_GROUP_ASM(KEYA_FAST, KEYA_MASK, KEYA_R)                                        \
    asm volatile(                                                                            \
        "s_bitcmp1_b64 %[mfa], %[g]\n\t"             /* every live lane in band: FAST */    \
        "s_cbranch_scc0 5f\n\t"                                                              \
        PC_CNT(0) PC_CNT(1)                                                                  \
        PC_SCORES                                                                            \
        PC_PH1("a", "%[ea]") PC_PH1("b", "%[eb]")                                            \
        PC_FAST_CHAIN                                                                        \
        KEYA_FAST                                                                            \
        "v_pk_max_u16 %[key], %[key], %[pa]\n\t"                                             \
        "v_lshl_or_b32 %[pb], %[hb], 8, %[jjb]\n\t"                                          \
        "v_pk_max_u16 %[key], %[key], %[pb]\n"                                               \
        "3:\n"                                                                               \
        PC_OUTOFLINE("", PC_PH1, KEYA_MASK, "v_lshl_or_b32 %[pb], %[pb], 8, %[jjb]\n\t",     \
                     KEYA_R, "v_lshl_or_b32 %[c2], %[pb], 8, %[jjb]\n\t", "")                \
        : [ha] "+v"(ha), [hb] "+v"(hb), [ea] "+v"(ea), [eb] "+v"(eb), [f] "+v"(f),           \
          [h1] "+v"(h1), [key] "+v"(key), [y] "=&v"(y), [sa] "=&v"(sa), [sb] "=&v"(sb),     \
          [ta] "=&v"(ta), [tb] "=&v"(tb), [xa] "=&v"(xa), [xb] "=&v"(xb), [c0] "=&v"(c0),    \
          [c1] "=&v"(c1), [c2] "=&v"(c2), [pa] "=&v"(pa), [pb] "=&v"(pb), [fp] "=&v"(fp)    \
          PC_CNT_OPS                                                                         \
        : [q] "v"(q), [plo] "v"(plo), [phi] "v"(phi), [oe2] "s"(oe2), [ed2] "s"(ed2),        \
          [ed] "s"(ed), [e0e] "s"(e0e), [ee2] "s"(ee2), [men] "s"(r.enter), [mfa] "s"(r.fast), [mle] "s"(r.left),           \
          [endw] "v"(endw), [endm1w] "v"(endm1w),                                            \
          [begm2w] "v"(begm2w), [endv] "v"(endv), [begv] "v"(begv), [g] "i"(G),             \
          [jja] "s"(JJA), [jjb] "s"(JJB), [j0] "i"(4 * G), [j1] "i"(4 * G + 1),              \
          [j2] "i"(4 * G + 2), [j3] "i"(4 * G + 3), [r0] "i"(R0)                             \
        : "vcc", "scc")

// BSW_PC_JKEY (default 1): the FAST key from ONE scalar constant per group instead of two.  The
// key halves H << 8 | j (H <= 255 in this kernel's regime) are built by v_perm from the group's
// four column numbers as BYTES of one SGPR, J4 = {4G-1, 4G, 4G+1, 4G+2}, with two loop-invariant
// VGPR selectors (gfx9 VOP3 reads one SGPR): one s_mov per group instead of two for the packed
// {4G-1, 4G} / {4G+1, 4G+2} constants of v_lshl_or -- 24 fewer SALU on a C2 row.  The masked
// bodies (out of line, ~9% of groups) load those packed constants themselves (two s_mov there).
#ifndef BSW_PC_JKEY
#define BSW_PC_JKEY 1
#endif
#define PC_GROUP_ASM_J                                                                   \
    asm volatile(                                                                            \
        "s_bitcmp1_b64 %[mfa], %[g]\n\t"                                                     \
        "s_cbranch_scc0 5f\n\t"                                                              \
        PC_CNT(0) PC_CNT(1)                                                                  \
        PC_SCORES                                                                            \
        PC_PH1("a", "%[ea]") PC_PH1("b", "%[eb]")                                            \
        PC_FAST_CHAIN                                                                        \
        "v_perm_b32 %[pa], %[ha], %[j4], %[ska]\n\t"                                         \
        "v_pk_max_u16 %[key], %[key], %[pa]\n\t"                                             \
        "v_perm_b32 %[pb], %[hb], %[j4], %[skb]\n\t"                                         \
        "v_pk_max_u16 %[key], %[key], %[pb]\n"                                               \
        "3:\n"                                                                               \
        PC_OUTOFLINE("s_mov_b32 %[jja], %[ija]\n\t"   /* packed {4G-1, 4G}, {4G+1, 4G+2} */  \
                     "s_mov_b32 %[jjb], %[ijb]\n\t", PC_PH1,                                 \
                     "v_perm_b32 %[pa], %[pa], %[j4], %[ska]\n\t",                           \
                     "v_perm_b32 %[pb], %[pb], %[j4], %[skb]\n\t",                           \
                     "v_perm_b32 %[fp], %[c0], %[j4], %[ska]\n\t",                           \
                     "v_perm_b32 %[c2], %[pb], %[j4], %[skb]\n\t", "")                       \
        : [ha] "+v"(ha), [hb] "+v"(hb), [ea] "+v"(ea), [eb] "+v"(eb), [f] "+v"(f),           \
          [h1] "+v"(h1), [key] "+v"(key), [y] "=&v"(y), [sa] "=&v"(sa), [sb] "=&v"(sb),     \
          [ta] "=&v"(ta), [tb] "=&v"(tb), [xa] "=&v"(xa), [xb] "=&v"(xb), [c0] "=&v"(c0),    \
          [c1] "=&v"(c1), [c2] "=&v"(c2), [pa] "=&v"(pa), [pb] "=&v"(pb), [fp] "=&v"(fp),   \
          [jja] "=&s"(tja), [jjb] "=&s"(tjb)                                                 \
          PC_CNT_OPS                                                                         \
        : [q] "v"(q), [plo] "v"(plo), [phi] "v"(phi), [oe2] "s"(oe2), [ed2] "s"(ed2),        \
          [ed] "s"(ed), [e0e] "s"(e0e), [ee2] "s"(ee2), [men] "s"(r.enter), [mfa] "s"(r.fast), [mle] "s"(r.left),           \
          [endw] "v"(endw), [endm1w] "v"(endm1w),                                            \
          [begm2w] "v"(begm2w), [endv] "v"(endv), [begv] "v"(begv), [g] "i"(G),             \
          [j4] "s"(J4), [ska] "v"(bs.ka), [skb] "v"(bs.kb), [ija] "i"(JJA), [ijb] "i"(JJB),  \
          [j0] "i"(4 * G), [j1] "i"(4 * G + 1),                                              \
          [j2] "i"(4 * G + 2), [j3] "i"(4 * G + 3), [r0] "i"(R0)                             \
        : "vcc", "scc")

struct PcbSel { uint32_t ka, kb; };            // key selectors (VGPRs: v_perm takes one SGPR)

// One 4-column group G (columns / slots 4G .. 4G+3) as ONE asm statement: skip / FAST /
// MASKED (R: right edge only; L: also resets at beg) decided by scalar tests inside.
template <int G, bool JK>
__device__ __forceinline__ void pc_group(uint32_t &ha, uint32_t &hb, uint32_t &ea, uint32_t &eb,
                                         uint32_t q, uint32_t plo, uint32_t phi, int &f, int &h1,
                                         uint32_t &key, uint32_t oe2, uint32_t ed2, int ed,
                                         const PcRow &r, uint32_t endw, uint32_t endm1w,
                                         uint32_t begm2w, int endv, int begv, const PcbSel &bs,
                                         uint32_t (&ctr)[4])
{
    (void)ctr;
    (void)bs;
    // key slot s carries column j = s - 1: jj = {4G-1, 4G} and {4G+1, 4G+2}
    constexpr uint32_t JJA = ((uint32_t)(4 * G - 1) & 0xffffu) | ((uint32_t)(4 * G) << 16);
    constexpr uint32_t JJB = (uint32_t)(4 * G + 1) | ((uint32_t)(4 * G + 2) << 16);
    constexpr int R0 = (G == 0) ? -1 : 4 * G;   // no reset entering column 0 (the boundary)
    uint32_t y, sa, sb, ta, tb, xa, xb, c0, c1, c2, pa, pb, fp;
    const uint32_t e0e = (uint32_t)ed << 16;                          // {0, e}
    const uint32_t ee2 = (uint32_t)ed | ((uint32_t)(2 * ed) << 16);   // {e, 2e}
#define PC_K0_FAST "v_lshlrev_b32_e32 %[pa], 24, %[pa]\n\t"           /* pa = {H(0), H(1)} here */
#define PC_K0_MASK "v_lshl_or_b32 %[pa], %[c0], 24, 0\n\t"
#define PC_K0_R "v_lshlrev_b32_e32 %[fp], 24, %[pa]\n\t"
#define PC_KA_FAST "v_lshl_or_b32 %[pa], %[ha], 8, %[jja]\n\t"
#define PC_KA_MASK "v_lshl_or_b32 %[pa], %[pa], 8, %[jja]\n\t"
#define PC_KA_R "v_lshl_or_b32 %[fp], %[c0], 8, %[jja]\n\t"
    if constexpr (G == 0) {
        // slot 0 holds the column-0 boundary, not a cell: its key half is 0 (c0 << 24 | 0)
        PC_GROUP_ASM(PC_K0_FAST, PC_K0_MASK, PC_K0_R);
    } else if constexpr (JK) {
        constexpr uint32_t J4 = (uint32_t)(4 * G - 1) | ((uint32_t)(4 * G) << 8) | ((uint32_t)(4 * G + 1) << 16) |
                                ((uint32_t)(4 * G + 2) << 24);
        uint32_t tja, tjb;
        PC_GROUP_ASM_J;
    } else {
        PC_GROUP_ASM(PC_KA_FAST, PC_KA_MASK, PC_KA_R);
    }
}

// ---- byte planes (BY kernels, BSW_OPT_KERNEL8 = 2): the 8-bit regime's cells stored as bytes
//   HB[G] = bytes {H(i-1, 4G-1), H(i-1, 4G), H(i-1, 4G+1), H(i-1, 4G+2)}   (slots 4G .. 4G+3)
//   EB[G] = bytes {E(i, 4G), .., E(i, 4G+3)}
// half the plane registers of the int16 form.  A group unpacks its two bytes words into the
// int16 pairs the shared arithmetic runs on (4 v_perm, after the skip test: skipped groups pay
// nothing), and packs back: H by the two v_perm that replace the FAST chain's byte-aligns, E by
// one v_perm; the row-max key is built from HB by one v_perm per pair of slots (as v_lshl_or
// before).  Every stored H, E is in [0, 255] (H <= h0 + min(qlen, tlen) <= 255, the planner's
// contract; E <= H and E' clamped at 0 by PC_PH1B).
constexpr uint32_t kSelLo = 0x0C010C00u;       // {b0, b1} of a bytes word -> two int16 halves
constexpr uint32_t kSelHi = 0x0C030C02u;       // {b2, b3}
constexpr uint32_t kSelPk = 0x06040200u;       // v_perm(hi, lo): {lo.w0, lo.w1, hi.w0, hi.w1} -> bytes
constexpr uint32_t kSelA1 = 0x0C060402u;       // v_perm(pa, h1 in): {h1.b2, pa.b0, pa.b2, 0}
constexpr uint32_t kSelA2 = 0x04020100u;       // v_perm(h1 out, t): {t.b0, t.b1, t.b2, h1.b0}
constexpr uint32_t kSelKa = 0x05020400u;       // v_perm(HB, jj): {jj.b0, HB.b0, jj.b2, HB.b1} = H << 8 | j
constexpr uint32_t kSelKb = 0x07020600u;       // {jj.b0, HB.b2, jj.b2, HB.b3}
constexpr uint32_t kSelK0 = 0x050C0C0Cu;       // group 0: {0, 0, 0, HB.b1} (slot 0 is no cell)

#define PCB_UNPACK                                                                       \
    "v_perm_b32 %[ha], %[hw], %[hw], %[slo]\n\t"                                             \
    "v_perm_b32 %[hb], %[hw], %[hw], %[shi]\n\t"                                             \
    "v_perm_b32 %[ea], %[ew], %[ew], %[slo]\n\t"                                             \
    "v_perm_b32 %[eb], %[ew], %[ew], %[shi]\n\t"
#define PCB_PACK                                                                         \
    "v_perm_b32 %[hw], %[hb], %[ha], %[spk]\n\t"                                             \
    "v_perm_b32 %[ew], %[eb], %[ea], %[spk]\n\t"

#define PCB_GROUP_ASM(KEYA_FAST, KEYA_MASK, KEYA_R)                                       \
    asm volatile(                                                                            \
        "s_bitcmp1_b64 %[mfa], %[g]\n\t"             /* every live lane in band: FAST */    \
        "s_cbranch_scc0 5f\n\t"                                                              \
        PC_CNT(0) PC_CNT(1)                                                                  \
        PCB_UNPACK                                                                           \
        PC_SCORES                                                                            \
        PC_PH1B("a", "%[ea]") PC_PH1B("b", "%[eb]")                                          \
        PC_FAST_CHAIN_("v_perm_b32 %[hw], %[pa], %[h1], %[sa1]\n\t",                         \
                       "v_perm_b32 %[hw], %[h1], %[hw], %[sa2]\n\t")                         \
        "v_perm_b32 %[ew], %[eb], %[ea], %[spk]\n\t"                                         \
        KEYA_FAST                                                                            \
        "v_pk_max_u16 %[key], %[key], %[pa]\n\t"                                             \
        "v_perm_b32 %[pb], %[hw], %[jjb], %[vkb]\n\t"                                        \
        "v_pk_max_u16 %[key], %[key], %[pb]\n"                                               \
        "3:\n"                                                                               \
        PC_OUTOFLINE(PCB_UNPACK, PC_PH1B, KEYA_MASK, "v_lshl_or_b32 %[pb], %[pb], 8, %[jjb]\n\t", \
                     KEYA_R, "v_lshl_or_b32 %[c2], %[pb], 8, %[jjb]\n\t", PCB_PACK)          \
        : [hw] "+v"(hw), [ew] "+v"(ew), [ha] "=&v"(ha), [hb] "=&v"(hb), [ea] "=&v"(ea),      \
          [eb] "=&v"(eb), [f] "+v"(f),                                                       \
          [h1] "+v"(h1), [key] "+v"(key), [y] "=&v"(y), [sa] "=&v"(sa), [sb] "=&v"(sb),     \
          [ta] "=&v"(ta), [tb] "=&v"(tb), [xa] "=&v"(xa), [xb] "=&v"(xb), [c0] "=&v"(c0),    \
          [c1] "=&v"(c1), [c2] "=&v"(c2), [pa] "=&v"(pa), [pb] "=&v"(pb), [fp] "=&v"(fp)    \
          PC_CNT_OPS                                                                         \
        : [q] "v"(q), [plo] "v"(plo), [phi] "v"(phi), [oe2] "s"(oe2), [ed2] "s"(ed2),        \
          [ed] "s"(ed), [e0e] "s"(e0e), [ee2] "s"(ee2), [men] "s"(r.enter), [mfa] "s"(r.fast), [mle] "s"(r.left),           \
          [endw] "v"(endw), [endm1w] "v"(endm1w),                                            \
          [begm2w] "v"(begm2w), [endv] "v"(endv), [begv] "v"(begv), [g] "i"(G),             \
          [jja] "s"(JJA), [jjb] "s"(JJB), [j0] "i"(4 * G), [j1] "i"(4 * G + 1),              \
          [j2] "i"(4 * G + 2), [j3] "i"(4 * G + 3), [r0] "i"(R0),                            \
          [slo] "s"(kSelLo), [shi] "s"(kSelHi), [spk] "s"(kSelPk), [sa1] "s"(kSelA1),         \
          [sa2] "s"(kSelA2), [sk0] "s"(kSelK0), [vka] "v"(bs.ka), [vkb] "v"(bs.kb)            \
        : "vcc", "scc")

template <int G>
__device__ __forceinline__ void pcb_group(uint32_t &hw, uint32_t &ew, uint32_t q, uint32_t plo, uint32_t phi,
                                          int &f, int &h1, uint32_t &key, uint32_t oe2, uint32_t ed2, int ed,
                                          const PcRow &r, uint32_t endw, uint32_t endm1w, uint32_t begm2w,
                                          int endv, int begv, const PcbSel &bs, uint32_t (&ctr)[4])
{
    (void)ctr;
    constexpr uint32_t JJA = ((uint32_t)(4 * G - 1) & 0xffffu) | ((uint32_t)(4 * G) << 16);
    constexpr uint32_t JJB = (uint32_t)(4 * G + 1) | ((uint32_t)(4 * G + 2) << 16);
    constexpr int R0 = (G == 0) ? -1 : 4 * G;
    uint32_t ha, hb, ea, eb, y, sa, sb, ta, tb, xa, xb, c0, c1, c2, pa, pb, fp;
    const uint32_t e0e = (uint32_t)ed << 16;
    const uint32_t ee2 = (uint32_t)ed | ((uint32_t)(2 * ed) << 16);
#define PCB_K0_FAST "v_perm_b32 %[pa], %[hw], %[hw], %[sk0]\n\t"
#define PCB_KA_FAST "v_perm_b32 %[pa], %[hw], %[jja], %[vka]\n\t"
    if constexpr (G == 0) {
        PCB_GROUP_ASM(PCB_K0_FAST, PC_K0_MASK, PC_K0_R);
    } else {
        PCB_GROUP_ASM(PCB_KA_FAST, PC_KA_MASK, PC_KA_R);
    }
}

// plane registers per pair: two columns per VGPR (int16), four (bytes)
template <int QMAX, bool BY> struct PcNp { static constexpr int v = BY ? QMAX / 4 : QMAX / 2; };

template <int QMAX, bool BY, int G>
__device__ __forceinline__ void pc_group_if(uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)], uint32_t (&ee)[(BY ? QMAX / 4 : QMAX / 2)],
                                            const uint32_t (&qs)[QMAX / 4], uint32_t plo, uint32_t phi, int &f,
                                            int &h1, uint32_t &key, uint32_t oe2, uint32_t ed2, int ed,
                                            const PcRow &r, uint32_t endw, uint32_t endm1w, uint32_t begm2w, int endv,
                                            int begv, const PcbSel &bs, uint32_t (&ctr)[4])
{
    if constexpr (G < QMAX / 4) {
        if constexpr (BY)
            pcb_group<G>(hh[G], ee[G], qs[G], plo, phi, f, h1, key, oe2, ed2, ed, r, endw, endm1w, begm2w, endv,
                         begv, bs, ctr);
        else
            pc_group<G, BSW_PC_JKEY && QMAX >= 128>(hh[2 * G], hh[2 * G + 1], ee[2 * G], ee[2 * G + 1], qs[G], plo, phi, f, h1, key, oe2, ed2,
                        ed, r, endw, endm1w, begm2w, endv, begv, bs, ctr);
    }
}

// Segments of 8 groups behind one uniform test of the row's entered set: a segment no lane's
// band touches costs one s_and + branch instead of 8 x (FAST test + skip test + 2 branches)
// (one segment, no test, for QMAX <= 64: the tests' registers would cost the 64 class its
// fourth wave per SIMD, 127 -> 137 VGPRs)
#ifndef BSW_PC_SEG             // experiment builds (make ab AB_FLAGS=-DBSW_PC_SEG=4) only
#define BSW_PC_SEG 8
#endif
constexpr int kPcSeg = BSW_PC_SEG;
template <int QMAX> constexpr int pc_seg_len() { return QMAX <= 64 ? QMAX / 4 : kPcSeg; }
template <int QMAX, bool BY, int S, int... K>
__device__ __forceinline__ void pc_seg(std::integer_sequence<int, K...>, uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                       uint32_t (&ee)[(BY ? QMAX / 4 : QMAX / 2)], const uint32_t (&qs)[QMAX / 4], uint32_t plo,
                                       uint32_t phi, int &f, int &h1, uint32_t &key, uint32_t oe2, uint32_t ed2,
                                       int ed, const PcRow &r, uint32_t endw, uint32_t endm1w, uint32_t begm2w,
                                       int endv, int begv, const PcbSel &bs, uint32_t (&ctr)[4])
{
    constexpr int kSeg = sizeof...(K);
    constexpr uint64_t kSegMask = ((1ull << kSeg) - 1) << (kSeg * S);
    if (kSeg == QMAX / 4 || (r.enter & kSegMask))
        (pc_group_if<QMAX, BY, kSeg * S + K>(hh, ee, qs, plo, phi, f, h1, key, oe2, ed2, ed, r, endw, endm1w,
                                               begm2w, endv, begv, bs, ctr), ...);
}

template <int QMAX, bool BY, int... S>
__device__ __forceinline__ void pc_row(std::integer_sequence<int, S...>, uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                       uint32_t (&ee)[(BY ? QMAX / 4 : QMAX / 2)], const uint32_t (&qs)[QMAX / 4],
                                       uint32_t plo, uint32_t phi, int &f, int &h1, uint32_t &key,
                                       uint32_t oe2, uint32_t ed2, int ed, const PcRow &r,
                                       uint32_t endw, uint32_t endm1w, uint32_t begm2w, int endv,
                                       int begv, const PcbSel &bs, uint32_t (&ctr)[4])
{
    (pc_seg<QMAX, BY, S>(std::make_integer_sequence<int, pc_seg_len<QMAX>()>{}, hh, ee, qs, plo, phi, f, h1, key, oe2,
                         ed2, ed, r, endw, endm1w, begm2w, endv, begv, bs, ctr), ...);
}

// Lazy last positive column: when H(i, end-1) == 0 the lanes that need it
// look for the last slot s <= end (slot s = H(i, s-1)) holding H > 0; lp1 = that slot = 1 + lastH.
// Packed scan, two slots per instruction, registers from the one holding slot max(end) down:
//   c = min(H, 1) * s (slot or 0), cleared where s > end, lp = max(lp, c)
// 6 packed ops per register; a uniform test after each pair of registers stops the scan once
// every needing lane found its slot.  Slot 0 (the column -1 boundary) contributes 0 = none.
template <int K>
__device__ __forceinline__ void pc_lastpos_reg(uint32_t hv, uint32_t endp1w, uint32_t &lp)
{
    constexpr uint32_t SC = (uint32_t)(2 * K) | ((uint32_t)(2 * K + 1) << 16);
    uint32_t c, m;
    asm volatile(
        "v_pk_min_u16 %[c], %[h], 1 op_sel_hi:[1,0]\n\t"
        "v_pk_mul_lo_u16 %[c], %[c], %[sc]\n\t"
        "v_pk_sub_i16 %[m], %[sc], %[e1]\n\t"               // s - (end + 1) < 0  <=>  s <= end
        "v_pk_ashrrev_i16 %[m], 15, %[m] op_sel_hi:[0,1]\n\t"
        "v_and_b32_e32 %[c], %[c], %[m]\n\t"
        "v_pk_max_u16 %[lp], %[lp], %[c]\n\t"
        : [lp] "+v"(lp), [c] "=&v"(c), [m] "=&v"(m)
        : [h] "v"(hv), [sc] "s"(SC), [e1] "v"(endp1w));
}

template <int QMAX, bool BY, int GG>
__device__ __forceinline__ bool pc_lastpos_group(const uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)], uint32_t endp1w,
                                                 bool pending, uint32_t &lp, int gstart)
{
    if (GG > gstart) return pending;                      // uniform: above every lane's end
    if (__ballot(pending) == 0) return false;             // uniform: all found
    if constexpr (BY) {                                   // slots {4GG+2, 4GG+3}, {4GG, 4GG+1}
        pc_lastpos_reg<2 * GG + 1>(__builtin_amdgcn_perm(hh[GG], hh[GG], kSelHi), endp1w, lp);
        pc_lastpos_reg<2 * GG>(__builtin_amdgcn_perm(hh[GG], hh[GG], kSelLo), endp1w, lp);
    } else {
        if constexpr (2 * GG + 1 < QMAX / 2) pc_lastpos_reg<2 * GG + 1>(hh[2 * GG + 1], endp1w, lp);
        pc_lastpos_reg<2 * GG>(hh[2 * GG], endp1w, lp);
    }
    return pending & (lp == 0u);
}

template <int QMAX, bool BY, int... G>
__device__ __forceinline__ int pc_lastpos(std::integer_sequence<int, G...>, const uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                          int end, bool need, int gstart)
{
    bool pending = need;
    uint32_t lp = 0;
    const uint32_t endp1w = pack2(end + 1);
    ((pending = pc_lastpos_group<QMAX, BY, QMAX / 4 - 1 - G>(hh, endp1w, pending, lp, gstart)), ...);
    return (int)max(lp & 0xffffu, lp >> 16);
}

// Early stop: a lane whose band has reached the query's end (end == qlen) and
// left column 0 (beg > 0) retires once no cell of any later row can reach gscore (hence best):
// every later value is a path from one of this row's slots whose only gains are diagonal steps,
// at most 1 each (the pk_ok contract: match 1, the same fact the A.5 gate of PC_PH1 rests on) and
// at most qlen - 1 - j of them from column j.
//   BSW_PC_EARLY_STOP 0 : off (the literal loop; make ab AB_FLAGS=-DBSW_PC_EARLY_STOP=0)
//   scalar bound        : UB = m + min(qlen - 1 - beg, tlen - 1 - i), selects at the row end
//   per-cell bound      : UB = max over slots s in (beg, end] of H(i, s-1) + (qlen - s), a packed
//                         scan (BSW_PC_EARLY_SCAN 0: scalar bound only) behind one ballot
#ifndef BSW_PC_EARLY_STOP
#define BSW_PC_EARLY_STOP 1
#endif
#ifndef BSW_PC_EARLY_SCAN
#define BSW_PC_EARLY_SCAN 1
#endif
// rows on which a lane may ask for the scan: (i & BSW_PC_SCAN_PHASE) == BSW_PC_SCAN_PHASE, a
// wave-uniform test (3: every fourth row; 0, 1, 7 and 15 measured in DESIGN.md §4.5)
#ifndef BSW_PC_SCAN_PHASE
#define BSW_PC_SCAN_PHASE 3
#endif

// one plane register of the per-cell bound (slots 2K, 2K+1) of a lane with end == qlen:
// c = H + (qlen - s), cleared where s > qlen (= end: the gain's sign) or s <= beg, ub = max(ub, c).
// H <= 255 and 0 <= qlen - s < QMAX on the kept slots: the unsigned max is exact.
template <int K>
__device__ __forceinline__ void pc_ub_reg(uint32_t hv, uint32_t qw, uint32_t begw, uint32_t &ub)
{
    constexpr uint32_t SC = (uint32_t)(2 * K) | ((uint32_t)(2 * K + 1) << 16);
    uint32_t c, m;
    asm volatile(
        "v_pk_sub_i16 %[c], %[qw], %[sc]\n\t"               // qlen - s
        "v_pk_ashrrev_i16 %[m], 15, %[c] op_sel_hi:[0,1]\n\t"  // s > qlen
        "v_pk_add_u16 %[c], %[c], %[h]\n\t"
        "v_bfi_b32 %[c], %[m], 0, %[c]\n\t"
        "v_pk_sub_i16 %[m], %[bg], %[sc]\n\t"               // beg - s < 0  <=>  s > beg
        "v_pk_ashrrev_i16 %[m], 15, %[m] op_sel_hi:[0,1]\n\t"
        "v_and_b32_e32 %[c], %[c], %[m]\n\t"
        "v_pk_max_u16 %[ub], %[ub], %[c]\n\t"
        : [ub] "+v"(ub), [c] "=&v"(c), [m] "=&v"(m)
        : [h] "v"(hv), [qw] "v"(qw), [sc] "s"(SC), [bg] "v"(begw));
}

template <int QMAX, bool BY, int GG>
__device__ __forceinline__ void pc_ub_group(const uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)], uint32_t qw,
                                            uint32_t begw, uint32_t &ub, uint64_t enter)
{
    if (!((enter >> GG) & 1)) return;                     // uniform: outside [min beg, max end]
    if constexpr (BY) {
        pc_ub_reg<2 * GG + 1>(__builtin_amdgcn_perm(hh[GG], hh[GG], kSelHi), qw, begw, ub);
        pc_ub_reg<2 * GG>(__builtin_amdgcn_perm(hh[GG], hh[GG], kSelLo), qw, begw, ub);
    } else {
        pc_ub_reg<2 * GG + 1>(hh[2 * GG + 1], qw, begw, ub);
        pc_ub_reg<2 * GG>(hh[2 * GG], qw, begw, ub);
    }
}

// the per-cell bound of every lane with end == qlen over its slots (beg, end], registers from the
// one holding slot max(end) down to the one holding min beg (the row's entered set)
template <int QMAX, bool BY, int... G>
__device__ __forceinline__ int pc_ubscan(std::integer_sequence<int, G...>, const uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                         int qlen, int beg, uint64_t enter)
{
    uint32_t ub = 0;
    const uint32_t qw = pack2(qlen), begw = pack2(beg);
    (pc_ub_group<QMAX, BY, QMAX / 4 - 1 - G>(hh, qw, begw, ub, enter), ...);
    return (int)max(ub & 0xffffu, ub >> 16);
}

// Left skip: groups that lie wholly inside the all-zero left prefix common
// to the wave's live lanes are dropped from the row's entered set -- computing them rewrites zeros
// (§3 item 1).  gz is wave-uniform and never decreases; at the start of every row each live lane
// holds H == 0 and E <= 0 (bytes: E == 0) in every slot s < 4 gz, slot 0 (the column -1 boundary)
// included.  gz is refreshed at the row end, behind one uniform test, on rows with
// (i & BSW_PC_SKIP_MASK) == BSW_PC_SKIP_ROW: while group gz is zero in both planes for every lane
// that stays alive it advances, an unrolled walk over compile-time register indices with uniform
// skips (segments of 8 groups, then the group), as pc_ubscan and pc_lastpos.
//   BSW_PC_LEFT_SKIP 0 : off (make ab AB_FLAGS=-DBSW_PC_LEFT_SKIP=0)
//   BSW_PC_SKIP_QMIN   : the smallest QMAX class that carries the skip (the classes below it would
//                        pay for gz and the walk with a wave per SIMD)
#ifndef BSW_PC_LEFT_SKIP
#define BSW_PC_LEFT_SKIP 1
#endif
#ifndef BSW_PC_SKIP_MASK
#define BSW_PC_SKIP_MASK 3
#endif
#ifndef BSW_PC_SKIP_ROW
#define BSW_PC_SKIP_ROW 1
#endif
#ifndef BSW_PC_SKIP_QMIN
#define BSW_PC_SKIP_QMIN 96
#endif
template <int QMAX> constexpr bool pc_left_skip() { return BSW_PC_LEFT_SKIP && QMAX >= BSW_PC_SKIP_QMIN; }

// Left prune: at the refresh gz also passes over a NON-zero group when no
// cell of it can reach gscore (hence best) in any lane that stays alive -- the early stop's per-cell
// bound (item 10) applied to a prefix of the row.  Precheck (uniform, once per refresh): i > wl_max
// (every static beg > 0) and every staying lane has end == qlen and gsc > 0.  Then per lane
//   H plane: slots s > beg with H > 0:   H + (qlen - s)     < gsc
//   E plane: slots s >= beg with E > 0:  E + (qlen - 1 - s) < gsc
// in the style of pc_ub_reg; the group's plane registers are then zeroed in every lane (the left
// skip's invariant holds literally) and the wave is marked pruned: from the next row on the row-end
// certificate sends the lanes whose fate the zeroed cells could have changed to the redo pass.
//   BSW_PC_LEFT_PRUNE 0 : off, the walk of item 11 alone (make ab AB_FLAGS=-DBSW_PC_LEFT_PRUNE=0)
#ifndef BSW_PC_LEFT_PRUNE
#define BSW_PC_LEFT_PRUNE 1
#endif
//   BSW_PC_PRUNE_QMIN   : the smallest QMAX class that carries it.  The byte planes never do: the rule's
//                        state costs them scratch (QMAX 128, 160) or a wave per SIMD (96), as it costs the
//                        int16 96 class its third wave (168 -> 175 VGPRs)
#ifndef BSW_PC_PRUNE_QMIN
#define BSW_PC_PRUNE_QMIN 128
#endif
template <int QMAX, bool BY> constexpr bool pc_left_prune()
{
    return BSW_PC_LEFT_PRUNE && !BY && pc_left_skip<QMAX>() && QMAX >= BSW_PC_PRUNE_QMIN;
}
//   BSW_PC_PRUNE_BRANCH : 1, the row-end certificate behind one uniform branch on the wave's mark; 0, as
//                        selects on every row (not separable on the GPU)
#ifndef BSW_PC_PRUNE_BRANCH
#define BSW_PC_PRUNE_BRANCH 1
#endif
constexpr int kPcPruned = 1 << 8;         // the wave's pruned mark, a spare bit of gz's register
template <bool PRUNE> __device__ __forceinline__ int pc_gz_of(int gz) { return PRUNE ? (gz & (kPcPruned - 1)) : gz; }

// Right prune: a wave-uniform right cap.  Past the first rows the insertion tail of
// the diagonal is positive out to the query's end, so every row runs FAST groups to qlen although most of
// those cells can no longer reach the lane's current best.  cap4 (a slot index, a multiple of 4; 4 NG = no
// cap) clamps every lane's band end at the row head: the groups above it leave the entered set through the
// band-end reduction and group cap4 / 4 runs as the row's right-edge group.  At the refresh the cap walks
// down over groups whose every slot, in every staying lane, has UB + SLACK < T = best - MARGIN (pc_rp_group);
// every row of a marked wave checks what leaves the computed columns -- it all goes through h1 -- against
// T, and a lane is final only with gsc >= P, the largest threshold ever applied to it: the others are computed
// again by the redo pass.  The rule speculates on the lane's final gscore alone.
//   MARGIN, SLACK, SLACK2, K, ROW0: T = best - MARGIN; the zeroing test's and the soft retreat's distance from T;
//   the rows since a staying lane's last new best and the first row the precheck allows (profiles/right_prune/ab.txt)
//   BSW_PC_RIGHT_PRUNE 0 : off (make ab AB_FLAGS=-DBSW_PC_RIGHT_PRUNE=0); the classes of BSW_PC_PRUNE_QMIN
#ifndef BSW_PC_RIGHT_PRUNE
#define BSW_PC_RIGHT_PRUNE 1
#endif
#ifndef BSW_PC_RP_MARGIN
#define BSW_PC_RP_MARGIN 20
#endif
#ifndef BSW_PC_RP_SLACK
#define BSW_PC_RP_SLACK 12
#endif
#ifndef BSW_PC_RP_SLACK2
#define BSW_PC_RP_SLACK2 11
#endif
#ifndef BSW_PC_RP_K
#define BSW_PC_RP_K 16
#endif
#ifndef BSW_PC_RP_WALK_MASK        // a marked wave walks on refresh rows with (i & MASK) == (BSW_PC_SKIP_ROW & MASK)
#define BSW_PC_RP_WALK_MASK 15
#endif
#ifndef BSW_PC_RP_RWIN             // the retreat looks at lanes whose band end is within RWIN slots of the cap
#define BSW_PC_RP_RWIN 4
#endif
#ifndef BSW_PC_RP_ROW0
#define BSW_PC_RP_ROW0 25
#endif
template <int QMAX, bool BY> constexpr bool pc_right_prune() { return BSW_PC_RIGHT_PRUNE && pc_left_prune<QMAX, BY>(); }
// per-lane state of the rule, in bits of the pair pointer's high half that no address uses (bits 53 .. 63): the
// lane's P as max(T, 0) + 1 in the top ten bits (0: no threshold was ever applied; H <= 255 in this kernel's
// regime, so T < 256), where a plain unsigned max of the high dword updates it, and the clipped mark under it
constexpr int kPcPShift = 54;                          // P field: bits 54 .. 63
constexpr uintptr_t kPcClipped = (uintptr_t)1 << 53;   // the lane's band end has sat at the cap: it takes the
                                                       // row's crossing certificate from then on
constexpr uint32_t kPcClipHi = (uint32_t)(kPcClipped >> 32), kPcLowHi = (1u << (kPcPShift - 32)) - 1u;
__device__ __forceinline__ uint32_t pc_sp_hi(const SeqPair *sp) { return (uint32_t)((uintptr_t)sp >> 32); }
__device__ __forceinline__ SeqPair *pc_sp_set(const SeqPair *sp, uint32_t hi, bool rd)
{
    return (SeqPair *)(((uintptr_t)hi << 32) | (uintptr_t)(uint32_t)(uintptr_t)sp | (uintptr_t)rd);
}
// the pointer's high dword `hi` with its P field raised to max(t, 0) + 1
__device__ __forceinline__ uint32_t pc_rp_raise(uint32_t hi, int t)
{
    return max(hi, ((uint32_t)(max(t, 0) + 1) << (kPcPShift - 32)) | (hi & kPcLowHi));
}

// one plane register of the prune bound (slots 2K, 2K+1): c = v + gain where v > 0 (gw = packed
// qlen for H, qlen - 1 for E), cleared where the slot is left of the lane's first one (bw = packed
// beg for H: s > beg; beg - 1 for E: s >= beg), ub = max(ub, c).  0 <= v <= 255; a positive v sits in
// a slot <= qlen (slots past qlen are never written and start at 0), so the gain is >= 0 there.
template <int K>
__device__ __forceinline__ void pc_pb_reg(uint32_t v, uint32_t gw, uint32_t bw, uint32_t &ub)
{
    constexpr uint32_t SC = (uint32_t)(2 * K) | ((uint32_t)(2 * K + 1) << 16);
    uint32_t c, m;
    asm volatile(
        "v_pk_sub_i16 %[c], %[gw], %[sc]\n\t"               // the slot's gain
        "v_pk_min_u16 %[m], %[v], 1 op_sel_hi:[1,0]\n\t"    // v > 0
        "v_pk_mul_lo_u16 %[c], %[c], %[m]\n\t"
        "v_pk_add_u16 %[c], %[c], %[v]\n\t"
        "v_pk_sub_i16 %[m], %[bw], %[sc]\n\t"               // first - s < 0  <=>  s > first
        "v_pk_ashrrev_i16 %[m], 15, %[m] op_sel_hi:[0,1]\n\t"
        "v_and_b32_e32 %[c], %[c], %[m]\n\t"
        "v_pk_max_u16 %[ub], %[ub], %[c]\n\t"
        : [ub] "+v"(ub), [c] "=&v"(c), [m] "=&v"(m)
        : [v] "v"(v), [gw] "v"(gw), [sc] "s"(SC), [bw] "v"(bw));
}

// positive parts of an int16 E register (the E plane is unclamped, PC_PH1)
__device__ __forceinline__ uint32_t pc_pos2(uint32_t e)
{
    uint32_t r;
    asm volatile("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(e));
    return r;
}

struct PcPrune {                          // the refresh's prune state
    bool pre;                             // uniform: the precheck holds on this row
    int qlen, beg, gsc;                   // per lane
    uint32_t npr;                         // BSW_PC_STATS: groups pruned
};

// group G of the walk: taken only when gz == G (uniform); z = the group's H registers or-ed with
// the positive parts of its E registers (the int16 E plane is unclamped, PC_PH1)
template <int QMAX, bool BY, bool PRUNE, int G>
__device__ __forceinline__ void pc_gz_group(uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                            uint32_t (&ee)[(BY ? QMAX / 4 : QMAX / 2)], bool live, int &gz, PcPrune &pp)
{
    if constexpr (G < QMAX / 4) {
        if (pc_gz_of<PRUNE>(gz) != G) return;
        uint32_t z;
        if constexpr (BY) {
            asm volatile("v_or_b32_e32 %0, %1, %2" : "=v"(z) : "v"(hh[G]), "v"(ee[G]));
        } else {
            uint32_t t;
            asm volatile("v_pk_max_i16 %0, %2, 0\n\t"
                         "v_pk_max_i16 %1, %3, 0\n\t"
                         "v_or3_b32 %0, %0, %1, %4\n\t"
                         "v_or_b32_e32 %0, %0, %5"
                         : "=&v"(z), "=&v"(t)
                         : "v"(ee[2 * G]), "v"(ee[2 * G + 1]), "v"(hh[2 * G]), "v"(hh[2 * G + 1]));
        }
        if (__ballot(live && z != 0u) == 0) {
            gz = PRUNE ? gz + 1 : G + 1;
        } else if constexpr (PRUNE) {
            if (!pp.pre) return;                           // uniform
            uint32_t ub = 0;
            const uint32_t qw = pack2(pp.qlen), qm1w = pack2(pp.qlen - 1);
            const uint32_t bgw = pack2(pp.beg), bgm1w = pack2(pp.beg - 1);
            static_assert(!BY, "the byte planes are compiled without the prune");
            pc_pb_reg<2 * G + 1>(hh[2 * G + 1], qw, bgw, ub);
            pc_pb_reg<2 * G>(hh[2 * G], qw, bgw, ub);
            pc_pb_reg<2 * G + 1>(pc_pos2(ee[2 * G + 1]), qm1w, bgm1w, ub);
            pc_pb_reg<2 * G>(pc_pos2(ee[2 * G]), qm1w, bgm1w, ub);
            const int u = (int)max(ub & 0xffffu, ub >> 16);
            if (__ballot(live && u >= pp.gsc) == 0) {
                hh[2 * G] = 0u; hh[2 * G + 1] = 0u; ee[2 * G] = 0u; ee[2 * G + 1] = 0u;
                gz = (G + 1) | kPcPruned;
#ifdef BSW_PC_STATS
                pp.npr += 1;
#endif
            }
        }
    }
}

template <int QMAX, bool BY, bool PRUNE, int S, int... K>
__device__ __forceinline__ void pc_gz_seg(std::integer_sequence<int, K...>, uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                          uint32_t (&ee)[(BY ? QMAX / 4 : QMAX / 2)], bool live, int &gz, PcPrune &pp)
{
    if ((pc_gz_of<PRUNE>(gz) >> 3) != S) return;            // uniform
    (pc_gz_group<QMAX, BY, PRUNE, 8 * S + K>(hh, ee, live, gz, pp), ...);
}

template <int QMAX, bool BY, bool PRUNE, int... S>
__device__ __forceinline__ void pc_gz_refresh(std::integer_sequence<int, S...>, uint32_t (&hh)[(BY ? QMAX / 4 : QMAX / 2)],
                                              uint32_t (&ee)[(BY ? QMAX / 4 : QMAX / 2)], bool live, int &gz, PcPrune &pp)
{
    (pc_gz_seg<QMAX, BY, PRUNE, S>(std::make_integer_sequence<int, 8>{}, hh, ee, live, gz, pp), ...);
}

// group G of the right cap's walk: taken only when it is the group under the cap (uniform) and lies at or
// above gz + 2.  ub = the largest UB of its slots (pc_pb_reg without a left limit) and the floor
// 1 + (qlen - 4G): a zero slot may turn positive on the next row through the F chain.
template <int QMAX, int G>
__device__ __forceinline__ void pc_rp_group(uint32_t (&hh)[QMAX / 2], uint32_t (&ee)[QMAX / 2], bool live, int gzv,
                                            int &cap4, int qlen, int t, uint32_t &nev)
{
    if (cap4 != 4 * G + 4 || G < gzv + 2) return;              // uniform
    uint32_t ub = 0;
    const uint32_t qw = pack2(qlen), qm1w = pack2(qlen - 1), allw = 0xffffffffu;   // every slot: s > -1
    pc_pb_reg<2 * G + 1>(hh[2 * G + 1], qw, allw, ub);
    pc_pb_reg<2 * G>(hh[2 * G], qw, allw, ub);
    pc_pb_reg<2 * G + 1>(pc_pos2(ee[2 * G + 1]), qm1w, allw, ub);
    pc_pb_reg<2 * G>(pc_pos2(ee[2 * G]), qm1w, allw, ub);
    const int u = max((int)max(ub & 0xffffu, ub >> 16), 1 + qlen - 4 * G);
    if (__ballot(live && u + BSW_PC_RP_SLACK >= t) == 0) {
        hh[2 * G] = 0u; hh[2 * G + 1] = 0u; ee[2 * G] = 0u; ee[2 * G + 1] = 0u;
        cap4 = 4 * G;
        nev += 1;
    }
}

template <int QMAX, int S, int... K>
__device__ __forceinline__ void pc_rp_seg(std::integer_sequence<int, K...>, uint32_t (&hh)[QMAX / 2],
                                          uint32_t (&ee)[QMAX / 2], bool live, int gzv, int &cap4, int qlen, int t,
                                          uint32_t &nev)
{
    if (((cap4 - 4) >> 5) < S) return;                      // uniform: the cap lies below this segment
    (pc_rp_group<QMAX, 8 * S + 7 - K>(hh, ee, live, gzv, cap4, qlen, t, nev), ...);
}

// the walk, from the group under the cap downward (segments of 8 groups, top first)
template <int QMAX, int... S>
__device__ __forceinline__ void pc_rp_walk(std::integer_sequence<int, S...>, uint32_t (&hh)[QMAX / 2],
                                           uint32_t (&ee)[QMAX / 2], bool live, int gzv, int &cap4, int qlen, int t,
                                           uint32_t &nev)
{
    constexpr int NS = sizeof...(S);
    (pc_rp_seg<QMAX, NS - 1 - S>(std::make_integer_sequence<int, 8>{}, hh, ee, live, gzv, cap4, qlen, t, nev), ...);
}

// WPB waves per workgroup: with 1, a wave's slot (and its LDS) is reused as soon as that wave
// ends, instead of when the slowest of its block's waves ends.
//
// The classes that carry the left prune (§3 item 12) send their redo lanes to a second pass: such a
// lane stores no outputs and appends its pair index to redo[] (one atomic add on *rcnt per wave).
// REDO: that second pass, the instance without the rule -- `order` is the redo list and its lane
// count is *rcnt, at most n.  It is launched for the worst case (every pair listed) with WPB = 4,
// which quarters the blocks that find nothing to do.
template <int QMAX, int WPB, bool BY, bool REDO>
__global__ __launch_bounds__(64 * WPB, BY ? 3 : 2) void pc_kernel(const KParams kp, const int32_t w,
                                                    SeqPair *__restrict__ pairs,
                                                    const int32_t *__restrict__ order,
                                                    const int32_t n_in,
                                                    const uint8_t *__restrict__ ref,
                                                    const uint8_t *__restrict__ qer,
                                                    int32_t *__restrict__ err,
                                                    int32_t *__restrict__ redo,
                                                    int32_t *__restrict__ rcnt)
{
    constexpr bool PRUNE = !REDO && pc_left_prune<QMAX, BY>();
    constexpr bool RP = !REDO && pc_right_prune<QMAX, BY>();
    constexpr int NG = QMAX / 4;        // groups = query words (4 codes each)
    constexpr int CDW = kPcChunkDw;     // target dwords per lane per 64-row chunk
#ifdef BSW_PC_STATS
    const unsigned long long t_wave0 = wall_clock64();
#endif
    __shared__ uint32_t s_tgt[WPB][2][CDW][64];   // 8.7 KB per wave
    __shared__ uint2 s_prof[8];                           // per-row score profiles, by target code
    int32_t n = n_in;
    if constexpr (REDO) {               // the list's length, read once, before any other access;
        n = min(n, *rcnt);              // a block past it has nothing to do
        if ((int)(blockIdx.x * blockDim.x) >= n) return;
    }
    if (threadIdx.x < 8) s_prof[threadIdx.x] = make_uint2(kp.prof[threadIdx.x][0], kp.prof[threadIdx.x][1]);
    __syncthreads();
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = gid < n;
    const int idx = valid ? (order ? order[gid] : gid) : 0;
    SeqPair *sp = pairs + idx;
    int idr = 0, idq = 0, tlen = 0, qlen = 0, h0 = 0;
    if (valid) {
        idr = sp->idr; idq = sp->idq; tlen = sp->len1; qlen = sp->len2; h0 = sp->h0;
        if (qlen >= QMAX || qlen < 0 || tlen < 0 || h0 < 0 || h0 + min(qlen, tlen) > 255 || idr < 0 || idq < 0) {
            atomicOr(err, 1);
            valid = false;
        }
        if constexpr (!REDO && pc_right_prune<QMAX, BY>()) {      // the rule's bits of the pair pointer must be free
            if ((uintptr_t)sp >> 53) {
                atomicOr(err, 1);
                valid = false;
            }
        }
    }
    // query codes, 4 per VGPR in byte order {c0, c2, c1, c3}: aligned dword loads (a dword
    // holding a byte of the query never leaves that byte's page), realigned by v_alignbyte
    uint32_t qs[NG];
    {
        uint32_t wv[NG + 1];
        const uintptr_t qa = (uintptr_t)(qer + idq);
        const uint32_t *wp = (const uint32_t *)(qa & ~(uintptr_t)3);
        const int sh = (int)(qa & 3);
        const int nw = (valid && qlen > 0) ? (sh + qlen + 3) >> 2 : 0;
        if (nw > 0) {
#pragma unroll
            for (int g = 0; g <= NG; ++g) wv[g] = wp[min(g, nw - 1)];
        } else {
#pragma unroll
            for (int g = 0; g <= NG; ++g) wv[g] = 0;
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint32_t c = __builtin_amdgcn_alignbyte(wv[g + 1], wv[g], sh);
            qs[g] = __builtin_amdgcn_perm(c, c, 0x03010200u);
        }
    }
    // A.1 first row: slot 0 = h0, slot j = max(h0 - oe_ins - (j-1) e_ins, 0) for 1 <= j <= qlen
    constexpr int NP = (BY ? QMAX / 4 : QMAX / 2);
    uint32_t hh[NP], ee[NP];
    {
        const int oe_ins = kp.o_ins + kp.e_ins;
        if constexpr (BY) {
            __builtin_amdgcn_sched_barrier(0);     // after the query words: their loads' registers
                                                   // are dead before the planes are built
#pragma unroll
            for (int k = 0; k < NP; ++k) {         // h0 <= 255 (the 8-bit regime): bytes
                uint32_t v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = 4 * k + t;
                    v[t] = (j == 0) ? (uint32_t)h0 : (j <= qlen) ? (uint32_t)max(h0 - oe_ins - (j - 1) * kp.e_ins, 0) : 0u;
                }
                hh[k] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
                asm volatile("" : "+v"(hh[k]));   // built here, not sunk to the loop (the
                ee[k] = 0u;                        // bytes of every word live at once: +40 VGPRs)
            }
        } else {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int j0 = 2 * k, j1 = 2 * k + 1;
                const uint32_t a = (j0 == 0) ? (uint32_t)h0
                                 : (j0 <= qlen) ? (uint32_t)max(h0 - oe_ins - (j0 - 1) * kp.e_ins, 0) : 0u;
                const uint32_t b = (j1 <= qlen) ? (uint32_t)max(h0 - oe_ins - (j1 - 1) * kp.e_ins, 0) : 0u;
                hh[k] = a | (b << 16);
                ee[k] = 0u;
            }
        }
    }
    // A.2 per-lane band cap, integer form of (int)((double)N / e + 1.)
    int wl = w;
    {
        const int ni = qlen * kp.maxsc + kp.end_bonus - kp.o_ins;
        const int nd = qlen * kp.maxsc + kp.end_bonus - kp.o_del;
        wl = min(wl, max((ni + kp.e_ins) / kp.e_ins, 1));
        wl = min(wl, max((nd + kp.e_del) / kp.e_del, 1));
    }
    int best = h0, best_i = -1, best_j = -1, max_ie = -1, gsc = -1, moff = 0, endc = qlen;
    bool alive = valid && tlen > 0;
    // an invalid lane stores nothing: kept as a null pair pointer, not as a lane mask that would
    // hold an SGPR pair across the row loop (the loop has none to spare: it was spilled to a VGPR)
    if (!valid) sp = nullptr;
    asm volatile("" : "+v"(sp));          // made here: the select is not sunk below the loop with its mask
    // target bases HBM -> LDS by LDS-DMA, 64-row chunks double-buffered (as the lane kernel)
    const uint8_t *tp = ref + idr;
    const int tsh = (int)((uintptr_t)tp & 3);
    const uint32_t *twp = (const uint32_t *)(tp - tsh);
    const int tlast = max((tsh + tlen - 1) >> 2, 0);
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    auto issue_chunk = [&](int ch) {
        uint32_t *dst = &s_tgt[wv][ch & 1][0][0];
#pragma unroll
        for (int k = 0; k < CDW; ++k)
            __builtin_amdgcn_global_load_lds((gptr_t)(twp + min(16 * ch + k, tlast)),
                                             (lptr_t)(dst + 64 * k), 4, 0, 0);
    };
    if (alive) { issue_chunk(0); issue_chunk(1); }
    uint32_t tcur = 0;
    const int wl_max = wave_max(alive ? wl : -1);
    const int wl_min = wave_min(alive ? wl : INT_MAX);
    const uint32_t oe2 = (uint32_t)(kp.o_del + kp.e_del) * 0x10001u;
    const uint32_t ed2 = (uint32_t)kp.e_del * 0x10001u;
    uint32_t ctr[4] = {0, 0, 0, 0};                       // BSW_PC_STATS group-path counters
    // key selectors in VGPRs: the byte planes' (BY) or the JKEY ones (int16 planes)
    // (the JKEY selectors only where the two VGPRs cost no occupancy: QMAX >= 128 runs at two
    // waves per SIMD either way; the 96 / 64 classes would drop from 3 / 4 waves)
    PcbSel bs{BY ? kSelKa : 0x06010400u, BY ? kSelKb : 0x06030402u};
    if constexpr (BY || (BSW_PC_JKEY && QMAX >= 128)) asm volatile("" : "+v"(bs.ka), "+v"(bs.kb));
#ifdef BSW_PC_STATS
    uint32_t nrows = 0, nlast = 0, nue = 0;
    uint32_t nscan = 0, nstop_s = 0, nstop_c = 0;   // early stop: scan rows; this lane retired by bound
    (void)nscan; (void)nstop_s; (void)nstop_c;
#endif

#if BSW_PC_EXP_HALFHEAD
    int emax = 0, emin = 0;                 // (experiment: the row head's state outlives its row)
    PcRow r{0, 0, 0};
#endif
    int gz = 0;                             // left skip: groups below gz are all-zero in every live lane
    (void)gz;
    PcPrune pp{false, 0, 0, 0, 0u};         // left prune: the refresh's inputs
    int cap4 = QMAX;                        // right prune: the cap's slot (QMAX = 4 NG: none), wave-uniform
    bool rmark = false;                     // ... and the wave's mark: the cap has been set at least once
    uint32_t nrev = 0;                      // (BSW_PC_STATS: groups the cap's walk passed over)
    (void)cap4; (void)rmark; (void)nrev;
#ifdef BSW_PC_STATS
    uint32_t nrcap = 0, nrret = 0, rcause = 0;   // groups the cap removed, retreats (uniform); this lane's redo cause
    (void)nrcap; (void)nrret; (void)rcause;
#endif
    for (int i = 0;; ++i) {
        const bool act = alive && i < tlen;
        alive = act;
        if (__ballot(act) == 0) break;
        // the row's target base and score profile first: their LDS reads then overlap the band
        // bookkeeping below instead of stalling the first group (lgkmcnt wait)
        // every lane reads (a dead lane's slots are harmless): no exec-masked block on the row's path
        if ((i & 3) == 0) {                // new 4-row block: bases from LDS
            if ((i & 63) == 0) {              // chunk boundary: its DMA was issued 64 rows ago
                __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
                __builtin_amdgcn_sched_barrier(0);
            }
            const int k = (i >> 2) & 15;
            // the two dwords by inline asm: the compiler would otherwise put a vmcnt(0) before
            // every LDS read (it cannot tell this buffer from the one the in-flight LDS-DMA
            // refill writes) -- this chunk's DMA was waited for at its first row above
            const uint32_t la = (uint32_t)(uintptr_t)(lptr_t)&s_tgt[wv][(i >> 6) & 1][k][ln];
            uint2 d;
            asm volatile("ds_read2st64_b32 %0, %1 offset1:1\n\ts_waitcnt lgkmcnt(0)"
                         : "=v"(d) : "v"(la) : "memory");
            tcur = __builtin_amdgcn_alignbyte(d.y, d.x, tsh);
            if ((i & 63) == 0) {
                __builtin_amdgcn_sched_barrier(0);
                if (i > 0 && act) issue_chunk((i >> 6) + 1);   // refill the buffer just drained
            }
        }
        // per-row score profile of target base t (8 bytes: mat[t][q], q = 0..7)
        const uint32_t tcode = (tcur >> (8 * (i & 3))) & 0xffu;
        const uint2 pr = s_prof[min(tcode, 7u)];   // one ds_read_b64 (codes > 4 score as N)
        __builtin_amdgcn_sched_barrier(0);
        const int beg = max(0, i - wl);
        int endcl = min(min(endc, i + wl + 1), qlen);
#ifdef BSW_PC_STATS
        if constexpr (RP) {                // the groups between the cap and the static band end
            const int eu = wave_max(act ? min(i + wl + 1, qlen) : -1), ec = wave_max(act ? min(endcl, cap4) : -1);
            if (cap4 < QMAX && ec >= 0) nrcap += (uint32_t)max((min(eu, QMAX - 1) >> 2) - (min(ec, QMAX - 1) >> 2), 0);
        }
#endif
        if constexpr (RP) endcl = min(endcl, cap4);   // the right cap (§3 item 13): one v_min with a uniform operand
        const int end = endcl;
        endc = end;
#if BSW_PC_EXP_HALFHEAD
        // experiment build only (make ab AB_FLAGS=-DBSW_PC_EXP_HALFHEAD=1; WRONG outputs): the row
        // head -- band-end reductions and the three group sets -- on even rows only, the odd rows
        // reusing the previous row's: the time a two-rows-per-pass schedule could save on row heads
        // (-1.3%)
        if (i & 1) goto row_body;
#else
        int emax, emin;
        PcRow r;
#endif
        wave_maxmin_bc(act ? end : -1, act ? end : INT_MAX, emax, emin);
        {
            const int ulo = __builtin_amdgcn_readfirstlane(max(0, i - wl_max));  // min beg
            const int uhi = __builtin_amdgcn_readfirstlane(emax);                // max end
            const int flo = __builtin_amdgcn_readfirstlane(max(0, i - wl_min));  // max beg
            const int fhi = __builtin_amdgcn_readfirstlane(emin);                // min end
            const int glo = ulo >> 2;
            const int gsp = max((min(uhi, QMAX - 1) >> 2) - glo, -1);      // uhi >= 0: a live lane
            // FAST needs 4G > every beg (entering chain valid) -- or one common beg == 4G with
            // nothing computed before it -- and 4G + 4 <= every end
            const int gfa = (ulo == flo && (flo & 3) == 0) ? (flo >> 2) : (flo >> 2) + 1;
            const int gfn = max((fhi >> 2) - gfa, 0);
            const int gln = (flo >> 2) - glo;
            r.enter = gbits(glo, gsp + 1);
            r.fast = gbits(gfa, gfn);
            r.left = gbits(glo, gln + 1);
            if constexpr (pc_left_skip<QMAX>()) {   // groups below gz leave the entered set; the FAST
                const uint64_t keep = ~0ull << pc_gz_of<PRUNE>(gz);   // test comes first in a group, so its set too
                r.enter &= keep;
                r.fast &= keep;
            }
        }
#if BSW_PC_EXP_HALFHEAD
    row_body:
#endif
        {   // every lane runs the row (dead lanes' registers take garbage); state updates are
            // gated by act below, so no exec-masked block wraps the row
            // h1 = H(i, j-1) entering each group, in the HIGH half (PC_FAST_CHAIN)
            // (a mask, not a select: the compiler turned the select into an exec-masked block)
            int h1 = (int)((uint32_t)max(h0 - (kp.o_del + kp.e_del * (i + 1)), 0) << 16) & -(int)(beg == 0);
            int f = 0;
            uint32_t key = 0;
            const uint32_t endw = pack2(end);
            const uint32_t endm1w = pack2(end - 1);                         // end = 0: {-1, -1}
            const uint32_t begm2w = pack2(beg - 2);
            // wave priority: the row's serial scalar / DPP chain (row end, next row's head) issues
            // ahead of the partner wave's group VALU; the groups themselves run at the base level
            __builtin_amdgcn_s_setprio(0);
            pc_row<QMAX, BY>(std::make_integer_sequence<int, (NG + pc_seg_len<QMAX>() - 1) / pc_seg_len<QMAX>()>{}, hh, ee,
                             qs, pr.x, pr.y, f, h1, key, oe2, ed2, kp.e_del, r, endw, endm1w, begm2w, end, beg, bs,
                             ctr);
            __builtin_amdgcn_s_setprio(2);
            h1 = (int)((uint32_t)h1 >> 16);               // H(i, end-1)
            const uint32_t k32 = max(key & 0xffffu, key >> 16);
            const int m = (int)(k32 >> 8), mj = (int)(k32 & 0xffu);
            {                                     // A.4: j == qlen; h1 = H(i, qlen - 1)
                const bool atq = act && end == qlen;
                max_ie = (atq && !(gsc > h1)) ? i : max_ie;
                gsc = atq ? max(gsc, h1) : gsc;
            }
            // A.4 row end as selects, no branches on the row's path: m <= 0 ends the lane; a new
            // best moves (best, best_i, best_j, max_off); otherwise z-drop against the old best
            {
                const int di = i - best_i, dj = mj - best_j;
                // |di - dj| and e are small and non-negative: 24-bit multiplies (full rate)
                const int dz = (di > dj) ? best - m - (int)__umul24((unsigned)(di - dj), (unsigned)kp.e_del)
                                         : best - m - (int)__umul24((unsigned)(dj - di), (unsigned)kp.e_ins);
                const bool better = act && m > best;       // best >= h0 >= 0: never with m <= 0
                const bool zdropped = kp.zdrop > 0 && dz > kp.zdrop;
                alive = act && m > 0 && (better || !zdropped);
                moff = better ? max(moff, abs(mj - i)) : moff;
                best_i = better ? i : best_i;
                best_j = better ? mj : best_j;
                best = better ? m : best;
                if constexpr (PRUNE) {
                    // the certificate of a pruned wave (§3 item 12), before the early stop: zeroed
                    // cells only lower values, all below gscore, so a lane whose row has a new best
                    // or is far from z-drop whatever mj is (dz <= best - m) is in its true state;
                    // one whose row maximum is 0 retires with its outputs final; the others -- and a
                    // lane whose band end would leave qlen (h1 == 0) -- are computed again.  The
                    // mark travels in the low bit of sp (SeqPair is 4-byte aligned).
                    // (a wave under the right cap, item 13, takes the z-drop half of it on its own mark)
#if BSW_PC_PRUNE_BRANCH
                    if ((gz & kPcPruned) || (RP && rmark))
#endif
                    {
                        const bool rd = ((gz & kPcPruned) != 0 || (RP && rmark)) &&
                                        ((act && !better && m > 0 && kp.zdrop > 0 && best - m > kp.zdrop) ||
                                         ((gz & kPcPruned) != 0 && alive && h1 == 0));
                        alive = alive && !rd;
                        sp = (SeqPair *)((uintptr_t)sp | (uintptr_t)rd);
#ifdef BSW_PC_STATS
                        rcause = (rd && !rcause) ? 2u : rcause;
#endif
                    }
                }
                if constexpr (RP) {
                    // the crossing certificate of a wave under the right cap (§3 item 13), behind one uniform
                    // test: a lane whose band end has sat at the cap lets H(i, end-1) = h1 leave the computed
                    // columns, diagonally or along the row, and h1's potential must stay below T = best - MARGIN
                    if (rmark) {
                        const int t = best - BSW_PC_RP_MARGIN, phi = h1 + (qlen - end);
                        uint32_t hi = pc_sp_hi(sp);
                        const bool cl = act && end < qlen && (end == cap4 || (hi & kPcClipHi) != 0);
                        const bool rdc = cl && h1 > 0 && phi >= t;
                        hi = cl ? pc_rp_raise(hi | kPcClipHi, t) : hi;    // (a redo lane's P is never read)
                        sp = pc_sp_set(sp, hi, rdc);
                        alive = alive && !rdc;
#ifdef BSW_PC_STATS
                        rcause = (rdc && !rcause) ? 1u : rcause;
#endif
                    }
                }
            }
#if BSW_PC_EARLY_STOP
            {   // early stop, after this row's best / gscore updates.  gsc <= best
                // always (gsc is an H value of some row, best >= every row's maximum), so UB < gsc
                // covers UB <= best; both are written as the rule states them.  Selects only.
                // (the three differences by inline asm: written in C++, the loop-invariant parts
                // qlen - 1, tlen - 1 and the scan's packed qlen are hoisted into registers that
                // live across the groups, which costs the 96 and 64 classes a wave per SIMD)
                int gq, gt, gm;                    // qlen - beg, tlen - i, qlen - mj
                asm volatile("v_sub_u32_e32 %0, %3, %4\n\t"
                             "v_subrev_u32_e32 %1, %5, %6\n\t"
                             "v_sub_u32_e32 %2, %3, %7"
                             : "=&v"(gq), "=&v"(gt), "=&v"(gm)
                             : "v"(qlen), "v"(beg), "s"(i), "v"(tlen), "v"(mj));
                const bool edge = end == qlen && gq < qlen;    // beg > 0, from the opaque difference: a
                                                               // test of beg is made at the row head and
                                                               // its mask kept across the groups
                const int ubs = m - 1 + min(gq, gt);
                const bool stop = edge && ubs <= best && ubs < gsc;
#ifdef BSW_PC_STATS
                nstop_s += alive && stop;
#endif
                alive = alive && !stop;
#if BSW_PC_EARLY_SCAN
                // the per-cell bound, on rows of one phase (wave-uniform: every fourth) and only for lanes
                // whose arg-max cell already passes it (a necessary condition: false all along the
                // diagonal phase, true right after it).  Not for QMAX <= 64: there the scan's
                // registers cost the int16 form its fourth wave per SIMD (127 -> 137 VGPRs)
                const int ubm = m - 1 + gm;
                const bool want = QMAX > 64 && alive && edge && ubm <= best && ubm < gsc;
                if (QMAX > 64 && (i & BSW_PC_SCAN_PHASE) == BSW_PC_SCAN_PHASE && __ballot(want)) {
                    const int ubc = pc_ubscan<QMAX, BY>(std::make_integer_sequence<int, NG>{}, hh, gq + beg, beg, r.enter);
                    const bool stopc = want && ubc <= best && ubc < gsc;
#ifdef BSW_PC_STATS
                    nscan += 1;
                    nstop_c += stopc;
#endif
                    alive = alive && !stopc;
                }
#endif
            }
#endif
            if constexpr (pc_left_skip<QMAX>()) {
                if ((i & BSW_PC_SKIP_MASK) == BSW_PC_SKIP_ROW) {
                    if constexpr (PRUNE) {         // the prune's precheck: every static beg > 0, and
                                                   // every staying lane at the query's end with gsc > 0
                        pp.pre = i > wl_max && __ballot(alive && !(end == qlen && gsc > 0)) == 0;
                        // (qlen through an opaque move: its packed forms are then built in the walk,
                        // not hoisted into registers that live across the groups)
                        asm volatile("v_mov_b32_e32 %0, %1" : "=v"(pp.qlen) : "v"(qlen));
                        pp.beg = beg; pp.gsc = gsc;
                    }
                    pc_gz_refresh<QMAX, BY, PRUNE>(std::make_integer_sequence<int, (NG + 7) / 8>{}, hh, ee, alive, gz,
                                                   pp);
                    if constexpr (RP) {
                        // the right cap: precheck (i >= ROW0 and every staying lane with a new best in the last
                        // K rows: on a growing diagonal, where gscore will follow best), then the walk; a
                        // failed precheck under a cap retreats one group
                        if (__ballot(alive && !(i >= BSW_PC_RP_ROW0 && i - best_i <= BSW_PC_RP_K))) {
                            if (cap4 < QMAX) {
                                cap4 += 4;
#ifdef BSW_PC_STATS
                                nrret += 1;
#endif
                            }
                        } else if ((!rmark || (i & BSW_PC_RP_WALK_MASK) == (BSW_PC_SKIP_ROW & BSW_PC_RP_WALK_MASK)) &&
                                   __ballot(alive)) {
                            int ql;                 // (opaque, as pp.qlen)
                            asm volatile("v_mov_b32_e32 %0, %1" : "=v"(ql) : "v"(qlen));
                            const uint32_t nev0 = nrev;
                            pc_rp_walk<QMAX>(std::make_integer_sequence<int, NG / 8>{}, hh, ee, alive,
                                             pc_gz_of<PRUNE>(gz), cap4, ql, best - BSW_PC_RP_MARGIN, nrev);
                            if (nrev != nev0) {     // uniform: T was applied to every staying lane
                                rmark = true;
                                sp = pc_sp_set(sp, alive ? pc_rp_raise(pc_sp_hi(sp), best - BSW_PC_RP_MARGIN) : pc_sp_hi(sp), false);
                            }
                        }
                        // the soft retreat, after the walk: one group up when a staying lane's crossing value, at the
                        // cap or within RWIN slots under it, comes near its threshold (one ballot; the certificate
                        // is what soundness rests on).  A cap the walk has just put above a moving band edge is
                        // taken back before the edge reaches it: a band narrower than the query never clips
                        if (rmark && cap4 < QMAX &&
                            __ballot(alive && end < qlen && end + BSW_PC_RP_RWIN >= cap4 &&
                                     h1 + (qlen - end) + BSW_PC_RP_SLACK2 >= best - BSW_PC_RP_MARGIN)) {
                            cap4 += 4;
#ifdef BSW_PC_STATS
                            nrret += 1;
#endif
                        }
                    }
                }
            }
#ifdef BSW_PC_STATS
            nrows += act;
            nue += act && (emax == emin);  // every live lane has the same band end
#endif
            {                                      // end_{i+1} = min(lastH + 3, ...), DESIGN.md §3
                const bool need = alive && h1 == 0;  // H(i, end-1) == 0 -> lastH < end - 1
                int lp1 = end;
                if (__ballot(need)) {
#ifdef BSW_PC_STATS
                    nlast += 1;
#endif
                    const int lp = pc_lastpos<QMAX, BY>(std::make_integer_sequence<int, NG>{}, hh, end, need,
                                                        emax >> 2);
                    lp1 = need ? lp : end;
                }
                endc = alive ? min(lp1 + 2, qlen) : endc;
            }
        }
    }
#ifdef BSW_PC_STATS
    {   // per wave: rows (max over lanes), group paths, lastpos scans; lane 0 adds
        const unsigned rows = (unsigned)wave_max((int)nrows);
        const unsigned nl = (unsigned)wave_max((int)nlast);
        const unsigned nu = (unsigned)wave_max((int)nue);
        const unsigned ns = (unsigned)wave_max((int)nscan);               // uniform: rows the scan ran on
        const unsigned rs = (unsigned)__popcll(__ballot(nstop_s != 0));   // lanes retired by the scalar bound
        const unsigned rc = (unsigned)__popcll(__ballot(nstop_c != 0));   // ... by the per-cell bound
        unsigned cmax[4];
        for (int k = 0; k < 4; ++k) cmax[k] = (unsigned)wave_max((int)ctr[k]);   // the longest lane
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&g_pc_stats[0], (unsigned long long)rows);
            for (int k = 0; k < 4; ++k) atomicAdd(&g_pc_stats[1 + k], (unsigned long long)cmax[k]);
            atomicAdd(&g_pc_stats[5], (unsigned long long)nl);
            atomicAdd(&g_pc_stats[6], 1ull);
            atomicAdd(&g_pc_stats[7], (unsigned long long)nu);
            atomicAdd(&g_pc_stats[8], (unsigned long long)ns);
            atomicAdd(&g_pc_stats[9], (unsigned long long)rs);
            atomicAdd(&g_pc_stats[10], (unsigned long long)rc);
        }
        const unsigned wid = blockIdx.x * WPB + (threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && wid < (unsigned)kPcTimesMax) {
            unsigned xcc, hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            g_pc_times[wid][0] = t_wave0;
            g_pc_times[wid][1] = wall_clock64();
            g_pc_times[wid][2] = ((unsigned long long)xcc << 32) | hw;
            g_pc_times[wid][3] = rows;
        }
    }
#endif
    if constexpr (PRUNE) {
        // redo lanes: their pair index (read again: no register held it across the loop) appended to
        // the class's list, one atomic add per wave, lanes at base + rank.  At most one entry per
        // valid lane of the launch, so every index written is below the class's pair count.
        if constexpr (RP) {
            // the final certificate: a lane is final only when gscore reached every threshold applied to it;
            // then the rule's bits leave the pointer
            const int pf = (int)((uintptr_t)sp >> kPcPShift);
            const bool rdf = pf != 0 && gsc < pf - 1;
#ifdef BSW_PC_STATS
            rcause = (rdf && !((uintptr_t)sp & 1u)) ? 3u : rcause;
#endif
            sp = (SeqPair *)((((uintptr_t)sp) | (uintptr_t)rdf) & (kPcClipped - 1));
        }
        const bool rd = ((uintptr_t)sp & 1u) != 0;          // never an invalid lane (sp == nullptr)
        const unsigned long long rb = __ballot(rd);
        if (rb) {                                           // uniform
            int base = 0;
            if (ln == __ffsll((long long)rb) - 1) base = atomicAdd(rcnt, (int)__popcll(rb));
            base = __shfl(base, __ffsll((long long)rb) - 1);
            if (rd) {
                const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
                redo[base + (int)__popcll(rb & ((1ull << ln) - 1ull))] = order ? order[g] : (int)g;
            }
        }
#ifdef BSW_PC_STATS
        if (ln == 0) {
            atomicAdd(&g_pc_stats[11], (unsigned long long)pp.npr);
            atomicAdd(&g_pc_stats[12], (unsigned long long)__popcll(rb));
            atomicAdd(&g_pc_stats[13], (unsigned long long)nrev);
            atomicAdd(&g_pc_stats[14], (unsigned long long)nrcap);
            atomicAdd(&g_pc_stats[15], (unsigned long long)nrret);
        }
        for (unsigned c = 1; c <= 3; ++c) {
            const unsigned nc = (unsigned)__popcll(__ballot(rd && rcause == c));
            if (ln == 0 && nc) atomicAdd(&g_pc_stats[15 + c], (unsigned long long)nc);
        }
#endif
        if (rd) sp = nullptr;
    }
    if (sp) {
        sp->score = best;
        sp->tle = best_i + 1;
        sp->gtle = max_ie + 1;
        sp->qle = best_j + 1;
        sp->gscore = gsc;
        sp->max_off = moff;
    }
}

#ifdef BSW_PC_STATS
// [rows, groups entered, fast, masked-R, masked-L, lastpos scans, waves, uniform-end rows, early-stop scan
// rows, lanes retired by the scalar bound, lanes retired by the per-cell bound, non-zero groups the left
// prune passed over, redo lanes, groups the right cap's walk passed over, groups the cap removed from rows (up
// to the static band end: an upper bound of what the cap removes), cap retreats, redo lanes by cause: crossing,
// item 12's certificate (z-drop, or h1 == 0 in a left-pruned wave), final]
// summed over waves
extern "C" int bsw_pc_stats(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pc_stats), 19 * sizeof(unsigned long long)) != hipSuccess) return -5;
    if (reset) {
        unsigned long long z[19] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_pc_stats), z, sizeof(z)) != hipSuccess) return -5;
    }
    return 0;
}
// the per-wave schedule records of the last launch (n waves, 4 x u64 each)
extern "C" int bsw_pc_times(unsigned long long *out, int n)
{
    n = n < kPcTimesMax ? n : kPcTimesMax;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pc_times), (size_t)n * 32) != hipSuccess) return -5;
    return n;
}
#endif

template <int QMAX>
static void launch_pc_q(const KParams &kp, int32_t w, SeqPair *pairs, const int32_t *order, int32_t n,
                        const uint8_t *ref, const uint8_t *qer, int32_t *err, int32_t *redo, int32_t *rcnt,
                        hipStream_t s)
{
    const unsigned grid = (unsigned)((n + 63) / 64);
    // one wave per workgroup: a finished wave's slot and LDS are reused at once
    if (kp.kern8 == 2)                 // byte planes (BSW_OPT_KERNEL8 = 2)
        hipLaunchKernelGGL((pc_kernel<QMAX, 1, true, false>), dim3(grid), dim3(64), 0, s, kp, w, pairs, order, n,
                           ref, qer, err, redo, rcnt);
    else
        hipLaunchKernelGGL((pc_kernel<QMAX, 1, false, false>), dim3(grid), dim3(64), 0, s, kp, w, pairs, order,
                           n, ref, qer, err, redo, rcnt);
    if constexpr (pc_left_prune<QMAX, false>()) {
        // the redo pass behind it on the same stream: no host round trip, so
        // the grid is sized for every pair listed and the blocks past *rcnt return at once
        constexpr int kRedoWpb = 4;
        const unsigned rgrid = (unsigned)((n + 64 * kRedoWpb - 1) / (64 * kRedoWpb));
        if (kp.kern8 != 2)             // (the byte planes do not carry the rule)
            hipLaunchKernelGGL((pc_kernel<QMAX, kRedoWpb, false, true>), dim3(rgrid), dim3(64 * kRedoWpb), 0, s, kp, w,
                               pairs, redo, n, ref, qer, err, nullptr, rcnt);
    }
}

hipError_t launch_pc_kernel(int qmax, const KParams &kp, int32_t w, SeqPair *pairs,
                            const int32_t *order, int32_t n, const uint8_t *ref,
                            const uint8_t *qer, int32_t *err, int32_t *redo, int32_t *rcnt, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (!redo || !rcnt) return hipErrorInvalidValue;
    switch (qmax) {
    case 32: launch_pc_q<32>(kp, w, pairs, order, n, ref, qer, err, redo, rcnt, s); break;
    case 64: launch_pc_q<64>(kp, w, pairs, order, n, ref, qer, err, redo, rcnt, s); break;
    case 96: launch_pc_q<96>(kp, w, pairs, order, n, ref, qer, err, redo, rcnt, s); break;
    case 128: launch_pc_q<128>(kp, w, pairs, order, n, ref, qer, err, redo, rcnt, s); break;
    case 160: launch_pc_q<160>(kp, w, pairs, order, n, ref, qer, err, redo, rcnt, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace bsw
