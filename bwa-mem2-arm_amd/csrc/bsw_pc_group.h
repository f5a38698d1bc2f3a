// bsw_pc_group.h -- one 4-column group of the packed-column kernel (bsw_pc.hip, whose head comment gives the
// layout and the arithmetic) as ONE asm statement: the macros the statement is assembled from and the two
// functions that hold it, pc_group (int16 planes) and pcb_group (byte planes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsw {

struct PcRow {                           // per-row uniform (SGPR) group sets, bit G = group G
    uint64_t enter;                      // groups touching slots [min beg, max end]
    uint64_t fast;                       // FAST groups
    uint64_t left;                       // groups containing some lane's beg (masked-L)
};

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

// masked body of the L (left-reset) form: phase 1 PH, the per-cell chain CH0 .. CH3
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

// Right-edge (masked-R) group on the packed chain (the per-cell form it replaced is
// measured in profiles/right_edge/).  An R group holds no lane's beg, so the entering f / h1 are valid for
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
    PC_REDGE(PH, KA_R, KB_R)                                                                 \
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

// The operands every group statement takes: the chain state and the temporaries (outputs), the row's
// invariants and the group's compile-time column numbers (inputs).  A statement puts its plane registers in
// front of the first list and its key constants behind the second.
#define PC_OUT_OPS                                                                       \
    [f] "+v"(f), [h1] "+v"(h1), [key] "+v"(key), [y] "=&v"(y), [sa] "=&v"(sa), [sb] "=&v"(sb),  \
    [ta] "=&v"(ta), [tb] "=&v"(tb), [xa] "=&v"(xa), [xb] "=&v"(xb), [c0] "=&v"(c0),          \
    [c1] "=&v"(c1), [c2] "=&v"(c2), [pa] "=&v"(pa), [pb] "=&v"(pb), [fp] "=&v"(fp)
#define PC_IN_OPS                                                                        \
    [q] "v"(q), [plo] "v"(plo), [phi] "v"(phi), [oe2] "s"(oe2), [ed2] "s"(ed2), [ed] "s"(ed), \
    [e0e] "s"(e0e), [ee2] "s"(ee2), [men] "s"(r.enter), [mfa] "s"(r.fast), [mle] "s"(r.left), \
    [endw] "v"(endw), [endm1w] "v"(endm1w), [begm2w] "v"(begm2w), [endv] "v"(endv),          \
    [begv] "v"(begv), [g] "i"(G), [j0] "i"(4 * G), [j1] "i"(4 * G + 1), [j2] "i"(4 * G + 2), \
    [j3] "i"(4 * G + 3), [r0] "i"(R0)

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
        : [ha] "+v"(ha), [hb] "+v"(hb), [ea] "+v"(ea), [eb] "+v"(eb), PC_OUT_OPS PC_CNT_OPS  \
        : PC_IN_OPS, [jja] "s"(JJA), [jjb] "s"(JJB)                                          \
        : "vcc", "scc")

// The J form (template parameter JK, QMAX >= 128): the FAST key from ONE scalar constant per group instead of two.  The
// key halves H << 8 | j (H <= 255 in this kernel's regime) are built by v_perm from the group's
// four column numbers as BYTES of one SGPR, J4 = {4G-1, 4G, 4G+1, 4G+2}, with two loop-invariant
// VGPR selectors (gfx9 VOP3 reads one SGPR): one s_mov per group instead of two for the packed
// {4G-1, 4G} / {4G+1, 4G+2} constants of v_lshl_or -- 24 fewer SALU on a C2 row.  The masked
// bodies (out of line, ~9% of groups) load those packed constants themselves (two s_mov there).
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
        : [ha] "+v"(ha), [hb] "+v"(hb), [ea] "+v"(ea), [eb] "+v"(eb), PC_OUT_OPS,            \
          [jja] "=&s"(tja), [jjb] "=&s"(tjb) PC_CNT_OPS                                      \
        : PC_IN_OPS, [j4] "s"(J4), [ska] "v"(bs.ka), [skb] "v"(bs.kb), [ija] "i"(JJA), [ijb] "i"(JJB) \
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
          [eb] "=&v"(eb), PC_OUT_OPS PC_CNT_OPS                                              \
        : PC_IN_OPS, [jja] "s"(JJA), [jjb] "s"(JJB),                                         \
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

// plane registers per pair: two columns per VGPR (int16), four (bytes); a pair's H or E plane
template <int QMAX, bool BY> struct PcNp { static constexpr int v = BY ? QMAX / 4 : QMAX / 2; };
template <int QMAX, bool BY> using PcPlane = uint32_t[PcNp<QMAX, BY>::v];

}  // namespace bsw
