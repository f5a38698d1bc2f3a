// bsw_pc_scan.h -- the packed-column kernel's row-end scans and walks over the plane registers (bsw_pc.hip):
// the lazy last positive column, the early stop's per-cell bound, the refresh of the left skip's prefix bound gz
// with the left prune, and the right cap's walk.  Unrolled over compile-time register indices behind uniform
// tests; none of them is on the path of a row that does not ask for it.
#pragma once
#include "bsw_pc_group.h"
#include "bsw_pc_rules.h"

namespace bsw {

// {v, v} as two int16 halves
__device__ __forceinline__ uint32_t pack2(int v) { return ((uint32_t)v & 0xffffu) * 0x10001u; }

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
__device__ __forceinline__ bool pc_lastpos_group(const PcPlane<QMAX, BY> &hh, uint32_t endp1w,
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
__device__ __forceinline__ int pc_lastpos(std::integer_sequence<int, G...>, const PcPlane<QMAX, BY> &hh,
                                          int end, bool need, int gstart)
{
    bool pending = need;
    uint32_t lp = 0;
    const uint32_t endp1w = pack2(end + 1);
    ((pending = pc_lastpos_group<QMAX, BY, QMAX / 4 - 1 - G>(hh, endp1w, pending, lp, gstart)), ...);
    return (int)max(lp & 0xffffu, lp >> 16);
}

// ---- the early stop's per-cell bound
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
__device__ __forceinline__ void pc_ub_group(const PcPlane<QMAX, BY> &hh, uint32_t qw,
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
__device__ __forceinline__ int pc_ubscan(std::integer_sequence<int, G...>, const PcPlane<QMAX, BY> &hh,
                                         int qlen, int beg, uint64_t enter)
{
    uint32_t ub = 0;
    const uint32_t qw = pack2(qlen), begw = pack2(beg);
    (pc_ub_group<QMAX, BY, QMAX / 4 - 1 - G>(hh, qw, begw, ub, enter), ...);
    return (int)max(ub & 0xffffu, ub >> 16);
}

// ---- the refresh of gz and the right cap's walk (item 13)
constexpr int kPcPruned = 1 << 8;         // the wave's pruned mark, a spare bit of gz's register
template <bool PRUNE> __device__ __forceinline__ int pc_gz_of(int gz) { return PRUNE ? (gz & (kPcPruned - 1)) : gz; }

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
__device__ __forceinline__ void pc_gz_group(PcPlane<QMAX, BY> &hh,
                                            PcPlane<QMAX, BY> &ee, bool live, int &gz, PcPrune &pp)
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
__device__ __forceinline__ void pc_gz_seg(std::integer_sequence<int, K...>, PcPlane<QMAX, BY> &hh,
                                          PcPlane<QMAX, BY> &ee, bool live, int &gz, PcPrune &pp)
{
    if ((pc_gz_of<PRUNE>(gz) >> 3) != S) return;            // uniform
    (pc_gz_group<QMAX, BY, PRUNE, 8 * S + K>(hh, ee, live, gz, pp), ...);
}

template <int QMAX, bool BY, bool PRUNE, int... S>
__device__ __forceinline__ void pc_gz_refresh(std::integer_sequence<int, S...>, PcPlane<QMAX, BY> &hh,
                                              PcPlane<QMAX, BY> &ee, bool live, int &gz, PcPrune &pp)
{
    (pc_gz_seg<QMAX, BY, PRUNE, S>(std::make_integer_sequence<int, 8>{}, hh, ee, live, gz, pp), ...);
}

// group G of the right cap's walk: taken only when it is the group under the cap (uniform) and lies at or
// above gz + 2.  ub = the largest UB of its slots (pc_pb_reg without a left limit) and the floor
// 1 + (qlen - 4G): a zero slot may turn positive on the next row through the F chain.
template <int QMAX, int G>
__device__ __forceinline__ void pc_rp_group(PcPlane<QMAX, false> &hh, PcPlane<QMAX, false> &ee, bool live, int gzv,
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
__device__ __forceinline__ void pc_rp_seg(std::integer_sequence<int, K...>, PcPlane<QMAX, false> &hh,
                                          PcPlane<QMAX, false> &ee, bool live, int gzv, int &cap4, int qlen, int t,
                                          uint32_t &nev)
{
    if (((cap4 - 4) >> 5) < S) return;                      // uniform: the cap lies below this segment
    (pc_rp_group<QMAX, 8 * S + 7 - K>(hh, ee, live, gzv, cap4, qlen, t, nev), ...);
}

// the walk, from the group under the cap downward (segments of 8 groups, top first)
template <int QMAX, int... S>
__device__ __forceinline__ void pc_rp_walk(std::integer_sequence<int, S...>, PcPlane<QMAX, false> &hh,
                                           PcPlane<QMAX, false> &ee, bool live, int gzv, int &cap4, int qlen, int t,
                                           uint32_t &nev)
{
    constexpr int NS = sizeof...(S);
    (pc_rp_seg<QMAX, NS - 1 - S>(std::make_integer_sequence<int, 8>{}, hh, ee, live, gzv, cap4, qlen, t, nev), ...);
}

}  // namespace bsw
