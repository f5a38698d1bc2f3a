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
#include "bsw_pc_rules.h"
#include "bsw_pc_group.h"
#include "bsw_pc_scan.h"

namespace bsw {

constexpr int kPcChunkDw = 17;           // dwords per lane per 64-row target chunk (as lane kernel)
#ifdef BSW_PC_STATS
__device__ unsigned long long g_pc_stats[19];
// per-wave schedule record (tools/pc_times.py): start / end (s_memrealtime, 100 MHz), XCC id and
// HW_ID (CU / SIMD / SE), rows run -- the launch's occupancy over time, ramp-up and tail
constexpr int kPcTimesMax = 1 << 16;
__device__ unsigned long long g_pc_times[kPcTimesMax][4];
#endif

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

// the same for a width the caller has already bounded (0 <= n <= 63): no clamp, so a uniform n stays in SGPRs
__device__ __forceinline__ uint64_t gbits_nc(int lo, int n)
{
    uint64_t m;
    asm("s_bfm_b64 %0, %1, %2" : "=s"(m)
        : "s"(__builtin_amdgcn_readfirstlane(n)), "s"(__builtin_amdgcn_readfirstlane(lo)));
    return m;
}

// Lane conditions of the row loop as wave masks: a compare writes its SGPR pair, and / or / not of
// conditions are scalar instructions, a vote is a test of the pair, and a select takes the pair as it is.  (A bool
// that is not itself a compare costs v_cndmask 0, 1 + v_cmp_ne at every __ballot, and the short-circuit forms
// of && and || come back as exec-masked blocks.)  The row loop runs with every lane enabled.
typedef uint64_t lmask;
__device__ __forceinline__ lmask m_eq(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 32); }
__device__ __forceinline__ lmask m_ne(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 33); }
__device__ __forceinline__ lmask m_gt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 38); }
__device__ __forceinline__ lmask m_ge(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 39); }
__device__ __forceinline__ lmask m_lt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 40); }
__device__ __forceinline__ lmask m_le(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 41); }
// this lane's bit of a mask, for a select or a helper that takes a lane's bool (no instruction)
__device__ __forceinline__ bool m_on(lmask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// a select on a lane mask as one v_cndmask that the compiler cannot turn back into an exec-masked block
__device__ __forceinline__ int pc_sel(lmask mask, int a, int b)
{
    int r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(mask));
    return r;
}

// group G of a row, where the class has it: its query word and plane registers to the group statement
template <int QMAX, bool BY, int G>
__device__ __forceinline__ void pc_group_if(PcPlane<QMAX, BY> &hh, PcPlane<QMAX, BY> &ee,
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
            pc_group<G, QMAX >= 128>(hh[2 * G], hh[2 * G + 1], ee[2 * G], ee[2 * G + 1], qs[G], plo, phi, f, h1, key, oe2, ed2,
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
__device__ __forceinline__ void pc_seg(std::integer_sequence<int, K...>, PcPlane<QMAX, BY> &hh,
                                       PcPlane<QMAX, BY> &ee, const uint32_t (&qs)[QMAX / 4], uint32_t plo,
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
__device__ __forceinline__ void pc_row(std::integer_sequence<int, S...>, PcPlane<QMAX, BY> &hh,
                                       PcPlane<QMAX, BY> &ee, const uint32_t (&qs)[QMAX / 4],
                                       uint32_t plo, uint32_t phi, int &f, int &h1, uint32_t &key,
                                       uint32_t oe2, uint32_t ed2, int ed, const PcRow &r,
                                       uint32_t endw, uint32_t endm1w, uint32_t begm2w, int endv,
                                       int begv, const PcbSel &bs, uint32_t (&ctr)[4])
{
    (pc_seg<QMAX, BY, S>(std::make_integer_sequence<int, pc_seg_len<QMAX>()>{}, hh, ee, qs, plo, phi, f, h1, key, oe2,
                         ed2, ed, r, endw, endm1w, begm2w, endv, begv, bs, ctr), ...);
}

// ---- the row-level rules.  Their switches and constants: bsw_pc_rules.h; their scans
// and walks over the plane registers: bsw_pc_scan.h; here what each rule is and which classes carry it.
//
// Early stop: a lane whose band has reached the query's end (end == qlen) and
// left column 0 (beg > 0) retires once no cell of any later row can reach gscore (hence best):
// every later value is a path from one of this row's slots whose only gains are diagonal steps,
// at most 1 each (the pk_ok contract: match 1, the same fact the A.5 gate of PC_PH1 rests on) and
// at most qlen - 1 - j of them from column j.
//   scalar bound        : UB = m + min(qlen - 1 - beg, tlen - 1 - i), selects at the row end
//   per-cell bound      : UB = max over slots s in (beg, end] of H(i, s-1) + (qlen - s), a packed
//                         scan (pc_ubscan) behind one ballot, on the rows of one phase
//
// Left skip: groups that lie wholly inside the all-zero left prefix common
// to the wave's live lanes are dropped from the row's entered set -- computing them rewrites zeros
// (§3 item 1).  gz is wave-uniform and never decreases; at the start of every row each live lane
// holds H == 0 and E <= 0 (bytes: E == 0) in every slot s < 4 gz, slot 0 (the column -1 boundary)
// included.  gz is refreshed at the row end, behind one uniform test, on rows with
// (i & BSW_PC_SKIP_MASK) == BSW_PC_SKIP_ROW: while group gz is zero in both planes for every lane
// that stays alive it advances, an unrolled walk over compile-time register indices with uniform
// skips (segments of 8 groups, then the group), as pc_ubscan and pc_lastpos.  Only the classes from
// BSW_PC_SKIP_QMIN up carry it.
template <int QMAX> constexpr bool pc_left_skip() { return BSW_PC_LEFT_SKIP && QMAX >= BSW_PC_SKIP_QMIN; }

// Left prune: at the refresh gz also passes over a NON-zero group when no
// cell of it can reach gscore (hence best) in any lane that stays alive -- the early stop's per-cell
// bound (item 10) applied to a prefix of the row.  Precheck (uniform, once per refresh): i > wl_max
// (every static beg > 0) and every staying lane has end == qlen and gsc > 0.  Then per lane
//   H plane: slots s > beg with H > 0:   H + (qlen - s)     < gsc
//   E plane: slots s >= beg with E > 0:  E + (qlen - 1 - s) < gsc
// in the style of pc_ub_reg; the group's plane registers are then zeroed in every lane (the left
// skip's invariant holds literally) and the wave is marked pruned: from the next row on the row-end
// certificate sends the lanes whose fate the zeroed cells could have changed to the redo pass.  Only the int16
// classes from BSW_PC_PRUNE_QMIN up carry it.
template <int QMAX, bool BY> constexpr bool pc_left_prune()
{
    return BSW_PC_LEFT_PRUNE && !BY && pc_left_skip<QMAX>() && QMAX >= BSW_PC_PRUNE_QMIN;
}

// Right prune: a wave-uniform right cap.  Past the first rows the insertion tail of
// the diagonal is positive out to the query's end, so every row runs FAST groups to qlen although most of
// those cells can no longer reach the lane's current best.  cap4 (a slot index, a multiple of 4; 4 NG = no
// cap) clamps every lane's band end at the row head: the groups above it leave the entered set through the
// band-end reduction and group cap4 / 4 runs as the row's right-edge group.  At the refresh the cap walks
// down over groups whose every slot, in every staying lane, has UB + SLACK < T = best - MARGIN (pc_rp_group);
// every row of a marked wave checks what leaves the computed columns -- it all goes through h1 -- against
// T, and a lane is final only with gsc >= P, the largest threshold ever applied to it: the others are computed
// again by the redo pass.  The rule speculates on the lane's final gscore alone.  MARGIN, SLACK, SLACK2, K, ROW0,
// WALK_MASK and RWIN are bsw_pc_rules.h's BSW_PC_RP_*; the rule runs in the classes of the left prune.
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
// the same on a clipped lane's row, with the clipped mark, without the max: a lane's best never falls, so the
// threshold of the row at hand is at least every threshold the field has held
__device__ __forceinline__ uint32_t pc_rp_put(uint32_t hi, int t)
{
    return (hi & kPcLowHi) | (((uint32_t)max(t, 0) << (kPcPShift - 32)) + ((1u << (kPcPShift - 32)) | kPcClipHi));
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
    constexpr int NP = PcNp<QMAX, BY>::v;
    PcPlane<QMAX, BY> hh, ee;
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
    int best = h0, best_i = -1, best_d = 0, max_ie = -1, gsc = -1, moff = 0, endc = qlen;
    const bool alive0 = valid && tlen > 0;
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
    if (alive0) { issue_chunk(0); issue_chunk(1); }
    uint32_t tcur = 0;
    const int wl_max = __builtin_amdgcn_readfirstlane(wave_max(alive0 ? wl : -1));
    const int wl_min = __builtin_amdgcn_readfirstlane(wave_min(alive0 ? wl : INT_MAX));
    const uint32_t oe2 = (uint32_t)(kp.o_del + kp.e_del) * 0x10001u;
    const uint32_t ed2 = (uint32_t)kp.e_del * 0x10001u;
    uint32_t ctr[4] = {0, 0, 0, 0};                       // BSW_PC_STATS group-path counters
    // key selectors in VGPRs: the byte planes' (BY) or the J form's (int16 planes)
    // (the J form's only where the two VGPRs cost no occupancy: QMAX >= 128 runs at two
    // waves per SIMD either way; the 96 / 64 classes would drop from 3 / 4 waves)
    PcbSel bs{BY ? kSelKa : 0x06010400u, BY ? kSelKb : 0x06030402u};
    if constexpr (BY || QMAX >= 128) asm volatile("" : "+v"(bs.ka), "+v"(bs.kb));
#ifdef BSW_PC_STATS
    uint32_t nrows = 0, nlast = 0, nue = 0;
    uint32_t nscan = 0, nstop_s = 0, nstop_c = 0;   // early stop: scan rows; this lane retired by bound
    (void)nscan; (void)nstop_s; (void)nstop_c;
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
    const int zdrop = kp.zdrop > 0 ? kp.zdrop : INT_MAX;   // z-drop off: a distance no row reaches
    lmask alive = __ballot(alive0);         // the lanes still running, a wave mask (lmask, above) all through the loop
    for (int i = 0;; ++i) {
        const lmask act = alive & m_lt(i, tlen);
        alive = act;
        if (act == 0) break;
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
                if (i > 0 && m_on(act)) issue_chunk((i >> 6) + 1);   // refill the buffer just drained
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
            const int eu = wave_max(m_on(act) ? min(i + wl + 1, qlen) : -1), ec = wave_max(m_on(act) ? min(endcl, cap4) : -1);
            if (cap4 < QMAX && ec >= 0) nrcap += (uint32_t)max((min(eu, QMAX - 1) >> 2) - (min(ec, QMAX - 1) >> 2), 0);
        }
#endif
        if constexpr (RP) endcl = min(endcl, cap4);   // the right cap (§3 item 13): one v_min with a uniform operand
        const int end = endcl;
        endc = end;
        int emax, emin;
        PcRow r;
        wave_maxmin_bc(m_on(act) ? end : -1, m_on(act) ? end : INT_MAX, emax, emin);
        {
            const int ulo = __builtin_amdgcn_readfirstlane(max(0, i - wl_max));  // min beg
            const int uhi = __builtin_amdgcn_readfirstlane(emax);                // max end
            const int flo = __builtin_amdgcn_readfirstlane(max(0, i - wl_min));  // max beg
            const int fhi = __builtin_amdgcn_readfirstlane(emin);                // min end
            const int glo = ulo >> 2;
            const int gsp = max((min(uhi, QMAX - 1) >> 2) - glo, -1);      // uhi >= 0: a live lane
            // FAST needs 4G > every beg (entering chain valid) -- or one common beg == 4G with
            // nothing computed before it -- and 4G + 4 <= every end
            // (gfa = flo >> 2 for one common beg on a group boundary, else (flo >> 2) + 1, in three scalar
            // instructions: flo rounded up to a group, one more when the begs differ.  gfn <= NG: fhi is a live
            // lane's end, so its set takes no clamp)
            int gfa;
            asm("s_cmp_lg_u32 %1, %2\n\ts_addc_u32 %0, %2, 3" : "=s"(gfa) : "s"(ulo), "s"(flo) : "scc");
            gfa >>= 2;
            const int gfn = max((fhi >> 2) - gfa, 0);
            r.fast = gbits_nc(gfa, gfn);
            const int gln = (flo >> 2) - glo;
            r.enter = gbits(glo, gsp + 1);
            r.left = gbits(glo, gln + 1);
            if constexpr (pc_left_skip<QMAX>()) {   // groups below gz leave the entered set; the FAST
                const uint64_t keep = ~0ull << pc_gz_of<PRUNE>(gz);   // test comes first in a group, so its set too
                r.enter &= keep;
                r.fast &= keep;
            }
        }
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
            // (each compare once: a mask built by a builtin is not merged with its twin)
            const lmask atend = m_eq(end, qlen), h1z = m_eq(h1, 0);   // end <= qlen and h1 >= 0 always
            {                                     // A.4: j == qlen; h1 = H(i, qlen - 1)
                const lmask atq = act & atend;
                max_ie = m_on(atq & ~m_gt(gsc, h1)) ? i : max_ie;
                gsc = m_on(atq) ? max(gsc, h1) : gsc;
            }
            // A.4 row end, straight-line: m <= 0 ends the lane; a new best moves (best, best_i,
            // best_j, max_off); otherwise z-drop against the old best
            {
                // the lane carries best_d = best_i - best_j in place of best_j: d = di - dj = x - best_d with x =
                // i - mj, which max_off shares; one of the two products is 0 (|d| and e are small and non-negative:
                // 24-bit multiplies, full rate).  dz is made opaque, so it is computed on every row and not inside
                // an exec-masked block for the lanes with m > 0
                const int x = i - mj;
                int dz = best - m - (int)__umul24((unsigned)max(x - best_d, 0), (unsigned)kp.e_del)
                                  - (int)__umul24((unsigned)max(best_d - x, 0), (unsigned)kp.e_ins);
                asm volatile("" : "+v"(dz));
                const lmask pos = m_gt(m, 0);
                const lmask better = act & m_gt(m, best);        // best >= h0 >= 0: never with m <= 0
                alive = act & pos & (better | m_le(dz, zdrop));
                const int zb = best - m;                         // against the old best, where the row has no new one
                moff = pc_sel(better, max(moff, abs(x)), moff);
                best_i = pc_sel(better, i, best_i);
                best_d = pc_sel(better, x, best_d);
                best = pc_sel(better, m, best);
                if constexpr (PRUNE) {
                    // a marked wave (left-pruned, item 12; under the right cap, item 13): both certificates in one
                    // block behind one uniform test.  Item 12, before the early stop: zeroed cells only lower
                    // values, all below gscore, so a lane whose row has a new best or is far from z-drop whatever
                    // mj is (dz <= best - m) is in its true state; one whose row maximum is 0 retires with its
                    // outputs final; the others -- and, in a left-pruned wave, a lane whose band end would leave
                    // qlen (h1 == 0) -- are computed again.  Item 13, the crossing certificate: a lane whose band
                    // end has sat at the cap lets H(i, end-1) = h1 leave the computed columns, diagonally or along
                    // the row, and h1's potential must stay below T = best - MARGIN.  Without rmark the cap is QMAX
                    // and no lane carries the clipped mark, so cl is empty and item 13's half needs no test of its
                    // own.  The redo mark travels in the low bit of sp (SeqPair is 4-byte aligned), one bit for both.
                    if ((gz & kPcPruned) || (RP && rmark)) {     // uniform: the wave's marks
                        lmask rd = (act ^ better) & pos & m_gt(zb, zdrop);
                        if (gz & kPcPruned) rd |= alive & h1z;
#ifdef BSW_PC_STATS
                        rcause = (m_on(rd) && !rcause) ? 2u : rcause;
#endif
                        if constexpr (RP) {
                            const int t = best - BSW_PC_RP_MARGIN, phi = h1 + (qlen - end);
                            const uint32_t hi = pc_sp_hi(sp);
                            const lmask cl = act & ~atend & (m_eq(end, cap4) | m_ne((int)(hi & kPcClipHi), 0));
                            const lmask rdc = cl & ~h1z & m_ge(phi, t);
#ifdef BSW_PC_STATS
                            rcause = (m_on(rdc) && !rcause) ? 1u : rcause;
#endif
                            rd |= rdc;
                            // (a redo lane's P is never read)
                            sp = pc_sp_set(sp, (uint32_t)pc_sel(cl, (int)pc_rp_put(hi, t), (int)hi), m_on(rd));
                        } else {
                            sp = (SeqPair *)((uintptr_t)sp | (uintptr_t)m_on(rd));
                        }
                        alive &= ~rd;
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
                const lmask edge = atend & m_lt(gq, qlen);         // beg > 0, from the opaque difference: a
                                                               // test of beg is made at the row head and
                                                               // its mask kept across the groups
                const int ubs = m - 1 + min(gq, gt);
                const lmask stop = edge & m_le(ubs, best) & m_lt(ubs, gsc);
#ifdef BSW_PC_STATS
                nstop_s += m_on(alive & stop);
#endif
                alive &= ~stop;
#if BSW_PC_EARLY_SCAN
                // the per-cell bound, on rows of one phase (wave-uniform: every fourth) and only for lanes
                // whose arg-max cell already passes it (a necessary condition: false all along the
                // diagonal phase, true right after it).  Not for QMAX <= 64: there the scan's
                // registers cost the int16 form its fourth wave per SIMD (127 -> 137 VGPRs)
                if (QMAX > 64 && (i & BSW_PC_SCAN_PHASE) == BSW_PC_SCAN_PHASE) {
                    const int ubm = m - 1 + gm;
                    const lmask want = alive & edge & m_le(ubm, best) & m_lt(ubm, gsc);
                    if (want) {
                        const int ubc = pc_ubscan<QMAX, BY>(std::make_integer_sequence<int, NG>{}, hh, gq + beg, beg, r.enter);
                        const lmask stopc = want & m_le(ubc, best) & m_lt(ubc, gsc);
#ifdef BSW_PC_STATS
                        nscan += 1;
                        nstop_c += m_on(stopc);
#endif
                        alive &= ~stopc;
                    }
                }
#endif
            }
#endif
            if constexpr (pc_left_skip<QMAX>()) {
                if ((i & BSW_PC_SKIP_MASK) == BSW_PC_SKIP_ROW) {
                    if constexpr (PRUNE) {         // the prune's precheck: every static beg > 0, and
                                                   // every staying lane at the query's end with gsc > 0
                        pp.pre = i > wl_max && (alive & ~(atend & m_gt(gsc, 0))) == 0;
                        // (qlen through an opaque move: its packed forms are then built in the walk,
                        // not hoisted into registers that live across the groups)
                        asm volatile("v_mov_b32_e32 %0, %1" : "=v"(pp.qlen) : "v"(qlen));
                        pp.beg = beg; pp.gsc = gsc;
                    }
                    pc_gz_refresh<QMAX, BY, PRUNE>(std::make_integer_sequence<int, (NG + 7) / 8>{}, hh, ee, m_on(alive),
                                                   gz, pp);
                    if constexpr (RP) {
                        // the right cap: precheck (i >= ROW0 and every staying lane with a new best in the last
                        // K rows: on a growing diagonal, where gscore will follow best), then the walk; a
                        // failed precheck under a cap retreats one group
                        if (alive & (i < BSW_PC_RP_ROW0 ? ~0ull : m_gt(i - best_i, BSW_PC_RP_K))) {
                            if (cap4 < QMAX) {
                                cap4 += 4;
#ifdef BSW_PC_STATS
                                nrret += 1;
#endif
                            }
                        } else if ((!rmark || (i & BSW_PC_RP_WALK_MASK) == (BSW_PC_SKIP_ROW & BSW_PC_RP_WALK_MASK)) && alive) {
                            int ql;                 // (opaque, as pp.qlen)
                            asm volatile("v_mov_b32_e32 %0, %1" : "=v"(ql) : "v"(qlen));
                            const uint32_t nev0 = nrev;
                            pc_rp_walk<QMAX>(std::make_integer_sequence<int, NG / 8>{}, hh, ee, m_on(alive),
                                             pc_gz_of<PRUNE>(gz), cap4, ql, best - BSW_PC_RP_MARGIN, nrev);
                            if (nrev != nev0) {     // uniform: T was applied to every staying lane
                                rmark = true;
                                sp = pc_sp_set(sp, m_on(alive) ? pc_rp_raise(pc_sp_hi(sp), best - BSW_PC_RP_MARGIN) : pc_sp_hi(sp), false);
                            }
                        }
                        // the soft retreat, after the walk: one group up when a staying lane's crossing value, at the
                        // cap or within RWIN slots under it, comes near its threshold (one vote; the certificate
                        // is what soundness rests on).  A cap the walk has just put above a moving band edge is
                        // taken back before the edge reaches it: a band narrower than the query never clips
                        if (rmark && cap4 < QMAX &&
                            (alive & ~atend & m_ge(end + BSW_PC_RP_RWIN, cap4) &
                             m_ge(h1 + (qlen - end) + BSW_PC_RP_SLACK2, best - BSW_PC_RP_MARGIN))) {
                            cap4 += 4;
#ifdef BSW_PC_STATS
                            nrret += 1;
#endif
                        }
                    }
                }
            }
#ifdef BSW_PC_STATS
            nrows += m_on(act);
            nue += m_on(act) && (emax == emin);  // every live lane has the same band end
#endif
            {                                      // end_{i+1} = min(lastH + 3, ...), DESIGN.md §3
                const lmask need = alive & h1z;          // H(i, end-1) == 0 -> lastH < end - 1
                int lp1 = end;
                if (need) {
#ifdef BSW_PC_STATS
                    nlast += 1;
#endif
                    const int lp = pc_lastpos<QMAX, BY>(std::make_integer_sequence<int, NG>{}, hh, end, m_on(need),
                                                        emax >> 2);
                    lp1 = m_on(need) ? lp : end;
                }
                endc = m_on(alive) ? min(lp1 + 2, qlen) : endc;
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
        sp->qle = best_i - best_d + 1;
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
