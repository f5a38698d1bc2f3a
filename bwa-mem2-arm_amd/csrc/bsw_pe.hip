// bsw_pe.hip -- the paired-end stage (include/bsw_pe.h: mem_pestat's counting, mem_pair and the
// decision block of mem_sam_pe) over the arrays bsw_regs_select_resident leaves:
//   pe_stat_kernel         : one work item per pair -- cal_sub of both ends, infer_dir, the insert
//                            size counted per direction.  A block gathers its pairs' (dir, is) in
//                            an LDS table (open addressing) and adds each distinct key to the
//                            global bins once; a key that finds no slot goes to the bins directly
//   pe_pair_fast_kernel    : four pairs per work item -- a pair with at most one region per end is
//                            finished here from registers (no sort, no loop); the others go to a
//                            list through LDS and one atomic per block.  The outcome counters are
//                            added up per wave, then per block, into one of 32 slots by block
//   pe_pair_general_kernel : the listed pairs, its count read on the device -- the second primary
//                            marking of both reads (bsw_sel_dev.h) on work lists in HBM, v sorted
//                            in HBM with the introsort's stack in LDS, mem_pair's loop twice (the
//                            best and the runner-up, then n_sub: u is never stored), the decision
// MAPQ, log and erfc in double precision.  Plain C++ with vector stores only; no private arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "bsw_pe_k.h"
#include "bsw_sel_dev.h"
#include "bsw_stage_k.h"

namespace bsw {

constexpr int kPeTable = 2048;          // pe_stat_kernel: LDS slots per block (key + count, 16 KB)
constexpr int kPeTableBits = 11;
constexpr int kPeProbes = 8;
constexpr int kPeStatBlock = 256;
constexpr int kPeStatPer = 16;          // pairs per work item: 4096 pairs share a table

struct LtPeV {                          // v by (x, y)
    typedef PeV E;
    struct K { int64_t x; uint64_t y; };
    static __device__ __forceinline__ K key(const PeV &v) { return K{v.x, v.y}; }
    static __device__ __forceinline__ bool lt(const K &a, const K &b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }
    static __device__ __forceinline__ void swap(PeV *a, PeV *b)
    {
        uint4 *p = reinterpret_cast<uint4 *>(a), *q = reinterpret_cast<uint4 *>(b);
        const uint4 t = *p, u = *q;
        *p = u;
        *q = t;
    }
};

// the three offsets of pair pr, checked: everything a kernel touches lies in [f0, f2) of [0, n_regs)
__device__ __forceinline__ bool pe_bounds(const int32_t *__restrict__ first, int pr, int n_regs, int &f0, int &f1, int &f2)
{
    f0 = first[2 * pr]; f1 = first[2 * pr + 1]; f2 = first[2 * pr + 2];
    return f0 >= 0 && f0 <= f1 && f1 <= f2 && f2 <= n_regs && f1 - f0 <= BSW_SEL_MAX_PER_READ &&
           f2 - f1 <= BSW_SEL_MAX_PER_READ;
}

__device__ __forceinline__ int pe_cal_sub(const SelParams &p, const bsw_alnreg_t *__restrict__ a, int n)
{
    const int qb0 = a[0].qb, qe0 = a[0].qe;
    for (int j = 1; j < n; ++j) {
        const int qb = a[j].qb, qe = a[j].qe;
        const int b_max = max(qb, qb0), e_min = min(qe, qe0);
        if (e_min > b_max) {
            const int min_l = min(qe - qb, qe0 - qb0);
            if ((float)(e_min - b_max) >= (float)min_l * p.mask_level) return a[j].score;
        }
    }
    return p.min_seed_len * p.a;
}

// the hits at rb0 and rb1 lie on one contig (with no table: always)
__device__ __forceinline__ bool pe_same_rid(const PeParams &p, int64_t rb0, int64_t rb1)
{
    return !p.ctg.off || contig_rid(p.ctg, rb0) == contig_rid(p.ctg, rb1);
}

__global__ __launch_bounds__(kPeStatBlock) void pe_stat_kernel(const PeParams p, const bsw_alnreg_t *__restrict__ regs,
                                                               const int32_t *__restrict__ first,
                                                               int32_t *__restrict__ hist, int32_t *__restrict__ meta)
{
    __shared__ int s_key[kPeTable];
    __shared__ int s_cnt[kPeTable];
    for (int k = threadIdx.x; k < kPeTable; k += kPeStatBlock) {
        s_key[k] = -1;
        s_cnt[k] = 0;
    }
    __syncthreads();
    const int bins = p.max_ins + 1;
    const int64_t two_l = p.s.l_pac << 1;
    int err = 0;
    for (int it = 0; it < kPeStatPer; ++it) {
        const int64_t pr64 = ((int64_t)blockIdx.x * kPeStatPer + it) * kPeStatBlock + threadIdx.x;
        if (pr64 >= p.n_pairs) break;
        const int pr = (int)pr64;
        int f0, f1, f2;
        if (!pe_bounds(first, pr, p.n_regs, f0, f1, f2)) {
            err = 1;
            continue;
        }
        bool bad = false;
        for (int k = f0; k < f2; ++k) {
            const int64_t rb = regs[k].rb;
            bad |= rb < 0 || rb >= two_l;
        }
        if (bad) {
            err = 1;
            continue;
        }
        if (f1 == f0 || f2 == f1) continue;
        const bsw_alnreg_t *a0 = regs + f0, *a1 = regs + f1;
        if ((double)pe_cal_sub(p.s, a0, f1 - f0) > 0.8 * a0[0].score) continue;
        if ((double)pe_cal_sub(p.s, a1, f2 - f1) > 0.8 * a1[0].score) continue;
        if (!pe_same_rid(p, a0[0].rb, a1[0].rb)) continue;   // (mem_pestat: r[0]->a[0].rid != r[1]->a[0].rid)
        int64_t is;
        const int dir = infer_dir(p.s.l_pac, a0[0].rb, a1[0].rb, is);
        if (is == 0 || is > p.max_ins) continue;
#ifdef BSW_PE_STAT_DIRECT                               // experiment build: no table, DESIGN.md §4.18
        atomicAdd(&hist[dir * bins + (int)is], 1);
        continue;
#endif
        const int key = dir << 17 | (int)is;            // is <= BSW_PE_MAX_INS = 2^16
        unsigned h = ((unsigned)key * 2654435761u) >> (32 - kPeTableBits);
        bool done = false;
        for (int probe = 0; probe < kPeProbes && !done; ++probe) {
            const int prev = atomicCAS(&s_key[h], -1, key);
            if (prev == -1 || prev == key) {
                atomicAdd(&s_cnt[h], 1);
                done = true;
            }
            h = (h + 1) & (kPeTable - 1);
        }
        if (!done) atomicAdd(&hist[dir * bins + (int)is], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kPeTable; k += kPeStatBlock) {
        const int key = s_key[k];
        if (key >= 0) atomicAdd(&hist[(key >> 17) * bins + (key & 0x1ffff)], s_cnt[k]);
    }
    if (err) atomicOr(&meta[kPeErr], 1);
}

// ---------------------------------------------------------------- pairing
__device__ __forceinline__ int pe_raw(int d, int a) { return (int)(6.02 * d / a + .499); }

// mem_pair's q of two hits `dist` apart under direction d
__device__ __forceinline__ int pe_q(const PeDir &d, int64_t dist, uint32_t si, uint32_t sk, int a)
{
    const double ns = ((double)dist - d.avg) / d.std;
    const int q = (int)((double)((uint64_t)si + (uint64_t)sk) + .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * a + .499);
    return max(q, 0);
}

// mem_sam_pe's choice of branch: 0 = no_pairing, 1 = paired with o > score_un, 2 = paired without
__device__ __forceinline__ int pe_decide(const PeParams &p, bool both, int o, int sub, int n_sub, bool multi, int s0,
                                         int s1, float fr0, float fr1, int &q_pe, bool &was_multi)
{
    q_pe = 0;
    was_multi = false;
    if (!both || o <= 0) return 0;
    if (multi) {
        was_multi = true;
        return 0;
    }
    const int score_un = s0 + s1 - p.pen_unpaired;
    const int subo = max(sub, score_un);
    q_pe = pe_raw(o - subo, p.s.a);
    if (n_sub > 0) q_pe -= (int)(4.343 * log((double)(n_sub + 1)) + .499);
    q_pe = max(min(q_pe, 60), 0);
    q_pe = (int)(q_pe * (1. - .5 * (fr0 + fr1)) + .499);
    return o > score_un ? 1 : 2;
}

// the paired branch's MAPQ of the chosen region c (its secondary already < 0)
__device__ __forceinline__ int pe_qse(const PeParams &p, const SelW &c, float fr, int q_pe)
{
    int q_se = sel_mapq(p.s, c, fr);
    q_se = q_se > q_pe ? q_se : min(q_pe, q_se + 40);
    return min(q_se, pe_raw(c.r.score - c.csub, p.s.a));
}

// no_pairing's proper flag from the two first regions
__device__ __forceinline__ int pe_unpaired_proper(const PeParams &p, const PeDir *pes, int64_t rb0, int64_t rb1)
{
    int64_t dist;
    const PeDir d = pes[infer_dir(p.s.l_pac, rb0, rb1, dist)];
    return !d.failed && dist >= d.low && dist <= d.high && pe_same_rid(p, rb0, rb1);
}

__device__ __forceinline__ void pe_load_pes(const PeParams &p, PeDir *s_pes)
{
    if (threadIdx.x == 0) {
        s_pes[0] = p.pes[0];
        s_pes[1] = p.pes[1];
        s_pes[2] = p.pes[2];
        s_pes[3] = p.pes[3];
    }
    __syncthreads();
}

// outcome bits of one pair (the counters of bsw_pe_stats_t)
constexpr int kPeFErr = 1, kPeFTried = 2, kPeFPaired = 4, kPeFUnp = 8, kPeFProper = 16, kPeFHasU = 32;

// A pair with at most one region per end, [f0, f1) and [f1, f2), from registers -> its outcome bits
__device__ __forceinline__ int pe_fast_pair(const PeParams &p, const PeDir *s_pes, const bsw_alnreg_t *__restrict__ regs,
                                            bsw_selinfo_t *__restrict__ info, bsw_pair_t *__restrict__ pairs, int pr,
                                            int f0, int f1, int f2)
{
    const int n0 = f1 - f0, n1 = f2 - f1;
    const int64_t two_l = p.s.l_pac << 1;
    SelW x0{}, x1{};
    float fr0 = 0.f, fr1 = 0.f;
    bool err = false;
    if (n0) {
        const bsw_selinfo_t f = info[f0];
        selw_load(x0, regs[f0], f, 0);
        fr0 = f.frac_rep;
        err |= x0.r.rb < 0 || x0.r.rb >= two_l;
    }
    if (n1) {
        const bsw_selinfo_t f = info[f1];
        selw_load(x1, regs[f1], f, 0);
        fr1 = f.frac_rep;
        err |= x1.r.rb < 0 || x1.r.rb >= two_l;
    }
    if (err) return kPeFErr;
    int flags = 0;
    // step 1 on a list of one: nothing to sort or mark
    x0.sub = 0; x0.secondary = -1; x0.mapq = n0 ? sel_mapq(p.s, x0, fr0) : 0;
    x1.sub = 0; x1.secondary = -1; x1.mapq = n1 ? sel_mapq(p.s, x1, fr1) : 0;
    // step 2: v has two entries, u at most one
    int o = 0;
    if (n0 && n1) {
        flags |= kPeFTried;
        const int st0 = x0.r.rb >= p.s.l_pac, st1 = x1.r.rb >= p.s.l_pac;
        const int64_t v0 = st0 ? two_l - 1 - x0.r.rb : x0.r.rb, v1 = st1 ? two_l - 1 - x1.r.rb : x1.r.rb;
        const uint64_t y0 = (uint64_t)(uint32_t)x0.r.score << 32 | (uint64_t)(st0 << 1);
        const uint64_t y1 = (uint64_t)(uint32_t)x1.r.score << 32 | (uint64_t)(st1 << 1 | 1);
        const bool end0_first = v0 < v1 || (v0 == v1 && y0 < y1);
        const int sa = end0_first ? st0 : st1, sb = end0_first ? st1 : st0;  // strands in v's order
        const PeDir d = s_pes[sa << 1 | sb];
        const int64_t dist = end0_first ? v1 - v0 : v0 - v1;
        if (!d.failed && dist <= d.high && dist >= d.low && pe_same_rid(p, x0.r.rb, x1.r.rb)) {
            flags |= kPeFHasU;
            o = pe_q(d, dist, (uint32_t)x0.r.score, (uint32_t)x1.r.score, p.s.a);
        }
    }
    // step 3
    bsw_pair_t out;
    int q_pe;
    bool wm;
    const int br = pe_decide(p, n0 && n1, o, 0, 0, false, x0.r.score, x1.r.score, fr0, fr1, q_pe, wm);
    out.score = o; out.sub = 0; out.n_sub = 0; out.q_pe = q_pe;
    if (br == 0) {
        const int w0 = n0 && x0.r.score >= p.T ? 0 : -1, w1 = n1 && x1.r.score >= p.T ? 0 : -1;
        out.paired = 0;
        out.z[0] = w0; out.z[1] = w1;
        out.mapq[0] = w0 == 0 ? x0.mapq : 0;
        out.mapq[1] = w1 == 0 ? x1.mapq : 0;
        out.proper = w0 == 0 && w1 == 0 ? pe_unpaired_proper(p, s_pes, x0.r.rb, x1.r.rb) : 0;
    } else {
        out.paired = 1;
        out.z[0] = 0; out.z[1] = 0;
        out.proper = br == 1;
        out.mapq[0] = br == 1 ? pe_qse(p, x0, fr0, q_pe) : x0.mapq;
        out.mapq[1] = br == 1 ? pe_qse(p, x1, fr1, q_pe) : x1.mapq;
        flags |= kPeFPaired | (br == 2 ? kPeFUnp : 0);
    }
    if (out.proper) flags |= kPeFProper;
    pairs[pr] = out;
    if (n0) { info[f0].sub = 0; info[f0].secondary = -1; info[f0].mapq = x0.mapq; }
    if (n1) { info[f1].sub = 0; info[f1].secondary = -1; info[f1].mapq = x1.mapq; }
    return flags;
}

// the counters of block b go to slot b % kPeSlots (one 64-B line each): every wave adding to one
// line held this kernel at 0.82 ms for 1M pairs
__device__ __forceinline__ int32_t *pe_slot(int32_t *meta) { return meta + (blockIdx.x % kPeSlots) * kPeMetaWords; }

__global__ __launch_bounds__(kPeFastBlock) void pe_pair_fast_kernel(const PeParams p, const bsw_alnreg_t *__restrict__ regs,
                                                                    bsw_selinfo_t *__restrict__ info,
                                                                    const int32_t *__restrict__ first,
                                                                    bsw_pair_t *__restrict__ pairs,
                                                                    int32_t *__restrict__ list, int32_t *__restrict__ meta)
{
    __shared__ PeDir s_pes[4];
    __shared__ int s_cnt[8];            // err, tried, paired, unpaired, proper, u.n, general pairs, list base
    __shared__ int s_list[kPeFastBlock * kPeFastPer];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    pe_load_pes(p, s_pes);
    int we = 0, wt = 0, wp = 0, wu = 0, wo = 0, wn = 0;      // wave totals
#pragma unroll 1
    for (int it = 0; it < kPeFastPer; ++it) {
        const int64_t pr64 = ((int64_t)blockIdx.x * kPeFastPer + it) * kPeFastBlock + threadIdx.x;
        const int pr = (int)pr64;
        int flags = 0, f0, f1, f2;
        if (pr64 < p.n_pairs) {
            if (!pe_bounds(first, pr, p.n_regs, f0, f1, f2)) flags = kPeFErr;
            else if (f1 - f0 > 1 || f2 - f1 > 1) s_list[atomicAdd(&s_cnt[6], 1)] = pr;
            else flags = pe_fast_pair(p, s_pes, regs, info, pairs, pr, f0, f1, f2);
        }
        we += __popcll(__ballot(flags & kPeFErr)); wt += __popcll(__ballot(flags & kPeFTried));
        wp += __popcll(__ballot(flags & kPeFPaired)); wu += __popcll(__ballot(flags & kPeFUnp));
        wo += __popcll(__ballot(flags & kPeFProper)); wn += __popcll(__ballot(flags & kPeFHasU));
    }
    if ((threadIdx.x & 63) == 0) {
        if (we) atomicAdd(&s_cnt[0], we);
        if (wt) atomicAdd(&s_cnt[1], wt);
        if (wp) atomicAdd(&s_cnt[2], wp);
        if (wu) atomicAdd(&s_cnt[3], wu);
        if (wo) atomicAdd(&s_cnt[4], wo);
        if (wn) atomicAdd(&s_cnt[5], wn);
    }
    __syncthreads();
    int32_t *slot = pe_slot(meta);
    if (threadIdx.x == 0 && s_cnt[0]) atomicOr(&meta[kPeErr], 1);
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&slot[kPeTried], s_cnt[1]);
    if (threadIdx.x == 2 && s_cnt[2]) atomicAdd(&slot[kPePaired], s_cnt[2]);
    if (threadIdx.x == 3 && s_cnt[3]) atomicAdd(&slot[kPeUnpaired], s_cnt[3]);
    if (threadIdx.x == 4 && s_cnt[4]) atomicAdd(&slot[kPeProper], s_cnt[4]);
    if (threadIdx.x == 5 && s_cnt[5])
        atomicAdd(reinterpret_cast<unsigned long long *>(slot + kPeNu), (unsigned long long)s_cnt[5]);
    if (threadIdx.x == 6 && s_cnt[6]) s_cnt[7] = atomicAdd(&meta[kPeGeneral], s_cnt[6]);
    __syncthreads();
    const int ng = s_cnt[6], base = s_cnt[7];
    for (int k = threadIdx.x; k < ng; k += kPeFastBlock) list[base + k] = s_list[k];
}

// mem_pair's loop over the sorted v.  mode 0: the largest u entry (bx, by), the runner-up's q
// (sub) and u.n;  mode 1: cnt = the entries with sub_in - q <= tmp (the largest among them)
__device__ __forceinline__ void pe_scan(const PeParams &p, const PeDir *pes, const PeV *__restrict__ V, int n, int32_t t,
                                        int mode, int sub_in, int tmp, uint64_t &bx, uint64_t &by, int &sub,
                                        long long &nu, int &cnt)
{
    int l0 = -1, l1 = -1, l2 = -1, l3 = -1;
    for (int i = 0; i < n; ++i) {
        const int64_t xi = V[i].x;
        const uint64_t yi = V[i].y;
#pragma unroll 1
        for (int r = 0; r < 2; ++r) {
            const PeDir d = pes[r << 1 | (int)(yi >> 1 & 1)];
            if (d.failed) continue;
            const int which = r << 1 | (int)((yi & 1) ^ 1);
            const int lw = which == 0 ? l0 : which == 1 ? l1 : which == 2 ? l2 : l3;
            for (int k = lw; k >= 0; --k) {
                const uint64_t yk = V[k].y;
                if ((int)(yk & 3) != which) continue;
                const int64_t dist = xi - V[k].x;
                if (dist > d.high) break;
                if (dist < d.low) continue;
                const int q = pe_q(d, dist, (uint32_t)(yi >> 32), (uint32_t)(yk >> 32), p.s.a);
                if (mode == 0) {
                    const uint64_t uy = (uint64_t)k << 32 | (uint64_t)i;
                    const uint64_t ux = (uint64_t)q << 32 | (hash_64(uy ^ (uint64_t)(int64_t)t) & 0xffffffffull);
                    ++nu;
                    if (nu == 1) {
                        bx = ux; by = uy;
                    } else if (ux > bx || (ux == bx && uy > by)) {
                        sub = (int)(bx >> 32);
                        bx = ux; by = uy;
                    } else {
                        sub = max(sub, q);
                    }
                } else if (sub_in - q <= tmp) {
                    ++cnt;
                }
            }
        }
        const int w = (int)(yi & 3);
        l0 = w == 0 ? i : l0; l1 = w == 1 ? i : l1; l2 = w == 2 ? i : l2; l3 = w == 3 ? i : l3;
    }
}

__global__ __launch_bounds__(64) void pe_pair_general_kernel(const PeParams p, bsw_alnreg_t *__restrict__ regs,
                                                             bsw_selinfo_t *__restrict__ info,
                                                             const int32_t *__restrict__ first,
                                                             bsw_pair_t *__restrict__ pairs,
                                                             const int32_t *__restrict__ list, SelW *__restrict__ work,
                                                             int32_t *__restrict__ zbuf, PeV *__restrict__ v,
                                                             int32_t *__restrict__ meta)
{
    __shared__ int s_stk[kSelStack * 3 * 64];
    __shared__ PeDir s_pes[4];
    pe_load_pes(p, s_pes);
    int *stk = s_stk + threadIdx.x;
    const int n_list = min(meta[kPeGeneral], p.n_pairs);
    const int64_t two_l = p.s.l_pac << 1;
    for (int64_t t64 = (int64_t)blockIdx.x * 64 + threadIdx.x; t64 < n_list; t64 += (int64_t)gridDim.x * 64) {
        const int pr = list[t64];
        const int f0 = first[2 * pr], f1 = first[2 * pr + 1], f2 = first[2 * pr + 2];   // (checked by the fast kernel)
        const int n0 = f1 - f0, n1 = f2 - f1;
        SelW *W0 = work + f0, *W1 = work + f1;
        const float fr0 = n0 ? info[f0].frac_rep : 0.f, fr1 = n1 ? info[f1].frac_rep : 0.f;
        bool bad = false;
        for (int k = f0; k < f2; ++k) {
            SelW x;
            selw_load(x, regs[k], info[k], 0);
            bad |= x.r.rb < 0 || x.r.rb >= two_l;
            work[k] = x;
        }
        if (bad) {
            atomicOr(&meta[kPeErr], 1);
            continue;
        }
        // step 1
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
            const int fb = e ? f1 : f0, n = e ? n1 : n0;
            if (n) sel_mark_mapq(p.s, 2 * pr + e, work + fb, n, stk, zbuf + fb, e ? fr1 : fr0);
        }
        // step 2
        bsw_pair_t out;
        out.score = 0; out.sub = 0; out.n_sub = 0;
        int o = 0, sub = 0, n_sub = 0, z0 = 0, z1 = 0;
        const bool both = n0 && n1;
        if (both) {
            atomicAdd(&pe_slot(meta)[kPeTried], 1);
            PeV *V = v + f0;
            const int n = n0 + n1;
            for (int k = 0; k < n; ++k) {
                const int e = k >= n0, i = e ? k - n0 : k;
                const SelW *c = work + f0 + k;
                const int64_t rb = c->r.rb;
                const int st = rb >= p.s.l_pac;
                PeV x;
                x.x = st ? two_l - 1 - rb : rb;
                if (p.ctg.off) x.x += (int64_t)contig_of(p.ctg, x.x) << kPeRidShift;   // (bsw_pe_k.h)
                x.y = (uint64_t)(uint32_t)c->r.score << 32 | (uint64_t)(uint32_t)(i << 2 | st << 1 | e);
                V[k] = x;
            }
            sel_introsort(n, V, stk, LtPeV());
            const int32_t id32 = (int32_t)((p.s.id0 >> 1) + pr);
            const int32_t t = (int32_t)((uint32_t)id32 << 8);
            const int tmp = max(max(p.s.a + p.s.b, p.s.o_del + p.s.e_del), p.s.o_ins + p.s.e_ins);
            uint64_t bx = 0, by = 0;
            long long nu = 0;
            int cnt = 0;
            pe_scan(p, s_pes, V, n, t, 0, 0, tmp, bx, by, sub, nu, cnt);
            if (nu > 0) {
                o = (int)(bx >> 32);
                if (nu == 2) {
                    n_sub = 1;
                } else if (nu > 2) {
                    pe_scan(p, s_pes, V, n, t, 1, sub, tmp, bx, by, sub, nu, cnt);
                    n_sub = cnt - 1;
                }
                const uint64_t yk = V[by >> 32].y, yi = V[by & 0xffffffffull].y;
                const int zk = (int)((uint32_t)yk >> 2), zi = (int)((uint32_t)yi >> 2);
                if (yk & 1) z1 = zk; else z0 = zk;
                if (yi & 1) z1 = zi; else z0 = zi;
                out.score = o; out.sub = sub; out.n_sub = n_sub;
                atomicAdd(reinterpret_cast<unsigned long long *>(pe_slot(meta) + kPeNu), (unsigned long long)nu);
            }
        }
        // step 3
        bool multi = false;
        for (int j = 1; j < n0; ++j) multi |= W0[j].secondary < 0 && W0[j].r.score >= p.T;
        for (int j = 1; j < n1; ++j) multi |= W1[j].secondary < 0 && W1[j].r.score >= p.T;
        int q_pe;
        bool wm;
        const int br = pe_decide(p, both, o, sub, n_sub, multi, both ? W0[0].r.score : 0, both ? W1[0].r.score : 0, fr0,
                                 fr1, q_pe, wm);
        out.q_pe = q_pe;
        if (wm) atomicAdd(&pe_slot(meta)[kPeMulti], 1);
        if (br == 0) {
            const int w0 = n0 && W0[0].r.score >= p.T ? 0 : -1, w1 = n1 && W1[0].r.score >= p.T ? 0 : -1;
            out.paired = 0;
            out.z[0] = w0; out.z[1] = w1;
            out.mapq[0] = w0 == 0 ? W0[0].mapq : 0;
            out.mapq[1] = w1 == 0 ? W1[0].mapq : 0;
            out.proper = w0 == 0 && w1 == 0 ? pe_unpaired_proper(p, s_pes, W0[0].r.rb, W1[0].r.rb) : 0;
        } else if (br == 1) {
            out.paired = 1; out.proper = 1;
            out.z[0] = z0; out.z[1] = z1;
            int m0 = 0, m1 = 0;
#pragma unroll 1
            for (int e = 0; e < 2; ++e) {
                SelW *L = e ? W1 : W0;
                SelW *c = L + (e ? z1 : z0);
                if (c->secondary >= 0) {
                    c->sub = L[c->secondary].r.score;
                    c->secondary = -2;
                }
                const int q_se = pe_qse(p, *c, e ? fr1 : fr0, q_pe);
                m0 = e ? m0 : q_se;
                m1 = e ? q_se : m1;
            }
            out.mapq[0] = m0; out.mapq[1] = m1;
        } else {
            out.paired = 1; out.proper = 0;
            out.z[0] = 0; out.z[1] = 0;
            out.mapq[0] = W0[0].mapq; out.mapq[1] = W1[0].mapq;
            atomicAdd(&pe_slot(meta)[kPeUnpaired], 1);
        }
        if (br) atomicAdd(&pe_slot(meta)[kPePaired], 1);
        if (out.proper) atomicAdd(&pe_slot(meta)[kPeProper], 1);
        pairs[pr] = out;
        for (int k = f0; k < f2; ++k) {
            const SelW *c = work + k;
            regs[k] = c->r;
            info[k] = selw_info(*c, k < f1 ? fr0 : fr1);
        }
    }
}

hipError_t launch_pe_stat(const PeParams &p, const bsw_alnreg_t *regs, const int32_t *first, int32_t *hist,
                          int32_t *meta, hipStream_t s)
{
    if (p.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(pe_stat_kernel, grid_for(p.n_pairs, kPeStatBlock * kPeStatPer), dim3(kPeStatBlock), 0, s, p,
                       regs, first, hist, meta);
    return hipGetLastError();
}

hipError_t launch_pe_pair_fast(const PeParams &p, const bsw_alnreg_t *regs, bsw_selinfo_t *info, const int32_t *first,
                               bsw_pair_t *pairs, int32_t *list, int32_t *meta, hipStream_t s)
{
    if (p.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(pe_pair_fast_kernel, grid_for(p.n_pairs, kPeFastBlock * kPeFastPer), dim3(kPeFastBlock), 0, s, p,
                       regs, info, first, pairs, list, meta);
    return hipGetLastError();
}

hipError_t launch_pe_pair_general(const PeParams &p, bsw_alnreg_t *regs, bsw_selinfo_t *info, const int32_t *first,
                                  bsw_pair_t *pairs, const int32_t *list, SelW *work, int32_t *zbuf, PeV *v,
                                  int32_t *meta, hipStream_t s)
{
    if (p.n_pairs <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>(((int64_t)p.n_pairs + 63) / 64, 4096);
    hipLaunchKernelGGL(pe_pair_general_kernel, dim3((unsigned)blocks), dim3(64), 0, s, p, regs, info, first, pairs, list,
                       work, zbuf, v, meta);
    return hipGetLastError();
}

}  // namespace bsw
