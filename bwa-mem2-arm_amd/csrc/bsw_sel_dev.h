// bsw_sel_dev.h -- device code shared by region selection (bsw_sel.hip), the paired-end stage
// (bsw_pe.hip) and mate rescue (bsw_matesw.hip): a region's moves as 16-byte words, klib's
// ks_introsort with its explicit stack in LDS, a work entry from / to the (region, info) pair the
// stages exchange, bwa's hash_64, primary marking and MAPQ, the dedup loop and its drops and sorts
// as include/bsw_sel.h states them.  Plain C++ with vector stores only; no private arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bsw_sel_k.h"

namespace bsw {

constexpr int kSelStack = 20;           // introsort frames: a push halves the range, n <= 2^20 (the
                                        //   pair sort's 2^21: a frame left out is sorted at the end)

// A region moves as five 16-byte words held in registers (a struct assignment between two
// possibly equal addresses was lowered through a stack temporary).
struct SelRaw { uint4 a, b, c, d, e; };
static_assert(sizeof(SelW) == 80 && alignof(SelW) == 16, "SelW moves as 5 x uint4");
__device__ __forceinline__ SelRaw sel_ld(const SelW *p)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    return SelRaw{q[0], q[1], q[2], q[3], q[4]};
}
__device__ __forceinline__ void sel_st(SelW *p, const SelRaw &v)
{
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = v.a; q[1] = v.b; q[2] = v.c; q[3] = v.d; q[4] = v.e;
}
__device__ __forceinline__ void sel_copy(SelW *dst, const SelW *src) { sel_st(dst, sel_ld(src)); }
__device__ __forceinline__ void sel_swap(SelW *x, SelW *y)
{
    const SelRaw a = sel_ld(x), b = sel_ld(y);
    sel_st(x, b);
    sel_st(y, a);
}

// (bsw_alnreg_t, bsw_selinfo_t), as the stages pass a region on, -> its work entry and back.  The
// info's frac_rep belongs to the read, not to the entry: the caller keeps it and says what hash holds.
__device__ __forceinline__ void selw_load(SelW &x, const bsw_alnreg_t &r, const bsw_selinfo_t &f, uint64_t hash)
{
    x.r = r;
    x.seedcov = f.seedcov; x.sub = f.sub; x.csub = f.csub; x.sub_n = f.sub_n; x.n_comp = f.n_comp;
    x.secondary = f.secondary; x.src = f.src; x.mapq = f.mapq; x.hash = hash;
}
__device__ __forceinline__ bsw_selinfo_t selw_info(const SelW &x, float frac_rep)
{
    bsw_selinfo_t f;
    f.seedcov = x.seedcov; f.sub = x.sub; f.csub = x.csub; f.sub_n = x.sub_n; f.n_comp = x.n_comp;
    f.secondary = x.secondary; f.mapq = x.mapq; f.src = x.src; f.frac_rep = frac_rep;
    return f;
}

// comparators over small keys (a pivot kept as a whole SelW went to scratch); E = the element
// type a comparator sorts, swap = how two of them change places
struct LtSelW {
    typedef SelW E;
    static __device__ __forceinline__ void swap(SelW *x, SelW *y) { sel_swap(x, y); }
};
struct LtRe : LtSelW {
    typedef int64_t K;
    static __device__ __forceinline__ K key(const SelW &x) { return x.r.re; }
    static __device__ __forceinline__ bool lt(const K &x, const K &y) { return x < y; }
};
struct LtScorePos : LtSelW {            // alnreg_slt2 + rb + qb
    struct K { int32_t score, qb; int64_t rb; };
    static __device__ __forceinline__ K key(const SelW &x) { return K{x.r.score, x.r.qb, x.r.rb}; }
    static __device__ __forceinline__ bool lt(const K &x, const K &y)
    {
        return x.score > y.score || (x.score == y.score && (x.rb < y.rb || (x.rb == y.rb && x.qb < y.qb)));
    }
};
struct LtScoreHash : LtSelW {           // alnreg_hlt
    struct K { int32_t score; uint64_t hash; };
    static __device__ __forceinline__ K key(const SelW &x) { return K{x.r.score, x.hash}; }
    static __device__ __forceinline__ bool lt(const K &x, const K &y)
    {
        return x.score > y.score || (x.score == y.score && x.hash < y.hash);
    }
};
#define SEL_LT(x, y) LT::lt(LT::key(x), LT::key(y))

template <class LT>
__device__ __forceinline__ void sel_insertsort(typename LT::E *s, typename LT::E *t, LT)
{
    for (typename LT::E *i = s + 1; i < t; ++i)
        for (typename LT::E *j = i; j > s && SEL_LT(*j, *(j - 1)); --j) LT::swap(j, j - 1);
}

template <class LT>
__device__ __forceinline__ void sel_combsort(int n, typename LT::E *a, LT)
{
    const double shrink_factor = 1.2473309501039786540366528676643;
    int do_swap, gap = n;
    do {
        if (gap > 2) {
            gap = (int)(gap / shrink_factor);
            if (gap == 9 || gap == 10) gap = 11;
        }
        do_swap = 0;
        for (typename LT::E *i = a; i < a + n - gap; ++i) {
            typename LT::E *j = i + gap;
            if (SEL_LT(*j, *i)) {
                LT::swap(i, j);
                do_swap = 1;
            }
        }
    } while (do_swap || gap > 2);
    if (gap != 1) sel_insertsort(a, a + n, LT());
}

// klib ks_introsort; stk = this thread's column of the LDS stack (frame f at stk[(3 f + k) * 64])
template <class LT>
__device__ __forceinline__ void sel_introsort(int n, typename LT::E *a, int *stk, LT)
{
    if (n < 2) return;
    if (n == 2) {
        if (SEL_LT(a[1], a[0])) LT::swap(a, a + 1);
        return;
    }
    int d, top = 0;
    for (d = 2; (1 << d) < n; ++d) ;
    int s = 0, t = n - 1, i, j, k;
    d <<= 1;
    while (true) {
        if (s < t) {
            if (--d == 0) {
                sel_combsort(t - s + 1, a + s, LT());
                t = s;
                continue;
            }
            i = s; j = t; k = i + ((j - i) >> 1) + 1;
            if (SEL_LT(a[k], a[i])) {
                if (SEL_LT(a[k], a[j])) k = j;
            } else {
                k = SEL_LT(a[j], a[i]) ? i : j;
            }
            const typename LT::K rp = LT::key(a[k]);
            if (k != t) LT::swap(a + k, a + t);
            for (;;) {
                do ++i; while (LT::lt(LT::key(a[i]), rp));
                do --j; while (i <= j && LT::lt(rp, LT::key(a[j])));
                if (j <= i) break;
                LT::swap(a + i, a + j);
            }
            LT::swap(a + i, a + t);
            int pl = -1, pr = -1;
            if (i - s > t - i) {
                if (i - s > 16) { pl = s; pr = i - 1; }
                s = t - i > 16 ? i + 1 : t;
            } else {
                if (t - i > 16) { pl = i + 1; pr = t; }
                t = i - s > 16 ? i - 1 : s;
            }
            if (pl >= 0 && top < kSelStack) {       // (a frame left out is sorted by the last insertion sort)
                stk[(3 * top) * 64] = pl; stk[(3 * top + 1) * 64] = pr; stk[(3 * top + 2) * 64] = d;
                ++top;
            }
        } else {
            if (top == 0) {
                sel_insertsort(a, a + n, LT());
                return;
            }
            --top;
            s = stk[(3 * top) * 64]; t = stk[(3 * top + 1) * 64]; d = stk[(3 * top + 2) * 64];
        }
    }
}

__device__ __forceinline__ uint64_t hash_64(uint64_t key)
{
    key += ~(key << 32);
    key ^= (key >> 22);
    key += ~(key << 13);
    key ^= (key >> 8);
    key += (key << 3);
    key ^= (key >> 15);
    key += ~(key << 27);
    key ^= (key >> 31);
    return key;
}

__device__ __forceinline__ int sel_mapq(const SelParams &p, const SelW &x, float frac_rep)
{
    if (x.secondary >= 0) return 0;
    const int score = x.r.score;
    int sub = x.sub ? x.sub : p.min_seed_len * p.a;
    sub = max(sub, x.csub);
    if (sub >= score) return 0;
    const int l = max(x.r.qe - x.r.qb, (int)(x.r.re - x.r.rb));
    const double identity = 1. - (double)(l * p.a - score) / (p.a + p.b) / l;
    int mapq;
    if (score == 0) {
        mapq = 0;
    } else if (p.mapQ_coef_len > 0) {
        double tmp = l < p.mapQ_coef_len ? 1. : p.mapQ_coef_fac / log((double)l);
        tmp *= identity * identity;
        mapq = (int)(6.02 * (score - sub) / p.a * tmp * tmp + .499);
    } else {
        mapq = (int)(30.0 * (1. - (double)sub / score) * log((double)x.seedcov) + .499);
        if (identity < 0.95) mapq = (int)(mapq * identity * identity + .499);
    }
    if (x.sub_n > 0) mapq -= (int)(4.343 * log((double)(x.sub_n + 1)) + .499);
    mapq = min(mapq, 60);
    mapq = max(mapq, 0);
    return (int)(mapq * (1. - frac_rep) + .499);
}

// PRIMARY MARKING and MAPQ of read r's list W[0, n), n >= 1, as it stands: the hash over the
// current positions, the hash sort, the z loop (Z: n words of the read's own), then every MAPQ.
__device__ __forceinline__ void sel_mark_mapq(const SelParams &p, int r, SelW *W, int n, int *stk, int32_t *Z,
                                              float frac_rep)
{
    for (int k = 0; k < n; ++k) {
        W[k].sub = 0;
        W[k].secondary = -1;
        W[k].hash = hash_64((uint64_t)p.id0 + (uint64_t)(int64_t)r + (uint64_t)k);
    }
    sel_introsort(n, W, stk, LtScoreHash());
    if (n > 1) {
        const int tmp = max(max(p.a + p.b, p.o_del + p.e_del), p.o_ins + p.e_ins);
        int nz = 1;
        Z[0] = 0;
        for (int i = 1; i < n; ++i) {
            const int iqb = W[i].r.qb, iqe = W[i].r.qe, isc = W[i].r.score;
            int k = 0;
            for (; k < nz; ++k) {
                const int j = Z[k];
                const int jqb = W[j].r.qb, jqe = W[j].r.qe;
                const int b_max = max(jqb, iqb), e_min = min(jqe, iqe);
                if (e_min > b_max) {
                    const int min_l = min(iqe - iqb, jqe - jqb);
                    if ((float)(e_min - b_max) >= (float)min_l * p.mask_level) {
                        if (W[j].sub == 0) W[j].sub = isc;
                        if (W[j].r.score - isc <= tmp) ++W[j].sub_n;
                        break;
                    }
                }
            }
            if (k < nz) W[i].secondary = Z[k];
            else Z[nz++] = i;
        }
    }
    for (int k = 0; k < n; ++k) W[k].mapq = sel_mapq(p, W[k], frac_rep);
}

// The i / j loop of read r from (i, j); have: score answers the patch_reg it was suspended at (a
// global score may be negative, so the score itself cannot say so).  Returns true when it
// suspends again (st[r] holds where; lq / rl its job's spans).
// mem_sort_dedup_patch's rid tests: two regions are compared (and patched) only on one contig
__device__ __forceinline__ bool sel_same_rid(const SelParams &p, const SelW &x, const SelW &y)
{
    return !p.ctg.off || contig_rid(p.ctg, x.r.rb) == contig_rid(p.ctg, y.r.rb);
}

__device__ __forceinline__ bool sel_dedup(const SelParams &p, int r, SelW *W, int n, int i, int j, int w, bool have,
                                          int score,
                          const uint8_t *__restrict__ q_codes, const uint8_t *__restrict__ ref, const int8_t *s_mat,
                          SelRd *st, int32_t *meta, int &lq_out, int &rl_out)
{
    for (; i < n; ++i, j = -2) {
        if (j == -2) {
            if (!sel_same_rid(p, W[i], W[i - 1]) || W[i].r.rb >= W[i - 1].r.re + p.max_chain_gap) continue;
            j = i - 1;
        }
        for (; j >= 0 && sel_same_rid(p, W[i], W[j]) && W[i].r.rb < W[j].r.re + p.max_chain_gap; --j) {
            const bsw_alnreg_t P = W[i].r, Q = W[j].r;
            if (!have) {
                if (Q.qe == Q.qb) continue;
                const int64_t orr = Q.re - P.rb;
                const int oq = Q.qb < P.qb ? Q.qe - P.qb : P.qe - Q.qb;
                const int64_t mr = min(Q.re - Q.rb, P.re - P.rb);
                const int mq = min(Q.qe - Q.qb, P.qe - P.qb);
                if ((float)orr > p.mask_level_redun * (float)mr && (float)oq > p.mask_level_redun * (float)mq) {
                    atomicAdd(&meta[kSelRedundant], 1);
                    if (P.score < Q.score) {
                        W[i].r.qe = P.qb;
                        break;
                    }
                    W[j].r.qe = Q.qb;
                    continue;
                }
                if (!(Q.rb < P.rb)) continue;
                // patch_reg(a = Q, b = P)
                if (p.patch == 0) continue;
                if (Q.rb < p.l_pac && P.rb >= p.l_pac) continue;
                if (Q.qb >= P.qb || Q.qe >= P.qe || Q.re >= P.re) continue;
                int64_t w64 = (Q.re - P.rb) - (int64_t)(Q.qe - P.qb);
                w64 = w64 > 0 ? w64 : -w64;
                const double rr = fabs((double)(Q.re - P.rb) / (double)(P.re - Q.rb) -
                                       (double)(Q.qe - P.qb) / (double)(P.qe - Q.qb));
                if (Q.re < P.rb || Q.qe < P.qb) {
                    if (w64 > (int64_t)(p.W << 1) || rr >= 0.05) continue;
                } else {
                    if (w64 > (int64_t)(p.W << 2) || rr >= 0.10) continue;
                }
                w = (int)min(w64 + Q.w + P.w, (int64_t)(p.W << 2));
                atomicAdd(&meta[kSelTried], 1);
                const int64_t lq = (int64_t)P.qe - Q.qb, rl = P.re - Q.rb;
                if (lq > BSW_MAX_LEN || rl > BSW_MAX_LEN) {
                    atomicOr(&meta[kSelErr], 1);
                    continue;
                }
                if (lq <= 0 || rl <= 0 ||
                    (p.ctg.off ? contig_crosses(p.ctg, Q.rb, P.re) : (p.l_pac > 0 && Q.rb < p.l_pac && P.re > p.l_pac))) {
                    score = 0;                              // gen_cigar2 rejects the span
                } else if (lq == rl && w == 0) {
                    score = 0;                              // gen_cigar2's gap-free shortcut
                    for (int c = 0; c < (int)lq; ++c)
                        score += s_mat[min((int)ref[Q.rb + c], 4) * 5 + min((int)q_codes[Q.qb + c], 4)];
                } else {
                    SelRd s;
                    s.n = n; s.i = i; s.j = j; s.w = w;
                    st[r] = s;
                    lq_out = (int)lq; rl_out = (int)rl;
                    return true;
                }
            }
            // the rest of patch_reg, then its caller
            const int sum = P.score + Q.score;
            const int q_s = (int)((double)(P.qe - Q.qb) / ((P.qe - P.qb) + (Q.qe - Q.qb)) * sum + .499);
            const int r_s = (int)((double)(P.re - Q.rb) / (double)((P.re - P.rb) + (Q.re - Q.rb)) * sum + .499);
            const int sc = score;
            have = false;
            if ((double)sc / max(q_s, r_s) < 0.90) {
                atomicAdd(&meta[kSelRatio], 1);
                continue;
            }
            if (sc <= 0) continue;
            atomicAdd(&meta[kSelOk], 1);
            const int ync = W[j].n_comp, ycov = W[j].seedcov, ysub = W[j].sub, ycsub = W[j].csub;
            W[i].n_comp += ync + 1;
            W[i].seedcov = max(W[i].seedcov, ycov);
            W[i].sub = max(W[i].sub, ysub);
            W[i].csub = max(W[i].csub, ycsub);
            W[i].r.qb = Q.qb; W[i].r.rb = Q.rb;
            W[i].r.truesc = W[i].r.score = sc;
            W[i].r.w = w;
            W[j].r.qb = Q.qe;
        }
    }
    return false;
}

// Steps 4..7 of DEDUP AND PATCH on a list whose i / j loop has ended: the drops, the score sort, the
// identical-hit rule; returns the number kept.
__device__ __forceinline__ int sel_dedup_drop(SelW *W, int n, int *stk, int32_t *meta)
{
    int m = 0;
    for (int k = 0; k < n; ++k)
        if (W[k].r.qe > W[k].r.qb) {
            if (m != k) sel_copy(W + m, W + k);
            ++m;
        }
    n = m;
    sel_introsort(n, W, stk, LtScorePos());
    int ident = 0;
    for (int k = 1; k < n; ++k)
        if (W[k].r.score == W[k - 1].r.score && W[k].r.rb == W[k - 1].r.rb && W[k].r.qb == W[k - 1].r.qb) {
            W[k].r.qe = W[k].r.qb;
            ++ident;
        }
    if (ident) {
        atomicAdd(&meta[kSelIdentical], ident);
        m = 1;
        for (int k = 1; k < n; ++k)
            if (W[k].r.qe > W[k].r.qb) {
                if (m != k) sel_copy(W + m, W + k);
                ++m;
            }
        n = m;
    }
    return n;
}

}  // namespace bsw
