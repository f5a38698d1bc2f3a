// bsw_sel_dev.h -- device code shared by region selection (bsw_sel.hip) and the paired-end stage
// (bsw_pe.hip): a region's moves as 16-byte words, klib's ks_introsort with its explicit stack in
// LDS, bwa's hash_64, primary marking and MAPQ as include/bsw_sel.h states them.  Plain C++ with
// vector stores only; no private arrays.
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

}  // namespace bsw
