// bsw_formulas.h -- upstream's integer formulas over plain integers, each stated once for the host
// builder (bsw_ext.cpp, plain g++) and for every stage kernel.  The (double) casts and the + 1. /
// + 2. terms are upstream's: outputs are compared bit for bit (tests/test_formulas.py pins these).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BSW_HD __host__ __device__ inline
#else
#define BSW_HD inline
#endif

namespace bsw {

BSW_HD int f_max(int x, int y) { return x > y ? x : y; }
BSW_HD int f_min(int x, int y) { return x < y ? x : y; }
BSW_HD int f_abs(int x) { return x < 0 ? -x : x; }

// mem_chain2aln's cal_max_gap (include/bsw_ext.h): the longest gap a stretch of qlen bases pays for
BSW_HD int cal_max_gap(int a, int o_del, int e_del, int o_ins, int e_ins, int w, int qlen)
{
    const int l_del = (int)((double)(qlen * a - o_del) / e_del + 1.);
    const int l_ins = (int)((double)(qlen * a - o_ins) / e_ins + 1.);
    int l = f_max(l_del, l_ins);
    l = f_max(l, 1);
    return f_min(l, w << 1);
}

// bwa_gen_cigar2's band for ksw_global2: the published bsw_gen_cigar_band (include/bsw_global.h)
BSW_HD int cigar_band(int a, int o_del, int e_del, int o_ins, int e_ins, int lq, int rlen, int w_)
{
    const int max_ins = (int)((double)(((lq + 1) >> 1) * a - o_ins) / e_ins + 1.);
    const int max_del = (int)((double)(((lq + 1) >> 1) * a - o_del) / e_del + 1.);
    const int max_gap = f_max(f_max(max_ins, max_del), 1);
    const int d = f_abs(rlen - lq);
    const int w = f_min((max_gap + d + 1) >> 1, w_);
    return f_max(w, d + 3);
}

// mem_reg2aln's infer_bw (include/bsw_aln.h): q, r = one gap kind's open and extend penalties
BSW_HD int infer_bw(int l1, int l2, int score, int a, int q, int r)
{
    if (l1 == l2 && l1 * a - score < (q + r - a) * 2) return 0;
    const int w = (int)((double)(f_min(l1, l2) * a - score - q) / r + 2.);
    return f_max(w, f_abs(l1 - l2));
}

// mem_infer_dir (include/bsw_pe.h): orientation (0 FF, 1 FR, 2 RF, 3 RR) and distance of hits at b1, b2
BSW_HD int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t &dist)
{
    const bool r1 = b1 >= l_pac, r2 = b2 >= l_pac;
    const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

}  // namespace bsw
