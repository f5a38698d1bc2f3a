/*
 * bsw_pe.h -- the paired-end stage on the GPU: insert-size statistics (mem_pestat), pairing
 * (mem_pair) and the decision block of mem_sam_pe as upstream runs them with rescue disabled
 * (MEM_F_NO_RESCUE, `bwa mem -S`); lh3/bwa bwamem_pair.c, kept unchanged by bwa-mem2
 * [UPSTREAM-RECALL]: the reference tree holds no source of them.  This text is the specification;
 * tests/pe_py.py pins it.  All arithmetic is C's: `int` truncation, `double` where written, a
 * float option times an integer in single precision.  Reads 2p and 2p + 1 are the two ends of
 * pair p; "list" = a read's regions as bsw_regs_select* left them (bsw_sel.h), a[0] its first.
 * With no contig table one reference sequence (rid = 0); no ALT (n_pri = n).  With a table
 * (bsw_set_contigs, bsw_contigs.h; it has to sum to opt->l_pac, BSW_E_INVAL otherwise) the rid of a
 * region is that of its rb, and hits on different contigs are never a pair: bsw_pe_stat* takes no
 * insert size from a pair whose two top regions differ in rid; mem_pair's v is sorted by upstream's
 * rid << 32 | forward position - offset, which is the order of the global forward position, and its
 * distance scan ends at a rid change; no_pairing's proper flag also needs equal rids.  Coordinates
 * stay global.  a = mat[0] and the gap penalties come from
 * the context, as in bsw_sel.h.  Mate rescue (mem_matesw) is bsw_matesw.h's: it consumes pes[] and
 * slots between the two calls below without changing them.
 *
 * infer_dir(b1, b2) -> (dir, dist):  r1 = b1 >= l_pac;  r2 = b2 >= l_pac
 *   p2 = r1 == r2 ? b2 : 2 * l_pac - 1 - b2;  dist = |p2 - b1|
 *   dir = (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3)                    (0 FF, 1 FR, 2 RF, 3 RR)
 *
 * cal_sub(list): the first j >= 1 with b_max = max(a[j].qb, a[0].qb), e_min = min(a[j].qe,
 *   a[0].qe), e_min > b_max and e_min - b_max >= min_l * mask_level (min_l = the shorter query span
 *   of the two; a float product) gives a[j].score; no such j: min_seed_len * a
 *
 * STATISTICS (mem_pestat).  Per pair: skipped when either list is empty or, for either end,
 *   cal_sub(list) > 0.8 * a[0].score (double);  (dir, is) = infer_dir(a0[0].rb, a1[0].rb);  `is`
 *   is kept under dir when is != 0 && is <= max_ins.  Per direction, q = its n kept values ascending:
 *     n < 10: failed = 1, every other field 0 (n is still reported)
 *     p25, p50, p75 = q[(int)(.25 * n + .499)], .50, .75, as int
 *     low = (int)(p25 - 2.0 * (p75 - p25) + .499), low = max(low, 1)
 *     high = (int)(p75 + 2.0 * (p75 - p25) + .499)
 *     avg = the mean of the x values in [low, high];  std = sqrt(sum((q - avg)^2) / x) over them
 *     low = (int)(p25 - 3.0 * (p75 - p25) + .499);  high = (int)(p75 + 3.0 * (p75 - p25) + .499)
 *     low > avg - 4.0 * std:  low = (int)(avg - 4.0 * std + .499)
 *     high < avg + 4.0 * std: high = (int)(avg + 4.0 * std + .499)
 *     low = max(low, 1)
 *   then, max = the largest n of the four: failed == 0 && n < max * 0.05 (double) gets failed = 1
 *   (its other fields stay).  The device counts `is` per direction in max_ins + 1 bins (is <=
 *   max_ins, so the counts replace upstream's sort exactly); the host derives the rest in double.
 *
 * PAIR CALL, step 1 (mem_sam_pe's second mem_mark_primary_se, seed id << 1 | end = id0 + read
 *   index for an even id0): bsw_sel.h's PRIMARY MARKING on every read's list as it stands --
 *   hash_64(id0 + r + i) over the current positions, sub and secondary reset, sub_n NOT reset (it
 *   accumulates, as upstream's does), the hash sort reorders the list -- then info.mapq again by
 *   bsw_sel.h's MAPQ rule.
 *
 * step 2 (mem_pair), when both lists are non-empty.  v: for end r, region i
 *     x = rb < l_pac ? rb : 2 * l_pac - 1 - rb
 *     y = (uint64)score << 32 | i << 2 | (rb >= l_pac) << 1 | r
 *   sorted by (x, y) ascending (the keys are distinct).  last[4] = -1.  For i over v, r in {0, 1}:
 *     dir = r << 1 | (y_i >> 1 & 1): skipped when pes[dir].failed
 *     which = r << 1 | ((y_i & 1) ^ 1): skipped when last[which] < 0
 *     for k = last[which] down to 0:  skip k when (y_k & 3) != which;  dist = x_i - x_k
 *       break when dist > high;  skip when dist < low;  ns = (dist - avg) / std
 *       q = (int)((y_i >> 32) + (y_k >> 32) + .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * a + .499)
 *       q = max(q, 0);  push to u:  y = (uint64)k << 32 | i,
 *         x = (uint64)q << 32 | (hash_64(y ^ (uint64)(int64)t) & 0xffffffff)
 *         with id32 = (int32)((id0 >> 1) + p), t = (int32)((uint32)id32 << 8)
 *   and after both r: last[y_i & 3] = i.  u empty: mem_pair returns 0.  Else, by (x, y): the
 *   largest entry's two v entries give z[y_v & 1] = (uint32)y_v >> 2 and o = its q; sub = the second
 *   largest's q (0 when u.n == 1); tmp = max(a + b, o_del + e_del, o_ins + e_ins); n_sub = the
 *   number of entries other than the largest with sub - q <= tmp.  u is never materialised.
 *
 * step 3 (mem_sam_pe).  raw(d) = (int)(6.02 * d / a + .499).  Both lists non-empty and o > 0:
 *     is_multi[e]: some j >= 1 has secondary < 0 && score >= T;  either end multi: no_pairing
 *     score_un = a0[0].score + a1[0].score - pen_unpaired;  subo = max(sub, score_un)
 *     q_pe = raw(o - subo);  n_sub > 0: q_pe -= (int)(4.343 * log(n_sub + 1) + .499)
 *     q_pe clamped to [0, 60];  q_pe = (int)(q_pe * (1. - .5 * (frac_rep0 + frac_rep1)) + .499)
 *       (the frac_rep of each end's a[0]; their sum in single precision)
 *     o > score_un: for each end c = list[z[e]]:
 *         c.secondary >= 0: c.sub = list[c.secondary].score, c.secondary = -2 (both to d_sel_info)
 *         q_se = MAPQ rule(c), which does not look at secondary
 *         q_se = q_se > q_pe ? q_se : min(q_pe, q_se + 40);  q_se = min(q_se, raw(c.score - c.csub))
 *       proper = 1
 *     else: z = {0, 0}, q_se = the MAPQ rule of each end's a[0], proper = 0
 *     paired = 1, mapq[e] = q_se
 *   no_pairing (paired = 0), per end: which = 0 when the list is non-empty and a[0].score >= T,
 *     else -1;  z = which;  mapq = info.mapq[which], 0 for -1;  proper = 1 when both which >= 0 and
 *     (dir, dist) = infer_dir(a0[0].rb, a1[0].rb) has !pes[dir].failed && low <= dist <= high
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_PE_API.
 */
#ifndef BSW_PE_H
#define BSW_PE_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_ext.h"
#include "bsw_sel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_PE_API 1

#define BSW_PE_MAX_INS (1 << 16)          /* opt->max_ins above it: BSW_E_INVAL                  */

typedef struct bsw_pestat_t {             /* upstream mem_pestat_t + the candidate count; index d: 0 FF, 1 FR, 2 RF, 3 RR */
    int32_t low, high, failed, n;
    double  avg, std;
} bsw_pestat_t;

typedef struct bsw_pe_opt_t {
    int64_t l_pac;                        /* > 0: the resident text is forward + reverse complement (BSW_E_INVAL otherwise) */
    int64_t id0;                          /* upstream's index of the batch's first read; even (BSW_E_INVAL otherwise) */
    int32_t max_ins;                      /* 10000 */
    int32_t min_seed_len;                 /* 19 */
    int32_t b;                            /* 4 */
    int32_t T;                            /* 30: minimum score to output */
    int32_t pen_unpaired;                 /* 17 */
    int32_t mapQ_coef_len, mapQ_coef_fac; /* 50, 3 */
    float   mask_level;                   /* 0.5 */
} bsw_pe_opt_t;

typedef struct bsw_pair_t {               /* one per pair p = reads 2p, 2p+1 */
    int32_t paired;                       /* 1: mem_sam_pe's paired branch; 0: its no_pairing branch */
    int32_t z[2];                         /* chosen region of each end, an index within the read's list; -1: none */
    int32_t mapq[2];
    int32_t proper;                       /* SAM flag 0x2 */
    int32_t score, sub, n_sub, q_pe;      /* mem_pair's o, subo (before the score_un max), n_sub; q_pe. 0 when mem_pair was not run or returned 0 */
} bsw_pair_t;

void bsw_pe_opt_default(bsw_pe_opt_t *opt);

/* The arrays are what bsw_regs_select_resident leaves, in HBM of the context's first device:
 * d_sel_regs / d_sel_info [n_regs] and d_read_first[n_reads + 1] (read r's list is
 * [d_read_first[r], d_read_first[r + 1]), d_read_first[n_reads] <= n_regs); n_reads is even.
 * bsw_pe_stat* changes nothing in them and writes pes[4] to the host.  `stream`: a hipStream_t or
 * NULL.  Errors: BSW_E_INVAL for an odd or negative n_reads, l_pac <= 0 (or a resident reference
 * whose length is not 2 * l_pac), an odd id0, max_ins outside [1, BSW_PE_MAX_INS]; BSW_E_RANGE for
 * a decreasing d_read_first (or one outside [0, n_regs]), a list above BSW_SEL_MAX_PER_READ, a
 * region with rb outside [0, 2 * l_pac). */
int bsw_pe_stat_resident(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_alnreg_t *d_sel_regs,
                         const bsw_selinfo_t *d_sel_info, const int32_t *d_read_first, int32_t n_reads,
                         int32_t n_regs, bsw_pestat_t *pes, void *stream);
/* The same with host arrays (n_regs = read_first[n_reads]).  Blocking. */
int bsw_pe_stat(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_alnreg_t *sel_regs, const bsw_selinfo_t *sel_info,
                const int32_t *read_first, int32_t n_reads, bsw_pestat_t *pes);

/* Steps 1 to 3 for every pair under the caller's pes[4] (from bsw_pe_stat*, or its own as
 * `bwa mem -I` gives them).  d_sel_regs and d_sel_info are updated in place: a list is permuted
 * within its read (d_sel_read of bsw_regs_select* stays valid), sub / sub_n / secondary / mapq are
 * rewritten.  d_pairs[n_reads / 2] is written.  Returns when the outputs are in HBM.  Errors as
 * above, and BSW_E_INVAL for a direction with failed == 0 whose std is not finite or is <= 0
 * (upstream divides by it).  After an error the in-place arrays are unspecified. */
int bsw_pe_pair_resident(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_pestat_t *pes, bsw_alnreg_t *d_sel_regs,
                         bsw_selinfo_t *d_sel_info, const int32_t *d_read_first, int32_t n_reads, int32_t n_regs,
                         bsw_pair_t *d_pairs, void *stream);
/* The same with host arrays: uploads them, runs the resident form, downloads.  Blocking. */
int bsw_pe_pair(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_pestat_t *pes, bsw_alnreg_t *sel_regs,
                bsw_selinfo_t *sel_info, const int32_t *read_first, int32_t n_reads, bsw_pair_t *pairs);

typedef struct bsw_pe_stats_t {           /* of the last bsw_pe_stat* or bsw_pe_pair* call        */
    int32_t n_pairs;
    int32_t n_cand[4];                    /* stat call: kept insert sizes per direction           */
    int32_t n_pairing_tried;              /* pair call: mem_pair ran (both lists non-empty)       */
    int32_t n_paired;                     /*   paired = 1                                         */
    int32_t n_multi;                      /*   o > 0 but an end is multi: no_pairing              */
    int32_t n_unpaired_preferred;         /*   paired = 1 with o <= score_un                      */
    int32_t n_proper;
    int64_t n_u;                          /*   sum of u.n                                         */
    float   kernel_ms;                    /* the call's kernels (HIP events)                      */
    int32_t reserved;
} bsw_pe_stats_t;
int bsw_pe_last_stats(bsw_ctx_t *ctx, bsw_pe_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_PE_H */
