/*
 * bsw_sel.h -- region selection on the GPU: the three per-read steps upstream runs between
 * mem_chain2aln and mem_reg2aln -- mem_sort_dedup_patch, mem_mark_primary_se and
 * mem_approx_mapq_se (lh3/bwa bwamem.c, kept unchanged by bwa-mem2; [UPSTREAM-RECALL]: the
 * reference tree holds no source of them).  This text is the specification; tests/regsel_py.py
 * pins it.  All arithmetic is C's: where a float option meets an integer, the product and the
 * comparison are in single precision; `double` casts are written out.
 *
 * INPUT.  Per read, av = the regions of its extended seeds (extended[k] != 0) in upstream's
 * processing order: chains in seed_chain order, within a chain by (len * a descending, seed
 * index descending) -- the order bsw_chain2aln* extends them in.  An extended region with
 * qe == qb is treated as already excluded: it is not part of av.  Each entry also carries
 *   seedcov = the sum of len over ALL seeds of the region's chain (skipped ones included) with
 *             qbeg >= qb, qbeg + len <= qe, rbeg >= rb and rbeg + len <= re
 *   sub = 0, sub_n = 0, n_comp = 1, secondary = -1, src = its seed slot k
 *   csub = csub[k] (NULL: 0), frac_rep = frac_rep[read] (NULL: 0)
 *
 * DEDUP AND PATCH (mem_sort_dedup_patch); skipped when the read has at most one region.
 *   1. ks_introsort (klib ksort.h; tie order is klib's) with lt(a, b) = a.re < b.re
 *   2. for i = 1 .. n-1, p = a[i]:
 *        skip i when p.rb >= a[i-1].re + max_chain_gap
 *        for j = i-1 downwards while j >= 0 and p.rb < a[j].re + max_chain_gap, q = a[j]:
 *          skip q when q.qe == q.qb
 *          or = q.re - p.rb;  oq = q.qb < p.qb ? q.qe - p.qb : p.qe - q.qb
 *          mr = min(q.re - q.rb, p.re - p.rb);  mq = min(q.qe - q.qb, p.qe - p.qb)
 *          if or > mask_level_redun * mr && oq > mask_level_redun * mq:       (REDUNDANT)
 *              if p.score < q.score: p.qe = p.qb, break;  else q.qe = q.qb
 *          else if q.rb < p.rb and (score = patch_reg(q, p, &w)) > 0:         (PATCH)
 *              p.n_comp += q.n_comp + 1; p.seedcov, p.sub, p.csub = max of the two;
 *              p.qb = q.qb; p.rb = q.rb; p.truesc = p.score = score; p.w = w; q.qb = q.qe
 *   3. patch_reg(a, b, &w), a.rb <= b.rb  (upstream's mem_patch_reg):
 *        0 when opt->patch == 0
 *        0 when a.rb < l_pac && b.rb >= l_pac                                  (strands)
 *        0 when a.qb >= b.qb || a.qe >= b.qe || a.re >= b.re                   (not colinear)
 *        w = |(a.re - b.rb) - (a.qe - b.qb)|
 *        r = |(double)(a.re - b.rb) / (b.re - a.rb) - (double)(a.qe - b.qb) / (b.qe - a.qb)|
 *        if a.re < b.rb || a.qe < b.qb:  0 when w > W << 1 || r >= 0.05
 *        else:                           0 when w > W << 2 || r >= 0.10
 *        w += a.w + b.w;  w = min(w, W << 2)
 *        score = the score of gen_cigar2(w_ = w, query = read[a.qb, b.qe), rb = a.rb, re = b.re)
 *                exactly as bsw_aln.h defines it (reversal for rb >= l_pac, bsw_gen_cigar_band,
 *                the gap-free shortcut when the spans are equal and w_ == 0; a rejected span
 *                scores 0)
 *        q_s = (int)((double)(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * (b.score + a.score) + .499)
 *        r_s = (int)((double)(b.re - a.rb) / ((b.re - b.rb) + (a.re - a.rb)) * (b.score + a.score) + .499)
 *        0 when (double)score / max(q_s, r_s) < 0.90;  else score (and w)
 *   4. drop the regions with qe <= qb, keeping order
 *   5. ks_introsort with lt = (score descending, then rb ascending, then qb ascending)
 *   6. for i >= 1: a[i] with score, rb and qb equal to a[i-1]'s gets qe = qb     (IDENTICAL)
 *   7. drop those among i >= 1
 *
 * PRIMARY MARKING (mem_mark_primary_se; one reference, no ALT contigs: is_alt = 0).
 *   1. region i of read r: sub = 0, secondary = -1, hash = hash_64(id0 + r + i); sub_n is NOT
 *      reset.  hash_64 is bwa's, in 64-bit wrapping arithmetic:
 *        key += ~(key << 32); key ^= key >> 22; key += ~(key << 13); key ^= key >> 8;
 *        key += key << 3; key ^= key >> 15; key += ~(key << 27); key ^= key >> 31
 *   2. ks_introsort with lt = (score descending, hash ascending)
 *   3. tmp = max(a + b, o_del + e_del, o_ins + e_ins); z = [0]
 *   4. for i = 1 .. n-1: the first j in z with b_max = max(a[j].qb, a[i].qb), e_min =
 *      min(a[j].qe, a[i].qe), e_min > b_max and, min_l = the shorter query span of the two,
 *      e_min - b_max >= min_l * mask_level:
 *          if a[j].sub == 0: a[j].sub = a[i].score
 *          if a[j].score - a[i].score <= tmp: ++a[j].sub_n
 *          a[i].secondary = j
 *      no such j: push i onto z
 *
 * MAPQ (mem_approx_mapq_se); 0 for a region with secondary >= 0, as in mem_reg2aln.  Primaries:
 *   sub_ = sub ? sub : min_seed_len * a;  sub_ = max(sub_, csub);  0 when sub_ >= score
 *   l = max(qe - qb, re - rb);  identity = 1. - (double)(l * a - score) / (a + b) / l
 *   0 when score == 0
 *   mapQ_coef_len > 0:   t = l < mapQ_coef_len ? 1. : mapQ_coef_fac / log(l);  t *= identity * identity
 *                        mapq = (int)(6.02 * (score - sub_) / a * t * t + .499)
 *   mapQ_coef_len == 0:  mapq = (int)(30.0 * (1. - (double)sub_ / score) * log(seedcov) + .499)
 *                        identity < 0.95:  mapq = (int)(mapq * identity * identity + .499)
 *   sub_n > 0:  mapq -= (int)(4.343 * log(sub_n + 1) + .499)
 *   clamp to [0, 60];  mapq = (int)(mapq * (1. - frac_rep) + .499)
 * mapQ_coef_fac is an int upstream: log(50) truncates to 3, the default here.  The device
 * computes MAPQ in double precision.
 *
 * Scope: no ALT contigs; with no contig table ONE reference sequence, with one (bsw_set_contigs,
 * bsw_contigs.h; it has to sum to opt->l_pac) dedup and patch keep to one contig: the outer skip also
 * moves on when p and a[i - 1] lie on different contigs, the inner loop runs only while p and a[j]
 * lie on one, so no region is dropped for, or patched with, one of another contig.  a, b aside,
 * scoring comes from the context's parameters (a = mat[0], the gap penalties); b is an option because
 * the matrix does not name it.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_SEL_API.
 */
#ifndef BSW_SEL_H
#define BSW_SEL_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_SEL_API 1

#define BSW_SEL_MAX_PER_READ (1 << 20)   /* regions of one read (more: BSW_E_RANGE)              */

typedef struct bsw_sel_opt_t {
    int32_t w;                       /* band width (bwa -w, 100)                                 */
    int32_t max_chain_gap;           /* 10000                                                    */
    int64_t l_pac;                   /* as bsw_ext_opt_t: 0 = one-strand reference               */
    float   mask_level_redun;        /* 0.95                                                     */
    float   mask_level;              /* 0.5                                                      */
    int32_t min_seed_len;            /* 19                                                       */
    int32_t b;                       /* mismatch penalty (bwa -B, 4)                             */
    int32_t mapQ_coef_len;           /* 50                                                       */
    int32_t mapQ_coef_fac;           /* 3 = (int)log(50): an int upstream                        */
    int32_t patch;                   /* 1; 0: patch_reg always returns 0 (mem_matesw's call form) */
    int32_t reserved;
    int64_t id0;                     /* hash seed: upstream's index of the batch's first read    */
} bsw_sel_opt_t;

void bsw_sel_opt_default(bsw_sel_opt_t *opt);

typedef struct bsw_selinfo_t {       /* one per kept region                                      */
    int32_t seedcov;
    int32_t sub;
    int32_t csub;
    int32_t sub_n;
    int32_t n_comp;
    int32_t secondary;               /* -1, or an index within the read's list                   */
    int32_t mapq;
    int32_t src;                     /* seed slot of the region p it descends from               */
    float   frac_rep;
} bsw_selinfo_t;

/* Every array in HBM of the context's first device, against the resident reference
 * (bsw_set_reference; BSW_E_INVAL without one).  The inputs are exactly what
 * bsw_chain2aln_resident takes and leaves (d_regs = its d_out); d_csub (int32 per seed slot) and
 * d_frac_rep (float per read) may be NULL.  Outputs: the kept regions grouped by read, within a
 * read in the order after the hash sort -- d_sel_regs / d_sel_read (never decreasing) are exactly
 * the d_regs / d_reg_read bsw_reg2aln_resident takes; d_sel_info[k]; d_read_first[n_reads + 1]
 * each read's offset.  *n_sel = the number kept.  sel_cap < needed: BSW_E_RANGE with *n_sel = the
 * number needed (d_read_first is still written); sel_cap = n_seeds always suffices.
 * BSW_E_RANGE also for: an av region with [qb, qe) outside its read, rb < 0, rb > re or re past
 * the resident text; a read index outside [0, n_reads) or d_seed_read unsorted; a patch span
 * (b.qe - a.qb or b.re - a.rb) above BSW_MAX_LEN; more than BSW_SEL_MAX_PER_READ regions of one
 * read.  The dedup loop, the sorts, primary marking and MAPQ run on the GPU (csrc/bsw_sel.hip)
 * around the batched score-only ksw_global2 of the patch candidates; the host reads back one job
 * count per patch round.  `stream`: a hipStream_t or NULL.  Returns when the outputs are in HBM. */
int bsw_regs_select_resident(bsw_ctx_t *ctx, const bsw_sel_opt_t *opt, const uint8_t *d_reads,
                             const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                             const bsw_seed_t *d_seeds, const int32_t *d_seed_read, const int32_t *d_seed_chain,
                             const bsw_alnreg_t *d_regs, const int32_t *d_extended, int32_t n_seeds,
                             const int32_t *d_csub, const float *d_frac_rep, bsw_alnreg_t *d_sel_regs,
                             int32_t *d_sel_read, bsw_selinfo_t *d_sel_info, int32_t *d_read_first,
                             int32_t sel_cap, int32_t *n_sel, void *stream);

/* The same with host arrays: uploads them, runs the resident form, downloads.  Blocking. */
int bsw_regs_select(bsw_ctx_t *ctx, const bsw_sel_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                    const int32_t *read_len, int32_t n_reads, const bsw_seed_t *seeds, const int32_t *seed_read,
                    const int32_t *seed_chain, const bsw_alnreg_t *regs, const int32_t *extended, int32_t n_seeds,
                    const int32_t *csub, const float *frac_rep, bsw_alnreg_t *sel_regs, int32_t *sel_read,
                    bsw_selinfo_t *sel_info, int32_t *read_first, int32_t sel_cap, int32_t *n_sel);

typedef struct bsw_sel_stats_t {
    int32_t n_reads;
    int32_t n_regs_in;               /* av entries over all reads                                */
    int32_t n_redundant;             /* dropped by the redundancy rule (p or q)                  */
    int32_t n_identical;             /* dropped by the identical-hit rule                        */
    int32_t n_patch_tried;           /* patch_reg calls that reached the score                   */
    int32_t n_patch_ok;
    int32_t n_patch_ratio;           /* refused by the 0.90 ratio                                */
    int32_t n_dp;                    /* of the tried: scored by ksw_global2 (the others gap-free
                                        or rejected spans)                                       */
    int32_t rounds;                  /* DP rounds                                                */
    int32_t n_sel;
    float   dp_ms;                   /* ksw_global2 kernels (HIP events)                         */
    float   helper_ms;               /* every other kernel of the stage (HIP events)             */
} bsw_sel_stats_t;
int bsw_sel_last_stats(bsw_ctx_t *ctx, bsw_sel_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_SEL_H */
