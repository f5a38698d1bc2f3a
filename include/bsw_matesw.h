/*
 * bsw_matesw.h -- mate rescue on the GPU: mem_matesw and the rescue block of mem_sam_pe (lh3/bwa
 * bwamem_pair.c, kept unchanged by bwa-mem2) [UPSTREAM-RECALL]: the reference tree holds no source
 * of them.  This text is the specification; tests/matesw_py.py pins it.  All arithmetic is C's.
 * The stage runs between bsw_pe_stat* (whose pes[4] it consumes) and bsw_pe_pair* (whose step 1 is
 * the primary marking upstream runs after rescue): regs_select -> pe_stat -> matesw -> pe_pair ->
 * reg2aln.  Scope as bsw_pe.h: no ALT; with no contig table ONE reference sequence (rid = 0), with
 * one (bsw_set_contigs, bsw_contigs.h; it has to sum to opt->l_pac) a window, after its clamp to [0, 2 l_pac),
 * is clipped to the segment of its midpoint (rb + re) >> 1 instead of to that midpoint's strand, and its job
 * exists only when that segment's contig is the anchor's and re - rb >= min_seed_len.  The resident text T =
 * forward + reverse complement, 2 * l_pac bases; reads 2p and 2p + 1 are pair p; a read's list is
 * a[e] as bsw_regs_select* left it (before bsw_pe_pair*'s step 1).  a = mat[0] and the gap penalties
 * come from the context.
 *
 * PER PAIR (the rescue block of mem_sam_pe).  For each end e the candidates are b[e] = copies, in
 *   list order, of the regions a[e][j] with score >= a[e][0].score - pen_unpaired.  The copies are
 *   taken BEFORE any rescue of this pair: a candidate that is later dropped or moved in a[e] is
 *   still used as copied.  The calls run in order: for e = 0, j = 0 .. min(|b[0]|, max_matesw) - 1:
 *   matesw(anchor = b[0][j], mate read = 2p + 1, ma = a[1]); then e = 1 likewise into ma = a[0].
 *   Each call sees ma as the earlier calls left it.
 *
 * matesw(anchor, mate read ms of length l_ms, ma):
 *   1. skip[r] = pes[r].failed ? 1 : 0.  For every m in ma as it stands, (r, dist) =
 *      infer_dir(anchor.rb, m.rb) (bsw_pe.h): pes[r].low <= dist <= pes[r].high sets skip[r] = 1.
 *      All four set: the call changes nothing.
 *   2. n = 0.  For r = 0 .. 3 in order, skipping skip[r]:
 *        is_rev = (r >> 1) != (r & 1);  is_larger = !(r >> 1)
 *        seq = ms, or its reverse complement when is_rev (c < 4 ? 3 - c : 4)
 *        !is_rev: rb = is_larger ? anchor.rb + low : anchor.rb - high
 *                 re = (is_larger ? anchor.rb + high : anchor.rb - low) + l_ms
 *        is_rev:  rb = (is_larger ? anchor.rb + low : anchor.rb - high) - l_ms
 *                 re = is_larger ? anchor.rb + high : anchor.rb - low
 *        rb = max(rb, 0);  re = min(re, 2 * l_pac)
 *        if rb < re (the bns_fetch_seq rule): mid = (rb + re) >> 1;
 *                 mid < l_pac ? re = min(re, l_pac) : rb = max(rb, l_pac)
 *        if rb < re and re - rb >= min_seed_len, a job runs:
 *          xtra = KSW_XSUBO | KSW_XSTART | (l_ms * a < 250 ? KSW_XBYTE : 0) | (min_seed_len * a)
 *          aln = ksw_align2(query = seq, target = T[rb, re), xtra), exactly as bsw_mate.h defines it
 *          ++n
 *          when aln.score >= min_seed_len (NOT times a, as upstream) and aln.qb >= 0, a region x is
 *          built from zeros:
 *            qb = is_rev ? l_ms - (aln.qe + 1) : aln.qb;   qe = is_rev ? l_ms - aln.qb : aln.qe + 1
 *            x.rb = is_rev ? 2 * l_pac - (rb + aln.te + 1) : rb + aln.tb
 *            x.re = is_rev ? 2 * l_pac - (rb + aln.tb) : rb + aln.te + 1
 *            score = aln.score, csub = aln.score2 (may be -1), secondary = -1
 *            seedcov = min(x.re - x.rb, qe - qb) >> 1
 *            every other field 0 (truesc, w, seedlen0, sub, sub_n, n_comp, mapq, frac_rep); src = -1
 *          x is inserted before the first ma[i] with ma[i].score < x.score (after equal scores), or
 *          at the end.
 *        after every non-skipped r, whether or not a job ran for it: n > 0: ma = DEDUP AND PATCH of
 *        bsw_sel.h with patch = 0 (the redundancy rule, both sorts, the identical rule; lists of at
 *        most one region are returned as they are).
 *      skip[] is NOT recomputed inside a call.
 *   3. A list for which no job ever ran is returned byte for byte.  A list a job ran for carries
 *      every region's bsw_selinfo_t fields along unchanged; its `secondary` indices are stale until
 *      bsw_pe_pair* re-marks.
 *
 * The calls of a pair depend on one another, so the device runs rounds: per round every unfinished
 * pair advances to its next call that has a job, the round's jobs run as one batch of the engine's
 * ksw_align2, the results are applied in order; the host reads back one job count per round.  The
 * number of ksw_align2 jobs executed is the specification's; a batch in which every pair already has
 * a consistent hit runs no DP kernel.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_MATESW_API.
 */
#ifndef BSW_MATESW_H
#define BSW_MATESW_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_ext.h"
#include "bsw_mate.h"
#include "bsw_sel.h"
#include "bsw_pe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_MATESW_API 1

typedef struct bsw_matesw_opt_t {
    int64_t l_pac;                        /* > 0: the resident text is forward + reverse complement */
    int32_t max_matesw;                   /* 50: candidates tried per end                         */
    int32_t pen_unpaired;                 /* 17 */
    int32_t min_seed_len;                 /* 19 */
    int32_t max_chain_gap;                /* 10000 (the dedup's) */
    float   mask_level_redun;             /* 0.95 (the dedup's) */
    int32_t reserved;
} bsw_matesw_opt_t;

void bsw_matesw_opt_default(bsw_matesw_opt_t *opt);

/* Every array in HBM of the context's first device, against the resident reference
 * (bsw_set_reference).  The inputs (const) are the reads as bsw_regs_select_resident took them and
 * d_sel_regs / d_sel_info [n_regs] / d_read_first[n_reads + 1] as it left them; pes[4] is on the
 * host (from bsw_pe_stat*, or the caller's own).  The outputs have the shape bsw_pe_stat/pair_resident
 * and bsw_reg2aln_resident take: the regions grouped by read, d_out_read never decreasing,
 * d_out_first[n_reads + 1]; *n_out = their number.  out_cap < needed: BSW_E_RANGE with *n_out = the
 * number needed (d_out_first is still written).  Internal working storage gives read r room for
 * len + 4 * min(|b[mate]|, max_matesw) regions, the exact upper bound.
 * BSW_E_INVAL: an odd or negative n_reads, l_pac <= 0, a resident text whose length is not
 * 2 * l_pac or none, max_matesw < 0, min_seed_len <= 0, a non-failed direction with low > high,
 * scoring bsw_ksw_align2 rejects (o_ins == 0 or max(mat) < 1).  BSW_E_RANGE: d_read_first
 * decreasing or outside [0, n_regs], a region with rb outside [0, 2 * l_pac), a job whose query
 * exceeds BSW_MATE_MAX_QLEN or whose window exceeds BSW_MAX_LEN.  After an error the outputs are
 * unspecified.  `stream`: a hipStream_t or NULL.  Returns when the outputs are in HBM. */
int bsw_matesw_resident(bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes,
                        const uint8_t *d_reads, const int64_t *d_read_off, const int32_t *d_read_len,
                        int32_t n_reads, const bsw_alnreg_t *d_sel_regs, const bsw_selinfo_t *d_sel_info,
                        const int32_t *d_read_first, int32_t n_regs, bsw_alnreg_t *d_out_regs,
                        int32_t *d_out_read, bsw_selinfo_t *d_out_info, int32_t *d_out_first, int32_t out_cap,
                        int32_t *n_out, void *stream);
/* The same with host arrays (n_regs = read_first[n_reads]).  Blocking. */
int bsw_matesw(bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes, const uint8_t *reads,
               const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *sel_regs,
               const bsw_selinfo_t *sel_info, const int32_t *read_first, bsw_alnreg_t *out_regs,
               int32_t *out_read, bsw_selinfo_t *out_info, int32_t *out_first, int32_t out_cap, int32_t *n_out);

typedef struct bsw_matesw_stats_t {       /* of the last bsw_matesw* call                          */
    int32_t n_pairs;
    int32_t n_calls;                      /* matesw calls (candidates tried)                       */
    int32_t n_calls_all_skipped;          /*   with all four directions skipped                    */
    int32_t n_jobs;                       /* ksw_align2 jobs                                       */
    int32_t n_jobs_u8;                    /*   with KSW_XBYTE                                      */
    int32_t n_short_window;               /* non-skipped directions whose window ran no job        */
    int32_t n_pushed;                     /* regions inserted                                      */
    int32_t n_redundant;                  /* dropped by the dedup's redundancy rule                */
    int32_t n_identical;                  /* dropped by its identical-hit rule                     */
    int32_t n_lists_changed;              /* lists at least one job ran for                        */
    int32_t rounds;                       /* rounds that ran jobs                                  */
    int32_t n_out;
    float   sw_ms;                        /* ksw_align2 kernels (HIP events)                       */
    float   helper_ms;                    /* every other kernel of the stage (HIP events)          */
} bsw_matesw_stats_t;
int bsw_matesw_last_stats(bsw_ctx_t *ctx, bsw_matesw_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_MATESW_H */
