/*
 * bsw_aln.h -- final alignments on the GPU: alignment regions (bsw_alnreg_t, bsw_ext.h) to
 * position, CIGAR, NM and MD.  The step upstream runs for every reported alignment,
 * mem_reg2aln -> bwa_gen_cigar2 (lh3/bwa bwamem.c / bwa.c, kept unchanged by bwa-mem2;
 * [UPSTREAM-RECALL]: the reference tree holds no source of them), restated:
 *
 *   infer_bw(l1, l2, score, a, q, r):
 *       if l1 == l2 and l1*a - score < ((q + r - a) << 1): return 0
 *       w = (int)((double)(min(l1,l2)*a - score - q) / r + 2.)
 *       return max(w, |l1 - l2|)
 *
 *   region (qb, qe, rb, re, truesc, w_reg) of a read of l_query bases; a = mat[0], W = opt->w:
 *   w2 = max(infer_bw(qe-qb, re-rb, truesc, a, o_del, e_del), infer_bw(.., a, o_ins, e_ins))
 *   if w2 > W: w2 = min(w2, w_reg)
 *   i = 0; last_sc = -(1<<30)
 *   do {
 *       w2 = min(w2, W << 2)
 *       (score, cigar, NM, MD) = gen_cigar2(w_ = w2, query = read[qb, qe), rb, re)
 *       if score == last_sc or w2 == W << 2: break
 *       last_sc = score; w2 <<= 1
 *   } while (++i < 3 and score < truesc - a)          -- at most 3 passes, the last one is kept
 *
 *   gen_cigar2(w_, query (lq bases), rb, re):
 *       rejected if lq <= 0 or rb >= re or (rb < l_pac and re > l_pac)
 *       rseq = T[rb, re); if rb >= l_pac: reverse (not complement) both query and rseq, so that
 *       indels come out left-aligned on the forward strand
 *       if lq == re - rb and w_ == 0: cigar = [lq M], score = sum mat[rseq[i]*5 + query[i]]  (no DP)
 *       else ksw_global2 (bsw_global.h) with w = bsw_gen_cigar_band(lq, re-rb, w_, ...)
 *       NM / MD: walk the CIGAR with x (query), y (rseq) and a match run u --
 *         M: a column with query[x+i] != rseq[y+i] emits u, then the base letter of rseq[y+i],
 *            ++n_mm, u = 0; an equal column does ++u
 *         D: only when it is neither the first nor the last op: emits u, '^', its len base
 *            letters, u = 0, n_gap += len; y += len always
 *         I: x += len, n_gap += len
 *         finally u is emitted.  Letters "ACGTN"[code] when rb < l_pac, "TGCAN"[code] otherwise.
 *         NM = n_mm + n_gap
 *
 *   is_rev = rb >= l_pac; pos = is_rev ? 2*l_pac - re : rb
 *   a leading D is dropped and pos += its length; else a trailing D is dropped (MD unchanged)
 *   if qb != 0 or qe != l_query: clip5 = is_rev ? l_query - qe : qb, clip3 = is_rev ? qb :
 *   l_query - qe; a nonzero clip5 is prepended, a nonzero clip3 appended as S
 *
 * CIGAR words are len << 4 | op, M = 0, I = 1, D = 2, S = 3.  Scope: pos is the 0-based forward
 * coordinate on the concatenated text, with or without a contig table (no rid, no contig offset is
 * stored).  With a table (bsw_set_contigs, bsw_contigs.h) the reject test reads it: a region with
 * seg(rb) != seg(re - 1) is BSW_ALN_REJECTED (bns_intv2rid < 0), of which the l_pac test is the
 * one-contig case; the table has to sum to opt->l_pac (l_pac == 0: to the resident length), or the
 * call returns BSW_E_INVAL.  No ALT contigs.  opt->l_pac == 0
 * is a one-strand reference: every region is forward.
 *
 * A REJECTED region -- gen_cigar2's rejects above, rb < 0 or re < 0 (upstream's unmapped
 * record) and the zeroed regions bsw_chain2aln* writes for skipped seeds -- is one pass with no
 * DP: pos = -1, n_cigar = 0, NM = -1, md_len = 0, score = 0, flag BSW_ALN_REJECTED (upstream
 * reads an uninitialised score there).  It is not an error.  Any other region whose [qb, qe)
 * lies outside its read, whose re is past the resident text, whose query or reference span
 * exceeds BSW_MAX_LEN, or whose read index is outside [0, n_reads) fails the call with
 * BSW_E_RANGE.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_ALN_API.
 */
#ifndef BSW_ALN_H
#define BSW_ALN_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_ALN_API 1

#define BSW_ALN_REJECTED 1      /* no alignment (see above)                                    */
#define BSW_ALN_NODP     2      /* the last pass took the gap-free shortcut (no DP)            */
#define BSW_ALN_OVERFLOW 4      /* CIGAR longer than cigar_stride or MD longer than md_stride  */

typedef struct bsw_aln_t {       /* one per region                                              */
    int64_t pos;                 /* 0-based forward-strand position of the first aligned base   */
    int32_t is_rev;
    int32_t n_cigar;             /* ops incl. clips; -1: the DP CIGAR or the clipped CIGAR has
                                    more than cigar_stride ops -- then only score, w, n_pass
                                    and flags are defined                                       */
    int32_t NM;
    int32_t score;               /* the last pass's global score                                */
    int32_t w;                   /* the w_ of the last pass                                     */
    int32_t n_pass;              /* gen_cigar2 passes run (1..3)                                */
    int32_t md_len;              /* MD bytes (no terminator); -1: longer than md_stride; 0 when
                                    MD is skipped                                               */
    int32_t flags;               /* BSW_ALN_*                                                   */
} bsw_aln_t;

/* Regions -> alignments with every array in HBM of the context's first device, against the
 * resident reference (bsw_set_reference; BSW_E_INVAL without one).  Reads as in bsw_ext.h
 * (codes 0..4 at d_reads[d_read_off[i], + d_read_len[i])); region k belongs to read
 * d_reg_read[k] -- d_regs / d_reg_read are exactly what bsw_chain2aln_resident leaves in d_out /
 * d_seed_read.  Of opt only w and l_pac are read.  Outputs: d_aln[k], the CIGAR in
 * d_cigar[k * cigar_stride ...] (cigar_stride >= 1) and the MD bytes in d_md[k * md_stride ...];
 * d_md == NULL with md_stride == 0 skips MD.  Plan, gap-free regions, job building, the band
 * loop's decisions and NM / MD run on the GPU (csrc/bsw_aln.hip) around the batched ksw_global2;
 * the host reads back only job counts, once per pass.  `stream`: a hipStream_t or NULL.
 * Returns when the outputs are in HBM. */
int bsw_reg2aln_resident(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads,
                         const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                         const bsw_alnreg_t *d_regs, const int32_t *d_reg_read, int32_t n_regs,
                         bsw_aln_t *d_aln, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                         int32_t md_stride, void *stream);

/* The same with host arrays: uploads them, runs the resident form against the resident
 * reference, downloads aln / cigar / md.  Blocking. */
int bsw_reg2aln(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *regs, const int32_t *reg_read,
                int32_t n_regs, bsw_aln_t *aln, uint32_t *cigar, int32_t cigar_stride, uint8_t *md,
                int32_t md_stride);

typedef struct bsw_aln_stats_t {
    int32_t n_regs;              /* regions in the call                                         */
    int32_t n_rejected;
    int32_t n_gapfree;           /* regions finished by the gap-free kernel (no DP job)         */
    int32_t n_dp[3];             /* ksw_global2 jobs of pass 1, 2, 3                            */
    float   dp_ms;               /* ksw_global2 kernels (HIP events)                            */
    float   helper_ms;           /* plan, gap-free, job build and finish kernels (HIP events)   */
} bsw_aln_stats_t;
int bsw_aln_last_stats(bsw_ctx_t *ctx, bsw_aln_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_ALN_H */
