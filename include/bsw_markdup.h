/*
 * bsw_markdup.h -- duplicate marking on the GPU: flag 0x400 on the records of bsw_records* (bsw_rec.h) before
 * bsw_sam_text* / bsw_bam_records* print them, so that the mark reaches SAM, BAM, the sort and the index.
 * [SPEC-RECALL: the duplicate rules of Picard MarkDuplicates and samtools markdup as commonly described]:
 * neither tool is at hand and byte parity with either is not claimed.  This text is the specification;
 * tests/markdup_py.py pins it with a restatement that compares every candidate with every other.
 *
 * SCOPE.  One call marks one batch; duplicates across batches are the caller's, and so are optical duplicates,
 * UMIs / barcodes, the removal of marked records and the `@PG` line of the header.
 *
 * THE CHAIN.   bsw_records* -> bsw_mark_duplicates* -> bsw_sam_text* / bsw_bam_records* -> bsw_bam_sort* -> ...
 *
 * INPUTS, as bsw_sam_text_resident takes them: d_recs[n_rec], d_rec_first[n_reads + 1], d_aln[n_aln], d_cigar with
 *   cigar_stride, d_read_off / d_read_len, d_quals (the printed characters, parallel to the reads, quals_len bytes;
 *   or NULL) and `paired` (reads 2p and 2p + 1 are the ends of pair p).  No reference text and no read base is
 *   read.  The context's contig table (bsw_contigs.h) is read when one is set; it has to sum to opt->l_pac.
 *
 * CANDIDATE END.  Read r is a candidate when it has a record and its first record d_recs[d_rec_first[r]] (the
 *   one with which == 0) has 0x4 clear in `flag`.  For that end
 *     rid = contig_rid of the record's pos, or 0 with no table;     s = the record's is_rev;
 *     u   = the unclipped 5' coordinate, from the CIGAR of alignment rec.aln:
 *             forward:  u = pos - (length of a leading clip)
 *             reverse:  u = pos + rlen - 1 + (length of a trailing clip),   rlen = the sum of the M and D lengths.
 *   A clip is op 3 or op 4 (one op at that end of the CIGAR).  u may fall below 0 or below its contig's start:
 *   it is compared as a signed global coordinate, never clamped or re-mapped to another contig.
 *
 * SCORE.  A read's score is the sum over its quality characters q of (q - 33) for those with q - 33 >= min_qual;
 *   0 when d_quals is NULL.
 *
 * PAIRS.  With paired != 0, pair p is a pair candidate when both of its reads are candidates.  Its two ends are
 *   ordered by the tuple (rid, u, s): lo and hi.  The key is (rid_lo, u_lo, s_lo, rid_hi, u_hi, s_hi); it does not
 *   record which end is read 1.  The pair's score is the sum of both reads' scores.  Pair candidates with equal
 *   keys form a set: the member with the highest score survives, equal scores broken by the lowest p; every other
 *   member is a duplicate, both reads (BSW_DUP_PAIR).
 *
 * FRAGMENTS.  A fragment is a candidate read that is not in a pair candidate: every candidate when paired == 0,
 *   and an end whose mate is unmapped.  Its key is (rid, u, s).  It is a duplicate when any end of any pair
 *   candidate, lo or hi, has the same (rid, u, s), whatever its score (BSW_DUP_FRAG_BY_PAIR).  Otherwise, among
 *   the fragments of equal key, the one with the highest score, then the lowest read index, survives; the rest are
 *   duplicates (BSW_DUP_FRAG).
 *
 * RECORDS.  Every record of a duplicate read that has 0x4 clear, supplementary and secondary records included,
 *   gets 0x400 in `flag` and in `sam_flag`; every other record has 0x400 cleared in both.  The result is thus a
 *   function of the inputs and the call can be repeated.  Unmapped records are never marked.
 *
 * OUTPUTS.  d_recs in place; d_dup[n_reads]: 0, or one of BSW_DUP_*; the stats.
 *
 * LIMITS.  0 < l_pac <= 2^39 and at most 2^23 - 1 contigs, so that an end's (rid, u, s) is one 64-bit word.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_MARKDUP_API.
 */
#ifndef BSW_MARKDUP_H
#define BSW_MARKDUP_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_aln.h"
#include "bsw_rec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_MARKDUP_API 1

#define BSW_DUP_PAIR         1       /* both reads of a pair that lost to a better pair of its set    */
#define BSW_DUP_FRAG         2       /* a fragment that lost to a better fragment of its set          */
#define BSW_DUP_FRAG_BY_PAIR 3       /* a fragment at the (rid, u, s) of some pair candidate's end    */

#define BSW_MARKDUP_MAX_L_PAC ((int64_t)1 << 39)
#define BSW_MARKDUP_MAX_CONTIGS ((1 << 23) - 1)

typedef struct bsw_markdup_opt_t {
    int64_t  l_pac;                  /* > 0: the forward strand's bases (the contig table's sum)      */
    int32_t  min_qual;               /* 15: qualities below it do not count into the score; >= 0      */
    uint32_t flags;                  /* none defined: 0                                               */
} bsw_markdup_opt_t;

void bsw_markdup_opt_default(bsw_markdup_opt_t *opt);     /* l_pac = 0 is the caller's to set */

/* Every array in HBM of the context's first device.  n_reads == 0 is a valid call that runs nothing.
 * BSW_E_INVAL: a null ctx / opt; l_pac outside (0, BSW_MARKDUP_MAX_L_PAC]; min_qual < 0; an unknown flag; negative
 *   sizes; an odd n_reads with paired; cigar_stride < 1; with n_reads > 0 a null d_rec_first / d_read_off /
 *   d_read_len / d_dup, with n_rec > 0 a null d_recs, with n_aln > 0 a null d_aln / d_cigar; a contig table that
 *   does not sum to l_pac or has more than BSW_MARKDUP_MAX_CONTIGS contigs.
 * BSW_E_RANGE, all found through one readback before any byte of d_recs or d_dup is written: a d_rec_first that
 *   decreases, does not start at 0 or does not end at n_rec; a record whose `read` is not the read it is listed
 *   under; an `aln` outside [-1, n_aln); a candidate's first record whose aln is -1, whose alignment's n_cigar is
 *   <= 0 or above cigar_stride, whose pos is outside [0, l_pac), or whose u is outside [-2^31, 2^40 - 2^31) (a CIGAR
 *   whose rlen plus clip passes 2^31: no read has one); with d_quals a negative read offset or length or a read that
 *   reaches past quals_len.
 * `stream`: a hipStream_t or NULL.  Returns when the outputs are in HBM. */
int bsw_mark_duplicates_resident(bsw_ctx_t *ctx, const bsw_markdup_opt_t *opt, bsw_rec_t *d_recs,
                                 const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                                 const uint32_t *d_cigar, int32_t cigar_stride, int32_t n_aln,
                                 const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                                 const uint8_t *d_quals, int64_t quals_len, int32_t paired, uint8_t *d_dup,
                                 void *stream);
/* The same with host arrays.  Blocking. */
int bsw_mark_duplicates(bsw_ctx_t *ctx, const bsw_markdup_opt_t *opt, bsw_rec_t *recs, const int32_t *rec_first,
                        int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                        int32_t n_aln, const int64_t *read_off, const int32_t *read_len, int32_t n_reads,
                        const uint8_t *quals, int64_t quals_len, int32_t paired, uint8_t *dup);

#define BSW_MARKDUP_ROUTE_NONE  0    /* nothing to sort, or no key bit varied                         */
#define BSW_MARKDUP_ROUTE_ONE   1    /* the varying bits fit one 64-bit word: one radix sort          */
#define BSW_MARKDUP_ROUTE_MULTI 2    /* stable LSD passes of the 64-bit sort, low field first         */

typedef struct bsw_markdup_stats_t { /* of the last bsw_mark_duplicates* call                         */
    int32_t n_reads;
    int32_t n_cand;                  /* candidate ends                                                */
    int32_t n_pair_cand;             /* pair candidates                                               */
    int32_t n_dup_pairs;             /* pairs marked BSW_DUP_PAIR                                     */
    int32_t n_dup_frag;              /* reads marked BSW_DUP_FRAG                                     */
    int32_t n_dup_frag_by_pair;      /* reads marked BSW_DUP_FRAG_BY_PAIR                             */
    int32_t n_pair_sets;             /* pair-key sets with more than one member                       */
    int32_t n_end_sets;              /* (rid, u, s) sets of candidate ends with more than one member  */
    int32_t n_flagged;               /* records that carry 0x400 afterwards                           */
    int32_t pair_key_bits;           /* bits of the pair key and score that varied over the batch     */
    int32_t end_key_bits;            /* the same of the end sort's key                                */
    int32_t pair_route, end_route;   /* BSW_MARKDUP_ROUTE_*                                           */
    float   score_ms;                /* the score kernel (HIP events)                                 */
    float   key_ms;                  /* end, candidate and key kernels, their scans                   */
    float   sort_ms;                 /* packing, radix sorts, gathers                                 */
    float   mark_ms;                 /* set heads, decisions and the mark kernel                      */
    int32_t reserved;
} bsw_markdup_stats_t;
int bsw_markdup_last_stats(bsw_ctx_t *ctx, bsw_markdup_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_MARKDUP_H */
