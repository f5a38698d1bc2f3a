/*
 * bsw_rec.h -- SAM records on the GPU: which regions become records, their flags, MAPQ caps, mate
 * fields, TLEN, the SA / XA / MC cross-references and the text of every line.  The step upstream
 * runs last: mem_reg2sam, mem_gen_alt, mem_aln2sam and the output block of mem_sam_pe (lh3/bwa
 * bwamem.c, bwamem_extra.c, bwamem_pair.c, kept unchanged by bwa-mem2; [UPSTREAM-RECALL]: the
 * reference tree holds no source of them).  This text is the specification; tests/rec_py.py pins
 * it.  "list" = a read's regions as bsw_regs_select* (single-end) or bsw_pe_pair* (paired-end) left
 * them, info = their bsw_selinfo_t; reads 2p and 2p + 1 are the two ends of pair p.
 *
 * SCOPE.  With no contig table one reference sequence (rid 0, its name opt->rname).  With a table
 * (bsw_set_contigs, bsw_contigs.h) the rids are derived from the global positions: a record's from
 * pos, its mate's from mpos, both after cross-linking (an unmapped end takes its mate's); TLEN is 0
 * unless the two are equal (mem_aln2sam: p->rid == m->rid); the text prints the contig's name for
 * `rname` and pos - offset + 1 for `pos + 1` wherever they stand below, each SA:Z / XA:Z entry its
 * own contig's, and RNEXT is `=` only when the rids are equal, else the mate's contig name.
 * opt->rname is then not printed (the argument check on it stays, so that it needs no context), and
 * opt->l_pac has to be the sum of the contig lengths in the text calls too (BSW_E_INVAL).  pos, mpos
 * and every bsw_aln_t.pos stay global.  No ALT contigs (is_alt = 0, n_pri = n, secondary_all ==
 * secondary); MEM_F_ALL (-a) off; no RG tag, no comment.  File I/O, the header and the command line
 * are the caller's.
 *
 * ALIGNMENTS (mem_reg2aln).  The unmapped alignment (mem_reg2aln(.., 0)): pos -1, flag 0x4,
 *   n_cigar 0, everything else 0 -- `AS:i:0 XS:i:0` are printed.  The alignment of region r takes
 *   pos / is_rev / CIGAR / NM / MD from bsw_reg2aln (bsw_aln.h); score = r.score (not truesc),
 *   sub = max(info.sub, info.csub); mapq = info.mapq when secondary < 0 (-2 included), else 0; flag
 *   0x100 when secondary >= 0.  Only the regions that records need are aligned: the records' own
 *   and their XA members.  A needed region that bsw_reg2aln rejects (BSW_ALN_REJECTED, upstream's
 *   assert(q->rid >= 0)) fails the call with BSW_E_RANGE; so does one whose CIGAR or MD overflows
 *   its stride (their number is in the stats).
 *
 * SECONDARY_ALL.  bsw_selinfo_t carries `secondary` alone.  They are equal but for the region z
 *   bsw_pe_pair* chose in its paired branch, whose secondary it overwrote with -2.  For a region
 *   with secondary == -2, secondary_all is recomputed by PRIMARY MARKING step 4's overlap test
 *   (bsw_sel.h, with opt->mask_level) against the EARLIER regions of the list whose secondary ==
 *   -1, in list order, taking the first that passes; -1 when none does.  That is the value the
 *   marking gave it: the marking tested the same regions in the same order.
 *
 * RECORD LIST (mem_reg2sam): single-end reads (extra_flag = 0, no mate) and both ends of a pair
 *   with pairs.paired == 0 (extra_flag = 0x41 for end 0, 0x81 for end 1, plus 0x2 when
 *   pairs.proper).  For k in list order: skipped when score < T; skipped when secondary >= 0.  The
 *   l-th kept region (l = 0, 1, ..) is record `which` = l: flag = extra_flag, for l >= 1 also 0x800,
 *   or 0x10000 under BSW_REC_NO_MULTI; mapq = its alignment's, for l >= 1 lowered to record 0's
 *   unless BSW_REC_KEEP_SUPP_MAPQ.  No region kept: one record of the unmapped alignment with
 *   extra_flag.  n_list = the number of records of the read.
 *
 * PAIRED BRANCH (pairs.paired == 1): exactly one record per end e, region z[e] (outside the list:
 *   BSW_E_RANGE); mapq = pairs.mapq[e]; flag = 0x40 << e | 0x1 | (proper ? 0x2 : 0); which = 0,
 *   n_list = 1.  Before XA, the primary switch on a working copy of secondary_all: k =
 *   secondary_all[z]; if k >= 0, every j with secondary_all[j] == k, and j == k itself, gets z, and
 *   secondary_all[z] = -1.
 *
 * MATE.  The mate alignment of a record of end e is the other end's list[pairs.z[other]], or the
 *   unmapped alignment when that z is -1.  With pairs as bsw_pe_pair* leaves them that is, in both
 *   branches, the alignment of the other end's record 0 (no_pairing: z is 0 when list[0].score >= T
 *   and -1 otherwise, and list[0] is then record 0), and that is what the stage takes: pairs.z is
 *   read and range-checked in the paired branch only and IGNORED when pairs.paired == 0.
 *
 * XA (mem_gen_alt), on the (switched) secondary_all:  pri(i) = k = secondary_all[i] when k >= 0 and
 *   score[i] >= score[k] * XA_drop_ratio (the product in double, from the float option), else -1.
 *   cnt[r] = the number of i with pri(i) == r (no T test).  A record of region r carries, in
 *   ascending i, the i with pri(i) == r, but only when cnt[r] <= max_XA_hits.  Members of primaries
 *   that produce no record are never aligned.  Text per member: `rname,+-pos+1,CIGAR,NM;` with
 *   bsw_reg2aln's own soft clips (S).
 *
 * CROSS-LINKING (mem_aln2sam), on copies p (the record's alignment) and m (the mate's; none for
 *   single-end):  0x1 when m exists; 0x4 when p is unmapped; 0x8 when m is unmapped.  p unmapped and
 *   m mapped: p takes m's pos and is_rev, p's n_cigar becomes 0.  m unmapped and p mapped: m takes
 *   p's pos and is_rev, m's n_cigar becomes 0.  Then 0x10 from p.is_rev, 0x20 from m.is_rev.
 *   Printed flag = (flag & 0xffff) | (flag & 0x10000 ? 0x100 : 0).
 *   TLEN: 0 when either n_cigar is 0; else p0 = p.pos + (p.is_rev ? rlen(p) - 1 : 0), p1 likewise
 *   of m, tlen = -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0)); rlen = the sum of the M and D
 *   lengths.
 *
 * TEXT.  QNAME \t FLAG \t RNAME \t POS \t MAPQ \t CIGAR \t RNEXT \t PNEXT \t TLEN \t SEQ \t QUAL,
 *   the tags (each with a leading \t), \n.
 *   RNAME POS MAPQ CIGAR: `rname, pos + 1, mapq, CIGAR` when p has a position (its own or the
 *     mate's), the CIGAR `*` when n_cigar is 0; otherwise `* 0 0 *`.  Clip ops (3, 4) print as
 *     (which ? 'H' : 'S') unless BSW_REC_SOFTCLIP, under which they print as they are ("MIDSH"[op]).
 *   RNEXT PNEXT TLEN: `= mpos + 1 tlen` when m has a position; otherwise `* 0 0`.
 *   SEQ / QUAL: is_rev == 0: "ACGTN"[code] and the quals as given; is_rev == 1 (an unmapped record
 *     that took its mate's strand included): reversed, "TGCAN"[code], the quals reversed.  When
 *     n_cigar != 0 && which != 0 && !BSW_REC_SOFTCLIP the leading and trailing clip of the CIGAR
 *     are cut from the printed (strand-oriented) sequence.  No quals: `*`.
 *   Tags, in this order:  NM:i and MD:Z when p's n_cigar != 0;  MC:Z when m's n_cigar != 0 -- the
 *     mate's CIGAR with clips printed by THIS record's which (upstream's add_cigar(opt, m, str,
 *     which));  AS:i;  XS:i when sub >= 0;  SA:Z only when the record's flag lacks 0x100 and the
 *     read has another record without 0x100: those records in list order as
 *     `rname,pos+1,+-,CIGAR,mapq,NM;` with S clips;  XA:Z when the record has members.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_REC_API.
 */
#ifndef BSW_REC_H
#define BSW_REC_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_ext.h"
#include "bsw_aln.h"
#include "bsw_sel.h"
#include "bsw_pe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_REC_API 1

#define BSW_REC_SOFTCLIP       1     /* bwa mem -Y: soft clips for supplementary records too        */
#define BSW_REC_NO_MULTI       2     /* bwa mem -M: further records are 0x100, not 0x800             */
#define BSW_REC_KEEP_SUPP_MAPQ 4     /* bwa mem -q: supplementary MAPQs are not lowered              */

#define BSW_REC_MAX_RNAME 63         /* bytes of opt->rname before its terminator                    */
#define BSW_REC_MAX_NAME  255        /* bytes of a read name (longer: BSW_E_RANGE)                   */

typedef struct bsw_rec_opt_t {
    int64_t l_pac;                   /* > 0: the resident text is forward + reverse complement       */
    int32_t w;                       /* band width of bsw_reg2aln (100)                              */
    int32_t T;                       /* 30: minimum score to output                                  */
    int32_t max_XA_hits;             /* 5                                                            */
    float   XA_drop_ratio;           /* 0.8                                                          */
    float   mask_level;              /* 0.5 (the overlap test of SECONDARY_ALL)                      */
    int32_t flags;                   /* BSW_REC_*                                                    */
    char    rname[BSW_REC_MAX_RNAME + 1];   /* the reference's name, 1..63 bytes, NUL-terminated     */
} bsw_rec_opt_t;

typedef struct bsw_rec_t {           /* one per SAM line                                             */
    int64_t pos;                     /* 0-based, after cross-linking (its own or the mate's); -1: none */
    int64_t mpos;                    /* the mate's, after cross-linking; -1: none (single-end too)   */
    int64_t tlen;
    int32_t read;
    int32_t reg;                     /* index into d_sel_regs; -1: the unmapped alignment            */
    int32_t aln;                     /* index into d_aln / d_cigar / d_md; -1: n_cigar is 0          */
    int32_t which, n_list;           /* its index among, and the number of, the read's records       */
    int32_t flag;                    /* internal (with 0x10000)                                      */
    int32_t sam_flag;                /* printed                                                      */
    int32_t is_rev;                  /* after cross-linking                                          */
    int32_t mapq;
    int32_t score, sub;              /* AS, XS                                                       */
    int32_t m_is_rev;
    int32_t m_aln;                   /* the mate's alignment; -1: none, or its n_cigar is 0          */
    int32_t xa_first, xa_n;          /* XA members: alignments [xa_first, xa_first + xa_n)           */
    int32_t reserved;
} bsw_rec_t;

void bsw_rec_opt_default(bsw_rec_opt_t *opt);     /* l_pac = 0 and rname = "" are the caller's to set */

/* CALL 1: regions to records.  Every array in HBM of the context's first device, against the
 * resident reference (bsw_set_reference; its length has to be 2 * l_pac, BSW_E_INVAL otherwise).
 * Reads as bsw_reg2aln* takes them; d_sel_regs / d_sel_info [n_regs] / d_read_first[n_reads + 1] as
 * bsw_pe_pair* (paired-end) or bsw_regs_select* (single-end) leave them; d_pairs[n_reads / 2], or
 * NULL for single-end.  Nothing in them is changed.  Outputs:
 *   d_recs[rec_cap]         the records, grouped by read, within a read in list order
 *   d_rec_first[n_reads+1]  read r's records are [d_rec_first[r], d_rec_first[r + 1])
 *   d_aln[aln_cap], d_cigar[aln_cap * cigar_stride], d_md[aln_cap * md_stride]  as bsw_aln.h; both
 *                           strides >= 1.  A record's own alignment is followed by its XA members'
 *                           in ascending list order: the flat XA member list is d_aln_reg over the
 *                           records' [xa_first, xa_first + xa_n)
 *   d_aln_reg[aln_cap]      the region (index into d_sel_regs) of every alignment
 *   *n_rec, *n_aln          the numbers written
 * rec_cap < *n_rec or aln_cap < *n_aln: BSW_E_RANGE with both counts set to what is needed
 * (d_rec_first is still written); rec_cap = n_reads + n_regs and aln_cap = n_regs always suffice.
 * BSW_E_INVAL for an odd n_reads with d_pairs, l_pac <= 0, w < 0, max_XA_hits < 0, an rname that is
 * empty or unterminated, a stride < 1.  BSW_E_RANGE besides: a decreasing d_read_first (or one
 * outside [0, n_regs]), a z outside its list in the paired branch, a rejected or overflowing needed
 * region, and bsw_reg2aln's own.  `stream`: a hipStream_t or NULL.  Returns when the outputs are
 * in HBM.  The alignments run on bsw_reg2aln's kernels but leave bsw_aln_last_stats alone: their
 * count and time are n_aln and aln_ms of bsw_rec_last_stats. */
int bsw_records_resident(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const uint8_t *d_reads,
                         const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                         const bsw_alnreg_t *d_sel_regs, const bsw_selinfo_t *d_sel_info,
                         const int32_t *d_read_first, int32_t n_regs, const bsw_pair_t *d_pairs,
                         bsw_rec_t *d_recs, int32_t *d_rec_first, int32_t rec_cap, bsw_aln_t *d_aln,
                         int32_t *d_aln_reg, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                         int32_t md_stride, int32_t aln_cap, int32_t *n_rec, int32_t *n_aln, void *stream);
/* The same with host arrays (n_regs = read_first[n_reads]).  Blocking. */
int bsw_records(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *sel_regs,
                const bsw_selinfo_t *sel_info, const int32_t *read_first, const bsw_pair_t *pairs,
                bsw_rec_t *recs, int32_t *rec_first, int32_t rec_cap, bsw_aln_t *aln, int32_t *aln_reg,
                uint32_t *cigar, int32_t cigar_stride, uint8_t *md, int32_t md_stride, int32_t aln_cap,
                int32_t *n_rec, int32_t *n_aln);

/* CALL 2: records to SAM lines.  Call 1's outputs (n_rec records, n_aln alignments) and the reads;
 * names: read (single-end, paired == 0) or pair (paired != 0) i's name is d_names[d_name_off[i],
 * d_name_off[i + 1]) -- n_reads + 1 or n_reads / 2 + 1 offsets; d_quals: the printed quality
 * characters, parallel to d_reads (the same offsets), or NULL for `*`.  Of opt, flags and rname
 * are read.  Outputs: record i's line is d_text[d_text_off[i], d_text_off[i + 1]); *n_bytes =
 * d_text_off[n_rec].  text_cap < *n_bytes: BSW_E_RANGE with *n_bytes = what is needed (d_text_off
 * is still written).  BSW_E_RANGE besides: a name longer than BSW_REC_MAX_NAME or decreasing name
 * offsets, a record whose read, aln, m_aln or XA range is outside the arrays. */
int bsw_sam_text_resident(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *d_recs,
                          const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                          const uint32_t *d_cigar, int32_t cigar_stride, const uint8_t *d_md, int32_t md_stride,
                          int32_t n_aln, const uint8_t *d_reads, const int64_t *d_read_off,
                          const int32_t *d_read_len, int32_t n_reads, const uint8_t *d_names,
                          const int64_t *d_name_off, const uint8_t *d_quals, int32_t paired, uint8_t *d_text,
                          int64_t *d_text_off, int64_t text_cap, int64_t *n_bytes, void *stream);
/* The same with host arrays.  Blocking. */
int bsw_sam_text(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *recs, const int32_t *rec_first,
                 int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                 const uint8_t *md, int32_t md_stride, int32_t n_aln, const uint8_t *reads,
                 const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const uint8_t *names,
                 const int64_t *name_off, const uint8_t *quals, int32_t paired, uint8_t *text, int64_t *text_off,
                 int64_t text_cap, int64_t *n_bytes);

typedef struct bsw_rec_stats_t {     /* of the last bsw_records* call; n_bytes / text_ms of the last bsw_sam_text* */
    int32_t n_rec;
    int32_t n_unmapped;              /* records of the unmapped alignment                            */
    int32_t n_supp;                  /* records with which >= 1                                      */
    int32_t n_xa;                    /* XA members                                                   */
    int32_t n_aln;                   /* regions aligned                                              */
    int32_t n_overflow;              /* needed regions whose CIGAR or MD overflowed its stride       */
    int64_t n_bytes;
    float   aln_ms;                  /* bsw_reg2aln's dp_ms + helper_ms over the needed regions      */
    float   helper_ms;               /* plan, scans, fill and finish kernels (HIP events)            */
    float   text_ms;                 /* length, scan and write kernels (HIP events)                  */
    int32_t reserved;
} bsw_rec_stats_t;
int bsw_rec_last_stats(bsw_ctx_t *ctx, bsw_rec_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_REC_H */
