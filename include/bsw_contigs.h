/*
 * bsw_contigs.h -- the contig table of a multi-contig reference.  The reference stays ONE
 * concatenated text (bsw_set_reference: forward + reverse complement of l_pac bases); the table says
 * where its contigs begin and what they are called.  Upstream keeps a rid beside every coordinate
 * (bntseq's bns_pos2rid / bns_intv2rid, [UPSTREAM-RECALL]); here the rid is never stored: every
 * public struct keeps GLOBAL coordinates on the concatenated text, and a stage that needs a rid
 * derives it where it reads the coordinate, by a binary search of the table (csrc/bsw_contig_seg.h,
 * one statement for the host and every kernel).
 *
 * SEGMENTS.  off[0..n] = the prefix sums of the lengths (off[n] = l_pac).  The strand boundary is
 *   one more join: the sorted boundaries of the two-strand text are 0, off[1], .., l_pac,
 *   2 l_pac - off[n-1], .., 2 l_pac.  seg(x) = the index of the interval that holds x; rid = seg < n
 *   ? seg : 2n - 1 - seg; "same contig and strand" = equal seg; [b, e) crosses a join when seg(b) !=
 *   seg(e - 1).  Every l_pac crossing test of the stages is the n = 1 case of that expression.
 *
 * WHAT READS THE TABLE (BSW_CONTIGS_API 1), from seeds to text:
 *   bsw_mem_chain_device (bsw_fmi.h; its table is set with bsw_fmi_set_contigs)  a seed with seg(rbeg) !=
 *                        seg(rbeg + len - 1) is dropped (bns_intv2rid < 0); test_and_merge returns 0 as its
 *                        first test when the seed's rid is not the chain's, which is that of its first seed.
 *   bsw_extend_seeds*, bsw_chain2aln* (bsw_ext.h)  after the rmax[] computation the target window is clipped
 *                        to the segment of the chain's first seed (bns_fetch_seq with mid = seeds[0].rbeg),
 *                        in the host builder and in both device builders alike; a seed over a join is
 *                        BSW_E_RANGE, as one over l_pac is.
 *   bsw_regs_select*     (bsw_sel.h)  mem_sort_dedup_patch compares, drops and patches regions of one contig
 *                        only: the outer skip also moves on when p and a[i - 1] differ in rid, the inner
 *                        loop runs only while p and a[j] agree.
 *   bsw_reg2aln*         (bsw_aln.h)  a region with seg(rb) != seg(re - 1) is BSW_ALN_REJECTED, exactly
 *                        as one crossing l_pac is with no table (bwa_gen_cigar2: bns_intv2rid < 0).
 *                        pos stays global.
 *   bsw_pe_stat*         (bsw_pe.h)   a pair whose two top regions lie on different contigs gives no
 *                        insert size (mem_pestat: r[0]->a[0].rid != r[1]->a[0].rid).
 *   bsw_pe_pair*         (bsw_pe.h)   mem_pair never pairs hits on different contigs (upstream's sort
 *                        key rid << 32 | position - offset: the order of the global forward position,
 *                        the distance scan ends at a rid change), and no_pairing's proper flag 0x2
 *                        also needs equal rids.
 *   bsw_matesw*          (bsw_matesw.h)  after the clamp to [0, 2 l_pac) a rescue window is clipped to the
 *                        segment of its midpoint (bns_fetch_seq), and its job exists only when that
 *                        segment's contig is the anchor's and min_seed_len bases are left.
 *   bsw_records*         (bsw_rec.h)  a record's rid comes from pos, its mate's from mpos, both after
 *                        cross-linking (an unmapped end takes its mate's).  TLEN is 0 unless the two
 *                        rids are equal.  pos / mpos stay global.
 *   bsw_sam_text*        (bsw_rec.h)  RNAME = the contig's name, POS = pos - off[rid] + 1; RNEXT `=`
 *                        when the rids are equal, else the mate's contig name; PNEXT contig-relative;
 *                        every SA:Z and XA:Z entry prints its own contig's name and relative position.
 *                        opt->rname is not printed (its argument check stays: 1..63 bytes).
 *   Every one of these calls checks its table against its l_pac: BSW_E_INVAL when l_pac is not the sum of
 *   the lengths (a one-strand reference, l_pac == 0: when the reference's length is not).  SMEM collection
 *   (bsw_mem_collect_intv*) reads no coordinate and no table.
 * OUT OF SCOPE: ALT contigs (is_alt, n_pri < n).  Set both tables (bsw_set_contigs on the context,
 *   bsw_fmi_set_contigs on the index) or neither: the stages do not check one against the other.
 *
 * With no table set every call behaves exactly as before this header existed.
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged).
 */
#ifndef BSW_CONTIGS_H
#define BSW_CONTIGS_H

#include <stdint.h>
#include "bsw.h"
#include "bsw_fmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_CONTIGS_API 1

#define BSW_CONTIG_MAX_NAME 63       /* bytes of a contig name (BSW_REC_MAX_RNAME)                   */
#define BSW_CONTIG_MAX_N   (1 << 22)            /* contigs in a table                                */
#define BSW_CONTIG_MAX_SUM ((int64_t)1 << 39)   /* the sum of their lengths (l_pac)                  */
/* (the pairing kernels tell contigs apart by moving contig k's hits k << 40 away: with these two limits
 * no two contigs come within any int32 insert-size bound of each other and nothing overflows 63 bits) */

/* The table of n contigs: len[i] > 0 bases, names[i] NUL-terminated, 1..BSW_CONTIG_MAX_NAME bytes.
 * Call it after bsw_set_reference; the table is copied to every device of the context (offsets,
 * flat name bytes and name offsets in HBM) and stays until the next call.  n = 0 removes it (len
 * and names are not read).  Waits for running stage calls, as bsw_set_reference does.  Every
 * device's copy is made before any device switches to it: a call that fails (BSW_E_INVAL,
 * BSW_E_NOMEM, BSW_E_HIP) leaves the table that was set, on every device.
 * bsw_set_reference does not touch the table: after a new reference the old table stays, and
 * every stage call returns BSW_E_INVAL until a table that sums to the new l_pac (or none) is set.
 * BSW_E_INVAL: n < 0 or > BSW_CONTIG_MAX_N, a length <= 0, an empty, over-long or null name, a
 * sum above BSW_CONTIG_MAX_SUM. */
int bsw_set_contigs(bsw_ctx_t *ctx, int32_t n, const int64_t *len, const char *const *names);

/* The same lengths for bsw_mem_chain_device (bsw_fmi.h), which has no context: the table lives with the
 * index, on its device.  n = 0 removes it.  bsw_mem_chain_device returns BSW_E_INVAL when the lengths do
 * not sum to the index's l_pac.  BSW_E_INVAL: n < 0 or > BSW_CONTIG_MAX_N, a length <= 0, a sum above
 * BSW_CONTIG_MAX_SUM; BSW_E_NODEV for a host-only index.  A failed call leaves the table that was set. */
int bsw_fmi_set_contigs(bsw_fmi_t *fmi, int32_t n, const int64_t *len);

#ifdef __cplusplus
}
#endif
#endif /* BSW_CONTIGS_H */
