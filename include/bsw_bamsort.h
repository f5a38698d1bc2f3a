/*
 * bsw_bamsort.h -- coordinate-sorted, indexed BAM on the GPU: the BAM alignment blocks of bsw_bam_records*
 * (bsw_bam.h) reordered by coordinate in HBM (bsw_bam_sort*), and, once bsw_bgzf* (bsw_bgzf.h) has compressed
 * the sorted blocks and left their virtual offsets, the complete .bai file in HBM (bsw_bam_index*).
 * [SPEC-RECALL: SAMv1 section 4.2, section 5.1.1, section 5.2]: neither htslib nor samtools nor a sample
 * index is at hand.  This text is the specification; tests/bai_py.py pins it with a builder that restates the
 * rules below and with an independent reader that follows SAMv1 section 5 from the query's side.  Byte parity
 * with `samtools index` is neither claimed nor needed: a reader of the format finds every record.
 *
 * SCOPE.  One call sorts one batch; merging the sorted runs of several batches, .csi indexes and file I/O are
 * the caller's (duplicates of one batch are marked upstream, bsw_markdup.h; duplicates across batches are the
 * caller's).  A run is a valid sorted BAM when the batch is the whole file.  The
 * `@HD SO:coordinate` line is part of the caller's header text (bsw_bam_header copies it as given).
 * Both stages read nothing but BAM bytes and offsets: any uncompressed BAM record stream will do.
 *
 * THE CHAIN.   bsw_bam_records* -> bsw_bam_sort* -> bsw_bgzf* on the sorted blocks -> bsw_bam_index*
 *
 * THE SORT KEY of record i, from its own bytes (refID at byte 4, pos at 8, flag at 18 of the block):
 *     (refID < 0 ? n_ref : refID,  pos + 1,  flag & 0x10)       ascending, compared left to right.
 *   The sort is stable: equal keys keep their input order, so mates at one position stay as given, a run of
 *   fully unmapped records stays as given, and the records with no refID go last.
 *
 * THE INDEX.  Every number is little-endian.
 *     magic       `BAI\1`
 *     n_ref       int32
 *     per reference:
 *       n_bin     int32
 *       per bin:  bin uint32, n_chunk int32, per chunk: chunk_beg uint64, chunk_end uint64
 *       n_intv    int32
 *       ioffset   uint64[n_intv]
 *     n_no_coor   uint64
 *   RECORD EXTENT.  beg = pos; end = pos + rlen, rlen the sum of the M, D, N, = and X lengths (ops 0, 2, 3, 7,
 *     8) of the block's CIGAR words; with n_cigar_op == 0 or rlen == 0, end = pos + 1.
 *   BINS.  The bin is reg2bin(beg, end) of the UCSC binning scheme (14-bit smallest bin, 5 levels),
 *     recomputed from the extent; the block's own bin field is not read.  Records with refID >= 0 are
 *     indexed, a placed unmapped mate (flag 0x4) included; records with refID < 0 only count into n_no_coor.
 *   CHUNKS.  The members of one (refID, bin) are taken in file order.  With voff[i] the record's virtual offset
 *     and vend(i) = voff[i + 1] (end_voff for the last record of the file), a member starts a new chunk when it
 *     is the first of its bin or when  voff[i] >> 16  >  vend(previous member) >> 16;  otherwise it extends
 *     the previous chunk.  (Adjacent records and records in one compressed block thus share a chunk.)  A chunk
 *     is [voff[first member], vend(last member)).
 *   BIN ORDER.  Ascending within a reference; the pseudo-bin 37450 last, and only for a reference that has
 *     records.  It holds two "chunks": (voff of the reference's first record, vend of its last) and
 *     (n_mapped, n_unmapped), unmapped meaning flag 0x4.  n_bin counts it.
 *   LINEAR INDEX.  ioffset[w] is the smallest voff of a record that overlaps the 16,384-base window w; a
 *     record's windows are beg >> 14 .. (end - 1) >> 14.  n_intv is the last touched window + 1; an untouched
 *     window below n_intv takes the value of the next touched window on its right.  A reference without
 *     records has n_bin = 0 and n_intv = 0.
 *   The bytes are a function of the input alone (minima, maxima and counts do not depend on update order).
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_BAMSORT_API.
 */
#ifndef BSW_BAMSORT_H
#define BSW_BAMSORT_H

#include <stdint.h>
#include "bsw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_BAMSORT_API 1

#define BSW_BAI_MAX_REF_LEN (1 << 29)   /* the binning scheme's limit on a reference's length */
#define BSW_BAI_PSEUDO_BIN  37450

typedef struct bsw_bamsort_opt_t {
    int32_t  n_ref;                  /* references of the header block; > 0                           */
    uint32_t flags;                  /* none defined: 0                                               */
} bsw_bamsort_opt_t;

/* The blocks d_bam[d_bam_off[i], d_bam_off[i + 1]), i < n_rec (d_bam_off[0] == 0), in key order:
 *   d_out[0, n_bytes)      the same blocks, contiguous; n_bytes = d_bam_off[n_rec]
 *   d_out_off[n_rec + 1]   their offsets
 *   d_perm[n_rec]          the input index of output record i
 * d_out has to be 4-byte aligned; no byte at or behind d_out + n_bytes is written; the input is not changed.
 * n_rec == 0 is a valid call that runs nothing.
 * BSW_E_INVAL: a null ctx / opt; n_ref <= 0; an unknown flag; negative sizes; with n_rec > 0 a null d_bam /
 *   d_bam_off / d_out_off / d_perm, a null d_out with out_cap > 0; a misaligned d_out; d_out overlapping d_bam
 *   (d_bam inside [d_out, d_out + out_cap) is found before any device work, the rest once n_bytes is known;
 *   nothing has been written then either).
 * BSW_E_RANGE, found before d_out, d_out_off or d_perm is written: out_cap < n_bytes; decreasing offsets or a
 *   d_bam_off[0] != 0; a block whose block_size field is not d_bam_off[i + 1] - d_bam_off[i] - 4, or is below
 *   32; a refID outside [-1, n_ref); a pos below -1.
 * `stream`: a hipStream_t or NULL.  Returns when the blocks are in HBM. */
int bsw_bam_sort_resident(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const uint8_t *d_bam,
                          const int64_t *d_bam_off, int32_t n_rec, uint8_t *d_out, int64_t out_cap,
                          int64_t *d_out_off, int32_t *d_perm, void *stream);
/* The same with host arrays.  Blocking. */
int bsw_bam_sort(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const uint8_t *bam, const int64_t *bam_off,
                 int32_t n_rec, uint8_t *out, int64_t out_cap, int64_t *out_off, int32_t *perm);

/* The .bai of the sorted blocks d_bam / d_bam_off (n_rec of them) into d_bai[0, *n_bytes).
 *   ref_len[opt->n_ref]  host array: the references' lengths
 *   d_voff[n_rec]        the records' virtual offsets as bsw_bgzf* left them
 *   end_voff             the virtual offset behind the last record:
 *                        (base_coffset + d_blk_off[n_blocks]) << 16 of that bsw_bgzf* call
 * d_bai has to be 4-byte aligned; no byte at or behind d_bai + *n_bytes is written.  bai_cap < *n_bytes:
 * BSW_E_RANGE with *n_bytes = what is needed, nothing written.  The only readback is one copy of the byte
 * count, the error word and the counters of the stats.
 * BSW_E_INVAL: a null ctx / opt / ref_len / n_bytes; n_ref <= 0; an unknown flag; negative sizes or end_voff;
 *   with n_rec > 0 a null d_bam / d_bam_off / d_voff; a null d_bai with bai_cap > 0; a misaligned d_bai.
 * BSW_E_RANGE: a ref_len outside [0, BSW_BAI_MAX_REF_LEN] (found on the host); records not in the sort's
 *   order ((refID, pos) compared with the predecessor's, refID < 0 last); a record with refID >= 0 and
 *   pos < 0, or with end > ref_len[refID]; a decreasing d_voff, or one above end_voff; a CIGAR that overruns its
 *   block; everything the sort rejects in a block. */
int bsw_bam_index_resident(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const int32_t *ref_len, const uint8_t *d_bam,
                           const int64_t *d_bam_off, int32_t n_rec, const int64_t *d_voff, int64_t end_voff,
                           uint8_t *d_bai, int64_t bai_cap, int64_t *n_bytes, void *stream);
/* The same with host arrays.  Blocking. */
int bsw_bam_index(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const int32_t *ref_len, const uint8_t *bam,
                  const int64_t *bam_off, int32_t n_rec, const int64_t *voff, int64_t end_voff, uint8_t *bai,
                  int64_t bai_cap, int64_t *n_bytes);

typedef struct bsw_bamsort_stats_t { /* the sort's fields of the last bsw_bam_sort*, the index's of the last bsw_bam_index* */
    int32_t n_rec;                   /* of the last sort                                              */
    int32_t key_bits;                /* key bits that varied over the batch (the radix sort's span)   */
    int64_t n_bytes;                 /* bytes moved by the last sort                                  */
    float   key_ms;                  /* key kernel (HIP events)                                       */
    float   sort_ms;                 /* radix sort of (key, index)                                    */
    float   copy_ms;                 /* lengths, scan and the permute kernel                          */
    float   index_ms;                /* every kernel of the last index call                           */
    int32_t n_bins;                  /* bins written, the pseudo-bins not counted                     */
    int32_t n_chunks;                /* chunks written, those of the pseudo-bins not counted          */
    int64_t n_intv;                  /* linear-index entries written, over all references             */
    int64_t n_no_coor;
    int64_t bai_bytes;
} bsw_bamsort_stats_t;
int bsw_bamsort_last_stats(bsw_ctx_t *ctx, bsw_bamsort_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_BAMSORT_H */
