/*
 * bsw_bam.h -- BAM records on the GPU: the records of bsw_records* (bsw_rec.h) as uncompressed BAM
 * alignment blocks in HBM, beside bsw_sam_text*: the same inputs, the same information, binary.
 * [SPEC-RECALL: SAMv1 section 4.2 and the conventions of htslib's text parser, sam_parse1]: neither
 * the reference tree nor the build machines hold htslib, samtools or a sample BAM file.  This text is
 * the specification; tests/bam_py.py pins it, and ties it to the text of bsw_rec.h by decoding the
 * blocks back into SAM lines.
 *
 * SCOPE as bsw_rec.h: no ALT contigs, no -a, no RG tag, no comment.  File I/O and the command line are
 * the caller's: the header block (bsw_bam_header) followed by the records of any number of calls is an
 * uncompressed BAM stream; bsw_bgzf* (bsw_bgzf.h) cuts and compresses it into BGZF blocks on the device, and
 * bsw_bam_sort* / bsw_bam_index* (bsw_bamsort.h) put the blocks in coordinate order and build the .bai.
 *
 * THE RECORD.  p = recs[i]; "at" a global position = its contig, the contig's rid and offset
 *   (bsw_contigs.h); with no table rid 0, offset 0.  Every number is little-endian.
 *     block_size  int32   the bytes of the record behind this field
 *     refID       int32   p.pos >= 0: the rid at p.pos; else -1
 *     pos         int32   p.pos >= 0: p.pos - offset (0-based); else -1
 *     l_read_name uint8   the name's length + 1
 *     mapq        uint8   p.pos >= 0 ? p.mapq : 0  (the text prints `* 0 0 *` when p.pos < 0)
 *     bin         uint16  the low 16 bits of reg2bin(pos, end), the UCSC binning scheme with a 14-bit
 *                         smallest bin and 5 levels; end = pos + rlen (the sum of the M and D lengths)
 *                         when the record has a CIGAR, else pos + 1.  pos = -1 gives 4680.
 *     n_cigar_op  uint16  the alignment's n_cigar; 0 when p.aln < 0
 *     flag        uint16  p.sam_flag
 *     l_seq       int32   the bases printed: the read's length, less the hard clips where the text
 *                         cuts them (n_cigar != 0 && which != 0 && !BSW_REC_SOFTCLIP)
 *     next_refID  int32   p.mpos >= 0: the rid at p.mpos; else -1
 *     next_pos    int32   p.mpos >= 0: p.mpos - offset; else -1
 *     tlen        int32   p.tlen
 *     read_name   the name, NUL
 *     cigar       uint32[n_cigar_op]   len << 4 | op with M 0, I 1, D 2, S 4, H 5.  This library's ops 3
 *                         and 4 are clips and take the letter the text prints: S for which == 0, H
 *                         otherwise; under BSW_REC_SOFTCLIP as stored (3 -> S, 4 -> H)
 *     seq         uint8[(l_seq + 1) / 2]   two bases per byte, the first in the high nibble: A 1, C 2,
 *                         G 4, T 8, every code >= 4 15; strand-oriented as the text (is_rev: reversed and
 *                         complemented); the unused low nibble of an odd length is 0
 *     qual        uint8[l_seq]   (uint8_t)(q - 33) of the printed quality characters, in the text's
 *                         order; with no quals 0xFF, l_seq times
 *     tags        in the text's order and under the text's conditions: NM, MD:Z, MC:Z, AS, XS, SA:Z,
 *                         XA:Z.  A tag is its two letters, a type byte and the value.  Z values are byte
 *                         for byte what the text prints behind `XX:Z:`, then NUL.  The integer tags NM,
 *                         AS and XS take the smallest type that holds the value, as the text parser
 *                         chooses it:  0..255 C (uint8), 256..65535 S (uint16), above I (uint32);
 *                         -128..-1 c (int8), -32768..-129 s (int16), below i (int32).
 *
 * THE HEADER BLOCK (bsw_bam_header): `BAM\1`, l_text int32, the caller's SAM header text (l_text
 *   bytes, possibly none, copied as given), n_ref int32, then per reference l_name int32 (with the
 *   NUL), the name, NUL, l_ref int32.  With a contig table the references are its contigs in order;
 *   with none one reference, opt->rname of length opt->l_pac.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged) and to bsw_rec.h; this header
 * carries its own BSW_BAM_API.
 */
#ifndef BSW_BAM_H
#define BSW_BAM_H

#include <stdint.h>
#include "bsw_rec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_BAM_API 1

#define BSW_BAM_MAX_NAME 254         /* bytes of a read name: l_read_name is a byte and counts the NUL */

/* Records to BAM alignment blocks.  The arguments are those of bsw_sam_text_resident (bsw_rec.h) with
 * `bam` in place of `text`: call 1's outputs, the reads, names and quals; of opt, flags, rname and
 * l_pac are read.  Outputs: record i's block is d_bam[d_bam_off[i], d_bam_off[i + 1]); *n_bytes =
 * d_bam_off[n_rec].  d_bam has to be 4-byte aligned; no byte at or behind d_bam + *n_bytes is
 * written.  bam_cap < *n_bytes: BSW_E_RANGE with *n_bytes = what is needed (d_bam_off is still
 * written).  BSW_E_INVAL as bsw_sam_text_resident.  BSW_E_RANGE besides, found before anything is
 * written to d_bam: everything bsw_sam_text* rejects; a name longer than BSW_BAM_MAX_NAME; a
 * contig-relative pos or next_pos above INT32_MAX; a tlen outside int32; an n_cigar above 65535.
 * `stream`: a hipStream_t or NULL.  Returns when the blocks are in HBM. */
int bsw_bam_records_resident(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *d_recs,
                             const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                             const uint32_t *d_cigar, int32_t cigar_stride, const uint8_t *d_md, int32_t md_stride,
                             int32_t n_aln, const uint8_t *d_reads, const int64_t *d_read_off,
                             const int32_t *d_read_len, int32_t n_reads, const uint8_t *d_names,
                             const int64_t *d_name_off, const uint8_t *d_quals, int32_t paired, uint8_t *d_bam,
                             int64_t *d_bam_off, int64_t bam_cap, int64_t *n_bytes, void *stream);
/* The same with host arrays.  Blocking. */
int bsw_bam_records(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *recs, const int32_t *rec_first,
                    int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                    const uint8_t *md, int32_t md_stride, int32_t n_aln, const uint8_t *reads,
                    const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const uint8_t *names,
                    const int64_t *name_off, const uint8_t *quals, int32_t paired, uint8_t *bam, int64_t *bam_off,
                    int64_t bam_cap, int64_t *n_bytes);

/* The uncompressed header block into out[0, *n_bytes).  Host only: no device work.  sam_text: the SAM
 * header text (@HD, @SQ, @PG lines), l_text bytes, or NULL with l_text == 0.  cap < *n_bytes:
 * BSW_E_RANGE with *n_bytes = what is needed, nothing written.  BSW_E_INVAL: the option checks of
 * bsw_sam_text*, l_text < 0, cap < 0, and a contig table that does not sum to opt->l_pac.
 * BSW_E_RANGE: a reference longer than INT32_MAX. */
int bsw_bam_header(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const char *sam_text, int32_t l_text, uint8_t *out,
                   int64_t cap, int64_t *n_bytes);

typedef struct bsw_bam_stats_t {     /* of the last bsw_bam_records* call                            */
    int32_t n_rec;
    int32_t reserved;
    int64_t n_bytes;
    float   len_ms;                  /* length kernel and scan (HIP events)                          */
    float   write_ms;                /* write kernel (HIP events)                                    */
} bsw_bam_stats_t;
int bsw_bam_last_stats(bsw_ctx_t *ctx, bsw_bam_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_BAM_H */
