/*
 * bsw_bgzf.h -- BGZF on the GPU: a byte stream in HBM (the BAM blocks of bsw_bam_records*, a header block,
 * SAM text) as a sequence of whole, compressed BGZF blocks in HBM, with the block starts and the
 * records' virtual offsets that an index needs.  The deflate encoder runs on the device; there is no
 * zlib in this library.
 * [SPEC-RECALL: SAMv1 section 4.1, RFC 1951, RFC 1952]: neither htslib nor a sample file is at hand.
 * This text is the specification; tests/bgzf_py.py pins it with Python's zlib and gzip as the
 * independent decoders.
 *
 * SCOPE.  File I/O, the .csi index and the command line are the caller's; the .bai of coordinate-sorted blocks is
 * bsw_bam_index* (bsw_bamsort.h), which reads the d_voff of this call.  Blocks are cut
 * at byte counts, not at record boundaries; one deflate block per BGZF block; one compression level;
 * no decompression.
 *
 * THE BLOCK.  One gzip member:
 *     1f 8b 08 04         ID1, ID2, CM = deflate, FLG = FEXTRA
 *     00 00 00 00         MTIME 0
 *     00 ff               XFL 0, OS unknown
 *     06 00               XLEN 6
 *     42 43 02 00         the subfield 'B' 'C', its length 2
 *     BSIZE   uint16      the block's total bytes - 1
 *     one deflate stream
 *     CRC32   uint32      of the uncompressed bytes
 *     ISIZE   uint32      their count
 *   Header and trailer are 26 bytes.  A block holds at most 0xff00 input bytes and is at most 65,536
 *   bytes: the stored form (5 + 0xff00 + 26 = 65,311) always fits.
 * THE CUTS.  The input is cut at multiples of opt->block_bytes; the last chunk is shorter.  Records may
 *   straddle blocks.  Zero input bytes give zero blocks.
 * THE EOF MARKER (BSW_BGZF_EOF), 28 bytes behind the last block:
 *     1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00
 * The outputs of successive calls, concatenated, are a valid BGZF stream; the caller compresses the
 *   header block (bsw_bam_header) with a call of its own, so that the records start a fresh block.
 *
 * THE DEFLATE STREAM of a block is one deflate block with BFINAL = 1, the smallest of three forms, ties
 *   to the simpler:
 *     stored   (BTYPE 0)  01, LEN, ~LEN, the bytes.  opt->level == 0: every block.
 *     fixed    (BTYPE 1)  LZ77 tokens under the fixed codes.
 *     dynamic  (BTYPE 2)  LZ77 tokens under Huffman codes of the block's own symbol counts: code lengths
 *                         <= 15, sent through the code-length alphabet (run symbols 16 / 17 / 18, lengths
 *                         <= 7, HCLEN order); HLIT >= 257, HDIST >= 1; a block with no match has one distance
 *                         code of length 0; canonical codes, bit-reversed into the LSB-first stream.
 *   Matches are 3..258 bytes (258: symbol 285, no extra bits) at distances 1..32,768 and never reach
 *   outside the block.  The bytes are a function of the input and the options alone: the same call
 *   gives the same bytes on every run.
 *
 * Purely additive to ABI version 8 (bsw_abi_version() is unchanged); this header carries its own
 * BSW_BGZF_API.
 */
#ifndef BSW_BGZF_H
#define BSW_BGZF_H

#include <stdint.h>
#include "bsw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSW_BGZF_API 1

#define BSW_BGZF_MAX_BLOCK 0xff00    /* input bytes of a block, at most */
#define BSW_BGZF_EOF 1u              /* flags: the 28-byte EOF marker behind the last block */

typedef struct bsw_bgzf_opt_t {
    int32_t  level;                  /* 0: stored blocks; 1: the encoder (default)                    */
    int32_t  block_bytes;            /* input bytes per block, 1 .. BSW_BGZF_MAX_BLOCK (default)      */
    uint32_t flags;                  /* BSW_BGZF_EOF                                                  */
    int32_t  reserved;
    int64_t  base_coffset;           /* the file offset of this call's first block (virtual offsets)  */
} bsw_bgzf_opt_t;
void bsw_bgzf_opt_default(bsw_bgzf_opt_t *opt);

/* d_in[0, n_in) -> *n_blocks = ceil(n_in / block_bytes) BGZF blocks, contiguous in d_out[0, *n_bytes); block b
 * is d_out[d_blk_off[b], d_blk_off[b + 1]) (d_blk_off: n_blocks + 1 entries, blk_cap >= that); the EOF marker,
 * when asked for, lies at d_blk_off[n_blocks] and counts in *n_bytes.
 * d_rec_off (optional, NULL with n_rec == 0): the d_bam_off of bsw_bam_records*, n_rec + 1 offsets into d_in.
 * Then d_voff[i], i < n_rec, is the virtual offset of the record's first byte,
 *     (opt->base_coffset + d_blk_off[b]) << 16 | d_rec_off[i] - b * block_bytes,  b = d_rec_off[i] / block_bytes
 * (an offset of n_in on a cut names the end: b = n_blocks).
 * d_out has to be 4-byte aligned; no byte at or behind d_out + *n_bytes is written.
 * BSW_E_RANGE: blk_cap < *n_blocks + 1 (*n_blocks = the blocks; nothing is run); out_cap < *n_bytes (*n_bytes =
 *   what is needed; d_blk_off and d_voff are still written); a d_rec_off outside [0, n_in].
 * BSW_E_INVAL, before any device work: a null ctx / opt / n_blocks / n_bytes / d_blk_off, d_in with n_in > 0,
 *   d_out with out_cap > 0, d_rec_off or d_voff with n_rec > 0; a misaligned d_out; negative sizes; a
 *   block_bytes outside 1 .. BSW_BGZF_MAX_BLOCK; an unknown flag or level.
 * `stream`: a hipStream_t or NULL.  Returns when the blocks are in HBM. */
int bsw_bgzf_resident(bsw_ctx_t *ctx, const bsw_bgzf_opt_t *opt, const uint8_t *d_in, int64_t n_in,
                      const int64_t *d_rec_off, int32_t n_rec, uint8_t *d_out, int64_t out_cap, int64_t *d_blk_off,
                      int32_t blk_cap, int64_t *d_voff, int32_t *n_blocks, int64_t *n_bytes, void *stream);
/* The same with host arrays.  Blocking. */
int bsw_bgzf(bsw_ctx_t *ctx, const bsw_bgzf_opt_t *opt, const uint8_t *in, int64_t n_in, const int64_t *rec_off,
             int32_t n_rec, uint8_t *out, int64_t out_cap, int64_t *blk_off, int32_t blk_cap, int64_t *voff,
             int32_t *n_blocks, int64_t *n_bytes);

typedef struct bsw_bgzf_stats_t {    /* of the last bsw_bgzf* call                                    */
    int32_t n_blocks;
    int32_t n_stored, n_fixed, n_dynamic;   /* blocks of each form                                    */
    int64_t n_in, n_out;             /* bytes in; bytes out, the EOF marker included                  */
    float   deflate_ms;              /* staging clear, deflate kernel, scan, offsets (HIP events)     */
    float   pack_ms;                 /* compaction into d_out (HIP events)                            */
} bsw_bgzf_stats_t;
int bsw_bgzf_last_stats(bsw_ctx_t *ctx, bsw_bgzf_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BSW_BGZF_H */
