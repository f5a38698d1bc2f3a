// bsw_rec_k.h -- launch interface of the record-stage kernels (bsw_rec.hip, include/bsw_rec.h).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/bsw_rec.h"
#include "../../include/bsw_bam.h"
#include "bsw_contig_seg.h"

namespace bsw {

struct RecParams {
    int32_t n_reads, n_regs;
    int32_t T, max_XA_hits, flags;
    float mask_level;
    double xa_ratio;                    // (double)opt->XA_drop_ratio
};

struct RecLists {                       // the lists of one call, either form
    const bsw_alnreg_t *regs;
    const bsw_selinfo_t *info;
    const int32_t *first;
    const bsw_pair_t *pairs;            // nullptr: single-end
};

struct RecText {                        // call 2's arrays and options
    const bsw_rec_t *recs;
    const int32_t *rec_first;
    const bsw_aln_t *aln;
    const uint32_t *cigar;
    const uint8_t *md;
    const uint8_t *reads, *names, *quals;
    const uint8_t *rname;               // opt->rname in device memory (a by-value array would live in scratch)
    const int64_t *read_off, *name_off;
    const int32_t *read_len;
    int32_t n_rec, n_aln, n_reads, n_names, cigar_stride, md_stride, paired, flags, rname_len;
    ContigView ctg;                     // off != nullptr: names and relative positions from the table, rname unread
};

// meta words (one int32 array, zeroed per call); the counters are added once per block
constexpr int kRecErr = 0, kRecUnmapped = 1, kRecSupp = 2, kRecXa = 3, kRecOverflow = 4, kRecRejected = 5,
              kRecMetaWords = 16,
              kRecNameWords = (BSW_REC_MAX_RNAME + 1) / 4;   // opt->rname, behind the meta words
#ifndef BSW_REC_TEXT_GROUP
#define BSW_REC_TEXT_GROUP 4            // measured: 4 / 8 / 16 / 32 / 64 lanes (`make abrec AB_FLAGS=-DBSW_REC_TEXT_GROUP=N`)
#endif
constexpr int kRecTextGroup = BSW_REC_TEXT_GROUP;       // lanes per record in the write kernel
constexpr int kRecTextBlock = 256;      // its block: 256 / kRecTextGroup records, consecutive in the text
static_assert(kRecTextGroup >= 4 && 64 % kRecTextGroup == 0, "a group is lanes of one wave, four of them take the edge bytes");
#ifndef BSW_REC_BAM_GROUP
#define BSW_REC_BAM_GROUP 4             // measured: 4 / 8 / 16 lanes gave write_ms 1.02 / 1.15 / 1.58 (`make abrec AB_FLAGS=-DBSW_REC_BAM_GROUP=N`)
#endif
constexpr int kRecBamGroup = BSW_REC_BAM_GROUP;         // lanes per record in the BAM write kernel, same block
static_assert(kRecBamGroup >= 4 && 64 % kRecBamGroup == 0, "a group is lanes of one wave, four of them take the edge bytes");

// One work item per read.  Count pass: nrec[r] and naln[r] (nrec[n_reads] = naln[n_reads] = 0),
// validation into meta[kRecErr].  Fill pass (rec_first / aln_first = their exclusive scans): the
// records but for what cross-linking gives, aln_reg, and the needed regions compact in creg /
// creg_read for the alignment stage.
hipError_t launch_rec_count(const RecParams &p, const RecLists &l, int32_t *nrec, int32_t *naln, int32_t *meta,
                            hipStream_t s);
hipError_t launch_rec_fill(const RecParams &p, const RecLists &l, const int32_t *rec_first, const int32_t *aln_first,
                           bsw_rec_t *recs, int32_t *aln_reg, bsw_alnreg_t *creg, int32_t *creg_read, hipStream_t s);
// One work item per record and per alignment: cross-linking, TLEN, the printed flag; rejected and
// overflowing alignments and the stage's counters into meta.  With a contig table TLEN stays 0
// unless pos and mpos lie in one contig.
hipError_t launch_rec_finish(const RecLists &l, const ContigView &ctg, const int32_t *rec_first, bsw_rec_t *recs,
                             int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                             int32_t n_aln, int32_t *meta, hipStream_t s);
// len[i] = the bytes of record i's line (len[n_rec] = 0); validation into meta[kRecErr]
hipError_t launch_rec_text_len(const RecText &t, int64_t *len, int32_t *meta, hipStream_t s);
// the lines at text + text_off[i]; text is 4-byte aligned
hipError_t launch_rec_text_write(const RecText &t, const int64_t *text_off, uint8_t *text, hipStream_t s);
// the same two passes for BAM alignment blocks (include/bsw_bam.h): len[i] = the bytes of record i's block,
// validation (the text's and what the binary fields cannot hold) into meta[kRecErr]; the blocks at
// bam + bam_off[i], bam 4-byte aligned, no byte at or behind bam + bam_off[n_rec] written
hipError_t launch_rec_bam_len(const RecText &t, int64_t *len, int32_t *meta, hipStream_t s);
hipError_t launch_rec_bam_write(const RecText &t, const int64_t *bam_off, uint8_t *bam, hipStream_t s);

}  // namespace bsw
