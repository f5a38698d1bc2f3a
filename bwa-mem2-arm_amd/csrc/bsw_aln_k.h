// bsw_aln_k.h -- launch interface of the final-alignment kernels (bsw_aln.hip, include/bsw_aln.h).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/bsw_seqpair.h"
#include "../../include/bsw_aln.h"
#include "bsw_contig_seg.h"

namespace bsw {

struct AlnParams {
    int32_t W, a;                       // opt->w, mat[0]
    int32_t o_del, e_del, o_ins, e_ins;
    int32_t n_reads;
    int32_t cigar_stride, md_stride;    // the caller's (md_stride 0: no MD)
    int32_t qstride, tstride;           // per-job code-buffer strides (set after the plan)
    int64_t ref_len, l_pac;
    ContigView ctg;                     // off == nullptr: no table, the reject test is the l_pac one
    int8_t mat[25];
};

struct AlnState {                       // per region, between the passes
    int32_t w2;                         // w_ of the pass to run (already min(w2, W << 2))
    int32_t last_sc;
    int32_t n_pass;                     // passes run so far
    int32_t kind;                       // kAln*
};
constexpr int kAlnRejected = 0, kAlnGapFree = 1, kAlnDP = 2;

// plan meta, as ext_scan's: meta[slot * 16 + k], slot = block % kAlnMetaSpread; k = 0 input
// error, 1 rejected, 2 gap-free, 3 longest DP query, 4 longest DP reference span
constexpr int kAlnMetaSpread = 32;
constexpr int kAlnCntWords = 4;         // cnt[p]: jobs in pass p's list

// Per region: validation, reject test, infer_bw and the first pass's w_ into st[]; rejected
// regions are finished here; DP regions are appended to list0 (count in cnt[0]).
hipError_t launch_aln_plan(const AlnParams &p, const int32_t *read_len, const bsw_alnreg_t *regs,
                           const int32_t *reg_read, int32_t n, AlnState *st, int32_t *list0, int32_t *cnt,
                           int32_t *meta, bsw_aln_t *aln, hipStream_t s);
// Gap-free regions (st[].kind == kAlnGapFree): score, NM, MD, CIGAR and pos straight from the
// read and the resident text, 16 lanes per region.
hipError_t launch_aln_gapfree(const AlnParams &p, const uint8_t *reads, const int64_t *read_off,
                              const int32_t *read_len, const bsw_alnreg_t *regs, const int32_t *reg_read, int32_t n,
                              const AlnState *st, const uint8_t *ref, bsw_aln_t *aln, uint32_t *cigar, uint8_t *md,
                              hipStream_t s);
// Jobs [0, nj) of list: SeqPair j (h0 = bsw_gen_cigar_band) and its query slice / reference span
// copied (reversed on the reverse strand) to qbuf + j * qstride / tbuf + j * tstride.
hipError_t launch_aln_build(const AlnParams &p, const uint8_t *reads, const int64_t *read_off,
                            const bsw_alnreg_t *regs, const int32_t *reg_read, const AlnState *st,
                            const int32_t *list, int32_t nj, const uint8_t *ref, SeqPair *pairs, uint8_t *qbuf,
                            uint8_t *tbuf, hipStream_t s);
// After the DP of jobs [0, nj): the band loop's decision per job; regions that go round again are
// appended to next (count *next_cnt) with the doubled w_, the others are finished (NM / MD walk,
// deletion squeeze, clips, pos) into the caller's arrays.
hipError_t launch_aln_finish(const AlnParams &p, const int32_t *read_len, const bsw_alnreg_t *regs,
                             const int32_t *reg_read, AlnState *st, const int32_t *list, int32_t nj,
                             const SeqPair *pairs, const uint8_t *qbuf, const uint8_t *tbuf, const uint32_t *jcigar,
                             const int32_t *jncig, int32_t *next, int32_t *next_cnt, bsw_aln_t *aln, uint32_t *cigar,
                             uint8_t *md, hipStream_t s);

}  // namespace bsw
