// bsw_sel_k.h -- launch interface of the region-selection kernels (bsw_sel.hip, include/bsw_sel.h).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/bsw_seqpair.h"
#include "../../include/bsw_sel.h"
#include "bsw_contig_seg.h"

namespace bsw {

struct SelParams {
    int32_t W, a, b;                    // opt->w, mat[0], opt->b
    int32_t o_del, e_del, o_ins, e_ins;
    int32_t n_reads, n_seeds;
    int32_t max_chain_gap, min_seed_len, mapQ_coef_len, mapQ_coef_fac, patch;
    float mask_level_redun, mask_level;
    int32_t qstride, tstride;           // per-job code-buffer strides (set after a round's step)
    int64_t ref_len, l_pac, id0;
    ContigView ctg;                     // off != nullptr: dedup and patch compare regions of one contig only
    int8_t mat[25];
};

struct alignas(16) SelW {             // one region of a read's work list (80 bytes)
    bsw_alnreg_t r;
    int32_t seedcov, sub, csub, sub_n, n_comp, secondary, src, mapq;
    uint64_t hash;
};

struct SelRd {                          // per read: the list's length and the suspended dedup loop
    int32_t n;
    int32_t i, j, w;                    // patch_reg(a[j], a[i]) waits for its score; w = its band
};

// meta words (one int32 array, zeroed per call)
constexpr int kSelErr = 0, kSelRegsIn = 1, kSelRedundant = 2, kSelIdentical = 3, kSelTried = 4, kSelOk = 5,
              kSelRatio = 6, kSelMaxQ = 7, kSelMaxT = 8, kSelCnt = 9 /* , 10: job counts (ping-pong) */,
              kSelMetaWords = 16;

// Per read: av in upstream's order with seedcov / csub into work[sbeg[r] ...], st[r].n; validation.
hipError_t launch_sel_gather(const SelParams &p, const int32_t *sbeg, const int32_t *send, const int32_t *read_len,
                             const bsw_seed_t *seeds, const int32_t *seed_chain, const bsw_alnreg_t *regs,
                             const int32_t *extended, const int32_t *csub, SelW *work, SelRd *st, int32_t *meta,
                             hipStream_t s);
// The dedup state machine.  list == nullptr: every read from the start (n = n_reads work items);
// else work item t resumes read list[t] with pairs[t].score.  A read that reaches a patch_reg past
// its cheap tests is appended to next (count *next_cnt) and left suspended; one that finishes the
// loop goes on through the drops, the sorts, primary marking and MAPQ, and leaves kept[r].
hipError_t launch_sel_step(const SelParams &p, const int32_t *list, int32_t n, const SeqPair *pairs,
                           const int32_t *sbeg, const uint8_t *reads, const int64_t *read_off, const float *frac_rep,
                           const uint8_t *ref, SelW *work, SelRd *st, int32_t *zbuf, int32_t *next,
                           int32_t *next_cnt, int32_t *kept, int32_t *meta, hipStream_t s);
// Jobs [0, nj) of list: SeqPair j (h0 = bsw_gen_cigar_band over the patch's band) and its query
// slice / reference span copied (reversed on the reverse strand) into the per-job strides.
hipError_t launch_sel_build(const SelParams &p, const int32_t *list, int32_t nj, const int32_t *sbeg,
                            const uint8_t *reads, const int64_t *read_off, const SelW *work, const SelRd *st,
                            const uint8_t *ref, SeqPair *pairs, uint8_t *qbuf, uint8_t *tbuf, hipStream_t s);
// The kept regions of every read, compact, to the caller's arrays (first = launch_scan32 of kept).
hipError_t launch_sel_emit(const SelParams &p, const int32_t *seed_read, const int32_t *sbeg, const int32_t *kept,
                           const int32_t *first, const SelW *work, const float *frac_rep, bsw_alnreg_t *sel_regs,
                           int32_t *sel_read, bsw_selinfo_t *sel_info, hipStream_t s);

}  // namespace bsw
