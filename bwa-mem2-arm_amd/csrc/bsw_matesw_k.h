// bsw_matesw_k.h -- launch interface of the mate-rescue stage's kernels (bsw_matesw.hip,
// include/bsw_matesw.h).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/bsw_seqpair.h"
#include "../../include/bsw_matesw.h"
#include "bsw_sel_k.h"
#include "bsw_contig_seg.h"

namespace bsw {

struct MswDir {                         // one direction of pes[] as the kernels read it
    int32_t low, high, failed, pad;
};

struct MswParams {
    SelParams s;                        // the dedup's: max_chain_gap, mask_level_redun, patch = 0; a, min_seed_len, l_pac
    int32_t n_pairs, n_regs;
    int32_t max_matesw, pen_unpaired;
    int32_t qstride, tstride;           // per-job code-buffer strides (set after a round's plan)
    MswDir pes[4];
    ContigView ctg;                     // off != nullptr: windows are clipped to the midpoint's segment (bsw_contig_seg.h)
};

struct MswSt {                          // per pair: the call its cursor stands at
    int32_t e, j;                       // end and candidate of the call; e == 2: finished
    int32_t jbase;                      // first job of the call in the round's job list
    int32_t mask;                       // bits 0..3: directions whose job ran; bits 4..7: directions not skipped
};

struct MswJob {                         // one ksw_align2 job of a round
    int64_t rb;                         // window [rb, rb + len) of the resident text
    int32_t len, read, rev, pad;        // the mate read; rev: its reverse complement is the query
};

// meta: kMswSlots slots of kMswMetaWords int32 (one 64-B line each), zeroed per call.  The outcome
// counters are spread over the slots by block (the host adds them up); kMswRedundant and
// kMswIdentical sit where the shared dedup (bsw_sel_dev.h) counts them.  kMswErr and the round's
// words (zeroed again per round) live in slot 0 alone.
constexpr int kMswErr = 0, kMswCalls = 1, kMswRedundant = 2, kMswIdentical = 3, kMswAllSkipped = 4, kMswJobs = 5,
              kMswJobsU8 = 6, kMswShort = 7, kMswPushed = 8, kMswChanged = 9,
              kMswNext = 10, kMswNJobs = 11, kMswMaxT = 12, kMswMaxQ = 13, kMswMetaWords = 16, kMswSlots = 32;
static_assert(kMswRedundant == kSelRedundant && kMswIdentical == kSelIdentical, "the shared dedup's counters");

// One work item per pair: d_read_first and every rb checked (meta[kMswErr]); ncand[r] = min(|b[r]|,
// max_matesw); capv[r] = read r's list length + 4 * ncand[its mate].  Both arrays hold n_reads + 1
// words, zeroed first.
hipError_t launch_msw_count(const MswParams &p, const bsw_alnreg_t *regs, const int32_t *first, int32_t *ncand,
                            int32_t *capv, int32_t *meta, hipStream_t s);
// One work item per pair.  list == nullptr: every pair, its lists copied into work[] at woff[r], its
// candidates' rb into cand[] at coff[r], the cursor at the first call.  Else work item t resumes pair
// list[t]: the results aln[jbase ...] of its pending call are applied (insert, dedup) and the cursor
// moves on.  Either way the pair then advances to its next call that has a job: the call's jobs go to
// jobs[] (count meta[kMswNJobs]), the pair to next[] (count meta[kMswNext]); a pair that reaches the
// end of its calls is finished.  nlist[r] = the current length of read r's list.
hipError_t launch_msw_step(const MswParams &p, const int32_t *list, int32_t n_items, const bsw_alnreg_t *regs,
                           const bsw_selinfo_t *info, const int32_t *first, const int32_t *read_len,
                           const int32_t *ncand, const int32_t *coff, const int32_t *woff, int64_t *cand, SelW *work,
                           int32_t *nlist, MswSt *st, const bsw_kswr_t *aln, MswJob *jobs, int32_t *next,
                           int32_t *meta, hipStream_t s);
// Jobs [0, nj) of jobs: SeqPair j (h0 = xtra) and the query (the read, or its reverse complement) /
// the window of the resident text copied into the per-job strides.
hipError_t launch_msw_build(const MswParams &p, const MswJob *jobs, int32_t nj, const uint8_t *reads,
                            const int64_t *read_off, const int32_t *read_len, const uint8_t *ref, SeqPair *pairs,
                            uint8_t *qbuf, uint8_t *tbuf, hipStream_t s);
// The lists, compact, to the caller's arrays (out_first = the scan of nlist).
hipError_t launch_msw_emit(const MswParams &p, const int32_t *woff, const int32_t *nlist, const int32_t *out_first,
                           const SelW *work, bsw_alnreg_t *out_regs, int32_t *out_read, bsw_selinfo_t *out_info,
                           hipStream_t s);

}  // namespace bsw
