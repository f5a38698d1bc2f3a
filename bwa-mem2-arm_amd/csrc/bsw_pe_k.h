// bsw_pe_k.h -- launch interface of the paired-end kernels (bsw_pe.hip, include/bsw_pe.h).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/bsw_pe.h"
#include "bsw_sel_k.h"
#include "bsw_contig_seg.h"

namespace bsw {

struct PeDir {                          // one direction of pes[] as the kernels read it
    double avg, std;
    int32_t low, high, failed, pad;
};

struct PeParams {
    SelParams s;                        // a, b, gaps, min_seed_len, mapQ_coef_*, mask_level, l_pac, id0
    int32_t n_pairs, n_regs;
    int32_t max_ins, T, pen_unpaired, pad;
    PeDir pes[4];
    ContigView ctg;                     // off != nullptr: hits on different contigs are no pair (bsw_contig_seg.h)
};

// mem_pair's sort key with a contig table: upstream's rid << 32 | (position - offset) orders the hits as
// the global forward position does, and a rid change ends the distance scan.  The same order and the same
// end come from the global position moved apart by rid << kPeRidShift: bsw_set_contigs admits at most
// BSW_CONTIG_MAX_N = 2^22 contigs that sum to at most BSW_CONTIG_MAX_SUM = 2^39, so two hits on different
// contigs are more than 2^39 apart -- beyond any int32 `high` -- and the largest coordinate is below 2^63
constexpr int kPeRidShift = 40;

struct alignas(16) PeV {                // mem_pair's v entry
    int64_t x;
    uint64_t y;
};

// meta: kPeSlots slots of kPeMetaWords int32 (one 64-B line each), zeroed per call.  The outcome
// counters are spread over the slots by block (the host adds them up); kPeErr and kPeGeneral live
// in slot 0 alone; kPeNu is a 64-bit counter at an even word
constexpr int kPeErr = 0, kPeTried = 1, kPePaired = 2, kPeMulti = 3, kPeUnpaired = 4, kPeProper = 5, kPeGeneral = 6,
              kPeNu = 8, kPeMetaWords = 16, kPeSlots = 32;
constexpr int kPeFastBlock = 256, kPeFastPer = 4;       // pe_pair_fast_kernel: pairs per block = their product

// One work item per pair: cal_sub of both ends, infer_dir, the insert size into hist[dir *
// (max_ins + 1) + is] (zeroed first) through a per-block table in LDS; validation into meta[kPeErr].
hipError_t launch_pe_stat(const PeParams &p, const bsw_alnreg_t *regs, const int32_t *first, int32_t *hist,
                          int32_t *meta, hipStream_t s);
// One work item per pair: a pair with at most one region per end is finished here; the others are
// appended to list (count meta[kPeGeneral]) for launch_pe_pair_general, which reads the count on
// the device: work[n_regs], zbuf[n_regs] and v[n_regs] are flat, a read's at its first region.
hipError_t launch_pe_pair_fast(const PeParams &p, const bsw_alnreg_t *regs, bsw_selinfo_t *info, const int32_t *first,
                               bsw_pair_t *pairs, int32_t *list, int32_t *meta, hipStream_t s);
hipError_t launch_pe_pair_general(const PeParams &p, bsw_alnreg_t *regs, bsw_selinfo_t *info, const int32_t *first,
                                  bsw_pair_t *pairs, const int32_t *list, SelW *work, int32_t *zbuf, PeV *v,
                                  int32_t *meta, hipStream_t s);

}  // namespace bsw
