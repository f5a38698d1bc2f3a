// bsw_engine.h -- the host engine's shared types (not installed): the owners of GPU objects, a
// call's Slot, the per-device slot pool and the context, plus the functions that cross the
// engine's translation units:
//   bsw_dispatch.hip : plan_kernel, run_plan / run_dp / run_device, finish_stats
//   bsw_sort.hip     : sort_order, the batch-order radix sort (bsw_sort.h)
//   bsw_pipeline.hip : staging kernels, the chunked host pipeline (host_shard), cross-call coalescing
//                      (its planning -- staging layout, chunk schedule, kStageBlk -- in bsw_stage_plan.h)
//   bsw_host.cpp     : contexts, recovery, mate / global / extension wrappers, options, the core C ABI
//   bsw_stages.cpp   : the stages behind the extension (final alignments, region selection, the
//                      paired-end stage, mate rescue, SAM records, BGZF, BAM sort and index), both forms of each, on shared
//                      call helpers
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/bsw.h"
#include "../../include/bsw_mate.h"
#include "../../include/bsw_global.h"
#include "../../include/bsw_aln.h"
#include "../../include/bsw_sel.h"
#include "../../include/bsw_pe.h"
#include "../../include/bsw_matesw.h"
#include "../../include/bsw_rec.h"
#include "../../include/bsw_bam.h"
#include "../../include/bsw_bgzf.h"
#include "../../include/bsw_bamsort.h"
#include "../../include/bsw_markdup.h"
#include "../../include/bsw_contigs.h"
#include "bsw_contig_seg.h"
#include "bsw_kernels.h"
#include "bsw_internal.h"
#include "bsw_stage_plan.h"

// engine-internal names that cross translation units stay out of the library's dynamic symbols
#define BSW_HIDDEN __attribute__((visibility("hidden")))

namespace bsw {

constexpr int kMetaCounts = 16;             // class counters per slot (one 64-B line per slot)
constexpr int kMetaSpread = 32;             // slots: block b adds into slot b % 32 (no hot line)
constexpr int kMetaMaxq = kMetaCounts * kMetaSpread;   // d_meta: counts[32][16], maxq_wide, err
constexpr int kMetaErr = kMetaMaxq + 1;
constexpr int kMetaFlag = kMetaErr + 1;     // row-group kernel: a pair outside its contract
constexpr int kMetaCnt = kMetaFlag + 1;     // extension pipeline: band-retry count readback
constexpr int kMetaRedo = kMetaCnt + 1;     // packed-column classes: redo-list lengths (left prune), device only
constexpr int kMetaRedoWords = 5;
constexpr int kMetaWords = kMetaRedo + kMetaRedoWords;
constexpr int kKeyBits = 32;                // 4 class + 8 qlen + 1 related + 11 tlen + 8 h0 bits

static inline int hip_rc(hipError_t e)
{
    if (e == hipSuccess) return BSW_OK;
    if (e == hipErrorOutOfMemory) return BSW_E_NOMEM;
    return BSW_E_HIP;
}
#define BSW_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return ::bsw::hip_rc(_e); } while (0)

// BSW_OPT_TEST_FAIL_ALLOC: this many upcoming buffer growths fail as out of memory (tests of the
// host-buffer call's recovery, bsw.h); process-wide, 0 in production
BSW_HIDDEN bool inject_nomem();

// ---------------------------------------------------------------- owners (move-only)
// Each frees its object in its destructor and converts to the raw pointer / handle.  A Slot sets
// its device before its members go (Slot::~Slot).
template <class P, class Free>
struct BSW_HIDDEN Owned {
    P p = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
    Owned &operator=(Owned &&o) noexcept { std::swap(p, o.p); return *this; }
    ~Owned() { reset(); }
    void reset() { if (p) (void)Free()(p); p = nullptr; }
    operator P() const { return p; }
};
struct BSW_HIDDEN FreeDev { hipError_t operator()(void *p) const { return hipFree(p); } };
struct BSW_HIDDEN FreeHost { hipError_t operator()(void *p) const { return hipHostFree(p); } };
struct BSW_HIDDEN FreeStream { hipError_t operator()(hipStream_t s) const { return hipStreamDestroy(s); } };
struct BSW_HIDDEN FreeEvent { hipError_t operator()(hipEvent_t e) const { return hipEventDestroy(e); } };
using Stream = Owned<hipStream_t, FreeStream>;     // created in place: hipStreamCreate*(&s.p, ...)
using Event = Owned<hipEvent_t, FreeEvent>;

// device (Free = FreeDev) or pinned host (FreeHost) array of `cap` elements
template <class T, class Free>
struct BSW_HIDDEN Buf : Owned<T *, Free> {
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : Owned<T *, Free>(std::move(o)), cap(std::exchange(o.cap, 0)) {}
    Buf &operator=(Buf &&o) noexcept { std::swap(this->p, o.p); std::swap(cap, o.cap); return *this; }
    void reset() { Owned<T *, Free>::reset(); cap = 0; }
    // exactly n elements, whatever is held now (no failure injection)
    hipError_t reserve_exact(size_t n)
    {
        reset();
        hipError_t e;
        if constexpr (std::is_same<Free, FreeDev>::value) e = hipMalloc((void **)&this->p, n * sizeof(T));
        else e = hipHostMalloc((void **)&this->p, n * sizeof(T), 0);
        if (e == hipSuccess) cap = n;
        else this->p = nullptr;
        return e;
    }
    // at least `need` elements, contents not kept.  25% headroom: the pipeline's chunks vary (ramp, a
    // merged remainder up to 1.25x) and slots rotate between them, so exact-fit growth reallocated
    // on many calls (hipFree syncs the device)
    size_t grown(size_t need) const { return std::max(need + need / 4, cap * 3 / 2); }
};
template <class T>
struct BSW_HIDDEN DevBuf : Buf<T, FreeDev> {
    hipError_t grow(size_t need)
    {
        if (need <= this->cap) return hipSuccess;
        if (inject_nomem()) return hipErrorOutOfMemory;
        return this->reserve_exact(this->grown(need));
    }
};
template <class T>
struct BSW_HIDDEN PinnedBuf : Buf<T, FreeHost> {           // (growth is never injected)
    hipError_t grow(size_t need) { return need <= this->cap ? hipSuccess : this->reserve_exact(this->grown(need)); }
};

// one device call: run_plan's arguments, kept in the slot for run_dp
struct PlanCall {
    SeqPair *d_pairs = nullptr;
    const uint8_t *d_ref = nullptr, *d_qer = nullptr;
    int32_t n = 0, w = 0;
    int cell_bits = 16;
    hipStream_t stream = nullptr;
    hipStream_t dp_stream = nullptr;    // the DP kernels' stream when not `stream` (host pipeline:
                                        //   everything else of a chunk runs on the helper stream)
    hipStream_t plan_stream = nullptr;  // plan + sort stream when not the slot's pstream
    // row-group kernel contract as the host checked it: gq_maxq >= 0 = every pair fits (longest
    // query gq_maxq, longest target gq_maxt); -2 = not checked (the kernel flags misfits, run_dp
    // falls back to the planned path); -1 = some pair does not fit (planned path at once)
    int gq_maxq = -2, gq_maxt = 0;
    int32_t *d_out24 = nullptr;         // row-group kernel, host-checked batch: outputs as 6 x int32
                                        //   per pair here instead of into d_pairs
};

struct ExtState;
struct AlnState;
struct SelW;
struct SelRd;
struct PeV;
struct MswSt;
struct MswJob;
// Everything one call needs on one device.  Members are destroyed in reverse order: buffers, then
// events, then streams.
struct BSW_HIDDEN Slot {
    int device = 0;
    std::atomic<int> *ownq_n = nullptr; // `stream` has a hardware queue of its own: the device's count
                                        //   of such slots (DeviceCtx::acquire), given back with the slot
    static constexpr int kSide = 3;
    // class launches of one batch fork over side streams (independent pairs; small batches are
    // bound by the longest wave of each class, so classes run side by side instead of in turn)
    Stream side[kSide];
    Stream stream;
    Stream pstream;                     // high-priority stream of run_plan
    Event ev0, ev1;
    Event ev2, ev3;                     // mate rescue: the reverse pass
    Event evf, evj[kSide];
    Event evm;                          // class-count readback of the last run_plan
    Event evh;                          // inputs ready on the call's stream (pstream waits)
    Event evd;                          // host pipeline: a chunk's DP done (its outputs' readback waits)
    Event evq0, evq1;                   // duplicate marking: its mark group (the other groups: ev0 / ev1, ev2 / ev3, evw0 / evw1)
    Event evw0, evw1;                   // mate-rescue stage: its helper kernels (the batched ksw_align2 times itself with ev0..ev3)
    // device buffers (grown on demand)
    DevBuf<SeqPair> d_pairs;
    DevBuf<uint8_t> d_ref, d_qer;
    DevBuf<uint32_t> d_keys, d_keys2;   // radix sort: the four grow together (grow_sort), d_order.cap
    DevBuf<int32_t> d_vals, d_order;    //   is their shared capacity
                                        // (d_keys2 after the sort: the packed-column classes' redo lists, run_dp)
    DevBuf<uint8_t> d_tmp;
    DevBuf<int32_t> d_meta;             // counts[kMetaCounts], maxq_wide, err
    PinnedBuf<int32_t> h_meta;          // pinned mirror
    DevBuf<int2> d_scratch;
    // host-buffer pipeline: pinned staging of one chunk and its device copy
    PinnedBuf<uint8_t> h_stage;
    DevBuf<uint8_t> d_stage;
    DevBuf<int32_t> d_bkt;              // staged exceptions: first word per 4096 positions
    // mate rescue (bsw_mate.h)
    DevBuf<int32_t> d_mjobs;
    DevBuf<uint16_t> d_mrows;
    DevBuf<int32_t> d_mmeta;
    PinnedBuf<int32_t> h_mmeta;
    DevBuf<unsigned long long> d_mcells;
    DevBuf<SeqPair> d_mpairs;
    DevBuf<bsw_kswr_t> d_maln;
    // global alignment (bsw_global.h)
    DevBuf<uint32_t> d_gz;
    DevBuf<int32_t> d_gmeta;
    PinnedBuf<int32_t> h_gmeta;
    DevBuf<uint32_t> d_gcig;
    DevBuf<int32_t> d_gncig;
    DevBuf<int32_t> d_gretry;           // narrow-window traceback retries: count, list
    // device extension pipeline (bsw_ext_dev.hip)
    DevBuf<SeqPair> d_xpairs, d_xsub;
    DevBuf<uint8_t> d_xq, d_xt;
    DevBuf<ExtState> d_xst;
    DevBuf<int64_t> d_xwin;             // per-read target windows (ext_scan)
    // final alignments (bsw_aln.h)
    DevBuf<AlnState> d_ast;             // per-region band-loop state
    DevBuf<int32_t> d_alist;            // compact DP job lists of two passes (ping-pong), n_regs each
    DevBuf<int32_t> d_acnt;             // their job counts
    DevBuf<SeqPair> d_apairs;
    DevBuf<uint8_t> d_aq, d_at;         // per-job query / reference codes
    DevBuf<uint8_t> d_aio;              // host form: the staged inputs and outputs
    // region selection (bsw_sel.h); its DP jobs use d_apairs / d_aq / d_at, its host form d_aio
    DevBuf<SelW> d_swork;               // per-read work lists, flat: a read's list at its first seed slot
    DevBuf<SelRd> d_sst;                // per-read list length and suspended loop
    DevBuf<int32_t> d_sz;               // primary marking's z lists (flat, as d_swork)
    DevBuf<int32_t> d_srun;             // sbeg[n_reads], send[n_reads]
    DevBuf<int32_t> d_skept;            // kept counts, n_reads + 1
    DevBuf<int32_t> d_slist;            // suspended reads of two rounds (ping-pong), n_reads each
    DevBuf<int32_t> d_smeta;            // kSelMetaWords
    // paired-end stage (bsw_pe.h); its general path marks in d_swork / d_sz, its host forms stage in d_aio
    DevBuf<int32_t> d_phist;            // insert-size counts, 4 x (max_ins + 1)
    DevBuf<int32_t> d_pmeta;            // kPeMetaWords
    DevBuf<int32_t> d_plist;            // pairs of the general path, n_pairs
    DevBuf<PeV> d_pv;                   // mem_pair's v (flat, a pair's at its first region)
    // mate-rescue stage (bsw_matesw.h); its work lists are d_swork, its jobs d_apairs / d_aq / d_at and
    // d_maln, its scans use d_tmp, its host form stages in d_aio
    DevBuf<int32_t> d_wint;             // ncand, capv, coff, woff, nlist (n_reads + 1 each), two pair lists
    DevBuf<int64_t> d_wcand;            // the candidates' rb, copied before any rescue
    DevBuf<MswSt> d_wst;                // per pair: cursor and pending call
    DevBuf<MswJob> d_wjobs;             // a round's jobs, at most 4 per pair
    DevBuf<int32_t> d_wmeta;            // kMswSlots x kMswMetaWords
    // record stage (bsw_rec.h); its alignments are reg2aln_device's on the same lease (the final-alignment
    // buffers above), its scans use d_tmp, its host forms stage in d_aio, its helper kernels are timed with
    // evw0 / evw1
    DevBuf<int32_t> d_rcnt;             // nrec, naln, aln_first: n_reads + 1 each
    DevBuf<bsw_alnreg_t> d_rregs;       // the needed regions, compact
    DevBuf<int32_t> d_rread;            // their reads
    DevBuf<int64_t> d_rlen;             // text: the lines' lengths, n_rec + 1
    DevBuf<int32_t> d_rmeta;            // kRecMetaWords
    // BGZF (bsw_bgzf.h); its scan uses d_tmp, its host form stages in d_aio, its kernels are timed with evw0 / evw1
    DevBuf<uint8_t> d_bstage;           // the blocks as compressed, 64 KB each
    DevBuf<uint16_t> d_btok;            // the deflate kernel's tokens, per workgroup
    DevBuf<int64_t> d_bsize;            // the blocks' sizes, n_blocks + 1
    DevBuf<int32_t> d_bmeta;            // kBgzfMetaWords
    // BAM sort and index (bsw_bamsort.h); the sorted lengths are d_rlen, scans and radix sorts use d_tmp, the host
    // forms stage in d_aio, the kernels are timed with evw0 / evw1
    DevBuf<uint64_t> d_qkey;            // keys in and out of the radix sort, 2 n_rec
    DevBuf<int32_t> d_qval;             // values likewise (the sort's output values are the caller's d_perm)
    DevBuf<int32_t> d_qints;            // sort: the output tiles' first records; index: kBiIntArrays arrays of n_rec + 1
    DevBuf<uint32_t> d_qref;            // index: kBiRefWords per reference
    DevBuf<uint32_t> d_qlin;            // index: the flat linear index, sum((ref_len + 16383) >> 14) entries
    DevBuf<int64_t> d_qref64;           // index: win_off, ref_size, ref_off (n_ref + 1 each), then ref_len
    DevBuf<int32_t> d_qmeta;            // kBsMetaWords / kBiMetaWords
    // duplicate marking (bsw_markdup.h); scans and radix sorts use d_tmp, the host form stages in d_aio, the kernel
    // groups are timed with ev0 / ev1, ev2 / ev3, evw0 / evw1 and evq0 / evq1
    DevBuf<uint64_t> d_dwords;          // end words, key words, the sorts' keys in and out
    DevBuf<int32_t> d_dints;            // scores, flags, scans, compact indices, the sorts' values, set heads; the marks
    DevBuf<int32_t> d_dmeta;            // kMdMetaWords
    bool timed = false;
    hipStream_t run_stream = nullptr;   // stream of the last run_device (finish_stats waits on it)
    bsw_stats_t stats{};
    PlanCall plan;                      // arguments of the last run_plan (run_dp's input)
    int fast = 0;                       // last run_plan launched the row-group kernel: 2 = host-
                                        //   checked batch, 1 = kernel-checked (flag read back)
    ~Slot()
    {
        if (ownq_n) ownq_n->fetch_sub(1);
        (void)hipSetDevice(device);
    }
};

struct AggReq;
struct DeviceCtx {
    int device = 0;
    std::atomic<int> inflight{0};       // host-buffer calls running on this logical device
    // cross-call coalescing (coalesced_call): small host-buffer calls queue here; up to
    // agg_leaders_max of their threads at a time each run everything queued as ONE batch
    std::mutex agg_mu;
    std::condition_variable agg_cv;
    std::deque<AggReq *> agg_q;
    int64_t agg_qn = 0;                 // pairs queued in agg_q
    int64_t agg_run = 0;                // pairs in the batches on the device
    int agg_nrun = 0;                   // batches on the device
    int agg_inside = 0;                 // callers inside coalesced_call
    int agg_lingering = 0;              // leaders waiting for a deeper queue
    int agg_leaders = 0;
    int agg_leaders_max = 4;            // BSW_OPT_COALESCE_LEADERS
    int agg_linger_us = 20;             // BSW_OPT_COALESCE_LINGER (20 us since round 6: 8 callers x 1K
                                        //   +15-30%, 16 equal or better, <= 4 never linger)
    std::atomic<int> ownq_n{0};         // slots whose stream got a hardware queue of its own (acquire)
    std::atomic<bool> copies_warm{false};   // host_shard's copy-engine warm-up ran (prime_copies)
    std::mutex mu;
    std::vector<std::unique_ptr<Slot>> free_slots;
    DevBuf<uint8_t> d_refres;           // resident reference (bsw_set_reference)
    int64_t refres_len = -1;
    std::shared_mutex refmu;            // extension calls hold it shared while they use d_refres
    // the contig table (bsw_set_contigs), under refmu like the reference; n_ctg == 0: none
    DevBuf<int64_t> d_ctg_off;          // [n_ctg + 1] prefix sums
    DevBuf<uint8_t> d_ctg_names;
    DevBuf<int32_t> d_ctg_name_off;     // [n_ctg + 1]
    int32_t n_ctg = 0;
    int64_t ctg_sum = 0;
    std::vector<int64_t> h_ctg_off;     // the prefix sums on the host (the host window builder, bsw_ext.cpp)
    std::vector<uint8_t> h_ctg_names;   // the names and their offsets on the host (bsw_bam_header)
    std::vector<int32_t> h_ctg_name_off;

    // the table fits a call that names l_pac (0: a one-strand reference of refres_len bases)
    bool ctg_ok(int64_t l_pac) const { return n_ctg == 0 || ctg_sum == (l_pac > 0 ? l_pac : refres_len); }
    ContigView ctg_view(int64_t l_pac) const
    {
        if (n_ctg == 0) return ContigView{nullptr, nullptr, nullptr, 0, l_pac};
        return ContigView{d_ctg_off.p, d_ctg_names.p, d_ctg_name_off.p, n_ctg, l_pac};
    }

    ~DeviceCtx() { (void)hipSetDevice(device); }        // (for d_refres; slots set it themselves)
    // A failed acquire destroys the half-made slot: what it had created is released and its
    // ownq_n reservation returned (Slot::~Slot)
    std::unique_ptr<Slot> acquire(int &rc)
    {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!free_slots.empty()) {
                auto s = std::move(free_slots.back());
                free_slots.pop_back();
                rc = BSW_OK;
                return s;
            }
        }
        auto s = std::make_unique<Slot>();
        s->device = device;
        rc = hip_rc(hipSetDevice(device));
        if (rc) return nullptr;
        // The slot's stream through a CU mask of EVERY CU: a masked stream gets a hardware queue of its
        // own, so concurrent kt_for-sized calls do not share the runtime's four queues
        // (GPU_MAX_HW_QUEUES) and serialise their kernels behind each other.  Measured (percall_bench,
        // 8 C++ callers, same box x2, profiles/r05/slot_ownq_percall.txt): 1K pairs per call without
        // coalescing 9.4-9.5 -> 10.7-11.0 M/s, 4K 30.4-30.8 -> 34.7-34.9, 10K 40.5-40.9 -> 42.1-42.5;
        // 1M-pair host calls unchanged.  The first 16 slots of a device.
        // A CU-masked stream is a BLOCKING stream (hipExtStreamCreateWithCUMask takes no flags): it
        // orders against the legacy null stream.  The library itself issues nothing on the null
        // stream (its copies run on non-blocking streams of its own: bsw_set_reference, the FM-index
        // build); a caller's own null-stream work waits for, and is waited on by, these slots'
        // kernels ("Streams")
        bool made = false;
        if (ownq_n.fetch_add(1) < 16) {
            hipDeviceProp_t pr;
            if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0 &&
                pr.multiProcessorCount <= 1024) {
                uint32_t m[32] = {};
                const int ncu = pr.multiProcessorCount;
                for (int c = 0; c < ncu; ++c) m[c / 32] |= 1u << (c % 32);
                made = hipExtStreamCreateWithCUMask(&s->stream.p, (uint32_t)((ncu + 31) / 32), m) == hipSuccess;
            }
            if (made) s->ownq_n = &ownq_n;
            else ownq_n.fetch_sub(1);
        } else {
            ownq_n.fetch_sub(1);
        }
        if (!made && (rc = hip_rc(hipStreamCreateWithFlags(&s->stream.p, hipStreamNonBlocking)))) return nullptr;
        if ((rc = hip_rc(hipEventCreate(&s->ev0.p)))) return nullptr;
        if ((rc = hip_rc(hipEventCreate(&s->ev1.p)))) return nullptr;
        if ((rc = hip_rc(s->d_meta.reserve_exact(kMetaWords)))) return nullptr;
        if ((rc = hip_rc(s->h_meta.reserve_exact(kMetaWords)))) return nullptr;
        return s;
    }
    // free every cached slot (streams, events, device and pinned buffers): the first step of a
    // failed call's recovery (scores_eb), so its rerun allocates afresh.  Slots other calls hold
    // are untouched; they come back to the pool as usual
    void trim()
    {
        std::vector<std::unique_ptr<Slot>> v;       // (its slots are destroyed outside the lock)
        {
            std::lock_guard<std::mutex> g(mu);
            v.swap(free_slots);
        }
    }
    // rc != 0: the call failed part-way and may have left work queued on the slot's streams
    // (or the caller's stream it ran on) that still reads or writes the slot's buffers -- drain
    // it before another call can take the slot
    void give_back(std::unique_ptr<Slot> s, int rc = 0)
    {
        if (rc) {
            (void)hipSetDevice(s->device);
            const hipStream_t sts[] = {s->stream, s->pstream, s->run_stream, s->side[0], s->side[1], s->side[2]};
            for (hipStream_t st : sts)
                if (st) (void)hipStreamSynchronize(st);
        }
        std::lock_guard<std::mutex> g(mu);
        free_slots.push_back(std::move(s));
    }
};

// A call's lease of one slot: take it, set the device, run body(slot), hand the slot back with
// the body's status (a failed body's queued work is drained first, DeviceCtx::give_back).
template <class F>
static inline int with_slot(DeviceCtx &dc, F &&body)
{
    int rc = BSW_OK;
    auto slot = dc.acquire(rc);
    if (!slot) return rc;
    rc = hip_rc(hipSetDevice(dc.device));
    if (!rc) rc = body(*slot);
    dc.give_back(std::move(slot), rc);
    return rc;
}

// ---- bsw_dispatch.hip (sort_order: bsw_sort.h)
BSW_HIDDEN void make_kparams(const bsw_params_t &p, KParams &kp);
BSW_HIDDEN hipError_t grow_sort(Slot &s, int32_t n);
BSW_HIDDEN int ensure_pstream(Slot &s);
BSW_HIDDEN int run_plan(const KParams &kp, Slot &s, const PlanCall &pc);
BSW_HIDDEN int run_dp(const KParams &kp, Slot &s);
BSW_HIDDEN int run_device(const KParams &kp, Slot &s, SeqPair *d_pairs, const uint8_t *d_ref, const uint8_t *d_qer,
                          int32_t n, int32_t w, int cell_bits, hipStream_t stream);
BSW_HIDDEN int finish_stats(Slot &s, bool spin = false);
// ---- bsw_pipeline.hip
BSW_HIDDEN int launch_stage_in(Slot &s, hipStream_t st, const uint8_t *ref2, int64_t r_tot, const uint8_t *qer2,
                               int64_t q_tot, const uint32_t *exc, int32_t n_r, int32_t ne, const PairIn *pin,
                               int32_t n, uint8_t *ref, uint8_t *qer, SeqPair *pairs, int32_t *zero2);
BSW_HIDDEN int launch_gather_outputs(const SeqPair *d_pairs, int32_t *d_out, int32_t n, hipStream_t st);
BSW_HIDDEN int host_shard(const KParams &kp, DeviceCtx &dc, SeqPair *pairs, const uint8_t *ref, const uint8_t *qer,
                          int32_t n, int32_t w, int cell_bits, int32_t chunk, bool two_bit, bsw_stats_t *st);
BSW_HIDDEN int coalesced_call(const KParams &kp, DeviceCtx &dc, SeqPair *pairs, const uint8_t *ref,
                              const uint8_t *qer, int32_t n, int32_t w, int cell_bits, int32_t chunk, bool two_bit,
                              bsw_stats_t *st);
// ---- bsw_host.cpp
struct MateParams;
struct GlobParams;
BSW_HIDDEN void make_mate_params(const bsw_params_t &p, MateParams &mp);
BSW_HIDDEN bool mate_params_ok(const bsw_params_t &p);
BSW_HIDDEN int mate_device(const MateParams &mp, Slot &s, const SeqPair *d_pairs, const uint8_t *d_ref,
                           const uint8_t *d_qer, int32_t n, bsw_kswr_t *d_aln, hipStream_t st, bsw_mate_stats_t *stats);
BSW_HIDDEN void make_glob_params(const bsw_params_t &p, int prefer_band, GlobParams &gp);
BSW_HIDDEN int glob_device(const GlobParams &gp, Slot &s, SeqPair *d_pairs, const uint8_t *d_ref, const uint8_t *d_qer,
                           int32_t n, uint32_t *d_cigar, int32_t stride, int32_t *d_ncig, hipStream_t st,
                           bsw_global_stats_t *stats);

}  // namespace bsw

struct bsw_ctx {
    bsw_params_t params;
    bsw::KParams kp;
    std::vector<std::unique_ptr<bsw::DeviceCtx>> devs;
    std::mutex stats_mu;
    bsw_stats_t last{};
    bsw_ext_stats_t ext_last{};
    bsw_chain_stats_t chain_last{};
    bsw_mate_stats_t mate_last{};
    bsw_global_stats_t glob_last{};
    bsw_aln_stats_t aln_last{};
    bsw_sel_stats_t sel_last{};
    bsw_pe_stats_t pe_last{};
    bsw_matesw_stats_t matesw_last{};
    bsw_rec_stats_t rec_last{};
    bsw_bam_stats_t bam_last{};
    bsw_bgzf_stats_t bgzf_last{};
    bsw_bamsort_stats_t bamsort_last{};
    bsw_markdup_stats_t markdup_last{};
    struct Pinned { std::mutex mu; bsw::PinnedBuf<uint8_t> b; } pin[2];
    int glob_band = 0;                  // BSW_OPT_GLOB_BAND
    int64_t ext_chunk = 0;              // BSW_OPT_EXT_CHUNK (0: the int32-offset bound)
    int32_t host_chunk = 196608;        // BSW_OPT_HOST_CHUNK: pairs per host-buffer pipeline chunk (round 6:
                                        //   48 blocks beat 64 by 3-4% per 1M-pair call on two boxes,
                                        //   profiles/r06/host_chunk_sweep.txt)
    int host_pack = 2;                  // BSW_OPT_HOST_PACK: 2-bit (2) or nibble (4) staging
    int64_t split_min = 131072;         // BSW_OPT_SPLIT_MIN: smaller calls go whole to one device
    int32_t coalesce = 8192;            // BSW_OPT_COALESCE: calls of <= this many pairs coalesce
    std::atomic<unsigned> rr{0};        // tie-break rotation of the one-device pick
};

namespace bsw {
// a call's stats into / out of the context's x_last member (every bsw_*_last_stats and its setter)
template <class T>
static inline void put_stats(bsw_ctx *ctx, T bsw_ctx::*last, const T &v)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->*last = v;
}
template <class T>
static inline int get_stats(bsw_ctx *ctx, T bsw_ctx::*last, T *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->*last;
    return BSW_OK;
}
}  // namespace bsw
