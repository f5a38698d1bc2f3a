// bsw_host.cpp -- host engine behind the C ABI (include/bsw.h): contexts, the multi-device
// policy and recovery of host-buffer calls, the mate-rescue, global-alignment and extension
// wrappers, options and stats.  (Layout of the engine: bsw_engine.h.)
//
// Replaces upstream BandedPairWiseSW's batch wrapper (smithWatermanBatchWrapper16/8:
// sort -> pad -> AoS->SoA -> kernel -> write back; SURVEY.md §3.2,
// docs-archive/WEEK1_WRAPPER_COMPLETE.md:27-118) with an MI355X pipeline that keeps the
// upstream AoS layout in HBM and does the "transpose" implicitly (one lane per pair;
// bsw_dispatch.hip).
//
// Concurrency: upstream calls getScores* from kt_for workers; every call here takes a Slot
// (own HIP stream + device buffers) from a per-device pool, so calls are reentrant.
// Host-buffer calls on an n_gpus context shard the batch by contiguous pair ranges across
// devices (one host thread per device) -- pairs are independent.
// Errors are returned as BSW_E* codes; there is no CPU path in this library.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <vector>
#include "bsw_engine.h"
#include "bsw_mate_k.h"
#include "bsw_global_k.h"
#include "bsw_ext_k.h"
#include "bsw_aln_k.h"
#include "bsw_sel_k.h"
#include "bsw_pe_k.h"
#include "bsw_matesw_k.h"

namespace bsw {

// BSW_OPT_TEST_FAIL_ALLOC (bsw_engine.h, inject_nomem)
static std::atomic<int> g_fail_alloc{0};
bool inject_nomem()
{
    int v = g_fail_alloc.load(std::memory_order_relaxed);
    while (v > 0)
        if (g_fail_alloc.compare_exchange_weak(v, v - 1)) return true;
    return false;
}

// ---------------------------------------------------------------- mate rescue (bsw_mate.h)
static void make_mate_params(const bsw_params_t &p, MateParams &mp)
{
    memset(&mp, 0, sizeof(mp));
    mp.e_del = p.e_del; mp.oe_del = p.o_del + p.e_del;
    mp.e_ins = p.e_ins; mp.oe_ins = p.o_ins + p.e_ins;
    int mn = 127, mx = 0;                                 // ksw_qinit: min(mat, 127), max(mat, 0)
    for (int i = 0; i < 25; ++i) { mn = std::min(mn, (int)p.mat[i]); mx = std::max(mx, (int)p.mat[i]); }
    mp.maxsc = mx;
    mp.shift = (uint8_t)(256 - (uint8_t)(int8_t)mn);
    for (int t = 0; t < 5; ++t) {
        uint8_t b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = 0; q < 5; ++q) b[q] = (uint8_t)p.mat[t * 5 + q];
        memcpy(mp.prof[t], b, 8);
    }
}

static bool mate_params_ok(const bsw_params_t &p)
{
    int mx = 0;
    for (int i = 0; i < 25; ++i) mx = std::max(mx, (int)p.mat[i]);
    return p.o_ins >= 1 && mx >= 1;
}

// Forward pass (ksw_u8 / ksw_i16 per job) then, for jobs with KSW_XSTART, the reverse pass;
// each pass: device bucketing by (P, slen), one readback of the bucket ranges, one launch per
// ncol class.  Blocking.
static int mate_device(const MateParams &mp, Slot &s, const SeqPair *d_pairs, const uint8_t *d_ref,
                       const uint8_t *d_qer, int32_t n, bsw_kswr_t *d_aln, hipStream_t st,
                       bsw_mate_stats_t *stats)
{
    *stats = bsw_mate_stats_t{};
    const size_t jcap = (size_t)n + 64 * kMateBuckets;
    BSW_TRY(s.d_mjobs.grow(jcap));
    if (!s.d_mmeta) BSW_TRY(s.d_mmeta.reserve_exact(kMateMetaWords));
    if (!s.h_mmeta) BSW_TRY(s.h_mmeta.reserve_exact(kMateMetaWords));
    if (!s.d_mcells) BSW_TRY(s.d_mcells.reserve_exact(1));
    if (!s.ev2) BSW_TRY(hipEventCreate(&s.ev2.p));
    if (!s.ev3) BSW_TRY(hipEventCreate(&s.ev3.p));
    BSW_TRY(hipMemsetAsync(s.d_mcells, 0, sizeof(unsigned long long), st));
    for (int mode = 0; mode < 2; ++mode) {
        BSW_TRY(launch_mate_prepare(d_pairs, d_aln, n, mode, s.d_mmeta, s.d_mjobs, (int32_t)jcap, st));
        BSW_TRY(hipMemcpyAsync(s.h_mmeta, s.d_mmeta, kMateMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        BSW_TRY(hipStreamSynchronize(st));
        const int32_t *m = s.h_mmeta;
        if (m[kMateMetaErr]) return BSW_E_RANGE;
        int32_t njobs = 0;
        for (int b = 0; b < kMateBuckets; ++b) njobs += m[kMateMetaCount + b];
        const int64_t total = m[kMateMetaTotal];
        uint16_t *rows = nullptr;
        if (mode == 0 && njobs > 0) {
            const size_t need = (size_t)std::max(m[kMateMetaTmax], 1) * (size_t)total;
            BSW_TRY(s.d_mrows.grow(need));
            rows = s.d_mrows;
        }
        hipEvent_t e0 = mode == 0 ? s.ev0 : s.ev2, e1 = mode == 0 ? s.ev1 : s.ev3;
        BSW_TRY(hipEventRecord(e0, st));
        for (int c = 0; c < kMateClasses; ++c)
            BSW_TRY(launch_mate_class(c, mp, d_pairs, s.d_mjobs, m[kMateMetaClass + 2 * c],
                                      m[kMateMetaClass + 2 * c + 1], d_ref, d_qer, d_aln, mode, rows, total,
                                      mode == 0 ? s.d_mcells.p : nullptr, st));
        BSW_TRY(hipEventRecord(e1, st));
        if (mode == 0) stats->n_fwd = njobs; else stats->n_rev = njobs;
    }
    unsigned long long cells = 0;
    BSW_TRY(hipMemcpyAsync(&cells, s.d_mcells, sizeof(cells), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&stats->fwd_ms, s.ev0, s.ev1));
    BSW_TRY(hipEventElapsedTime(&stats->rev_ms, s.ev2, s.ev3));
    stats->cells_fwd = (int64_t)cells;
    return BSW_OK;
}

// ---------------------------------------------------------------- global alignment (bsw_global.h)
static void make_glob_params(const bsw_params_t &p, int prefer_band, GlobParams &gp)
{
    memset(&gp, 0, sizeof(gp));
    gp.o_del = p.o_del; gp.e_del = p.e_del; gp.o_ins = p.o_ins; gp.e_ins = p.e_ins;
    gp.oe_del = p.o_del + p.e_del; gp.oe_ins = p.o_ins + p.e_ins;
    int mx = 0;
    for (int i = 0; i < 25; ++i) mx = std::max(mx, std::abs((int)p.mat[i]));
    gp.maxabs = mx;
    memcpy(gp.mat, p.mat, 25);
    gp.prefer_band = prefer_band ? 1 : 0;
    for (int t = 0; t < 8; ++t) {                        // codes > 4 score as N (as prof in KParams)
        const int tt = std::min(t, 4);
        uint8_t b[8];
        for (int q = 0; q < 8; ++q) b[q] = (uint8_t)p.mat[tt * 5 + std::min(q, 4)];
        gp.prof[t][0] = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
        gp.prof[t][1] = b[4] | (b[5] << 8) | (b[6] << 16) | ((uint32_t)b[7] << 24);
    }
}

constexpr int64_t kGlobZCapWords = (int64_t)2 << 30;     // traceback matrix per launch <= 8 GB

// plan -> sort (class, w, qlen, tlen) -> one readback of the class statistics -> per class the
// DP + traceback kernel over its slice of order[] (chunked so the matrix stays under the cap).
static int glob_device(const GlobParams &gp, Slot &s, SeqPair *d_pairs, const uint8_t *d_ref,
                       const uint8_t *d_qer, int32_t n, uint32_t *d_cigar, int32_t stride, int32_t *d_ncig,
                       hipStream_t st, bsw_global_stats_t *stats)
{
    *stats = bsw_global_stats_t{};
    stats->n_jobs = n;
    if (n == 0) return BSW_OK;
    BSW_TRY(grow_sort(s, n));
    if (!s.d_gmeta) BSW_TRY(s.d_gmeta.reserve_exact(kGMetaWords));
    if (!s.h_gmeta) BSW_TRY(s.h_gmeta.reserve_exact(kGMetaWords));
    if (!s.d_mcells) BSW_TRY(s.d_mcells.reserve_exact(1));
    BSW_TRY(launch_glob_plan(d_pairs, n, gp, s.d_keys, s.d_vals, s.d_gmeta, st));
    BSW_TRY(sort_order(s, n, kGlobKeyBits, st));
    BSW_TRY(hipMemcpyAsync(s.h_gmeta, s.d_gmeta, kGMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemsetAsync(s.d_mcells, 0, sizeof(unsigned long long), st));
    BSW_TRY(hipStreamSynchronize(st));
    int32_t m[kGMetaWordsPerSlot] = {};
    for (int sl = 0; sl < kGMetaSpread; ++sl) {
        const int32_t *v = s.h_gmeta + sl * kGMetaWordsPerSlot;
        for (int c = 0; c < kGlobClasses; ++c) {
            m[kGMetaCount + c] += v[kGMetaCount + c];
            m[kGMetaTmax + c] = std::max(m[kGMetaTmax + c], v[kGMetaTmax + c]);
            m[kGMetaWmax + c] = std::max(m[kGMetaWmax + c], v[kGMetaWmax + c]);
            m[kGMetaQmax + c] = std::max(m[kGMetaQmax + c], v[kGMetaQmax + c]);
        }
        m[kGMetaErr] |= v[kGMetaErr];
    }
    if (m[kGMetaErr]) return BSW_E_RANGE;
    const bool want = d_cigar && stride > 0;
    // column classes keep only a narrow corridor of the traceback matrix (glob_lane_kernel: 3 dwords
    // per row instead of the band's ~10 at bwa-shaped w); jobs whose path leaves it rerun below with
    // the full band window
    constexpr int tb_env = 3;
    if (want) BSW_TRY(s.d_gretry.grow((size_t)n + 1));
    BSW_TRY(hipEventRecord(s.ev0, st));
    int32_t off = 0;
    for (int c = 0; c < kGlobClasses; ++c) {
        const int32_t cnt = m[kGMetaCount + c];
        if (cnt <= 0) continue;
        const int tm = m[kGMetaTmax + c], wm = m[kGMetaWmax + c], qm = m[kGMetaQmax + c];
        const int cap_dw = glob_cap_dw(c, qm, wm);
        const bool col = c >= kGlobLane0 && c < kGlobWideClass;
        const int tb = (want && col && tb_env > 0 && tb_env < cap_dw) ? tb_env : 0;
        // one pass over the class (narrow window when tb > 0), then the retry list with the full window
        for (int pass = 0; pass < (tb > 0 ? 2 : 1); ++pass) {
            const int ptb = pass == 0 ? tb : 0;
            int32_t pcnt = cnt;
            const int32_t *ord = s.d_order + off;
            if (pass == 1) {                                // the jobs the narrow window could not serve
                int32_t nr = 0;
                BSW_TRY(hipMemcpyAsync(&nr, s.d_gretry, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                BSW_TRY(hipStreamSynchronize(st));
                stats->n_tb_retry += nr;
                if (nr <= 0) break;
                pcnt = nr;
                ord = s.d_gretry + 1;
            } else if (ptb > 0) {
                BSW_TRY(hipMemsetAsync(s.d_gretry, 0, sizeof(int32_t), st));
            }
            const int64_t zstride = (int64_t)std::max(tm, 1) * (ptb > 0 ? ptb : cap_dw) * 64;
            int32_t chunk = pcnt;
            if (want) {
                const int64_t waves = std::max<int64_t>(1, kGlobZCapWords / zstride);
                chunk = (int32_t)std::min<int64_t>(pcnt, waves * 64);
                BSW_TRY(s.d_gz.grow((size_t)((chunk + 63) / 64) * (size_t)zstride));
            }
            if (c == kGlobWideClass) BSW_TRY(s.d_scratch.grow((size_t)(qm + 1) * (size_t)chunk));
            for (int32_t a = 0; a < pcnt; a += chunk) {
                const int32_t b = std::min(pcnt, a + chunk);
                BSW_TRY(launch_glob_class(c, gp, d_pairs, ord + a, b - a, d_ref, d_qer,
                                          want ? s.d_gz.p : nullptr, zstride, cap_dw, s.d_scratch, d_cigar, stride,
                                          d_ncig, pass == 0 ? s.d_mcells.p : nullptr, st, ptb,
                                          ptb > 0 ? s.d_gretry.p : nullptr));
                stats->n_launches++;
                if (want) stats->z_bytes += (int64_t)((b - a + 63) / 64) * zstride * 4;
            }
        }
        if (c == kGlobWideClass) stats->n_wide += cnt;
        else stats->n_lane += cnt;
        off += cnt;
    }
    BSW_TRY(hipEventRecord(s.ev1, st));
    unsigned long long cells = 0;
    BSW_TRY(hipMemcpyAsync(&cells, s.d_mcells, sizeof(cells), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&stats->kernel_ms, s.ev0, s.ev1));
    stats->cells = (int64_t)cells;
    return BSW_OK;
}

// ---------------------------------------------------------------- device extension pipeline
// One side of bsw_extend_seeds on the GPU: build (sparse job per read) -> engine -> band retries
// -> interpretation.  Every step on `st`; the only host syncs are the engine's class-count
// readback and one retry count per retry round.
static int ext_side_device(const KParams &kp0, Slot &s, const ExtDevParams &xp, int left, const bsw_ext_opt_t &opt,
                           const uint8_t *d_reads, const int64_t *d_off, const int32_t *d_len,
                           const bsw_seed_t *d_seeds, const int64_t *d_win, int32_t n, const uint8_t *d_ref,
                           bsw_alnreg_t *d_out, int32_t *d_cnt, hipStream_t st, bsw_ext_stats_t &es)
{
    KParams kp = kp0;
    kp.end_bonus = left ? opt.pen_clip5 : opt.pen_clip3;
    BSW_TRY(launch_ext_build(left, xp, d_reads, d_off, d_len, d_seeds, d_win, n, d_ref, s.d_xst, s.d_xpairs, s.d_xq,
                             s.d_xt, d_out, st));
    int r = run_device(kp, s, s.d_xpairs, s.d_xt, s.d_xq, n, opt.w, 16, st);
    if (r) return r;
    // each DP batch, the next band-retry mark and its count readback are queued before one wait
    // (finish_stats), so a retry level costs one host round trip, not two
    for (int t = 1;; ++t) {
        const bool retry = t < opt.max_band_try;
        const int32_t wt = opt.w << (t - 1), wn = opt.w << t;
        if (retry) {
            BSW_TRY(launch_ext_retry_mark(t == 1 ? s.d_xpairs : s.d_xsub, s.d_xsub, s.d_xst, n, wt, d_cnt, st));
            BSW_TRY(hipMemcpyAsync(s.h_meta + kMetaCnt, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        if ((r = finish_stats(s))) return r;
        es.kernel_ms += s.stats.kernel_ms;
        if (!retry) break;
        BSW_TRY(hipStreamSynchronize(st));          // (idle already unless the batch was empty)
        const int32_t cnt = s.h_meta[kMetaCnt];
        if (cnt == 0) break;
        es.n_pairs[(left ? 0 : 2) + 1] += cnt;
        if ((r = run_device(kp, s, s.d_xsub, s.d_xt, s.d_xq, n, wn, 16, st))) return r;
        BSW_TRY(launch_ext_retry_merge(s.d_xpairs, s.d_xsub, s.d_xst, n, wn, left, st));
    }
    BSW_TRY(launch_ext_interp(left, xp, d_len, d_seeds, n, s.d_xpairs, s.d_xst, d_out, st));
    return BSW_OK;
}

}  // namespace bsw

// ====================================================================== C ABI
extern "C" {

void bsw_params_default(bsw_params_t *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->o_del = p->o_ins = 6;
    p->e_del = p->e_ins = 1;
    p->zdrop = 100;
    p->end_bonus = 5;
    p->w_match = 1;
    p->w_mismatch = -4;
    p->w_ambig = -1;
    for (int t = 0; t < 5; ++t)
        for (int q = 0; q < 5; ++q)
            p->mat[t * 5 + q] = (t == 4 || q == 4) ? -1 : (t == q ? 1 : -4);
}

static bool params_ok(const bsw_params_t *p)
{
    if (p->e_del < 1 || p->e_ins < 1 || p->o_del < 0 || p->o_ins < 0) return false;
    if (p->o_del + p->e_del > 32767 || p->o_ins + p->e_ins > 32767) return false;
    return true;
}

int bsw_create_on(const bsw_params_t *params, const int *devices, int n_devices, bsw_ctx_t **out)
{
    if (!params || !out || !devices || n_devices < 1 || !params_ok(params)) return BSW_E_INVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BSW_E_NODEV;
    for (int d = 0; d < n_devices; ++d)
        if (devices[d] < 0 || devices[d] >= ndev) return BSW_E_NODEV;
    auto *c = new bsw_ctx();
    c->params = *params;
    bsw::make_kparams(*params, c->kp);
    for (int d = 0; d < n_devices; ++d) {
        auto dc = std::make_unique<bsw::DeviceCtx>();
        dc->device = devices[d];
        c->devs.push_back(std::move(dc));
    }
    *out = c;
    return BSW_OK;
}

int bsw_create(const bsw_params_t *params, int device0, int n_gpus, bsw_ctx_t **out)
{
    if (!params || !out || n_gpus < 1 || device0 < 0 || n_gpus > 4096) return BSW_E_INVAL;
    std::vector<int> devs((size_t)n_gpus);
    for (int d = 0; d < n_gpus; ++d) devs[d] = device0 + d;
    return bsw_create_on(params, devs.data(), n_gpus, out);
}

void bsw_destroy(bsw_ctx_t *ctx) { delete ctx; }

static int validate(const SeqPair *pairs, int32_t n, int32_t w, int cell_bits)
{
    if (n < 0 || w < 0 || (cell_bits != 8 && cell_bits != 16)) return BSW_E_INVAL;
    if (n > 0 && !pairs) return BSW_E_INVAL;
    return BSW_OK;
}

}  // extern "C"

namespace bsw {

// Static band cells of one pair (rows i < tlen, columns [max(0, i - w), min(qlen, i + w + 1))):
// the work estimate behind the multi-device split.
static int64_t band_cells_est(int64_t qlen, int64_t tlen, int64_t w)
{
    if (qlen <= 0 || tlen <= 0) return 0;
    const int64_t T = std::min(tlen, qlen + w);                  // rows with a non-empty band
    auto ssum = [](int64_t a, int64_t b, int64_t c) {            // sum_{i=a}^{b-1} (i + c)
        return b > a ? (b - a) * (a + b - 1) / 2 + c * (b - a) : (int64_t)0;
    };
    const int64_t k = std::min(T, std::max<int64_t>(qlen - w, 0));   // rows with i + w + 1 <= qlen
    const int64_t hi = ssum(0, k, w + 1) + qlen * (T - k);
    const int64_t lo = ssum(std::min(T, w + 1), T, -w);              // rows with i > w
    return std::max<int64_t>(hi - lo, 0);
}

// nd + 1 cut points: device d takes pairs [cut[d], cut[d+1]), each range ~1/nd of the cells
// (plus a per-pair constant for the plan / sort / launch share)
static std::vector<int32_t> split_by_cells(const SeqPair *pairs, int32_t n, int32_t w, int nd)
{
    std::vector<int64_t> pre((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i)
        pre[i + 1] = pre[i] + 64 + band_cells_est(pairs[i].len2, pairs[i].len1, w);
    std::vector<int32_t> cut((size_t)nd + 1, n);
    cut[0] = 0;
    for (int d = 1; d < nd; ++d) {
        const int64_t target = pre[n] * d / nd;
        cut[d] = (int32_t)(std::lower_bound(pre.begin(), pre.end(), target) - pre.begin());
        cut[d] = std::max(cut[d], cut[d - 1]);
    }
    return cut;
}

// Multi-device policy (a context over several logical devices): a call of fewer than
// split_min items runs whole on ONE device -- the one with the fewest host-buffer calls in
// flight, ties rotating -- so kt_for-sized calls from concurrent workers spread over the
// devices instead of each paying every device's launch latency for a sliver of work; larger
// calls split into contiguous ranges, one per device.  Returns the device, or -1: split.
struct Inflight {
    DeviceCtx &dc;
    explicit Inflight(DeviceCtx &d) : dc(d) { dc.inflight.fetch_add(1); }
    ~Inflight() { dc.inflight.fetch_sub(1); }
};

static int one_device(bsw_ctx_t *ctx, int64_t n)
{
    const int nd = (int)ctx->devs.size();
    if (nd == 1) return 0;
    if (n >= ctx->split_min) return -1;
    const unsigned r = ctx->rr.fetch_add(1);
    int best = -1, load = INT32_MAX;
    for (int k = 0; k < nd; ++k) {
        const int d = (int)((r + (unsigned)k) % (unsigned)nd);
        const int l = ctx->devs[d]->inflight.load();
        if (l < load) { load = l; best = d; }
    }
    return best;
}

// Recovery of a host-buffer range whose run on device d0 failed with BSW_E_NOMEM / BSW_E_HIP
// (bsw.h, bsw_get_scores): 1. again on d0 after its cached slots are freed, 2. on each other
// device of the context, 3. (BSW_E_NOMEM only) in halves (down to one 4096-pair staging block),
// each half the same way.  No coalescing here: the range runs as a call of its own.  Outputs are identical to an
// undisturbed call -- pairs are independent, and a failed run writes no input field (staged
// records go back as outputs only or as the caller's own bytes).  `how` gets the deepest step
// used.  Upstream plans to degrade on engine errors instead of aborting the run
// (PHASE2_IMPLEMENTATION_SUMMARY.md:210-225); there is no CPU path to degrade to here.
static bool recoverable(int rc) { return rc == BSW_E_NOMEM || rc == BSW_E_HIP; }

static int recover_range(bsw_ctx_t *ctx, const KParams &kp, int d0, SeqPair *pairs, const uint8_t *ref,
                         const uint8_t *qer, int32_t n, int32_t w, int cell_bits, bsw_stats_t *st, int &how)
{
    const int nd = (int)ctx->devs.size();
    int rc = BSW_E_HIP;
    for (int k = 0; k < nd; ++k) {
        const int d = (d0 + k) % nd;
        DeviceCtx &dc = *ctx->devs[d];
        dc.trim();
        {
            Inflight g(dc);
            rc = host_shard(kp, dc, pairs, ref, qer, n, w, cell_bits, ctx->host_chunk, ctx->host_pack == 2, st);
        }
        if (rc == BSW_OK) {
            how = std::max(how, k == 0 ? 1 : 2);
            return BSW_OK;
        }
        if (!recoverable(rc)) return rc;
    }
    // halves only for memory: a smaller range needs smaller buffers, but it cannot fix a HIP error
    // (a sticky context error repeats on every rerun)
    if (rc != BSW_E_NOMEM || n <= kStageBlk) return rc;
    const int32_t h = std::max<int32_t>(kStageBlk, (n / 2) & ~(kStageBlk - 1));
    bsw_stats_t a{}, b{};
    if ((rc = recover_range(ctx, kp, d0, pairs, ref, qer, h, w, cell_bits, &a, how))) return rc;
    if ((rc = recover_range(ctx, kp, (d0 + 1) % nd, pairs + h, ref, qer, n - h, w, cell_bits, &b, how))) return rc;
    how = std::max(how, 3);
    *st = a;
    st->kernel_ms += b.kernel_ms; st->stage_ms += b.stage_ms; st->host_ms += b.host_ms;
    st->n_i16 += b.n_i16; st->n_u8 += b.n_u8; st->n_wide += b.n_wide; st->n_packed += b.n_packed;
    st->n_launches += b.n_launches; st->n_wave += b.n_wave; st->n_group += b.n_group;
    return BSW_OK;
}

int scores_eb(bsw_ctx_t *ctx, int32_t end_bonus, SeqPair *pairs, const uint8_t *seqBufRef,
              const uint8_t *seqBufQer, int32_t n, int32_t w, int cell_bits, bsw_stats_t *out)
{
    if (!ctx) return BSW_E_INVAL;
    int rc = validate(pairs, n, w, cell_bits);
    if (rc) return rc;
    *out = bsw_stats_t{};
    if (n == 0) return BSW_OK;
    if (!seqBufRef || !seqBufQer) return BSW_E_INVAL;
    KParams kp = ctx->kp;
    kp.end_bonus = end_bonus;
    const int one = one_device(ctx, n);
    const int nd = one >= 0 ? 1 : (int)ctx->devs.size();
    // one device: host_shard's parallel pre-pass validates; several: validate the whole batch
    // before any device starts
    if (nd > 1)
        for (int32_t i = 0; i < n; ++i)
            if (pairs[i].len1 < 0 || pairs[i].len2 < 0 || pairs[i].len1 > BSW_MAX_LEN ||
                pairs[i].len2 > BSW_MAX_LEN || pairs[i].idr < 0 || pairs[i].idq < 0)
                return BSW_E_RANGE;
    std::vector<int> rcs(nd, BSW_OK);
    std::vector<bsw_stats_t> st(nd);
    std::vector<int> how(nd, 0);
    if (nd == 1) {
        {
            Inflight g(*ctx->devs[one]);
            if (n <= ctx->coalesce)             // kt_for-sized: coalesce with concurrent callers
                rcs[0] = coalesced_call(kp, *ctx->devs[one], pairs, seqBufRef, seqBufQer, n, w, cell_bits,
                                        ctx->host_chunk, ctx->host_pack == 2, &st[0]);
            else
                rcs[0] = host_shard(kp, *ctx->devs[one], pairs, seqBufRef, seqBufQer, n, w, cell_bits,
                                    ctx->host_chunk, ctx->host_pack == 2, &st[0]);
        }
        if (recoverable(rcs[0]))
            rcs[0] = recover_range(ctx, kp, one, pairs, seqBufRef, seqBufQer, n, w, cell_bits, &st[0], how[0]);
    } else {
        // contiguous pair ranges of equal estimated work (static band cells)
        const std::vector<int32_t> cut = split_by_cells(pairs, n, w, nd);
        std::vector<std::thread> th;
        for (int d = 0; d < nd; ++d) {
            const int32_t a = cut[d], b = cut[d + 1];
            th.emplace_back([&, d, a, b] {
                {
                    Inflight g(*ctx->devs[d]);
                    rcs[d] = host_shard(kp, *ctx->devs[d], pairs + a, seqBufRef, seqBufQer, b - a, w,
                                        cell_bits, ctx->host_chunk, ctx->host_pack == 2, &st[d]);
                }
                if (recoverable(rcs[d]))
                    rcs[d] = recover_range(ctx, kp, d, pairs + a, seqBufRef, seqBufQer, b - a, w, cell_bits, &st[d],
                                           how[d]);
            });
        }
        for (auto &t : th) t.join();
    }
    bsw_stats_t agg{};
    for (int d = 0; d < nd; ++d) {
        if (rcs[d]) return rcs[d];
        agg.kernel_ms = std::max(agg.kernel_ms, st[d].kernel_ms);
        agg.n_i16 += st[d].n_i16; agg.n_u8 += st[d].n_u8; agg.n_wide += st[d].n_wide; agg.n_packed += st[d].n_packed;
        agg.n_launches += st[d].n_launches;
        agg.n_wave += st[d].n_wave; agg.n_group += st[d].n_group;
        agg.stage_ms = std::max(agg.stage_ms, st[d].stage_ms);
        agg.host_ms = std::max(agg.host_ms, st[d].host_ms);
        agg.recovery = std::max(agg.recovery, how[d]);
    }
    agg.n_devices = nd;
    *out = agg;
    return BSW_OK;
}

void ctx_params(const bsw_ctx_t *ctx, bsw_params_t *out) { *out = ctx->params; }
int ctx_device(const bsw_ctx_t *ctx) { return ctx->devs[0]->device; }
int64_t ctx_refres_len(bsw_ctx_t *ctx)
{
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> g(dc.refmu);
    return dc.d_refres ? dc.refres_len : -1;
}

void *pinned_acquire(bsw_ctx_t *ctx, int which, size_t bytes)
{
    auto &b = ctx->pin[which & 1];
    if (!b.mu.try_lock()) return nullptr;
    if (b.b.cap < bytes && b.b.reserve_exact(bytes) != hipSuccess) {
        b.mu.unlock();
        return nullptr;
    }
    return b.b.p;
}

void pinned_release(bsw_ctx_t *ctx, int which) { ctx->pin[which & 1].mu.unlock(); }

// reads per extension call chunk: the int32-offset bound, optionally lowered per context
// (BSW_OPT_EXT_CHUNK: exercises the chunked paths at small sizes)
int64_t ext_chunk_cap(const bsw_ctx_t *ctx)
{
    return ctx->ext_chunk > 0 ? ctx->ext_chunk : (int64_t)INT32_MAX;
}

void set_chain_stats(bsw_ctx_t *ctx, const bsw_chain_stats_t &s)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->chain_last = s;
}

int get_chain_stats(bsw_ctx_t *ctx, bsw_chain_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->chain_last;
    return BSW_OK;
}

void set_ext_stats(bsw_ctx_t *ctx, const bsw_ext_stats_t &s)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->ext_last = s;
}

int get_ext_stats(bsw_ctx_t *ctx, bsw_ext_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->ext_last;
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

int bsw_get_scores(bsw_ctx_t *ctx, SeqPair *pairs, const uint8_t *seqBufRef,
                   const uint8_t *seqBufQer, int32_t n, int32_t w, int cell_bits)
{
    if (!ctx) return BSW_E_INVAL;
    bsw_stats_t st{};
    const int rc = bsw::scores_eb(ctx, ctx->params.end_bonus, pairs, seqBufRef, seqBufQer, n, w,
                                  cell_bits, &st);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->last = st;
    return BSW_OK;
}

int bsw_get_scores_device(bsw_ctx_t *ctx, SeqPair *d_pairs, const uint8_t *d_ref,
                          const uint8_t *d_qer, int32_t n, int32_t w, int cell_bits, void *stream)
{
    if (!ctx) return BSW_E_INVAL;
    int rc = validate(d_pairs, n, w, cell_bits);
    if (rc) return rc;
    if (n == 0) return BSW_OK;
    if (!d_ref || !d_qer) return BSW_E_INVAL;
    return bsw::with_slot(*ctx->devs[0], [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        int r = bsw::run_device(ctx->kp, s, d_pairs, d_ref, d_qer, n, w, cell_bits, st);
        if (r) return r;
        if ((r = bsw::finish_stats(s))) return r;
        std::lock_guard<std::mutex> g(ctx->stats_mu);
        ctx->last = s.stats;
        return BSW_OK;
    });
}

// The packed wire form (bsw_pack_batch) scored in place: one stage_in_kernel (2-bit unpack of both
// extents, exception patches, 20-B records -> SeqPair, pads zeroed), the device pipeline, then the
// 24 output bytes per pair compacted into d_out -- the path of a batch that arrived over RCCL
int bsw_get_scores_packed_device(bsw_ctx_t *ctx, const void *d_packed, const bsw_packed_t *desc, int32_t w,
                                 int cell_bits, int32_t *d_out, void *stream)
{
    if (!ctx || !desc) return BSW_E_INVAL;
    const bsw_packed_t d = *desc;
    if (d.n < 0 || w < 0 || (cell_bits != 8 && cell_bits != 16)) return BSW_E_INVAL;
    if (d.n == 0) return BSW_OK;
    if (!d_packed || !d_out || d.ref_bytes < 0 || d.qer_bytes < 0 || d.n_exc_ref < 0 || d.n_exc_qer < 0 ||
        d.ref_bytes >= ((int64_t)1 << 30) || d.qer_bytes >= ((int64_t)1 << 30) ||
        ((d.rec_off | d.ref_off | d.qer_off | d.exc_off) & 3) != 0)
        return BSW_E_INVAL;
    return bsw::with_slot(*ctx->devs[0], [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        BSW_TRY(s.d_ref.grow((size_t)d.ref_bytes + 16));
        BSW_TRY(s.d_qer.grow((size_t)d.qer_bytes + 16));
        BSW_TRY(s.d_pairs.grow((size_t)d.n));
        const uint8_t *b = (const uint8_t *)d_packed;
        // the staging kernels on the slot's high-priority stream (after the caller's stream: the
        // piece may have been written there), as plan / sort already are: a piece's preparation is
        // then dispatched ahead of another piece's queued DP workgroups instead of behind them (the
        // RCCL leg's trace: the second piece's staging waited out the first piece's whole DP,
        // profiles/r06/rccl_leg_trace.txt).  Its DP, on `st`, waits for the plan (run_dp).
        if (int e = bsw::ensure_pstream(s)) return e;
        BSW_TRY(hipEventRecord(s.evh, st));
        BSW_TRY(hipStreamWaitEvent(s.pstream, s.evh, 0));
        if (int e = bsw::launch_stage_in(s, s.pstream, b + d.ref_off, d.ref_bytes, b + d.qer_off, d.qer_bytes,
                                         (const uint32_t *)(b + d.exc_off), d.n_exc_ref, d.n_exc_ref + d.n_exc_qer,
                                         (const bsw::PairIn *)(b + d.rec_off), d.n, s.d_ref, s.d_qer, s.d_pairs, nullptr))
            return e;
        // everything after it on `st` (the small-batch route launches there without a plan)
        BSW_TRY(hipEventRecord(s.evh, s.pstream));
        BSW_TRY(hipStreamWaitEvent(st, s.evh, 0));
        int r = bsw::run_device(ctx->kp, s, s.d_pairs, s.d_ref, s.d_qer, d.n, w, cell_bits, st);
        if (r) return r;
        if ((r = bsw::finish_stats(s))) return r;
        if ((r = bsw::launch_gather_outputs(s.d_pairs, d_out, d.n, st))) return r;
        BSW_TRY(hipStreamSynchronize(st));
        std::lock_guard<std::mutex> g(ctx->stats_mu);
        ctx->last = s.stats;
        return BSW_OK;
    });
}

int bsw_ksw_align2_device(bsw_ctx_t *ctx, const SeqPair *d_pairs, const uint8_t *d_ref,
                          const uint8_t *d_qer, int32_t n, bsw_kswr_t *d_aln, void *stream)
{
    if (!ctx || n < 0 || (n > 0 && (!d_pairs || !d_ref || !d_qer || !d_aln))) return BSW_E_INVAL;
    if (!bsw::mate_params_ok(ctx->params)) return BSW_E_INVAL;
    if (n == 0) return BSW_OK;
    bsw::MateParams mp;
    bsw::make_mate_params(ctx->params, mp);
    return bsw::with_slot(*ctx->devs[0], [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        bsw_mate_stats_t ms;
        const int r = bsw::mate_device(mp, s, d_pairs, d_ref, d_qer, n, d_aln, st, &ms);
        if (r) return r;
        std::lock_guard<std::mutex> g(ctx->stats_mu);
        ctx->mate_last = ms;
        return BSW_OK;
    });
}

}  // extern "C"

namespace bsw {
// The byte extents of jobs [0, n) in the caller's reference and query buffers -> the slot's
// d_ref / d_qer (grown to them), copied on the slot's stream.  d_ref / d_qer get the device
// pointers rebased so that the jobs' own idr / idq index them.
static int upload_extents(Slot &s, const SeqPair *pairs, int32_t n, const uint8_t *seqBufRef,
                          const uint8_t *seqBufQer, const uint8_t *&d_ref, const uint8_t *&d_qer)
{
    int64_t r_lo = INT64_MAX, r_hi = 0, q_lo = INT64_MAX, q_hi = 0;
    for (int32_t i = 0; i < n; ++i) {
        const SeqPair &p = pairs[i];
        if (p.len1 > 0) { r_lo = std::min<int64_t>(r_lo, p.idr); r_hi = std::max<int64_t>(r_hi, (int64_t)p.idr + p.len1); }
        if (p.len2 > 0) { q_lo = std::min<int64_t>(q_lo, p.idq); q_hi = std::max<int64_t>(q_hi, (int64_t)p.idq + p.len2); }
    }
    if (r_lo == INT64_MAX) r_lo = r_hi = 0;
    if (q_lo == INT64_MAX) q_lo = q_hi = 0;
    BSW_TRY(s.d_ref.grow((size_t)(r_hi - r_lo) + 1));
    BSW_TRY(s.d_qer.grow((size_t)(q_hi - q_lo) + 1));
    if (r_hi > r_lo) BSW_TRY(hipMemcpyAsync(s.d_ref, seqBufRef + r_lo, (size_t)(r_hi - r_lo), hipMemcpyHostToDevice, s.stream));
    if (q_hi > q_lo) BSW_TRY(hipMemcpyAsync(s.d_qer, seqBufQer + q_lo, (size_t)(q_hi - q_lo), hipMemcpyHostToDevice, s.stream));
    d_ref = s.d_ref - r_lo;
    d_qer = s.d_qer - q_lo;
    return BSW_OK;
}

// One device's share of a host-buffer mate-rescue call (contiguous job range).
static int mate_host_shard(const MateParams &mp, DeviceCtx &dc, const SeqPair *pairs, const uint8_t *seqBufRef,
                           const uint8_t *seqBufQer, int32_t n, bsw_kswr_t *aln, bsw_mate_stats_t *ms)
{
    *ms = bsw_mate_stats_t{};
    if (n == 0) return BSW_OK;
    return with_slot(dc, [&](Slot &s) -> int {
        const uint8_t *d_ref, *d_qer;
        BSW_TRY(s.d_mpairs.grow((size_t)n));
        BSW_TRY(s.d_maln.grow((size_t)n));
        BSW_TRY(hipMemcpyAsync(s.d_mpairs, pairs, (size_t)n * sizeof(SeqPair), hipMemcpyHostToDevice, s.stream));
        if (int r = upload_extents(s, pairs, n, seqBufRef, seqBufQer, d_ref, d_qer)) return r;
        if (int r = mate_device(mp, s, s.d_mpairs, d_ref, d_qer, n, s.d_maln, s.stream, ms)) return r;
        BSW_TRY(hipMemcpyAsync(aln, s.d_maln, (size_t)n * sizeof(bsw_kswr_t), hipMemcpyDeviceToHost, s.stream));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
}

// Run shard(d, a, b) for contiguous job ranges [a, b) on every device of the context (one host
// thread per device; jobs are independent), first non-zero status wins.
// Small calls run whole on one device (one_device's policy).
template <class F>
static int shard_devices(bsw_ctx_t *ctx, int32_t n, F shard)
{
    const int one = one_device(ctx, n);
    if (one >= 0) {
        Inflight g(*ctx->devs[one]);
        return shard(one, 0, n);
    }
    const int nd = (int)ctx->devs.size();
    std::vector<int> rcs(nd, BSW_OK);
    std::vector<std::thread> th;
    for (int d = 0; d < nd; ++d) {
        const int32_t a = (int32_t)((int64_t)n * d / nd), b = (int32_t)((int64_t)n * (d + 1) / nd);
        th.emplace_back([&, d, a, b] {
            Inflight g(*ctx->devs[d]);
            rcs[d] = shard(d, a, b);
        });
    }
    for (auto &t : th) t.join();
    for (int r : rcs)
        if (r) return r;
    return BSW_OK;
}
}  // namespace bsw

extern "C" {

int bsw_ksw_align2(bsw_ctx_t *ctx, const SeqPair *pairs, const uint8_t *seqBufRef, const uint8_t *seqBufQer,
                   int32_t n, bsw_kswr_t *aln)
{
    if (!ctx || n < 0 || (n > 0 && (!pairs || !seqBufRef || !seqBufQer || !aln))) return BSW_E_INVAL;
    if (!bsw::mate_params_ok(ctx->params)) return BSW_E_INVAL;
    if (n == 0) return BSW_OK;
    for (int32_t i = 0; i < n; ++i)
        if (pairs[i].len1 < 0 || pairs[i].len2 < 0 || pairs[i].len1 > BSW_MAX_LEN ||
            pairs[i].len2 > BSW_MATE_MAX_QLEN || pairs[i].idr < 0 || pairs[i].idq < 0)
            return BSW_E_RANGE;
    bsw::MateParams mp;
    bsw::make_mate_params(ctx->params, mp);
    std::vector<bsw_mate_stats_t> st(ctx->devs.size());
    const int rc = bsw::shard_devices(ctx, n, [&](int d, int32_t a, int32_t b) {
        return bsw::mate_host_shard(mp, *ctx->devs[d], pairs + a, seqBufRef, seqBufQer, b - a, aln + a, &st[d]);
    });
    if (rc) return rc;
    bsw_mate_stats_t agg{};
    for (const auto &x : st) {
        agg.fwd_ms = std::max(agg.fwd_ms, x.fwd_ms); agg.rev_ms = std::max(agg.rev_ms, x.rev_ms);
        agg.n_fwd += x.n_fwd; agg.n_rev += x.n_rev; agg.cells_fwd += x.cells_fwd;
    }
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->mate_last = agg;
    return BSW_OK;
}

int bsw_mate_last_stats(bsw_ctx_t *ctx, bsw_mate_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->mate_last;
    return BSW_OK;
}

int bsw_ksw_global2_device(bsw_ctx_t *ctx, SeqPair *d_pairs, const uint8_t *d_ref, const uint8_t *d_qer,
                           int32_t n, uint32_t *d_cigar, int32_t cigar_stride, int32_t *d_n_cigar,
                           void *stream)
{
    if (!ctx || n < 0 || cigar_stride < 0 || (n > 0 && (!d_pairs || !d_ref || !d_qer)) ||
        (n > 0 && cigar_stride > 0 && (!d_cigar || !d_n_cigar)))
        return BSW_E_INVAL;
    if (n == 0) return BSW_OK;
    bsw::GlobParams gp;
    bsw::make_glob_params(ctx->params, ctx->glob_band, gp);
    return bsw::with_slot(*ctx->devs[0], [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        bsw_global_stats_t gs;
        const int r = bsw::glob_device(gp, s, d_pairs, d_ref, d_qer, n, cigar_stride > 0 ? d_cigar : nullptr,
                                       cigar_stride, d_n_cigar, st, &gs);
        if (r) return r;
        std::lock_guard<std::mutex> g(ctx->stats_mu);
        ctx->glob_last = gs;
        return BSW_OK;
    });
}

}  // extern "C"

namespace bsw {
// One device's share of a host-buffer global-alignment call (contiguous job range).
static int glob_host_shard(const GlobParams &gp, DeviceCtx &dc, SeqPair *pairs, const uint8_t *seqBufRef,
                           const uint8_t *seqBufQer, int32_t n, uint32_t *cigar, int32_t cigar_stride,
                           int32_t *n_cigar, bsw_global_stats_t *gs)
{
    *gs = bsw_global_stats_t{};
    if (n == 0) return BSW_OK;
    return with_slot(dc, [&](Slot &s) -> int {
        const bool want = cigar_stride > 0;
        const uint8_t *d_ref, *d_qer;
        BSW_TRY(s.d_pairs.grow((size_t)n));
        BSW_TRY(hipMemcpyAsync(s.d_pairs, pairs, (size_t)n * sizeof(SeqPair), hipMemcpyHostToDevice, s.stream));
        if (int r = upload_extents(s, pairs, n, seqBufRef, seqBufQer, d_ref, d_qer)) return r;
        if (want) {
            BSW_TRY(s.d_gcig.grow((size_t)n * (size_t)cigar_stride));
            BSW_TRY(s.d_gncig.grow((size_t)n));
        }
        if (int r = glob_device(gp, s, s.d_pairs, d_ref, d_qer, n, want ? s.d_gcig.p : nullptr, cigar_stride,
                                want ? s.d_gncig.p : nullptr, s.stream, gs))
            return r;
        BSW_TRY(hipMemcpyAsync(pairs, s.d_pairs, (size_t)n * sizeof(SeqPair), hipMemcpyDeviceToHost, s.stream));
        if (want) {
            BSW_TRY(hipMemcpyAsync(cigar, s.d_gcig, (size_t)n * cigar_stride * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
            BSW_TRY(hipMemcpyAsync(n_cigar, s.d_gncig, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
        }
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
}
}  // namespace bsw

extern "C" {

int bsw_ksw_global2(bsw_ctx_t *ctx, SeqPair *pairs, const uint8_t *seqBufRef, const uint8_t *seqBufQer,
                    int32_t n, uint32_t *cigar, int32_t cigar_stride, int32_t *n_cigar)
{
    if (!ctx || n < 0 || cigar_stride < 0 || (n > 0 && (!pairs || !seqBufRef || !seqBufQer)) ||
        (n > 0 && cigar_stride > 0 && (!cigar || !n_cigar)))
        return BSW_E_INVAL;
    if (n == 0) return BSW_OK;
    for (int32_t i = 0; i < n; ++i)
        if (pairs[i].len1 < 0 || pairs[i].len2 < 0 || pairs[i].len1 > BSW_MAX_LEN || pairs[i].len2 > BSW_MAX_LEN ||
            pairs[i].idr < 0 || pairs[i].idq < 0 || pairs[i].h0 < 0)
            return BSW_E_RANGE;
    bsw::GlobParams gp;
    bsw::make_glob_params(ctx->params, ctx->glob_band, gp);
    std::vector<bsw_global_stats_t> st(ctx->devs.size());
    const int rc = bsw::shard_devices(ctx, n, [&](int d, int32_t a, int32_t b) {
        return bsw::glob_host_shard(gp, *ctx->devs[d], pairs + a, seqBufRef, seqBufQer, b - a,
                                    cigar_stride > 0 ? cigar + (size_t)a * cigar_stride : nullptr, cigar_stride,
                                    cigar_stride > 0 ? n_cigar + a : nullptr, &st[d]);
    });
    if (rc) return rc;
    bsw_global_stats_t agg{};
    for (const auto &x : st) {
        agg.kernel_ms = std::max(agg.kernel_ms, x.kernel_ms);
        agg.n_jobs += x.n_jobs; agg.n_lane += x.n_lane; agg.n_wide += x.n_wide; agg.n_launches += x.n_launches;
        agg.cells += x.cells; agg.z_bytes += x.z_bytes; agg.n_tb_retry += x.n_tb_retry;
    }
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->glob_last = agg;
    return BSW_OK;
}

int bsw_global_last_stats(bsw_ctx_t *ctx, bsw_global_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->glob_last;
    return BSW_OK;
}

int bsw_set_reference(bsw_ctx_t *ctx, const uint8_t *ref, int64_t ref_len)
{
    if (!ctx || ref_len < 0 || (ref_len > 0 && !ref)) return BSW_E_INVAL;
    for (auto &dcp : ctx->devs) {
        bsw::DeviceCtx &dc = *dcp;
        std::unique_lock<std::shared_mutex> g(dc.refmu);   // waits for running extension calls
        BSW_TRY(hipSetDevice(dc.device));
        dc.refres_len = -1;
        BSW_TRY(dc.d_refres.reserve_exact((size_t)ref_len + 64));
        if (ref_len > 0) {
            // on a non-blocking stream of its own: a null-stream copy would order against every
            // blocking (CU-masked) slot stream of the process (DeviceCtx::acquire)
            hipStream_t cs = nullptr;
            BSW_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
            hipError_t e = hipMemcpyAsync(dc.d_refres, ref, (size_t)ref_len, hipMemcpyHostToDevice, cs);
            if (e == hipSuccess) e = hipStreamSynchronize(cs);
            (void)hipStreamDestroy(cs);
            BSW_TRY(e);
        }
        dc.refres_len = ref_len;
    }
    return BSW_OK;
}

int bsw_extend_seeds_device(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads,
                            const int64_t *d_read_off, const int32_t *d_read_len, const bsw_seed_t *d_seeds,
                            int32_t n, bsw_alnreg_t *d_out, void *stream)
{
    return bsw::extend_seeds_device_win(ctx, opt, d_reads, d_read_off, d_read_len, d_seeds, nullptr, n, d_out, stream);
}

}  // extern "C"

int bsw::extend_seeds_device_win(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads,
                                 const int64_t *d_read_off, const int32_t *d_read_len, const bsw_seed_t *d_seeds,
                                 const int64_t *d_win, int32_t n, bsw_alnreg_t *d_out, void *stream)
{
    if (!ctx || !opt || n < 0 || (n > 0 && (!d_reads || !d_read_off || !d_read_len || !d_seeds || !d_out)))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (!dc.d_refres) return BSW_E_INVAL;
    if (const int rc = bsw::ext_opt_check(opt, dc.refres_len)) return rc;
    if (n == 0) return BSW_OK;
    const auto t0 = std::chrono::steady_clock::now();
    bsw_ext_stats_t es{};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        const bsw_params_t &p = ctx->params;
        bsw::ExtDevParams xp{};
        xp.w = opt->w; xp.pen_clip5 = opt->pen_clip5; xp.pen_clip3 = opt->pen_clip3; xp.a = p.mat[0];
        xp.o_del = p.o_del; xp.e_del = p.e_del; xp.o_ins = p.o_ins; xp.e_ins = p.e_ins;
        xp.ref_len = dc.refres_len;
        xp.l_pac = opt->l_pac;
        // scan: per-read validation and windows, longest read / window, job counts
        BSW_TRY(s.d_xwin.grow(2 * (size_t)n));
        BSW_TRY(bsw::launch_ext_scan(xp, d_read_len, d_seeds, d_win, n, s.d_xwin, s.d_meta, st));
        static_assert(bsw::kExtMetaSpread * 16 <= bsw::kMetaWords, "ext meta fits d_meta");
        BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_meta, bsw::kExtMetaSpread * 16 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        BSW_TRY(hipStreamSynchronize(st));
        int32_t m[5] = {0, 0, 0, 0, 0};
        for (int sl = 0; sl < bsw::kExtMetaSpread; ++sl) {
            const int32_t *v = s.h_meta + sl * 16;
            m[0] = std::max(m[0], v[0]); m[1] |= v[1]; m[2] += v[2]; m[3] += v[3]; m[4] = std::max(m[4], v[4]);
        }
        if (m[1]) return BSW_E_RANGE;                   // per read, as the host form (bsw_ext.cpp)
        es.n_pairs[0] = m[2];
        es.n_pairs[2] = m[3];
        xp.qstride = std::max(m[0], 1);                 // longest seeded read
        xp.tstride = std::max(m[4], 1);                 // longest target window (<= BSW_MAX_LEN)
        // SeqPair idr / idq are int32: chunk so i * tstride stays below 2^31
        const int32_t chunk = (int32_t)std::min<int64_t>(std::min<int64_t>(n, (int64_t)INT32_MAX /
                                                                                  std::max(xp.tstride, xp.qstride) - 1),
                                                         bsw::ext_chunk_cap(ctx));
        BSW_TRY(s.d_xpairs.grow((size_t)chunk));
        BSW_TRY(s.d_xsub.grow((size_t)chunk));
        BSW_TRY(s.d_xst.grow((size_t)chunk));
        BSW_TRY(s.d_xq.grow((size_t)chunk * xp.qstride));
        BSW_TRY(s.d_xt.grow((size_t)chunk * xp.tstride));
        if (!s.d_mcells) BSW_TRY(s.d_mcells.reserve_exact(1));
        int32_t *d_cnt = (int32_t *)s.d_mcells.p;
        for (int32_t a = 0; a < n; a += chunk) {
            const int32_t b = std::min(n, a + chunk);
            for (int left = 1; left >= 0; --left) {
                const int r = bsw::ext_side_device(ctx->kp, s, xp, left, *opt, d_reads, d_read_off + a, d_read_len + a,
                                                   d_seeds + a, s.d_xwin + 2 * (size_t)a, b - a, dc.d_refres,
                                                   d_out + a, d_cnt, st, es);
                if (r) return r;
            }
        }
        BSW_TRY(hipStreamSynchronize(st));
        return BSW_OK;
    });
    if (rc) return rc;
    es.engine_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bsw::set_ext_stats(ctx, es);
    return BSW_OK;
}

extern "C" {

int bsw_split_by_cells(const SeqPair *pairs, int32_t n, int32_t w, int32_t parts, int32_t *cut)
{
    if (n < 0 || w < 0 || parts < 1 || !cut || (n > 0 && !pairs)) return BSW_E_INVAL;
    const std::vector<int32_t> c = bsw::split_by_cells(pairs, n, w, parts);
    std::copy(c.begin(), c.end(), cut);
    return BSW_OK;
}

int bsw_set_option(bsw_ctx_t *ctx, int option, int64_t value)
{
    if (!ctx) return BSW_E_INVAL;
    const bool b01 = value == 0 || value == 1;
    switch (option) {
    case BSW_OPT_GQ32_MAX: if (value < 0 || value > INT32_MAX) return BSW_E_INVAL; ctx->kp.gq32_max = (int32_t)value; return BSW_OK;
    case BSW_OPT_KERNEL8: if (value < 0 || value > 2) return BSW_E_INVAL; ctx->kp.kern8 = (int8_t)value; return BSW_OK;
    case BSW_OPT_FORK: if (!b01) return BSW_E_INVAL; ctx->kp.fork = (int8_t)value; return BSW_OK;
    case BSW_OPT_SORTKEY: if (!b01) return BSW_E_INVAL; ctx->kp.keymode = value ? 2 : 0; return BSW_OK;
    case BSW_OPT_GLOB_BAND: if (!b01) return BSW_E_INVAL; ctx->glob_band = (int)value; return BSW_OK;
    case BSW_OPT_EXT_CHUNK: if (value < 0) return BSW_E_INVAL; ctx->ext_chunk = value; return BSW_OK;
    case BSW_OPT_LONG: if (value < 0 || value > 2) return BSW_E_INVAL; ctx->kp.long_route = (int8_t)value; return BSW_OK;
    case BSW_OPT_HOST_CHUNK: if (value < 1 || value > INT32_MAX) return BSW_E_INVAL; ctx->host_chunk = (int32_t)value; return BSW_OK;
    case BSW_OPT_HOST_PACK: if (value != 2 && value != 4) return BSW_E_INVAL; ctx->host_pack = (int)value; return BSW_OK;
    case BSW_OPT_SMALL_BATCH: if (value < 0 || value > INT32_MAX) return BSW_E_INVAL; ctx->kp.small_batch = (int32_t)value; return BSW_OK;
    case BSW_OPT_MID_BATCH: if (value < 0 || value > INT32_MAX) return BSW_E_INVAL; ctx->kp.mid_batch = (int32_t)value; return BSW_OK;
    case BSW_OPT_GROUP_KERNEL: if (!b01) return BSW_E_INVAL; ctx->kp.group_kernel = (int8_t)value; return BSW_OK;
    case BSW_OPT_SPLIT_MIN: if (value < 0) return BSW_E_INVAL; ctx->split_min = value; return BSW_OK;
    case BSW_OPT_COALESCE: if (value < 0 || value > INT32_MAX) return BSW_E_INVAL; ctx->coalesce = (int32_t)value; return BSW_OK;
    case BSW_OPT_COALESCE_LEADERS:
        if (value < 1 || value > 16) return BSW_E_INVAL;
        for (auto &d : ctx->devs) {
            std::lock_guard<std::mutex> g(d->agg_mu);
            d->agg_leaders_max = (int)value;
        }
        return BSW_OK;
    case BSW_OPT_COALESCE_LINGER:
        if (value < 0 || value > 100000) return BSW_E_INVAL;
        for (auto &d : ctx->devs) {
            std::lock_guard<std::mutex> g(d->agg_mu);
            d->agg_linger_us = (int)value;
        }
        return BSW_OK;
    case BSW_OPT_TEST_MISROUTE: if (!b01) return BSW_E_INVAL; ctx->kp.misroute = (int8_t)value; return BSW_OK;
    case BSW_OPT_TEST_FAIL_ALLOC:
        if (value < 0 || value > 1000000) return BSW_E_INVAL;
        bsw::g_fail_alloc.store((int)value);
        return BSW_OK;
    default: return BSW_E_INVAL;
    }
}

int bsw_last_stats(bsw_ctx_t *ctx, bsw_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->last;
    return BSW_OK;
}

const char *bsw_strerror(int code)
{
    switch (code) {
    case BSW_OK: return "ok";
    case BSW_E_INVAL: return "invalid argument";
    case BSW_E_NOMEM: return "out of device or pinned host memory";
    case BSW_E_NODEV: return "no such HIP device";
    case BSW_E_HIP: return "HIP runtime error";
    case BSW_E_RANGE: return "pair exceeds supported lengths";
    default: return "unknown error";
    }
}

int bsw_abi_version(void) { return BSW_ABI_VERSION; }

}  // extern "C"

// ---------------------------------------------------------------- final alignments (bsw_aln.h)
namespace bsw {

static_assert(kAlnMetaSpread * 16 <= kMetaMaxq && kMetaMaxq + kAlnCntWords <= kMetaWords, "aln meta fits d_meta");

// plan + gap-free -> per pass: build -> ksw_global2 (glob_device) -> finish.  Everything on `st`;
// the host waits once for the plan's counts and once per pass for the next pass's job count.
static int reg2aln_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_ext_opt_t &opt,
                          const uint8_t *d_reads, const int64_t *d_read_off, const int32_t *d_read_len,
                          int32_t n_reads, const bsw_alnreg_t *d_regs, const int32_t *d_reg_read, int32_t n,
                          bsw_aln_t *d_aln, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                          int32_t md_stride, bsw_aln_stats_t &as)
{
    const bsw_params_t &pr = ctx->params;
    AlnParams p{};
    p.W = opt.w; p.a = pr.mat[0];
    p.o_del = pr.o_del; p.e_del = pr.e_del; p.o_ins = pr.o_ins; p.e_ins = pr.e_ins;
    p.n_reads = n_reads;
    p.cigar_stride = cigar_stride; p.md_stride = md_stride;
    p.ref_len = dc.refres_len; p.l_pac = opt.l_pac;
    memcpy(p.mat, pr.mat, 25);
    GlobParams gp;
    make_glob_params(pr, ctx->glob_band, gp);
    BSW_TRY(s.d_ast.grow((size_t)n));
    BSW_TRY(s.d_alist.grow(2 * (size_t)n));
    BSW_TRY(s.d_acnt.grow(kAlnCntWords));
    if (!s.ev2) BSW_TRY(hipEventCreate(&s.ev2.p));
    if (!s.ev3) BSW_TRY(hipEventCreate(&s.ev3.p));
    int32_t *h_cnt = s.h_meta + kMetaMaxq;
    float ms = 0.f;
    BSW_TRY(hipEventRecord(s.ev2, st));
    BSW_TRY(launch_aln_plan(p, d_read_len, d_regs, d_reg_read, n, s.d_ast, s.d_alist, s.d_acnt, s.d_meta, d_aln, st));
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_meta, kAlnMetaSpread * 16 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_cnt, s.d_acnt, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    // (regions the plan found in error are marked rejected: the gap-free kernel skips them)
    BSW_TRY(launch_aln_gapfree(p, d_reads, d_read_off, d_read_len, d_regs, d_reg_read, n, s.d_ast, dc.d_refres, d_aln,
                               d_cigar, d_md, st));
    BSW_TRY(hipEventRecord(s.ev3, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
    as.helper_ms += ms;
    int32_t m[5] = {0, 0, 0, 0, 0};
    for (int sl = 0; sl < kAlnMetaSpread; ++sl) {
        const int32_t *v = s.h_meta + sl * 16;
        m[0] |= v[0]; m[1] += v[1]; m[2] += v[2]; m[3] = std::max(m[3], v[3]); m[4] = std::max(m[4], v[4]);
    }
    if (m[0]) return BSW_E_RANGE;
    as.n_rejected = m[1];
    as.n_gapfree = m[2];
    p.qstride = std::max(m[3], 1);                      // longest DP query / reference span
    p.tstride = std::max(m[4], 1);
    int32_t nj = h_cnt[0];
    for (int pass = 0; pass < 3 && nj > 0; ++pass) {
        as.n_dp[pass] = nj;
        const int32_t *list = s.d_alist + (size_t)(pass & 1) * n;
        int32_t *next = s.d_alist + (size_t)((pass + 1) & 1) * n;
        // SeqPair idr / idq are int32: chunk so j * stride stays below 2^31
        const int32_t chunk = (int32_t)std::min<int64_t>(nj, (int64_t)INT32_MAX / std::max(p.tstride, p.qstride) - 1);
        BSW_TRY(s.d_apairs.grow((size_t)chunk));
        BSW_TRY(s.d_aq.grow((size_t)chunk * p.qstride));
        BSW_TRY(s.d_at.grow((size_t)chunk * p.tstride));
        BSW_TRY(s.d_gcig.grow((size_t)chunk * (size_t)cigar_stride));
        BSW_TRY(s.d_gncig.grow((size_t)chunk));
        for (int32_t a = 0; a < nj; a += chunk) {
            const int32_t b = std::min(nj, a + chunk);
            BSW_TRY(hipEventRecord(s.ev2, st));
            BSW_TRY(launch_aln_build(p, d_reads, d_read_off, d_regs, d_reg_read, s.d_ast, list + a, b - a, dc.d_refres,
                                     s.d_apairs, s.d_aq, s.d_at, st));
            BSW_TRY(hipEventRecord(s.ev3, st));
            bsw_global_stats_t gs;
            if (int r = glob_device(gp, s, s.d_apairs, s.d_at, s.d_aq, b - a, s.d_gcig, cigar_stride, s.d_gncig, st, &gs))
                return r;
            as.dp_ms += gs.kernel_ms;
            {
                std::lock_guard<std::mutex> g(ctx->stats_mu);   // (bsw_global_last_stats: the last DP batch)
                ctx->glob_last = gs;
            }
            BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
            as.helper_ms += ms;
            BSW_TRY(hipEventRecord(s.ev2, st));
            BSW_TRY(launch_aln_finish(p, d_read_len, d_regs, d_reg_read, s.d_ast, list + a, b - a, s.d_apairs, s.d_aq,
                                      s.d_at, s.d_gcig, s.d_gncig, next, s.d_acnt + pass + 1, d_aln, d_cigar, d_md, st));
            BSW_TRY(hipEventRecord(s.ev3, st));
            BSW_TRY(hipMemcpyAsync(h_cnt, s.d_acnt + pass + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            BSW_TRY(hipStreamSynchronize(st));
            BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
            as.helper_ms += ms;
        }
        nj = pass < 2 ? h_cnt[0] : 0;
    }
    return BSW_OK;
}

// argument checks shared by both forms; the caller holds dc.refmu shared
static int reg2aln_check(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, DeviceCtx &dc, int32_t n_reads, int32_t n_regs,
                         int32_t cigar_stride, const void *md, int32_t md_stride)
{
    if (n_reads < 0 || n_regs < 0 || cigar_stride < 1 || md_stride < 0 || (md == nullptr) != (md_stride == 0))
        return BSW_E_INVAL;
    if (!dc.d_refres) return BSW_E_INVAL;
    if (opt->w < 0 || opt->w > (1 << 28) || opt->l_pac < 0 || (opt->l_pac > 0 && dc.refres_len != 2 * opt->l_pac))
        return BSW_E_INVAL;
    return BSW_OK;
}

static void set_aln_stats(bsw_ctx_t *ctx, const bsw_aln_stats_t &as)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->aln_last = as;
}

}  // namespace bsw

extern "C" {

int bsw_reg2aln_resident(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads,
                         const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                         const bsw_alnreg_t *d_regs, const int32_t *d_reg_read, int32_t n_regs,
                         bsw_aln_t *d_aln, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                         int32_t md_stride, void *stream)
{
    if (!ctx || !opt) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (const int rc = bsw::reg2aln_check(ctx, opt, dc, n_reads, n_regs, cigar_stride, d_md, md_stride)) return rc;
    if (n_regs > 0 && (!d_reads || !d_read_off || !d_read_len || !d_regs || !d_reg_read || !d_aln || !d_cigar))
        return BSW_E_INVAL;
    bsw_aln_stats_t as{};
    as.n_regs = n_regs;
    if (n_regs > 0) {
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            hipStream_t st = stream ? (hipStream_t)stream : s.stream;
            return bsw::reg2aln_device(ctx, dc, s, st, *opt, d_reads, d_read_off, d_read_len, n_reads, d_regs,
                                       d_reg_read, n_regs, d_aln, d_cigar, cigar_stride, d_md, md_stride, as);
        });
        if (rc) return rc;
    }
    bsw::set_aln_stats(ctx, as);
    return BSW_OK;
}

int bsw_reg2aln(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *regs, const int32_t *reg_read,
                int32_t n_regs, bsw_aln_t *aln, uint32_t *cigar, int32_t cigar_stride, uint8_t *md,
                int32_t md_stride)
{
    if (!ctx || !opt) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::reg2aln_check(ctx, opt, dc, n_reads, n_regs, cigar_stride, md, md_stride)) return rc;
    if (n_regs > 0 && (!reads || !read_off || !read_len || !regs || !reg_read || !aln || !cigar)) return BSW_E_INVAL;
    bsw_aln_stats_t as{};
    as.n_regs = n_regs;
    if (n_regs > 0) {
        int64_t rbytes = 0;
        for (int32_t i = 0; i < n_reads; ++i) {
            if (read_off[i] < 0 || read_len[i] < 0) return BSW_E_RANGE;
            rbytes = std::max<int64_t>(rbytes, read_off[i] + read_len[i]);
        }
        // one staged blob: inputs, then outputs, each part 16-B aligned
        const size_t n = (size_t)n_regs, nr = (size_t)n_reads;
        const size_t part[8] = {(size_t)rbytes, nr * sizeof(int64_t), nr * sizeof(int32_t), n * sizeof(bsw_alnreg_t),
                                n * sizeof(int32_t), n * sizeof(bsw_aln_t), n * (size_t)cigar_stride * sizeof(uint32_t),
                                n * (size_t)md_stride};
        size_t off[9] = {0};
        for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + ((part[k] + 15) & ~(size_t)15);
        const void *src[5] = {reads, read_off, read_len, regs, reg_read};
        void *dst[3] = {aln, cigar, md};
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            BSW_TRY(s.d_aio.grow(off[8] + 16));
            uint8_t *b = s.d_aio;
            // (rows the kernels leave unwritten -- rejected regions, overflows -- read back as zeros)
            BSW_TRY(hipMemsetAsync(b + off[6], 0, off[8] - off[6], s.stream));
            for (int k = 0; k < 5; ++k)
                if (part[k]) BSW_TRY(hipMemcpyAsync(b + off[k], src[k], part[k], hipMemcpyHostToDevice, s.stream));
            if (int r = bsw::reg2aln_device(ctx, dc, s, s.stream, *opt, b + off[0], (const int64_t *)(b + off[1]),
                                            (const int32_t *)(b + off[2]), n_reads, (const bsw_alnreg_t *)(b + off[3]),
                                            (const int32_t *)(b + off[4]), n_regs, (bsw_aln_t *)(b + off[5]),
                                            (uint32_t *)(b + off[6]), cigar_stride, md ? b + off[7] : nullptr,
                                            md_stride, as))
                return r;
            for (int k = 0; k < 3; ++k)
                if (part[5 + k]) BSW_TRY(hipMemcpyAsync(dst[k], b + off[5 + k], part[5 + k], hipMemcpyDeviceToHost, s.stream));
            BSW_TRY(hipStreamSynchronize(s.stream));
            return BSW_OK;
        });
        if (rc) return rc;
    }
    bsw::set_aln_stats(ctx, as);
    return BSW_OK;
}

int bsw_aln_last_stats(bsw_ctx_t *ctx, bsw_aln_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->aln_last;
    return BSW_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- region selection (bsw_sel.h)
namespace bsw {

struct SelIo {                          // device pointers of one call, either form
    const uint8_t *reads;
    const int64_t *read_off;
    const int32_t *read_len;
    const bsw_seed_t *seeds;
    const int32_t *seed_read, *seed_chain;
    const bsw_alnreg_t *regs;
    const int32_t *extended, *csub;
    const float *frac_rep;
    bsw_alnreg_t *sel_regs;
    int32_t *sel_read;
    bsw_selinfo_t *sel_info;
    int32_t *read_first;
};

// runs -> gather -> step; per patch round: build -> score-only ksw_global2 (glob_device) -> step
// over the suspended reads; then scan of the kept counts -> emit.  Everything on `st`; the host
// waits once per round for the next round's job count and once for the total.
static int regs_select_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_sel_opt_t &opt,
                              const SelIo &io, int32_t n_reads, int32_t n_seeds, int32_t sel_cap, int32_t *n_sel,
                              bsw_sel_stats_t &ss)
{
    const bsw_params_t &pr = ctx->params;
    SelParams p{};
    p.W = opt.w; p.a = pr.mat[0]; p.b = opt.b;
    p.o_del = pr.o_del; p.e_del = pr.e_del; p.o_ins = pr.o_ins; p.e_ins = pr.e_ins;
    p.n_reads = n_reads; p.n_seeds = n_seeds;
    p.max_chain_gap = opt.max_chain_gap; p.min_seed_len = opt.min_seed_len;
    p.mapQ_coef_len = opt.mapQ_coef_len; p.mapQ_coef_fac = opt.mapQ_coef_fac; p.patch = opt.patch;
    p.mask_level_redun = opt.mask_level_redun; p.mask_level = opt.mask_level;
    p.ref_len = dc.refres_len; p.l_pac = opt.l_pac; p.id0 = opt.id0;
    memcpy(p.mat, pr.mat, 25);
    GlobParams gp;
    make_glob_params(pr, ctx->glob_band, gp);
    const size_t nr = (size_t)n_reads, ns = (size_t)n_seeds;
    size_t scan_bytes = 0;
    BSW_TRY(launch_sel_scan(nullptr, &scan_bytes, nullptr, nullptr, n_reads, st));
    BSW_TRY(s.d_swork.grow(std::max<size_t>(ns, 1)));
    BSW_TRY(s.d_sz.grow(std::max<size_t>(ns, 1)));
    BSW_TRY(s.d_sst.grow(std::max<size_t>(nr, 1)));
    BSW_TRY(s.d_srun.grow(2 * nr + 1));
    BSW_TRY(s.d_skept.grow(nr + 1));
    BSW_TRY(s.d_slist.grow(2 * nr + 1));
    BSW_TRY(s.d_smeta.grow(kSelMetaWords));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    if (!s.ev2) BSW_TRY(hipEventCreate(&s.ev2.p));
    if (!s.ev3) BSW_TRY(hipEventCreate(&s.ev3.p));
    int32_t *sbeg = s.d_srun, *send = s.d_srun + nr;
    int32_t *h_meta = s.h_meta;
    float ms = 0.f;
    BSW_TRY(hipEventRecord(s.ev2, st));
    BSW_TRY(hipMemsetAsync(s.d_srun, 0, (2 * nr + 1) * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_skept, 0, (nr + 1) * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_smeta, 0, kSelMetaWords * sizeof(int32_t), st));
    BSW_TRY(launch_sel_runs(io.seed_read, n_seeds, n_reads, sbeg, send, s.d_smeta, st));
    BSW_TRY(launch_sel_gather(p, sbeg, send, io.read_len, io.seeds, io.seed_chain, io.regs, io.extended, io.csub,
                              s.d_swork, s.d_sst, s.d_smeta, st));
    BSW_TRY(launch_sel_step(p, nullptr, n_reads, nullptr, sbeg, io.reads, io.read_off, io.frac_rep, dc.d_refres,
                            s.d_swork, s.d_sst, s.d_sz, s.d_slist, s.d_smeta + kSelCnt, s.d_skept, s.d_smeta, st));
    BSW_TRY(hipEventRecord(s.ev3, st));
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_smeta, kSelMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
    ss.helper_ms += ms;
    if (h_meta[kSelErr]) return BSW_E_RANGE;
    int32_t nj = h_meta[kSelCnt];
    for (int round = 0; nj > 0; ++round) {
        ss.rounds++;
        ss.n_dp += nj;
        const int cur = round & 1, nxt = cur ^ 1;
        const int32_t *list = s.d_slist + (size_t)cur * nr;
        int32_t *next = s.d_slist + (size_t)nxt * nr;
        p.qstride = std::max(h_meta[kSelMaxQ], 1);          // longest patch query / reference span so far
        p.tstride = std::max(h_meta[kSelMaxT], 1);
        // SeqPair idr / idq are int32: chunk so j * stride stays below 2^31
        const int32_t chunk = (int32_t)std::min<int64_t>(nj, (int64_t)INT32_MAX / std::max(p.tstride, p.qstride) - 1);
        BSW_TRY(s.d_apairs.grow((size_t)chunk));
        BSW_TRY(s.d_aq.grow((size_t)chunk * p.qstride));
        BSW_TRY(s.d_at.grow((size_t)chunk * p.tstride));
        BSW_TRY(hipMemsetAsync(s.d_smeta + kSelCnt + nxt, 0, sizeof(int32_t), st));
        for (int32_t a = 0; a < nj; a += chunk) {
            const int32_t b = std::min(nj, a + chunk);
            BSW_TRY(hipEventRecord(s.ev2, st));
            BSW_TRY(launch_sel_build(p, list + a, b - a, sbeg, io.reads, io.read_off, s.d_swork, s.d_sst, dc.d_refres,
                                     s.d_apairs, s.d_aq, s.d_at, st));
            BSW_TRY(hipEventRecord(s.ev3, st));
            bsw_global_stats_t gs;
            if (int r = glob_device(gp, s, s.d_apairs, s.d_at, s.d_aq, b - a, nullptr, 0, nullptr, st, &gs)) return r;
            ss.dp_ms += gs.kernel_ms;
            {
                std::lock_guard<std::mutex> g(ctx->stats_mu);   // (bsw_global_last_stats: the last DP batch)
                ctx->glob_last = gs;
            }
            BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
            ss.helper_ms += ms;
            BSW_TRY(hipEventRecord(s.ev2, st));
            BSW_TRY(launch_sel_step(p, list + a, b - a, s.d_apairs, sbeg, io.reads, io.read_off, io.frac_rep,
                                    dc.d_refres, s.d_swork, s.d_sst, s.d_sz, next, s.d_smeta + kSelCnt + nxt, s.d_skept,
                                    s.d_smeta, st));
            BSW_TRY(hipEventRecord(s.ev3, st));
            BSW_TRY(hipMemcpyAsync(h_meta, s.d_smeta, kSelMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            BSW_TRY(hipStreamSynchronize(st));
            BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
            ss.helper_ms += ms;
            if (h_meta[kSelErr]) return BSW_E_RANGE;
        }
        nj = h_meta[kSelCnt + nxt];
    }
    ss.n_regs_in = h_meta[kSelRegsIn];
    ss.n_redundant = h_meta[kSelRedundant];
    ss.n_identical = h_meta[kSelIdentical];
    ss.n_patch_tried = h_meta[kSelTried];
    ss.n_patch_ok = h_meta[kSelOk];
    ss.n_patch_ratio = h_meta[kSelRatio];
    BSW_TRY(hipEventRecord(s.ev2, st));
    BSW_TRY(launch_sel_scan(s.d_tmp, &scan_bytes, s.d_skept, io.read_first, n_reads, st));
    BSW_TRY(hipMemcpyAsync(h_meta, io.read_first + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    *n_sel = ss.n_sel = h_meta[0];
    if (h_meta[0] > sel_cap) return BSW_E_RANGE;
    BSW_TRY(launch_sel_emit(p, io.seed_read, sbeg, s.d_skept, io.read_first, s.d_swork, io.frac_rep, io.sel_regs,
                            io.sel_read, io.sel_info, st));
    BSW_TRY(hipEventRecord(s.ev3, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ms, s.ev2, s.ev3));
    ss.helper_ms += ms;
    return BSW_OK;
}

// argument checks shared by both forms; the caller holds dc.refmu shared
static int regs_select_check(const bsw_sel_opt_t *opt, DeviceCtx &dc, int32_t n_reads, int32_t n_seeds,
                             int32_t sel_cap)
{
    if (n_reads < 0 || n_seeds < 0 || sel_cap < 0) return BSW_E_INVAL;
    if (!dc.d_refres) return BSW_E_INVAL;
    if (opt->w < 0 || opt->w > (1 << 28) || opt->l_pac < 0 || (opt->l_pac > 0 && dc.refres_len != 2 * opt->l_pac))
        return BSW_E_INVAL;
    if (opt->max_chain_gap < 0 || opt->mapQ_coef_len < 0 || opt->b < 0 || opt->min_seed_len < 0) return BSW_E_INVAL;
    return BSW_OK;
}

static void set_sel_stats(bsw_ctx_t *ctx, const bsw_sel_stats_t &ss)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->sel_last = ss;
}

}  // namespace bsw

extern "C" {

void bsw_sel_opt_default(bsw_sel_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->w = 100;
    opt->max_chain_gap = 10000;
    opt->l_pac = 0;
    opt->mask_level_redun = 0.95f;
    opt->mask_level = 0.5f;
    opt->min_seed_len = 19;
    opt->b = 4;
    opt->mapQ_coef_len = 50;
    opt->mapQ_coef_fac = 3;
    opt->patch = 1;
    opt->id0 = 0;
}

int bsw_regs_select_resident(bsw_ctx_t *ctx, const bsw_sel_opt_t *opt, const uint8_t *d_reads,
                             const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                             const bsw_seed_t *d_seeds, const int32_t *d_seed_read, const int32_t *d_seed_chain,
                             const bsw_alnreg_t *d_regs, const int32_t *d_extended, int32_t n_seeds,
                             const int32_t *d_csub, const float *d_frac_rep, bsw_alnreg_t *d_sel_regs,
                             int32_t *d_sel_read, bsw_selinfo_t *d_sel_info, int32_t *d_read_first,
                             int32_t sel_cap, int32_t *n_sel, void *stream)
{
    if (!ctx || !opt || !n_sel) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (const int rc = bsw::regs_select_check(opt, dc, n_reads, n_seeds, sel_cap)) return rc;
    if (!d_read_first || (n_reads > 0 && (!d_read_off || !d_read_len)) ||
        (n_seeds > 0 && (!d_reads || !d_seeds || !d_seed_read || !d_seed_chain || !d_regs || !d_extended)) ||
        (sel_cap > 0 && (!d_sel_regs || !d_sel_read || !d_sel_info)))
        return BSW_E_INVAL;
    bsw_sel_stats_t ss{};
    ss.n_reads = n_reads;
    const bsw::SelIo io = {d_reads, d_read_off, d_read_len, d_seeds, d_seed_read, d_seed_chain, d_regs, d_extended,
                           d_csub, d_frac_rep, d_sel_regs, d_sel_read, d_sel_info, d_read_first};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::regs_select_device(ctx, dc, s, st, *opt, io, n_reads, n_seeds, sel_cap, n_sel, ss);
    });
    if (rc) return rc;
    bsw::set_sel_stats(ctx, ss);
    return BSW_OK;
}

int bsw_regs_select(bsw_ctx_t *ctx, const bsw_sel_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                    const int32_t *read_len, int32_t n_reads, const bsw_seed_t *seeds, const int32_t *seed_read,
                    const int32_t *seed_chain, const bsw_alnreg_t *regs, const int32_t *extended, int32_t n_seeds,
                    const int32_t *csub, const float *frac_rep, bsw_alnreg_t *sel_regs, int32_t *sel_read,
                    bsw_selinfo_t *sel_info, int32_t *read_first, int32_t sel_cap, int32_t *n_sel)
{
    if (!ctx || !opt || !n_sel) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::regs_select_check(opt, dc, n_reads, n_seeds, sel_cap)) return rc;
    if (!read_first || (n_reads > 0 && (!read_off || !read_len)) ||
        (n_seeds > 0 && (!reads || !seeds || !seed_read || !seed_chain || !regs || !extended)) ||
        (sel_cap > 0 && (!sel_regs || !sel_read || !sel_info)))
        return BSW_E_INVAL;
    int64_t rbytes = 0;
    for (int32_t i = 0; i < n_reads; ++i) {
        if (read_off[i] < 0 || read_len[i] < 0) return BSW_E_RANGE;
        rbytes = std::max<int64_t>(rbytes, read_off[i] + read_len[i]);
    }
    bsw_sel_stats_t ss{};
    ss.n_reads = n_reads;
    // one staged blob: inputs, then outputs, each part 16-B aligned
    const size_t ns = (size_t)n_seeds, nr = (size_t)n_reads, nc = (size_t)sel_cap;
    constexpr int kIn = 10, kAll = 14;
    const size_t part[kAll] = {(size_t)rbytes, nr * sizeof(int64_t), nr * sizeof(int32_t), ns * sizeof(bsw_seed_t),
                               ns * sizeof(int32_t), ns * sizeof(int32_t), ns * sizeof(bsw_alnreg_t),
                               ns * sizeof(int32_t), csub ? ns * sizeof(int32_t) : 0, frac_rep ? nr * sizeof(float) : 0,
                               nc * sizeof(bsw_alnreg_t), nc * sizeof(int32_t), nc * sizeof(bsw_selinfo_t),
                               (nr + 1) * sizeof(int32_t)};
    size_t off[kAll + 1] = {0};
    for (int k = 0; k < kAll; ++k) off[k + 1] = off[k] + ((part[k] + 15) & ~(size_t)15);
    const void *src[kIn] = {reads, read_off, read_len, seeds, seed_read, seed_chain, regs, extended, csub, frac_rep};
    void *dst[4] = {sel_regs, sel_read, sel_info, read_first};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(s.d_aio.grow(off[kAll] + 16));
        uint8_t *b = s.d_aio;
        for (int k = 0; k < kIn; ++k)
            if (part[k]) BSW_TRY(hipMemcpyAsync(b + off[k], src[k], part[k], hipMemcpyHostToDevice, s.stream));
        const bsw::SelIo io = {b + off[0], (const int64_t *)(b + off[1]), (const int32_t *)(b + off[2]),
                               (const bsw_seed_t *)(b + off[3]), (const int32_t *)(b + off[4]),
                               (const int32_t *)(b + off[5]), (const bsw_alnreg_t *)(b + off[6]),
                               (const int32_t *)(b + off[7]), csub ? (const int32_t *)(b + off[8]) : nullptr,
                               frac_rep ? (const float *)(b + off[9]) : nullptr, (bsw_alnreg_t *)(b + off[10]),
                               (int32_t *)(b + off[11]), (bsw_selinfo_t *)(b + off[12]), (int32_t *)(b + off[13])};
        if (int r = bsw::regs_select_device(ctx, dc, s, s.stream, *opt, io, n_reads, n_seeds, sel_cap, n_sel, ss))
            return r;
        const size_t k = (size_t)*n_sel;
        const size_t got[4] = {k * sizeof(bsw_alnreg_t), k * sizeof(int32_t), k * sizeof(bsw_selinfo_t), part[13]};
        for (int o = 0; o < 4; ++o)
            if (got[o]) BSW_TRY(hipMemcpyAsync(dst[o], b + off[10 + o], got[o], hipMemcpyDeviceToHost, s.stream));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::set_sel_stats(ctx, ss);
    return BSW_OK;
}

int bsw_sel_last_stats(bsw_ctx_t *ctx, bsw_sel_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->sel_last;
    return BSW_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- paired-end stage (bsw_pe.h)
namespace bsw {

// argument checks of both calls and both forms, before anything touches a device
static int pe_check_args(const bsw_pe_opt_t *opt, int32_t n_reads, int32_t n_regs)
{
    if (!opt || n_reads < 0 || (n_reads & 1) || n_regs < 0) return BSW_E_INVAL;
    if (opt->l_pac <= 0 || (opt->id0 & 1) || opt->max_ins < 1 || opt->max_ins > BSW_PE_MAX_INS) return BSW_E_INVAL;
    if (opt->min_seed_len < 0 || opt->b < 0 || opt->mapQ_coef_len < 0) return BSW_E_INVAL;
    return BSW_OK;
}

static int pe_check_pes(const bsw_pestat_t *pes)
{
    if (!pes) return BSW_E_INVAL;
    for (int d = 0; d < 4; ++d)
        if (!pes[d].failed && !(std::isfinite(pes[d].std) && pes[d].std > 0 && std::isfinite(pes[d].avg)))
            return BSW_E_INVAL;
    return BSW_OK;
}

// the caller holds dc.refmu shared
static int pe_check_ref(const bsw_pe_opt_t &opt, DeviceCtx &dc)
{
    return dc.d_refres && dc.refres_len != 2 * opt.l_pac ? BSW_E_INVAL : BSW_OK;
}

static void make_pe_params(const bsw_ctx_t *ctx, const bsw_pe_opt_t &opt, int32_t n_reads, int32_t n_regs, PeParams &p)
{
    const bsw_params_t &pr = ctx->params;
    memset(&p, 0, sizeof(p));
    p.s.a = pr.mat[0]; p.s.b = opt.b;
    p.s.o_del = pr.o_del; p.s.e_del = pr.e_del; p.s.o_ins = pr.o_ins; p.s.e_ins = pr.e_ins;
    p.s.n_reads = n_reads;
    p.s.min_seed_len = opt.min_seed_len; p.s.mapQ_coef_len = opt.mapQ_coef_len; p.s.mapQ_coef_fac = opt.mapQ_coef_fac;
    p.s.mask_level = opt.mask_level;
    p.s.l_pac = opt.l_pac; p.s.id0 = opt.id0;
    p.n_pairs = n_reads / 2; p.n_regs = n_regs;
    p.max_ins = opt.max_ins; p.T = opt.T; p.pen_unpaired = opt.pen_unpaired;
}

// mem_pestat's per-direction arithmetic over the counts c[v] of insert size v (bsw_pe.h)
static void pestat_of_counts(const int32_t *hist, int bins, bsw_pestat_t *pes)
{
    int64_t nmax = 0;
    for (int d = 0; d < 4; ++d) {
        const int32_t *c = hist + (size_t)d * bins;
        int64_t n = 0;
        for (int v = 0; v < bins; ++v) n += c[v];
        bsw_pestat_t r{};
        r.n = (int32_t)n;
        nmax = std::max(nmax, n);
        if (n < 10) {
            r.failed = 1;
            pes[d] = r;
            continue;
        }
        auto at = [&](int k) {                      // the k-th smallest value
            int64_t acc = 0;
            for (int v = 0; v < bins; ++v) {
                acc += c[v];
                if (acc > k) return v;
            }
            return bins - 1;
        };
        const int p25 = at((int)(.25 * n + .499)), p75 = at((int)(.75 * n + .499));
        r.low = (int)(p25 - 2.0 * (p75 - p25) + .499);
        if (r.low < 1) r.low = 1;
        r.high = (int)(p75 + 2.0 * (p75 - p25) + .499);
        int64_t x = 0;
        const int v0 = std::max(r.low, 0), v1 = std::min(r.high, bins - 1);
        for (int v = v0; v <= v1; ++v) {
            r.avg += (double)c[v] * v;              // (sums of integers: exact in any order)
            x += c[v];
        }
        r.avg /= x;
        for (int v = v0; v <= v1; ++v) r.std += (double)c[v] * ((v - r.avg) * (v - r.avg));
        r.std = sqrt(r.std / x);
        r.low = (int)(p25 - 3.0 * (p75 - p25) + .499);
        r.high = (int)(p75 + 3.0 * (p75 - p25) + .499);
        if (r.low > r.avg - 4.0 * r.std) r.low = (int)(r.avg - 4.0 * r.std + .499);
        if (r.high < r.avg + 4.0 * r.std) r.high = (int)(r.avg + 4.0 * r.std + .499);
        if (r.low < 1) r.low = 1;
        pes[d] = r;
    }
    for (int d = 0; d < 4; ++d)
        if (pes[d].failed == 0 && pes[d].n < nmax * 0.05) pes[d].failed = 1;
}

static int pe_events(Slot &s)
{
    if (!s.ev2) BSW_TRY(hipEventCreate(&s.ev2.p));
    if (!s.ev3) BSW_TRY(hipEventCreate(&s.ev3.p));
    return BSW_OK;
}

// count kernel -> the four count arrays and the error word back -> the statistics on the host
static int pe_stat_device(bsw_ctx_t *ctx, Slot &s, hipStream_t st, const bsw_pe_opt_t &opt, const bsw_alnreg_t *regs,
                          const int32_t *first, int32_t n_reads, int32_t n_regs, bsw_pestat_t *pes, bsw_pe_stats_t &ps)
{
    PeParams p;
    make_pe_params(ctx, opt, n_reads, n_regs, p);
    const int bins = opt.max_ins + 1;
    BSW_TRY(s.d_phist.grow((size_t)4 * bins));
    BSW_TRY(s.d_pmeta.grow(kPeSlots * kPeMetaWords));
    if (int r = pe_events(s)) return r;
    std::vector<int32_t> h((size_t)4 * bins);
    int32_t *h_meta = s.h_meta;
    BSW_TRY(hipMemsetAsync(s.d_phist, 0, h.size() * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_pmeta, 0, kPeSlots * kPeMetaWords * sizeof(int32_t), st));
    BSW_TRY(hipEventRecord(s.ev2, st));
    BSW_TRY(launch_pe_stat(p, regs, first, s.d_phist, s.d_pmeta, st));
    BSW_TRY(hipEventRecord(s.ev3, st));
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_pmeta, kPeSlots * kPeMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h.data(), s.d_phist, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ps.kernel_ms, s.ev2, s.ev3));
    if (h_meta[kPeErr]) return BSW_E_RANGE;
    pestat_of_counts(h.data(), bins, pes);
    for (int d = 0; d < 4; ++d) ps.n_cand[d] = pes[d].n;
    return BSW_OK;
}

// fast kernel over every pair -> general kernel over the pairs it listed (their count stays on
// the device) -> the counters back
static int pe_pair_device(bsw_ctx_t *ctx, Slot &s, hipStream_t st, const bsw_pe_opt_t &opt, const bsw_pestat_t *pes,
                          bsw_alnreg_t *regs, bsw_selinfo_t *info, const int32_t *first, int32_t n_reads,
                          int32_t n_regs, bsw_pair_t *pairs, bsw_pe_stats_t &ps)
{
    PeParams p;
    make_pe_params(ctx, opt, n_reads, n_regs, p);
    for (int d = 0; d < 4; ++d) {
        p.pes[d].avg = pes[d].avg; p.pes[d].std = pes[d].std;
        p.pes[d].low = pes[d].low; p.pes[d].high = pes[d].high; p.pes[d].failed = pes[d].failed != 0;
    }
    const size_t ng = std::max<size_t>((size_t)n_regs, 1);
    BSW_TRY(s.d_swork.grow(ng));
    BSW_TRY(s.d_sz.grow(ng));
    BSW_TRY(s.d_pv.grow(ng));
    BSW_TRY(s.d_plist.grow(std::max<size_t>((size_t)p.n_pairs, 1)));
    BSW_TRY(s.d_pmeta.grow(kPeSlots * kPeMetaWords));
    if (int r = pe_events(s)) return r;
    int32_t *h_meta = s.h_meta;
    BSW_TRY(hipMemsetAsync(s.d_pmeta, 0, kPeSlots * kPeMetaWords * sizeof(int32_t), st));
    BSW_TRY(hipEventRecord(s.ev2, st));
    BSW_TRY(launch_pe_pair_fast(p, regs, info, first, pairs, s.d_plist, s.d_pmeta, st));
    BSW_TRY(launch_pe_pair_general(p, regs, info, first, pairs, s.d_plist, s.d_swork, s.d_sz, s.d_pv, s.d_pmeta, st));
    BSW_TRY(hipEventRecord(s.ev3, st));
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_pmeta, kPeSlots * kPeMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ps.kernel_ms, s.ev2, s.ev3));
    if (h_meta[kPeErr]) return BSW_E_RANGE;
    static_assert(kPeSlots * kPeMetaWords <= kMetaWords, "the slot's pinned mirror holds the pair counters");
    for (int k = 0; k < kPeSlots; ++k) {
        const int32_t *m = h_meta + k * kPeMetaWords;
        int64_t nu;
        memcpy(&nu, m + kPeNu, sizeof(nu));
        ps.n_pairing_tried += m[kPeTried];
        ps.n_paired += m[kPePaired];
        ps.n_multi += m[kPeMulti];
        ps.n_unpaired_preferred += m[kPeUnpaired];
        ps.n_proper += m[kPeProper];
        ps.n_u += nu;
    }
    return BSW_OK;
}

static void set_pe_stats(bsw_ctx_t *ctx, const bsw_pe_stats_t &ps)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->pe_last = ps;
}

// host forms: read_first as the device will check it, so the staged sizes can be trusted
static int pe_host_first(const int32_t *read_first, int32_t n_reads, int32_t &n_regs)
{
    if (!read_first) return BSW_E_INVAL;
    if (read_first[0] < 0) return BSW_E_RANGE;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_first[r + 1] < read_first[r]) return BSW_E_RANGE;
    n_regs = read_first[n_reads];
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

void bsw_pe_opt_default(bsw_pe_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->max_ins = 10000;
    opt->min_seed_len = 19;
    opt->b = 4;
    opt->T = 30;
    opt->pen_unpaired = 17;
    opt->mapQ_coef_len = 50;
    opt->mapQ_coef_fac = 3;
    opt->mask_level = 0.5f;
}

int bsw_pe_stat_resident(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_alnreg_t *d_sel_regs,
                         const bsw_selinfo_t *d_sel_info, const int32_t *d_read_first, int32_t n_reads,
                         int32_t n_regs, bsw_pestat_t *pes, void *stream)
{
    (void)d_sel_info;                   // (the statistics read the regions alone)
    if (const int rc = bsw::pe_check_args(opt, n_reads, n_regs)) return rc;
    if (!ctx || !pes || !d_read_first || (n_regs > 0 && !d_sel_regs)) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::pe_stat_device(ctx, s, st, *opt, d_sel_regs, d_read_first, n_reads, n_regs, pes, ps);
    });
    if (rc) return rc;
    bsw::set_pe_stats(ctx, ps);
    return BSW_OK;
}

int bsw_pe_stat(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_alnreg_t *sel_regs, const bsw_selinfo_t *sel_info,
                const int32_t *read_first, int32_t n_reads, bsw_pestat_t *pes)
{
    (void)sel_info;
    if (const int rc = bsw::pe_check_args(opt, n_reads, 0)) return rc;
    if (!ctx || !pes) return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && !sel_regs) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    const size_t part[2] = {(size_t)n_regs * sizeof(bsw_alnreg_t), ((size_t)n_reads + 1) * sizeof(int32_t)};
    const size_t off1 = (part[0] + 15) & ~(size_t)15;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(s.d_aio.grow(off1 + part[1] + 16));
        uint8_t *b = s.d_aio;
        if (part[0]) BSW_TRY(hipMemcpyAsync(b, sel_regs, part[0], hipMemcpyHostToDevice, s.stream));
        BSW_TRY(hipMemcpyAsync(b + off1, read_first, part[1], hipMemcpyHostToDevice, s.stream));
        return bsw::pe_stat_device(ctx, s, s.stream, *opt, (const bsw_alnreg_t *)b, (const int32_t *)(b + off1), n_reads,
                                   n_regs, pes, ps);
    });
    if (rc) return rc;
    bsw::set_pe_stats(ctx, ps);
    return BSW_OK;
}

int bsw_pe_pair_resident(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_pestat_t *pes, bsw_alnreg_t *d_sel_regs,
                         bsw_selinfo_t *d_sel_info, const int32_t *d_read_first, int32_t n_reads, int32_t n_regs,
                         bsw_pair_t *d_pairs, void *stream)
{
    if (const int rc = bsw::pe_check_args(opt, n_reads, n_regs)) return rc;
    if (const int rc = bsw::pe_check_pes(pes)) return rc;
    if (!ctx || !d_read_first || (n_regs > 0 && (!d_sel_regs || !d_sel_info)) || (n_reads > 0 && !d_pairs))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::pe_pair_device(ctx, s, st, *opt, pes, d_sel_regs, d_sel_info, d_read_first, n_reads, n_regs, d_pairs,
                                   ps);
    });
    if (rc) return rc;
    bsw::set_pe_stats(ctx, ps);
    return BSW_OK;
}

int bsw_pe_pair(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_pestat_t *pes, bsw_alnreg_t *sel_regs,
                bsw_selinfo_t *sel_info, const int32_t *read_first, int32_t n_reads, bsw_pair_t *pairs)
{
    if (const int rc = bsw::pe_check_args(opt, n_reads, 0)) return rc;
    if (const int rc = bsw::pe_check_pes(pes)) return rc;
    if (!ctx || (n_reads > 0 && !pairs)) return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && (!sel_regs || !sel_info)) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    // one staged blob: regions, info, offsets, pairs, each part 16-B aligned
    const size_t part[4] = {(size_t)n_regs * sizeof(bsw_alnreg_t), (size_t)n_regs * sizeof(bsw_selinfo_t),
                            ((size_t)n_reads + 1) * sizeof(int32_t), (size_t)(n_reads / 2) * sizeof(bsw_pair_t)};
    size_t off[5] = {0};
    for (int k = 0; k < 4; ++k) off[k + 1] = off[k] + ((part[k] + 15) & ~(size_t)15);
    const void *src[3] = {sel_regs, sel_info, read_first};
    void *dst[4] = {sel_regs, sel_info, nullptr, pairs};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(s.d_aio.grow(off[4] + 16));
        uint8_t *b = s.d_aio;
        for (int k = 0; k < 3; ++k)
            if (part[k]) BSW_TRY(hipMemcpyAsync(b + off[k], src[k], part[k], hipMemcpyHostToDevice, s.stream));
        if (int r = bsw::pe_pair_device(ctx, s, s.stream, *opt, pes, (bsw_alnreg_t *)(b + off[0]),
                                        (bsw_selinfo_t *)(b + off[1]), (const int32_t *)(b + off[2]), n_reads, n_regs,
                                        (bsw_pair_t *)(b + off[3]), ps))
            return r;
        for (int k = 0; k < 4; ++k)
            if (dst[k] && part[k]) BSW_TRY(hipMemcpyAsync(dst[k], b + off[k], part[k], hipMemcpyDeviceToHost, s.stream));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::set_pe_stats(ctx, ps);
    return BSW_OK;
}

int bsw_pe_last_stats(bsw_ctx_t *ctx, bsw_pe_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->pe_last;
    return BSW_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- mate rescue stage (bsw_matesw.h)
namespace bsw {

// argument checks of both forms, before anything touches a device
static int matesw_check_args(const bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes,
                             int32_t n_reads, int32_t n_regs, int32_t out_cap)
{
    if (!opt || !pes || n_reads < 0 || (n_reads & 1) || n_regs < 0 || out_cap < 0) return BSW_E_INVAL;
    if (opt->l_pac <= 0 || opt->max_matesw < 0 || opt->min_seed_len <= 0 || opt->max_chain_gap < 0) return BSW_E_INVAL;
    for (int d = 0; d < 4; ++d)
        if (!pes[d].failed && pes[d].low > pes[d].high) return BSW_E_INVAL;
    if (!ctx) return BSW_E_INVAL;
    return mate_params_ok(ctx->params) ? BSW_OK : BSW_E_INVAL;
}

struct MswIo {
    const uint8_t *reads;
    const int64_t *read_off;
    const int32_t *read_len;
    const bsw_alnreg_t *regs;
    const bsw_selinfo_t *info;
    const int32_t *first;
    bsw_alnreg_t *out_regs;
    int32_t *out_read;
    bsw_selinfo_t *out_info;
    int32_t *out_first;
};

// count + scans -> round 0's step -> per round: one readback of the job count, build, the batched
// ksw_align2, the next step -> the scan of the list lengths -> emit.  The caller holds dc.refmu shared.
static int matesw_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_matesw_opt_t &opt,
                         const bsw_pestat_t *pes, const MswIo &io, int32_t n_reads, int32_t n_regs, int32_t out_cap,
                         int32_t *n_out, bsw_matesw_stats_t &ws)
{
    *n_out = 0;
    const bsw_params_t &pr = ctx->params;
    MswParams p;
    memset(&p, 0, sizeof(p));
    p.s.a = pr.mat[0];
    p.s.max_chain_gap = opt.max_chain_gap; p.s.min_seed_len = opt.min_seed_len; p.s.patch = 0;
    p.s.mask_level_redun = opt.mask_level_redun;
    p.s.l_pac = opt.l_pac; p.s.n_reads = n_reads;
    p.n_pairs = n_reads / 2; p.n_regs = n_regs;
    p.max_matesw = opt.max_matesw; p.pen_unpaired = opt.pen_unpaired;
    for (int d = 0; d < 4; ++d) {
        p.pes[d].low = pes[d].low; p.pes[d].high = pes[d].high; p.pes[d].failed = pes[d].failed != 0;
    }
    MateParams mp;
    make_mate_params(pr, mp);
    if ((int64_t)n_regs * 5 > INT32_MAX) return BSW_E_RANGE;        // the work lists' offsets are int32
    const size_t nr = (size_t)n_reads, np = nr / 2, n1 = nr + 1;
    size_t scan_bytes = 0;
    BSW_TRY(launch_sel_scan(nullptr, &scan_bytes, nullptr, nullptr, n_reads, st));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    BSW_TRY(s.d_wint.grow(5 * n1 + 2 * np + 1));
    BSW_TRY(s.d_wmeta.grow(kMswSlots * kMswMetaWords));
    BSW_TRY(s.d_wst.grow(std::max<size_t>(np, 1)));
    BSW_TRY(s.d_wjobs.grow(std::max<size_t>(4 * np, 1)));
    BSW_TRY(s.d_maln.grow(std::max<size_t>(4 * np, 1)));
    if (!s.evw0) BSW_TRY(hipEventCreate(&s.evw0.p));
    if (!s.evw1) BSW_TRY(hipEventCreate(&s.evw1.p));
    static_assert(kMswSlots * kMswMetaWords <= kMetaWords, "the slot's pinned mirror holds the stage's counters");
    int32_t *ncand = s.d_wint, *capv = ncand + n1, *coff = capv + n1, *woff = coff + n1, *nlist = woff + n1;
    int32_t *lists = nlist + n1;
    int32_t *h_meta = s.h_meta;
    constexpr size_t kMetaBytes = kMswSlots * kMswMetaWords * sizeof(int32_t);
    float ms = 0.f;
    BSW_TRY(hipMemsetAsync(s.d_wint, 0, (5 * n1) * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_wmeta, 0, kMetaBytes, st));
    BSW_TRY(hipEventRecord(s.evw0, st));
    BSW_TRY(launch_msw_count(p, io.regs, io.first, ncand, capv, s.d_wmeta, st));
    BSW_TRY(launch_sel_scan(s.d_tmp, &scan_bytes, ncand, coff, n_reads, st));
    BSW_TRY(launch_sel_scan(s.d_tmp, &scan_bytes, capv, woff, n_reads, st));
    BSW_TRY(hipEventRecord(s.evw1, st));
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_wmeta, kMswMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_meta + kMswMetaWords, coff + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_meta + kMswMetaWords + 1, woff + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ms, s.evw0, s.evw1));
    ws.helper_ms += ms;
    if (h_meta[kMswErr]) return BSW_E_RANGE;
    const size_t n_cand = (size_t)h_meta[kMswMetaWords], n_work = (size_t)h_meta[kMswMetaWords + 1];
    BSW_TRY(s.d_wcand.grow(std::max<size_t>(n_cand, 1)));
    BSW_TRY(s.d_swork.grow(std::max<size_t>(n_work, 1)));
    int32_t n_items = p.n_pairs;
    const int32_t *list = nullptr;
    for (int round = 0;; ++round) {
        int32_t *next = lists + (size_t)(round & 1) * np;
        BSW_TRY(hipEventRecord(s.evw0, st));
        BSW_TRY(launch_msw_step(p, list, n_items, io.regs, io.info, io.first, io.read_len, ncand, coff, woff, s.d_wcand,
                                s.d_swork, nlist, s.d_wst, s.d_maln, s.d_wjobs, next, s.d_wmeta, st));
        BSW_TRY(hipEventRecord(s.evw1, st));
        BSW_TRY(hipMemcpyAsync(h_meta, s.d_wmeta, kMetaBytes, hipMemcpyDeviceToHost, st));
        BSW_TRY(hipStreamSynchronize(st));
        BSW_TRY(hipEventElapsedTime(&ms, s.evw0, s.evw1));
        ws.helper_ms += ms;
        if (h_meta[kMswErr]) return BSW_E_RANGE;
        const int32_t nj = h_meta[kMswNJobs];
        if (nj == 0) break;
        ++ws.rounds;
        n_items = h_meta[kMswNext];
        list = next;
        p.qstride = std::max(h_meta[kMswMaxQ], 1);
        p.tstride = std::max(h_meta[kMswMaxT], 1);
        // SeqPair idr / idq are int32: chunk so j * stride stays below 2^31
        const int32_t chunk = (int32_t)std::min<int64_t>(nj, (int64_t)INT32_MAX / std::max(p.tstride, p.qstride) - 1);
        BSW_TRY(s.d_apairs.grow((size_t)chunk));
        BSW_TRY(s.d_aq.grow((size_t)chunk * p.qstride));
        BSW_TRY(s.d_at.grow((size_t)chunk * p.tstride));
        BSW_TRY(hipMemsetAsync(s.d_wmeta + kMswNext, 0, 4 * sizeof(int32_t), st));      // the round's words
        for (int32_t a = 0; a < nj; a += chunk) {
            const int32_t b = std::min(nj, a + chunk);
            BSW_TRY(hipEventRecord(s.evw0, st));
            BSW_TRY(launch_msw_build(p, s.d_wjobs + a, b - a, io.reads, io.read_off, io.read_len, dc.d_refres, s.d_apairs,
                                     s.d_aq, s.d_at, st));
            BSW_TRY(hipEventRecord(s.evw1, st));
            bsw_mate_stats_t mst;
            if (int r = mate_device(mp, s, s.d_apairs, s.d_at, s.d_aq, b - a, s.d_maln + a, st, &mst)) return r;
            ws.sw_ms += mst.fwd_ms + mst.rev_ms;
            BSW_TRY(hipEventElapsedTime(&ms, s.evw0, s.evw1));
            ws.helper_ms += ms;
        }
    }
    for (int k = 0; k < kMswSlots; ++k) {
        const int32_t *m = h_meta + k * kMswMetaWords;
        ws.n_calls += m[kMswCalls];
        ws.n_calls_all_skipped += m[kMswAllSkipped];
        ws.n_jobs += m[kMswJobs];
        ws.n_jobs_u8 += m[kMswJobsU8];
        ws.n_short_window += m[kMswShort];
        ws.n_pushed += m[kMswPushed];
        ws.n_redundant += m[kMswRedundant];
        ws.n_identical += m[kMswIdentical];
        ws.n_lists_changed += m[kMswChanged];
    }
    BSW_TRY(hipEventRecord(s.evw0, st));
    BSW_TRY(launch_sel_scan(s.d_tmp, &scan_bytes, nlist, io.out_first, n_reads, st));
    BSW_TRY(hipMemcpyAsync(h_meta, io.out_first + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    *n_out = ws.n_out = h_meta[0];
    if (h_meta[0] > out_cap) return BSW_E_RANGE;
    BSW_TRY(launch_msw_emit(p, woff, nlist, io.out_first, s.d_swork, io.out_regs, io.out_read, io.out_info, st));
    BSW_TRY(hipEventRecord(s.evw1, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(hipEventElapsedTime(&ms, s.evw0, s.evw1));
    ws.helper_ms += ms;
    return BSW_OK;
}

static void set_matesw_stats(bsw_ctx_t *ctx, const bsw_matesw_stats_t &ws)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    ctx->matesw_last = ws;
}

}  // namespace bsw

extern "C" {

void bsw_matesw_opt_default(bsw_matesw_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->max_matesw = 50;
    opt->pen_unpaired = 17;
    opt->min_seed_len = 19;
    opt->max_chain_gap = 10000;
    opt->mask_level_redun = 0.95f;
}

int bsw_matesw_resident(bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes,
                        const uint8_t *d_reads, const int64_t *d_read_off, const int32_t *d_read_len,
                        int32_t n_reads, const bsw_alnreg_t *d_sel_regs, const bsw_selinfo_t *d_sel_info,
                        const int32_t *d_read_first, int32_t n_regs, bsw_alnreg_t *d_out_regs,
                        int32_t *d_out_read, bsw_selinfo_t *d_out_info, int32_t *d_out_first, int32_t out_cap,
                        int32_t *n_out, void *stream)
{
    if (const int rc = bsw::matesw_check_args(ctx, opt, pes, n_reads, n_regs, out_cap)) return rc;
    if (!n_out || !d_read_first || !d_out_first || (n_reads > 0 && (!d_reads || !d_read_off || !d_read_len)) ||
        (n_regs > 0 && (!d_sel_regs || !d_sel_info)) || (out_cap > 0 && (!d_out_regs || !d_out_read || !d_out_info)))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (!dc.d_refres || dc.refres_len != 2 * opt->l_pac) return BSW_E_INVAL;
    bsw_matesw_stats_t ws{};
    ws.n_pairs = n_reads / 2;
    const bsw::MswIo io = {d_reads, d_read_off, d_read_len, d_sel_regs, d_sel_info, d_read_first,
                           d_out_regs, d_out_read, d_out_info, d_out_first};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::matesw_device(ctx, dc, s, st, *opt, pes, io, n_reads, n_regs, out_cap, n_out, ws);
    });
    if (rc) return rc;
    bsw::set_matesw_stats(ctx, ws);
    return BSW_OK;
}

int bsw_matesw(bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes, const uint8_t *reads,
               const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *sel_regs,
               const bsw_selinfo_t *sel_info, const int32_t *read_first, bsw_alnreg_t *out_regs,
               int32_t *out_read, bsw_selinfo_t *out_info, int32_t *out_first, int32_t out_cap, int32_t *n_out)
{
    if (const int rc = bsw::matesw_check_args(ctx, opt, pes, n_reads, 0, out_cap)) return rc;
    if (!n_out || !out_first || (n_reads > 0 && (!reads || !read_off || !read_len)) ||
        (out_cap > 0 && (!out_regs || !out_read || !out_info)))
        return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && (!sel_regs || !sel_info)) return BSW_E_INVAL;
    int64_t rbytes = 0;
    for (int32_t i = 0; i < n_reads; ++i) {
        if (read_off[i] < 0 || read_len[i] < 0) return BSW_E_RANGE;
        rbytes = std::max<int64_t>(rbytes, read_off[i] + read_len[i]);
    }
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (!dc.d_refres || dc.refres_len != 2 * opt->l_pac) return BSW_E_INVAL;
    bsw_matesw_stats_t ws{};
    ws.n_pairs = n_reads / 2;
    // one staged blob: inputs, then outputs, each part 16-B aligned
    const size_t nr = (size_t)n_reads, ng = (size_t)n_regs, nc = (size_t)out_cap;
    constexpr int kIn = 6, kAll = 10;
    const size_t part[kAll] = {(size_t)rbytes, nr * sizeof(int64_t), nr * sizeof(int32_t), ng * sizeof(bsw_alnreg_t),
                               ng * sizeof(bsw_selinfo_t), (nr + 1) * sizeof(int32_t), nc * sizeof(bsw_alnreg_t),
                               nc * sizeof(int32_t), nc * sizeof(bsw_selinfo_t), (nr + 1) * sizeof(int32_t)};
    size_t off[kAll + 1] = {0};
    for (int k = 0; k < kAll; ++k) off[k + 1] = off[k] + ((part[k] + 15) & ~(size_t)15);
    const void *src[kIn] = {reads, read_off, read_len, sel_regs, sel_info, read_first};
    void *dst[4] = {out_regs, out_read, out_info, out_first};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(s.d_aio.grow(off[kAll] + 16));
        uint8_t *b = s.d_aio;
        for (int k = 0; k < kIn; ++k)
            if (part[k]) BSW_TRY(hipMemcpyAsync(b + off[k], src[k], part[k], hipMemcpyHostToDevice, s.stream));
        const bsw::MswIo io = {b + off[0], (const int64_t *)(b + off[1]), (const int32_t *)(b + off[2]),
                               (const bsw_alnreg_t *)(b + off[3]), (const bsw_selinfo_t *)(b + off[4]),
                               (const int32_t *)(b + off[5]), (bsw_alnreg_t *)(b + off[6]), (int32_t *)(b + off[7]),
                               (bsw_selinfo_t *)(b + off[8]), (int32_t *)(b + off[9])};
        const int r = bsw::matesw_device(ctx, dc, s, s.stream, *opt, pes, io, n_reads, n_regs, out_cap, n_out, ws);
        if (r == BSW_E_RANGE && *n_out > out_cap) {        // (d_out_first is still written)
            BSW_TRY(hipMemcpyAsync(out_first, b + off[9], part[9], hipMemcpyDeviceToHost, s.stream));
            BSW_TRY(hipStreamSynchronize(s.stream));
        }
        if (r) return r;
        const size_t k = (size_t)*n_out;
        const size_t got[4] = {k * sizeof(bsw_alnreg_t), k * sizeof(int32_t), k * sizeof(bsw_selinfo_t), part[9]};
        for (int o = 0; o < 4; ++o)
            if (got[o]) BSW_TRY(hipMemcpyAsync(dst[o], b + off[6 + o], got[o], hipMemcpyDeviceToHost, s.stream));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::set_matesw_stats(ctx, ws);
    return BSW_OK;
}

int bsw_matesw_last_stats(bsw_ctx_t *ctx, bsw_matesw_stats_t *out)
{
    if (!ctx || !out) return BSW_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    *out = ctx->matesw_last;
    return BSW_OK;
}

}  // extern "C"
