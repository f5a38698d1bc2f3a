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
#include "bsw_sort.h"
#include "bsw_mate_k.h"
#include "bsw_global_k.h"
#include "bsw_ext_k.h"

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
void make_mate_params(const bsw_params_t &p, MateParams &mp)
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

bool mate_params_ok(const bsw_params_t &p)
{
    int mx = 0;
    for (int i = 0; i < 25; ++i) mx = std::max(mx, (int)p.mat[i]);
    return p.o_ins >= 1 && mx >= 1;
}

// Forward pass (ksw_u8 / ksw_i16 per job) then, for jobs with KSW_XSTART, the reverse pass;
// each pass: device bucketing by (P, slen), one readback of the bucket ranges, one launch per
// ncol class.  Blocking.
int mate_device(const MateParams &mp, Slot &s, const SeqPair *d_pairs, const uint8_t *d_ref, const uint8_t *d_qer,
                int32_t n, bsw_kswr_t *d_aln, hipStream_t st, bsw_mate_stats_t *stats)
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
void make_glob_params(const bsw_params_t &p, int prefer_band, GlobParams &gp)
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
int glob_device(const GlobParams &gp, Slot &s, SeqPair *d_pairs, const uint8_t *d_ref, const uint8_t *d_qer,
                int32_t n, uint32_t *d_cigar, int32_t stride, int32_t *d_ncig, hipStream_t st,
                bsw_global_stats_t *stats)
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
    add_counters(*st, b);
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
            if (!pair_valid(pairs[i])) return BSW_E_RANGE;
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
        add_counters(agg, st[d]);
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

int ctx_contigs(bsw_ctx_t *ctx, int64_t l_pac, int64_t ref_len, ContigView *dev, std::vector<int64_t> *host_off)
{
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> g(dc.refmu);
    if (dc.n_ctg > 0 && dc.ctg_sum != (l_pac > 0 ? l_pac : ref_len)) return BSW_E_INVAL;
    if (dev) *dev = dc.ctg_view(l_pac);
    if (host_off) *host_off = dc.n_ctg > 0 ? dc.h_ctg_off : std::vector<int64_t>();
    return BSW_OK;
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

void set_chain_stats(bsw_ctx_t *ctx, const bsw_chain_stats_t &s) { put_stats(ctx, &bsw_ctx::chain_last, s); }
int get_chain_stats(bsw_ctx_t *ctx, bsw_chain_stats_t *out) { return get_stats(ctx, &bsw_ctx::chain_last, out); }
void set_ext_stats(bsw_ctx_t *ctx, const bsw_ext_stats_t &s) { put_stats(ctx, &bsw_ctx::ext_last, s); }
int get_ext_stats(bsw_ctx_t *ctx, bsw_ext_stats_t *out) { return get_stats(ctx, &bsw_ctx::ext_last, out); }

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
    bsw::put_stats(ctx, &bsw_ctx::last, st);
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
        bsw::put_stats(ctx, &bsw_ctx::last, s.stats);
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
        bsw::put_stats(ctx, &bsw_ctx::last, s.stats);
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
        bsw::put_stats(ctx, &bsw_ctx::mate_last, ms);
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
    bsw::put_stats(ctx, &bsw_ctx::mate_last, agg);
    return BSW_OK;
}

int bsw_mate_last_stats(bsw_ctx_t *ctx, bsw_mate_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::mate_last, out); }

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
        bsw::put_stats(ctx, &bsw_ctx::glob_last, gs);
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
    bsw::put_stats(ctx, &bsw_ctx::glob_last, agg);
    return BSW_OK;
}

int bsw_global_last_stats(bsw_ctx_t *ctx, bsw_global_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::glob_last, out); }

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

int bsw_set_contigs(bsw_ctx_t *ctx, int32_t n, const int64_t *len, const char *const *names)
{
    if (!ctx || n < 0 || (n > 0 && (!len || !names))) return BSW_E_INVAL;
    std::vector<int64_t> off((size_t)n + 1, 0);
    std::vector<int32_t> name_off((size_t)n + 1, 0);
    std::vector<uint8_t> bytes;
    for (int32_t i = 0; i < n; ++i) {
        if (len[i] <= 0 || len[i] > INT64_MAX / 2 - off[i] || !names[i]) return BSW_E_INVAL;
        const size_t l = strnlen(names[i], BSW_CONTIG_MAX_NAME + 1);
        if (l < 1 || l > BSW_CONTIG_MAX_NAME) return BSW_E_INVAL;
        off[i + 1] = off[i] + len[i];
        bytes.insert(bytes.end(), names[i], names[i] + l);
        name_off[i + 1] = (int32_t)bytes.size();
    }
    // the limits the pair kernels' sort coordinate relies on (kPeRidShift, bsw_pe_k.h): stated in bsw_contigs.h
    if (n > BSW_CONTIG_MAX_N || off[(size_t)n] > BSW_CONTIG_MAX_SUM) return BSW_E_INVAL;
    // every device's copy first, then the switch: a failure leaves the table that is set on all of them
    struct Staged {
        bsw::DevBuf<int64_t> off;
        bsw::DevBuf<uint8_t> names;
        bsw::DevBuf<int32_t> name_off;
    };
    std::vector<Staged> staged(ctx->devs.size());
    for (size_t d = 0; n > 0 && d < ctx->devs.size(); ++d) {
        Staged &t = staged[d];
        BSW_TRY(hipSetDevice(ctx->devs[d]->device));
        BSW_TRY(t.off.reserve_exact(off.size()));
        BSW_TRY(t.name_off.reserve_exact(name_off.size()));
        BSW_TRY(t.names.reserve_exact(bytes.size()));
        hipStream_t cs = nullptr;                           // (a stream of its own, as bsw_set_reference)
        BSW_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        hipError_t e = hipMemcpyAsync(t.off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, cs);
        if (e == hipSuccess)
            e = hipMemcpyAsync(t.name_off, name_off.data(), name_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipMemcpyAsync(t.names, bytes.data(), bytes.size(), hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipStreamSynchronize(cs);
        (void)hipStreamDestroy(cs);
        BSW_TRY(e);
    }
    for (size_t d = 0; d < ctx->devs.size(); ++d) {
        bsw::DeviceCtx &dc = *ctx->devs[d];
        std::unique_lock<std::shared_mutex> g(dc.refmu);   // waits for running stage calls
        (void)hipSetDevice(dc.device);                      // (the old buffers are freed below, on their device)
        std::swap(dc.d_ctg_off, staged[d].off);
        std::swap(dc.d_ctg_names, staged[d].names);
        std::swap(dc.d_ctg_name_off, staged[d].name_off);
        dc.n_ctg = n;
        dc.ctg_sum = off[(size_t)n];
        dc.h_ctg_off = off;
        dc.h_ctg_names = bytes;
        dc.h_ctg_name_off = name_off;
        staged[d] = Staged();
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
    if (!dc.ctg_ok(opt->l_pac)) return BSW_E_INVAL;
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
        xp.ctg = dc.ctg_view(opt->l_pac);
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

int bsw_last_stats(bsw_ctx_t *ctx, bsw_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::last, out); }

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
