// bsw_dispatch.hip -- one batch on one slot's device (bsw_engine.h): plan -> sort -> DP kernels.
//
//   plan_kernel   : per pair -> kernel class (lane QMAX bucket 32..160 | wide) + sort key
//                   (class, qlen desc, tlen desc) so every wavefront gets 64 like-shaped pairs
//   radix sort    : the stable LSD radix sort of bsw_sort.hip over the bits of the 32-bit key that
//                   vary in this batch (plan_kernel reduces them) -> order[] (= sortPairsLen)
//   DP kernels    : one launch per non-empty class over its slice of order[]
//   results       : written by the kernels straight into the SeqPair records
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "bsw_engine.h"
#include "bsw_sort.h"
#include <emmintrin.h>

namespace bsw {

constexpr int kNumLaneClasses = 5;          // QMAX 32, 64, 96, 128, 160
constexpr int kPkClass0 = kNumLaneClasses;  // packed kernel, same QMAX buckets (classes 5..9)
constexpr int kWideClass = kPkClass0 + kNumLaneClasses;   // index of the wide-kernel class
constexpr int kWvClass0 = kWideClass + 1;   // wave-per-alignment kernel, 4 / 8 / 16 columns per lane
constexpr int kNumWvClasses = 3;
constexpr int kWvCols[kNumWvClasses] = {4, 8, 16};
constexpr int kNumClasses = kWvClass0 + kNumWvClasses;
static_assert(kNumClasses <= kMetaKeyOr, "class counts, then the key mask's two words (bsw_sort.h)");
static_assert(kNumLaneClasses <= kMetaRedoWords && kMetaRedo + kMetaRedoWords <= kMetaWords, "redo-list lengths");

// Lifetime predictor for the sort key (scheduling only, results never depend on it): does the
// query look like an extension of the target near the seed?  Identity of query[10, 40) with
// target[10 + s, 40 + s), best over |s| <= 6; > 18 of 30 matches = related.  Unrelated pairs
// die within a few dozen rows and shrink their band ends on the way; giving them their own
// wavefronts keeps the related waves' band edges uniform (masked groups
// 25% -> 11% at C2 in simulation).  The identity count itself is the next sort field: it tracks
// the pair's score along the first rows, hence its band-end trajectory and its lifetime.
__device__ __forceinline__ int seed_matches(const uint8_t *__restrict__ q, int qlen,
                                            const uint8_t *__restrict__ r, int tlen)
{
    if (qlen < 40 || tlen < 46) return 31;
    uint8_t qb[30], rb[42];
#pragma unroll
    for (int j = 0; j < 30; ++j) qb[j] = q[10 + j];
#pragma unroll
    for (int j = 0; j < 42; ++j) rb[j] = r[4 + j];
    int best = 0;
#pragma unroll
    for (int sft = 0; sft <= 12; ++sft) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < 30; ++j) c += qb[j] == rb[j + sft];
        best = max(best, c);
    }
    return best;                    // identities of the best shift (of 30); > 18: related
}

// Per pair: class + sort key.  Lane classes need qlen <= QMAX and int16-safe scores.
// Wave-kernel class for a pair (bsw_wv.hip contract), -1 if it does not qualify.
__device__ __forceinline__ int wv_class(const KParams &kp, int32_t w, int qlen, int tlen, int h0)
{
    if (kp.maxsc != 1 || qlen > kWvQmax || h0 < 0) return -1;
    if ((int64_t)kp.e_ins * qlen >= 2700) return -1;
    // E and F live in int16 lanes updated by wrapping v_pk_sub_i16 (bsw_wv.hip): keep the gap
    // steps far from the int16 range
    if (128 + kp.o_del + 2 * kp.e_del >= 30000 || 128 + kp.o_ins + 2 * kp.e_ins >= 30000) return -1;
    if ((int64_t)h0 + min(qlen, tlen) + (int64_t)kp.e_ins * (qlen + 1) >= 30000) return -1;
    int wl = w;
    const int ni = qlen * kp.maxsc + kp.end_bonus - kp.o_ins;
    const int nd = qlen * kp.maxsc + kp.end_bonus - kp.o_del;
    wl = min(wl, max((ni + kp.e_ins) / kp.e_ins, 1));
    wl = min(wl, max((nd + kp.e_del) / kp.e_del, 1));
    for (int k = 0; k < kNumWvClasses; ++k)
        if (2 * wl + kWvCols[k] + 2 <= 64 * kWvCols[k]) return kWvClass0 + k;
    return -1;
}

__global__ void plan_kernel(const SeqPair *__restrict__ pairs, int32_t n, const KParams kp, int32_t w,
                            int32_t pc_route, int32_t wv_route, const uint8_t *__restrict__ ref,
                            const uint8_t *__restrict__ qer, uint32_t *__restrict__ keys,
                            int32_t *__restrict__ vals, int32_t *__restrict__ counts,
                            int32_t *__restrict__ maxq_wide, int keymode, int misroute)
{
    const int maxsc = kp.maxsc;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    SeqPair p{};
    if (valid) p = pairs[i];
    const int qlen = max(p.len2, 0), tlen = max(p.len1, 0);
    const int64_t hi = (int64_t)max(p.h0, 0) + (int64_t)max(maxsc, 0) * min(qlen, tlen);
    int c = kWideClass;
    // queries past the register kernels' 160 columns: the wave-per-alignment kernel
    // (BSW_OPT_LONG 1, default); BSW_OPT_LONG 2 sends every qualifying pair there (tests)
    const int wvc = wv_route ? wv_class(kp, w, qlen, tlen, p.h0) : -1;
    if (wv_route == 2 && wvc >= 0) c = wvc;
    else if (hi < 32768 && p.h0 >= 0) {
        if (qlen <= 32) c = 0;
        else if (qlen <= 64) c = 1;
        else if (qlen <= 96) c = 2;
        else if (qlen <= 128) c = 3;
        else if (qlen <= 160) c = 4;
        // 8-bit score regime (key H << 8 | j fits 16 bits, H <= h0 + min(qlen, tlen)) -> the
        // packed-column kernel (needs qlen < QMAX: bucket by qlen + 1)
        if (pc_route && c < kNumLaneClasses && p.h0 + min(qlen, tlen) <= 255 && qlen + 1 <= 160)
            c = kPkClass0 + (qlen + 1 <= 32 ? 0 : qlen + 1 <= 64 ? 1 : qlen + 1 <= 96 ? 2 : qlen + 1 <= 128 ? 3 : 4);
    }
    if (c == kWideClass && wvc >= 0) c = wvc;
    if (misroute) c = 0;          // BSW_OPT_TEST_MISROUTE: the QMAX=32 lane kernel's guard must trip
    uint32_t key = 0;
    if (valid) {
        if (c == kWideClass) atomicMax(maxq_wide, qlen);
        // (class, qlen desc, related first, tlen desc, h0 desc): like-shaped pairs share a
        // wavefront; equal h0 and relatedness give lanes similar band-end trajectories
        const int mt = (c == kWideClass) ? 31 : seed_matches(qer + p.idq, qlen, ref + p.idr, tlen);
        const int rel = mt > 18;
        // sort key (scheduling only; results never depend on it).  Default: (class, qlen desc,
        // related first, tlen / 32 desc, seed identities desc, h0 desc) -- pairs that align
        // alike share a wavefront, so their band ends move together (C2 kernel 9.58 -> 8.60 ms vs
        // the h0-only order, BSW_SORTKEY=0)
        if (keymode == 0)
            key = ((uint32_t)c << 28) | ((uint32_t)(255 - min(qlen, 255)) << 20) |
                      ((uint32_t)(1 - rel) << 19) | ((uint32_t)(2047 - min(tlen, 2047)) << 8) |
                      (uint32_t)(255 - min(max(p.h0, 0), 255));
        else
            key = ((uint32_t)c << 28) | ((uint32_t)(255 - min(qlen, 255)) << 20) |
                      ((uint32_t)(1 - rel) << 19) | ((uint32_t)(63 - min(tlen >> 5, 63)) << 13) |
                      ((uint32_t)(31 - min(mt, 31)) << 8) | (uint32_t)(255 - min(max(p.h0, 0), 255));
        keys[i] = key;
        vals[i] = i;
    }
    // class counts: wave ballots -> LDS per block -> one global add per block and class into the
    // block's slot (32 slots in separate 64-B lines; same-line atomics from every wave cost
    // ~10 ns each, 0.16-0.7 ms per 1M pairs)
    // the key mask rides on the same two barriers: which key bits vary in this batch (bsw_sort.h)
    __shared__ int s_cnt[kNumClasses];
    __shared__ uint32_t s_or[2];
    if (threadIdx.x < kNumClasses) s_cnt[threadIdx.x] = 0;
    key_mask_zero(s_or);
    __syncthreads();
    key_mask_add(key, valid, s_or);
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kNumClasses; ++k) {
        const unsigned long long m = __ballot(valid && c == k);
        if (m && lane == __ffsll((long long)m) - 1) atomicAdd(&s_cnt[k], __popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < kNumClasses && s_cnt[threadIdx.x])
        atomicAdd(&counts[(blockIdx.x % kMetaSpread) * kMetaCounts + threadIdx.x], s_cnt[threadIdx.x]);
    key_mask_flush(s_or, counts);
}

void make_kparams(const bsw_params_t &p, KParams &kp)
{
    memset(&kp, 0, sizeof(kp));
    kp.o_del = p.o_del; kp.e_del = p.e_del; kp.o_ins = p.o_ins; kp.e_ins = p.e_ins;
    kp.zdrop = p.zdrop; kp.end_bonus = p.end_bonus;
    int mx = 0;
    for (int i = 0; i < 25; ++i) mx = std::max(mx, (int)p.mat[i]);
    kp.maxsc = mx;
    memcpy(kp.mat, p.mat, 25);
    // prof[t] byte q = mat[t][q] for q < 5; q = 5..7 (invalid codes) score as N
    for (int t = 0; t < 8; ++t) {
        const int tt = std::min(t, 4);
        uint8_t b[8];
        for (int q = 0; q < 8; ++q) b[q] = (uint8_t)p.mat[tt * 5 + std::min(q, 4)];
        kp.prof[t][0] = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
        kp.prof[t][1] = b[4] | (b[5] << 8) | (b[6] << 16) | ((uint32_t)b[7] << 24);
    }
    // packed-column kernel scoring contract (bsw_pc.hip): match 1, one mismatch value in
    // [-127, -1], every N entry -1, symmetric gap penalties.
    bool ok = p.o_del == p.o_ins && p.e_del == p.e_ins && p.e_del > 0 && p.o_del + p.e_del < 4096;
    const int mis = p.mat[1];
    ok = ok && mis < 0 && mis >= -127;
    for (int a = 0; a < 5 && ok; ++a)
        for (int b = 0; b < 5 && ok; ++b) {
            const int v = p.mat[a * 5 + b];
            ok = (a == 4 || b == 4) ? v == -1 : (a == b ? v == 1 : v == mis);
        }
    kp.pk_ok = ok ? 1 : 0;
    // routing / scheduling defaults; bsw_set_option changes them per context
    kp.kern8 = 1;
    kp.keymode = 2;
    kp.misroute = 0;
    kp.fork = 1;
    kp.long_route = 1;
    kp.small_batch = 32768;          // 16-lane row-group form up to 32K pairs
    kp.mid_batch = 32768;
    kp.group_kernel = 1;
    // the row-group kernel's 32-lane latency form for batches of at most 2048 pairs: 1K calls 0.277
    // -> 0.25 ms, 8 callers without coalescing +8%; from 4K pairs the 16-lane form's fewer
    // instructions per cell win (percall_bench, same box, profiles/r05/gq32_percall.txt)
    kp.gq32_max = 2048;
}

// keys / keys2 / vals / order (radix-sort buffers) grow together
hipError_t grow_sort(Slot &s, int32_t n)
{
    if ((size_t)n <= s.d_order.cap) return hipSuccess;
    s.d_keys.reset(); s.d_keys2.reset(); s.d_vals.reset(); s.d_order.reset();
    const size_t cap = std::max((size_t)n, (size_t)1024);
    hipError_t e;
    if ((e = s.d_keys.reserve_exact(cap)) != hipSuccess) return e;
    if ((e = s.d_keys2.reserve_exact(cap)) != hipSuccess) return e;
    if ((e = s.d_vals.reserve_exact(cap)) != hipSuccess) return e;
    return s.d_order.reserve_exact(cap);
}

// The device pipeline on one slot's device; d_* are device pointers valid on `stream`, in two
// halves so a host pipeline can stage the next chunk between them:
//   run_plan : enqueue plan -> sort -> the class-count readback (nothing waits)
//   run_dp   : wait for that readback, enqueue the DP kernels and the readback of their
//              range-guard word into h_meta[kMetaErr]
// finish_stats() waits for the rest and turns a tripped guard into BSW_E_RANGE.
// the slot's high-priority stream (created on first use)
int ensure_pstream(Slot &s)
{
    if (!s.pstream) {
        int lo = 0, hi = 0;
        BSW_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        BSW_TRY(hipStreamCreateWithPriority(&s.pstream.p, hipStreamNonBlocking, hi));
        BSW_TRY(hipEventCreateWithFlags(&s.evh.p, hipEventDisableTiming));
    }
    return BSW_OK;
}

int run_plan(const KParams &kp, Slot &s, const PlanCall &pc)
{
    s.stats = bsw_stats_t{};
    s.timed = false;
    s.run_stream = pc.stream;
    s.plan = pc;
    s.fast = 0;
    if (pc.n == 0) return BSW_OK;
    const int32_t n = pc.n;
    // small batches (kt_for-sized calls): the row-group kernel (bsw_gq.hip) straight on the
    // call's stream -- no plan, no sort, no class-count readback
    // medium batches: the quad form (4 lanes per pair, targets <= 512 bytes); at most
    // kp.gq32_max pairs: the 32-lane latency form (two DPP rows per pair, ~21% fewer instructions
    // per row; BSW_OPT_GQ32_MAX) -- within the small-batch range (BSW_OPT_SMALL_BATCH 0 keeps every
    // batch off the 16/32-lane forms)
    const int32_t gq32_max = std::min<int32_t>(kp.gq32_max, kp.small_batch);
    const int gs = n <= gq32_max ? 32 : n <= kp.small_batch ? 16 : 4;
    const bool gq_size = n <= kp.small_batch || n <= kp.mid_batch;
    const bool gq_fit = pc.gq_maxq == -2 || (pc.gq_maxq >= 0 && (gs >= 16 || pc.gq_maxt <= 512));
    if (kp.group_kernel && gq_size && gq_fit && kp.long_route == 1 && kp.maxsc == 1 && !kp.misroute) {
        const bool checked = pc.gq_maxq >= 0;
        const int cols = checked ? gq_cols_for(pc.gq_maxq, gs) : (gs == 32 ? 6 : gs == 16 ? 10 : 40);
        int32_t *d_err = s.d_meta + kMetaErr;
        // the DP stream when the call has one (host pipeline: the helper stream holds few CUs)
        hipStream_t fs = pc.stream;
        if (pc.dp_stream && pc.dp_stream != pc.stream) {
            if (int r = ensure_pstream(s)) return r;           // (creates evh)
            BSW_TRY(hipEventRecord(s.evh, pc.stream));
            BSW_TRY(hipStreamWaitEvent(pc.dp_stream, s.evh, 0));
            fs = pc.dp_stream;
            s.run_stream = fs;
        }
        if (!pc.d_out24)                       // (the staged path's input kernel zeroed them)
            BSW_TRY(hipMemsetAsync(d_err, 0, 2 * sizeof(int32_t), fs));
        BSW_TRY(hipEventRecord(s.ev0, fs));
        BSW_TRY(launch_gq_kernel(gs, cols, kp, pc.w, pc.d_pairs, nullptr, n, pc.d_ref, pc.d_qer,
                                 d_err, checked ? nullptr : s.d_meta + kMetaFlag, checked ? pc.d_out24 : nullptr,
                                 fs));
        BSW_TRY(hipEventRecord(s.ev1, fs));
        BSW_TRY(hipMemcpyAsync(s.h_meta + kMetaErr, d_err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, fs));
        if (!checked) {
            if (!s.evm) BSW_TRY(hipEventCreateWithFlags(&s.evm.p, hipEventDisableTiming));
            BSW_TRY(hipEventRecord(s.evm, fs));
        }
        s.stats.n_launches = 1;
        s.stats.n_i16 = n;
        s.stats.n_group = n;
        s.fast = checked ? 2 : 1;
        return BSW_OK;
    }
    // plan + sort run on the slot's high-priority stream (ordered after the call's stream by an
    // event): while other chunks' DP kernels fill the GPU, their few blocks are dispatched
    // first instead of queuing behind thousands of DP workgroups (it delays the next chunk's
    // DP launch otherwise: 1-3 ms per chunk in the host pipeline's trace)
    if (int r = ensure_pstream(s)) return r;
    hipStream_t stream = pc.plan_stream ? pc.plan_stream : s.pstream;
    if (pc.stream != stream) {
        BSW_TRY(hipEventRecord(s.evh, pc.stream));
        BSW_TRY(hipStreamWaitEvent(stream, s.evh, 0));
    }
    BSW_TRY(grow_sort(s, n));
    BSW_TRY(hipMemsetAsync(s.d_meta, 0, kMetaWords * sizeof(int32_t), stream));
    int32_t *d_counts = s.d_meta, *d_maxq = s.d_meta + kMetaMaxq;
    // pairs in the 8-bit score regime (h0 + min(qlen, tlen) <= 255, bwa-style scoring) take the
    // packed-column kernel on both entry points (getScores8 / getScores16: identical results,
    // fewer instructions per cell), the rest the int16 lane kernel (on cell_bits = 8: the
    // overflow fallback) or the int32 wide kernel
    const int pc_route = (kp.pk_ok && kp.kern8) ? 1 : 0;
    // small batches (upstream's kt_for workers hand over a few thousand pairs per call): one
    // lane-per-pair wave lives ~1.2 ms whatever the batch size, so they are latency-bound; the
    // wave-per-alignment kernel spreads each pair over 64 lanes -- 0.35 vs 1.39 ms per call at
    // 1K C2 pairs, 1.05 vs 1.58 at 10K, slower past ~20K
    const int32_t long_route = (kp.long_route == 1 && n <= kp.small_batch) ? 2 : kp.long_route;
    hipLaunchKernelGGL(plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       pc.d_pairs, n, kp, pc.w, pc_route, long_route, pc.d_ref, pc.d_qer, s.d_keys,
                       s.d_vals, d_counts, d_maxq, (int)kp.keymode, (int)kp.misroute);
    BSW_TRY(hipGetLastError());
    BSW_TRY(sort_order(s, n, kKeyBits, stream, true, s.d_meta));
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_meta, kMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (!s.evm) BSW_TRY(hipEventCreateWithFlags(&s.evm.p, hipEventDisableTiming));
    BSW_TRY(hipEventRecord(s.evm, stream));
    return BSW_OK;
}

int run_dp(const KParams &kp, Slot &s)
{
    const PlanCall &pc = s.plan;
    if (pc.n == 0) return BSW_OK;
    hipStream_t stream = pc.dp_stream && !s.fast ? pc.dp_stream : pc.stream;
    const int32_t w = pc.w;
    const int cell_bits = pc.cell_bits;
    SeqPair *d_pairs = pc.d_pairs;
    const uint8_t *d_ref = pc.d_ref, *d_qer = pc.d_qer;
    int32_t *d_err = s.d_meta + kMetaErr;
    if (s.fast) {
        if (s.fast == 1) {
            BSW_TRY(hipEventSynchronize(s.evm));   // the row-group kernel's misfit flag
            if (s.h_meta[kMetaFlag] != 0) {
                // some pair is outside the row-group kernel's contract: the whole batch again on
                // the planned path (identical outputs; rare -- long or int16-unsafe pairs)
                PlanCall again = pc;
                again.gq_maxq = -1;
                const int r = run_plan(kp, s, again);
                if (r) return r;
                return run_dp(kp, s);
            }
        }
        s.timed = true;                            // ev0 / ev1 bracket the kernel; the guard
        return BSW_OK;                             //   word is on its way to h_meta[kMetaErr]
    }
    BSW_TRY(hipEventSynchronize(s.evm));           // the class counts are in h_meta
    BSW_TRY(hipStreamWaitEvent(stream, s.evm, 0)); // order / meta written on the plan stream
    int32_t counts[kNumClasses] = {};
    for (int sl = 0; sl < kMetaSpread; ++sl)
        for (int c = 0; c < kNumClasses; ++c) counts[c] += s.h_meta[sl * kMetaCounts + c];
    const int32_t maxq_wide = s.h_meta[kMetaMaxq];
    // DP kernels, one launch per non-empty class; event-timed as the hot region.  With more than
    // one class the launches fork over the slot's side streams and join back on `stream`.
    int nclass = 0;
    for (int c = 0; c < kNumClasses; ++c) nclass += counts[c] > 0;
    const bool fork = nclass > 1 && kp.fork;
    BSW_TRY(hipEventRecord(s.ev0, stream));
    if (fork) {
        if (!s.evf) BSW_TRY(hipEventCreateWithFlags(&s.evf.p, hipEventDisableTiming));
        for (int k = 0; k < Slot::kSide; ++k)
            if (!s.side[k]) {
                BSW_TRY(hipStreamCreateWithFlags(&s.side[k].p, hipStreamNonBlocking));
                BSW_TRY(hipEventCreateWithFlags(&s.evj[k].p, hipEventDisableTiming));
            }
        BSW_TRY(hipEventRecord(s.evf, stream));
        for (int k = 0; k < Slot::kSide; ++k) BSW_TRY(hipStreamWaitEvent(s.side[k], s.evf, 0));
    }
    int nl = 0;                        // launch k runs on stream k mod (1 + kSide)
    auto next_stream = [&]() {
        const int k = nl++ % (1 + Slot::kSide);
        return (fork && k > 0) ? s.side[k - 1] : stream;
    };
    // every launch of the fork; the join below runs whatever happens here, so no side stream
    // can still be reading this slot's buffers when the slot goes back to the pool
    const int lrc = [&]() -> int {
        int32_t off = 0;
        for (int c = 0; c < kNumLaneClasses; ++c) {
            if (counts[c] > 0) {
                BSW_TRY(launch_lane_kernel(kLaneQmax[c], kp, w, d_pairs, s.d_order + off, counts[c],
                                           d_ref, d_qer, d_err, next_stream()));
                s.stats.n_launches++;
                s.stats.n_i16 += counts[c];
            }
            off += counts[c];
        }
        for (int c = 0; c < kNumLaneClasses; ++c) {
            const int32_t np = counts[kPkClass0 + c];
            if (np > 0) {
                // its redo list: d_keys2's slice at the class's offset (the sort is done with it),
                // the length in the class's d_meta word, zeroed with the class counts (run_plan)
                BSW_TRY(launch_pc_kernel(kLaneQmax[c], kp, w, d_pairs, s.d_order + off, np, d_ref, d_qer,
                                         d_err, reinterpret_cast<int32_t *>(s.d_keys2.p) + off,
                                         s.d_meta + kMetaRedo + c, next_stream()));
                s.stats.n_launches++;
                s.stats.n_packed += np;
                if (cell_bits == 8) s.stats.n_u8 += np;
                else s.stats.n_i16 += np;
            }
            off += np;
        }
        if (counts[kWideClass] > 0) {
            const int32_t nw = counts[kWideClass];
            const size_t need = (size_t)(maxq_wide + 2) * (size_t)nw;
            BSW_TRY(s.d_scratch.grow(need));
            BSW_TRY(launch_wide_kernel(kp, w, d_pairs, s.d_order + off, nw, d_ref, d_qer, s.d_scratch,
                                       nw, next_stream()));
            s.stats.n_launches++;
            s.stats.n_wide += nw;
        }
        off += counts[kWideClass];
        for (int c = 0; c < kNumWvClasses; ++c) {
            const int32_t nv = counts[kWvClass0 + c];
            if (nv > 0) {
                BSW_TRY(launch_wv_kernel(kWvCols[c], kp, w, d_pairs, s.d_order + off, nv, d_ref, d_qer, d_err,
                                         next_stream()));
                s.stats.n_launches++;
                s.stats.n_i16 += nv;
                s.stats.n_wave += nv;
            }
            off += nv;
        }
        return BSW_OK;
    }();
    if (fork)
        for (int k = 0; k < Slot::kSide; ++k) {
            BSW_TRY(hipEventRecord(s.evj[k], s.side[k]));
            BSW_TRY(hipStreamWaitEvent(stream, s.evj[k], 0));
        }
    if (lrc) {
        (void)hipStreamSynchronize(stream);         // drain what was queued before the failure
        return lrc;
    }
    BSW_TRY(hipEventRecord(s.ev1, stream));
    // the DP kernels' range guard (a pair routed to a class that cannot hold it) -> host,
    // after every DP launch of this batch
    BSW_TRY(hipMemcpyAsync(s.h_meta + kMetaErr, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    s.run_stream = stream;
    s.timed = true;
    return BSW_OK;
}

int run_device(const KParams &kp, Slot &s, SeqPair *d_pairs, const uint8_t *d_ref,
                      const uint8_t *d_qer, int32_t n, int32_t w, int cell_bits, hipStream_t stream)
{
    PlanCall pc;
    pc.d_pairs = d_pairs; pc.d_ref = d_ref; pc.d_qer = d_qer;
    pc.n = n; pc.w = w; pc.cell_bits = cell_bits; pc.stream = stream;
    int r = run_plan(kp, s, pc);
    if (r) return r;
    return run_dp(kp, s);
}

// Wait for run_device's work (through the guard readback), record the DP kernel time; a
// tripped range guard is BSW_E_RANGE (the affected pairs' outputs were not written).
int finish_stats(Slot &s, bool spin)
{
    if (s.timed) {
        float ms = 0.f;
        s.timed = false;
        if (spin) {         // a short batch: poll instead of the runtime's blocking wait (wake-up latency)
            hipError_t q;
            while ((q = hipStreamQuery(s.run_stream)) == hipErrorNotReady) _mm_pause();
            BSW_TRY(q);
        }
        BSW_TRY(hipStreamSynchronize(s.run_stream));
        BSW_TRY(hipEventElapsedTime(&ms, s.ev0, s.ev1));
        s.stats.kernel_ms = ms;
        if (s.h_meta[kMetaErr] != 0) return BSW_E_RANGE;
    }
    return BSW_OK;
}

}  // namespace bsw
