// bsw_pipeline.hip -- host-buffer calls (bsw_engine.h): staging kernels, the chunked host pipeline
// of one device's share of a call (host_shard) and cross-call coalescing of small calls.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <vector>
#include "bsw_engine.h"
#include "bsw_sort.h"
#include "bsw_pool.h"
#include "bsw_stage_plan.h"

// experiment builds only (make abhost AB_FLAGS=-DBSW_HP_SLOTS=5 / -DBSW_HP_FIRST_BLK=8)
// Slots of one host_shard call; chunk k + slots stages only once chunk k's outputs are back.  4
// since round 4: with the helper stream the fourth slot lets the next chunk stage a DP generation
// earlier (same box, alternating: 84.7 / 87.7 vs 77.0 / 78.8 M/s per 1M-pair call; 5 slots pay
// more first-call allocation, profiles/r04/hostpath_slots_r4w.txt)
#ifndef BSW_HP_SLOTS
#define BSW_HP_SLOTS 4
#endif
// blocks of a pipelined call's first chunk (first_chunk_blocks, bsw_stage_plan.h)
#ifndef BSW_HP_FIRST_BLK
#define BSW_HP_FIRST_BLK 16
#endif

namespace bsw {

static_assert(sizeof(PairIn) == kPairInBytes, "stage_layout's 2-bit record is PairIn");

// bytes out[0, n) from nibbles in[0, (n + 1) / 2): 4 packed bytes -> 8 codes per thread
__global__ void unpack_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int64_t n)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t o = t * 8;
    if (o >= n) return;
    uint32_t v = 0;
    const int64_t ib = t * 4, nin = (n + 1) / 2;
    if (ib + 4 <= nin) v = *(const uint32_t *)(in + ib);
    else
        for (int k = 0; k < 4 && ib + k < nin; ++k) v |= (uint32_t)in[ib + k] << (8 * k);
    const uint32_t lo = (v & 0x0f0f0f0fu), hi = (v >> 4) & 0x0f0f0f0fu;
    // interleave: byte 2k = lo byte k, byte 2k + 1 = hi byte k
    const uint32_t w0 = __builtin_amdgcn_perm(hi, lo, 0x05010400u);
    const uint32_t w1 = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
    if (o + 8 <= n) {
        *(uint2 *)(out + o) = make_uint2(w0, w1);
    } else {
        const uint8_t b[8] = {(uint8_t)w0, (uint8_t)(w0 >> 8), (uint8_t)(w0 >> 16), (uint8_t)(w0 >> 24),
                              (uint8_t)w1, (uint8_t)(w1 >> 8), (uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24)};
        for (int k = 0; o + k < n; ++k) out[o + k] = b[k];
    }
}

// The whole staged input of a coalesced batch in one launch (what unpack2 x2 + patch_codes +
// expand_pairs + two pad memsets did in six): index space = ref 16-code units, qer units, pairs.
// Exception words (pos << 2 | code bits 2-3, bsw_pack.cpp) are ascending per buffer.  A lane
// unpacks 64 codes (16 packed bytes in, 64 bytes out; see unpack_unit for the interleaving), a wave 4096 consecutive positions: the
// wave reads the index of its first exception from exc_bucket_kernel's table (one entry per 4096
// positions), loads the next 64 words (one per lane) and every lane patches the ones inside its
// own codes from a uniform walk over those in the wave's range (~4 per wave at bwa's N rate).  A
// binary search per lane per 16 codes -- ~20 dependent loads each at 900K exceptions per 3M-pair
// piece -- made the staging kernel latency-bound: 1.8-3.0 ms per 3M pairs in the RCCL leg's trace,
// ahead of every piece's DP; one search per wave still 1.2-2.4 ms (profiles/r06/rccl_leg_trace.txt).
// Whole-wave function: every lane of the wave calls it (valid = the lane has codes to write).
constexpr int kUnitCodes = 64;          // codes per lane
__device__ __forceinline__ uint4 unpack16(uint32_t v)    // 16 codes from 4 packed bytes
{
    const uint32_t p0 = v & 0x03030303u, p1 = (v >> 2) & 0x03030303u;
    const uint32_t p2 = (v >> 4) & 0x03030303u, p3 = (v >> 6) & 0x03030303u;
    const uint32_t a01 = __builtin_amdgcn_perm(p1, p0, 0x05010400u), b01 = __builtin_amdgcn_perm(p1, p0, 0x07030602u);
    const uint32_t a23 = __builtin_amdgcn_perm(p3, p2, 0x05010400u), b23 = __builtin_amdgcn_perm(p3, p2, 0x07030602u);
    return make_uint4(__builtin_amdgcn_perm(a23, a01, 0x05040100u), __builtin_amdgcn_perm(a23, a01, 0x07060302u),
                      __builtin_amdgcn_perm(b23, b01, 0x05040100u), __builtin_amdgcn_perm(b23, b01, 0x07060302u));
}
__device__ __forceinline__ void unpack_unit(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int64_t n,
                                            int64_t wave_t0, int64_t units,
                                            const uint32_t *__restrict__ exc, int32_t ne,
                                            const int32_t *__restrict__ bkt)
{
    // the wave's 4096 positions [W, W + 4096) as 4 sub-units per lane, interleaved so that every
    // load / store instruction of the wave is contiguous: sub-unit u of lane L = the 16 codes at
    // W + 1024 u + 16 L (4 packed bytes in, one 16-B store out)
    if (wave_t0 >= units) return;                                // (the tail waves of a block: uniform)
    const int lane = (int)(threadIdx.x & 63);
    const int64_t W = wave_t0 * kUnitCodes, nin = (n + 3) / 4;
    uint4 w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t pos = W + 1024 * u + 16 * lane, ib = pos / 4;
        uint32_t v = 0;
        if (ib + 4 <= nin) v = *(const uint32_t *)(in + ib);
        else
            for (int k = 0; k < 4 && ib + k < nin; ++k) v |= (uint32_t)in[ib + k] << (8 * k);
        w[u] = unpack16(v);
    }
    if (ne > 0) {
        const int64_t whi = W + 64 * kUnitCodes;
        const int32_t lo = min(max(bkt[wave_t0 / 64], 0), ne);  // first exception at or past W (uniform)
        for (int32_t base = lo;; base += 64) {                   // uniform: 64 words per round
            const int32_t j = base + lane;
            const uint32_t e = j < ne ? exc[j] : 0u;
            const bool in_w = j < ne && (int64_t)(e >> 2) < whi;
            const int cnt = __popcll(__ballot(in_w));              // sorted: lanes 0 .. cnt - 1
            for (int q = 0; q < cnt; ++q) {
                const uint32_t eq = (uint32_t)__shfl((int)e, q);
                const int64_t k = (int64_t)(eq >> 2) - W;         // 0 .. 4095 (in the wave's range)
                if (k >= 0 && k < 4096 && (int)((k >> 4) & 63) == lane) {
                    const int u = (int)(k >> 10), c = (int)(k & 15);
                    const uint32_t bits = (eq & 3u) << (8 * (c & 3) + 2);   // code bits 2-3
                    const int d = c >> 2;
#pragma unroll
                    for (int uu = 0; uu < 4; ++uu) {
                        w[uu].x |= (u == uu && d == 0) ? bits : 0u;
                        w[uu].y |= (u == uu && d == 1) ? bits : 0u;
                        w[uu].z |= (u == uu && d == 2) ? bits : 0u;
                        w[uu].w |= (u == uu && d == 3) ? bits : 0u;
                    }
                }
            }
            if (cnt < 64) break;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t pos = W + 1024 * u + 16 * lane;
        if (pos + 16 <= n) {
            *(uint4 *)(out + pos) = w[u];
        } else {
            const uint32_t word[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
            for (int k = 0; pos + k < n; ++k) out[pos + k] = (uint8_t)(word[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// Blocks of 256 threads, each block inside one segment (so every wave is): [ref 64-code units |
// qer units | records]; stage_in_grid() is the matching grid size
__host__ __device__ inline int64_t stage_in_blocks(int64_t r_tot, int64_t q_tot, int64_t n, int64_t *br, int64_t *bq)
{
    *br = ((r_tot + kUnitCodes - 1) / kUnitCodes + 255) / 256;
    *bq = ((q_tot + kUnitCodes - 1) / kUnitCodes + 255) / 256;
    return *br + *bq + (n + 255) / 256;
}

// bkt[b] = the first exception word at or past position 4096 b: ref buckets [0, nbr), then qer
// buckets [nbr, nbr + nbq) indexing the qer words (exc + n_r).  One lane per bucket, its own binary
// search: ~nbr + nbq lanes instead of one search per staging wave
__global__ void exc_bucket_kernel(const uint32_t *__restrict__ exc, int32_t n_r, int32_t ne, int64_t nbr, int64_t nbq,
                                  int32_t *__restrict__ bkt)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbr + nbq) return;
    const bool q = b >= nbr;
    const uint32_t *e = q ? exc + n_r : exc;
    const int64_t pos = (q ? b - nbr : b) * 4096;
    int32_t lo = 0, hi = q ? ne - n_r : n_r;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if ((int64_t)(e[mid] >> 2) < pos) lo = mid + 1; else hi = mid;
    }
    bkt[b] = lo;
}

__global__ __launch_bounds__(256) void stage_in_kernel(const uint8_t *__restrict__ ref2, int64_t r_tot,
                                const uint8_t *__restrict__ qer2,
                                int64_t q_tot, const uint32_t *__restrict__ exc, int32_t n_r, int32_t ne,
                                const PairIn *__restrict__ pin, int32_t n, uint8_t *__restrict__ ref,
                                uint8_t *__restrict__ qer, SeqPair *__restrict__ pairs, int32_t *__restrict__ zero2,
                                const int32_t *__restrict__ bkt, int64_t nbr)
{
    const int64_t tr = (r_tot + kUnitCodes - 1) / kUnitCodes, tq = (q_tot + kUnitCodes - 1) / kUnitCodes;   // lanes
    int64_t br, bq;
    stage_in_blocks(r_tot, q_tot, n, &br, &bq);
    const int64_t blk = blockIdx.x;
    const int wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blk == 0 && threadIdx.x == 0) {
        *(uint32_t *)(ref + r_tot) = 0u;          // 4 zero bytes past each buffer
        *(uint32_t *)(qer + q_tot) = 0u;
        if (zero2) { zero2[0] = 0; zero2[1] = 0; }
    }
    if (blk < br) {
        unpack_unit(ref2, ref, r_tot, blk * 256 + 64 * wv, tr, exc, n_r, bkt);
        return;
    }
    if (blk < br + bq) {
        unpack_unit(qer2, qer, q_tot, (blk - br) * 256 + 64 * wv, tq, exc + n_r, ne - n_r, bkt + nbr);
        return;
    }
    const int64_t t = (blk - br - bq) * 256 + threadIdx.x;
    if (t < n) {
        const PairIn p = pin[t];
        SeqPair sp;
        memset(&sp, 0, sizeof(sp));
        sp.idr = p.idr; sp.idq = p.idq; sp.len1 = p.len1; sp.len2 = p.len2; sp.h0 = p.h0;
        pairs[t] = sp;
    }
}

// The whole staged input of one batch: the exceptions' bucket table (when there are exceptions),
// then stage_in_kernel -- on `st`, the slot's d_bkt grown to the table
int launch_stage_in(Slot &s, hipStream_t st, const uint8_t *ref2, int64_t r_tot, const uint8_t *qer2,
                           int64_t q_tot, const uint32_t *exc, int32_t n_r, int32_t ne, const PairIn *pin, int32_t n,
                           uint8_t *ref, uint8_t *qer, SeqPair *pairs, int32_t *zero2)
{
    const ExcBuckets nb = exc_buckets(r_tot, q_tot);
    const int64_t nbr = nb.nbr, nbq = nb.nbq;
    if (ne > 0) {
        BSW_TRY(s.d_bkt.grow(nb.total()));
        hipLaunchKernelGGL(exc_bucket_kernel, dim3((unsigned)((nbr + nbq + 255) / 256)), dim3(256), 0, st, exc, n_r,
                           ne, nbr, nbq, s.d_bkt);
        BSW_TRY(hipGetLastError());
    }
    int64_t br, bq;
    const unsigned grid = (unsigned)stage_in_blocks(r_tot, q_tot, n, &br, &bq);
    hipLaunchKernelGGL(stage_in_kernel, dim3(grid), dim3(256), 0, st, ref2, r_tot, qer2, q_tot, exc, n_r, ne, pin, n,
                       ref, qer, pairs, zero2, (const int32_t *)s.d_bkt, nbr);
    return hip_rc(hipGetLastError());
}

// the six outputs of each pair (SeqPair bytes 32..55) -> 24 B per pair for the D2H
__global__ void gather_outputs_kernel(const SeqPair *__restrict__ in, int32_t *__restrict__ out, int32_t n)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SeqPair &p = in[i];
    int32_t *o = out + 6 * (int64_t)i;
    o[0] = p.score; o[1] = p.tle; o[2] = p.gtle; o[3] = p.qle; o[4] = p.gscore; o[5] = p.max_off;
}

int launch_gather_outputs(const SeqPair *d_pairs, int32_t *d_out, int32_t n, hipStream_t st)
{
    hipLaunchKernelGGL(gather_outputs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pairs, d_out, n);
    return hip_rc(hipGetLastError());
}

// Pre-pass of a host-buffer call, one parallel sweep over the records: validation (the ABI's
// BSW_E_RANGE before any device work) and per-block extents of the byte buffers (BlkStat,
// bsw_stage_plan.h).
// blocks [b0, b1) of bs (sized for every block of the n pairs); false if any pair there is invalid
static bool prepass_range(const SeqPair *pairs, int32_t n, std::vector<BlkStat> &bs, int32_t b0, int32_t b1)
{
    auto blk = [&](int32_t b) {
        BlkStat t{INT64_MAX, 0, INT64_MAX, 0, 0, 0, false};
        const int32_t e = std::min(n, (b + 1) * kStageBlk);
        for (int32_t i = b * kStageBlk; i < e; ++i) {
            const SeqPair &p = pairs[i];
            t.bad |= !pair_valid(p);
            if (p.len1 > 0) { t.r_lo = std::min<int64_t>(t.r_lo, p.idr); t.r_hi = std::max<int64_t>(t.r_hi, (int64_t)p.idr + p.len1); t.r_sum += p.len1; }
            if (p.len2 > 0) { t.q_lo = std::min<int64_t>(t.q_lo, p.idq); t.q_hi = std::max<int64_t>(t.q_hi, (int64_t)p.idq + p.len2); t.q_sum += p.len2; }
        }
        bs[b] = t;
    };
    const int32_t nb = b1 - b0;
    if (nb < 16) {
        for (int32_t b = b0; b < b1; ++b) blk(b);
    } else {
        const int nt = std::min(HostPool::workers() + 1, (int)nb);
        HostPool::get().parallel_for(nt, [&](int t) {
            for (int32_t b = b0 + (int32_t)((int64_t)nb * t / nt); b < b0 + (int32_t)((int64_t)nb * (t + 1) / nt); ++b)
                blk(b);
        });
    }
    for (int32_t b = b0; b < b1; ++b)
        if (bs[b].bad) return false;
    return true;
}

static bool prepass(const SeqPair *pairs, int32_t n, std::vector<BlkStat> &bs)
{
    const int32_t nb = (n + kStageBlk - 1) / kStageBlk;
    bs.assign((size_t)nb, BlkStat{});
    return prepass_range(pairs, n, bs, 0, nb);
}

// One chunk of a host-buffer call staged in a slot's pinned buffer (StageMode and StageLayout,
// bsw_stage_plan.h).  Gathered chunks have their staged records' idr / idq rewritten (only outputs
// ever go back to the caller).
struct StagedChunk {
    int32_t n = 0;
    int mode = kStageGather;
    StageLayout lay;
    int32_t n_exr = 0, n_exq = 0;       // 2-bit: exception words for ref / qer
    size_t rb = 0, qb = 0;              // ref / qer bytes after unpacking
    int64_t r_base = 0, q_base = 0;     // staged ref byte 0 = caller byte r_base (bulk modes)
};

// 2-bit staging of a bulk chunk (c.rb / c.qb bytes from ref / qer).  Returns 1 (nothing staged)
// when the exception words would pass exc_cap.
static int stage_2bit(Slot &s, const SeqPair *pairs, const uint8_t *ref, const uint8_t *qer, int32_t n,
                      StagedChunk &c)
{
    const size_t cap = exc_cap(c.rb, c.qb);
    const StageLayout l = stage_layout(kStage2bit, (size_t)n, c.rb, c.qb, cap);
    BSW_TRY(s.h_stage.grow(l.bytes));
    uint8_t *h = s.h_stage;
    PairIn *pin = (PairIn *)(h + l.pair_off);
    const int np = (int)std::max<size_t>(1, ((size_t)n * sizeof(SeqPair)) >> 21);
    const int nr = (int)std::max<size_t>(1, c.rb >> 22), nq = (int)std::max<size_t>(1, c.qb >> 22);
    auto even = [](size_t total, int k, int parts) {     // piece bounds: multiples of 64 codes
        return k == parts ? total : (total * (size_t)k / (size_t)parts) & ~(size_t)63;
    };
    std::vector<std::vector<uint32_t>> ex((size_t)(nr + nq));
    HostPool::get().parallel_for(np + nr + nq, [&](int t) {
        if (t < np) {
            const int32_t a0 = (int32_t)((int64_t)n * t / np), a1 = (int32_t)((int64_t)n * (t + 1) / np);
            for (int32_t i = a0; i < a1; ++i)
                pin[i] = PairIn{pairs[i].idr, pairs[i].idq, pairs[i].len1, pairs[i].len2, pairs[i].h0};
        } else if (t < np + nr) {
            const size_t a0 = even(c.rb, t - np, nr), a1 = even(c.rb, t - np + 1, nr);
            pack_2bit(h + l.ref_off + a0 / 4, ref + a0, a1 - a0, (uint32_t)a0, ex[(size_t)(t - np)]);
        } else {
            const size_t a0 = even(c.qb, t - np - nr, nq), a1 = even(c.qb, t - np - nr + 1, nq);
            pack_2bit(h + l.qer_off + a0 / 4, qer + a0, a1 - a0, (uint32_t)a0, ex[(size_t)(t - np)]);
        }
    });
    size_t tot = 0, tr = 0;
    for (size_t k = 0; k < ex.size(); ++k) {
        tot += ex[k].size();
        if (k < (size_t)nr) tr += ex[k].size();
    }
    if (tot > cap) return 1;
    uint32_t *exw = (uint32_t *)(h + l.exc_off);
    for (size_t k = 0, o = 0; k < ex.size(); o += ex[k].size(), ++k)
        if (!ex[k].empty()) memcpy(exw + o, ex[k].data(), ex[k].size() * 4);
    c.n_exr = (int32_t)tr;
    c.n_exq = (int32_t)(tot - tr);
    c.lay = stage_layout(kStage2bit, (size_t)n, c.rb, c.qb, tot);
    memset(h + l.ref_off + l.ref_len, 0, 4);
    memset(h + l.qer_off + l.qer_len, 0, 4);
    return BSW_OK;
}

// pairs [0, n) = blocks bs[0, nblk)
static int stage_chunk(Slot &s, const SeqPair *pairs, const uint8_t *ref, const uint8_t *qer, int32_t n,
                       const BlkStat *bs, int32_t nblk, bool two_bit, StagedChunk &c)
{
    const BlkStat t = merge_blocks(bs, nblk);
    const int64_t r_lo = t.r_lo, q_lo = t.q_lo;
    c.n = n;
    c.mode = stage_mode(t, two_bit, &c.rb, &c.qb);
    const bool bulk = c.mode != kStageGather;
    c.r_base = bulk ? r_lo : 0;
    c.q_base = bulk ? q_lo : 0;
    if (c.mode == kStage2bit) {
        const int r = stage_2bit(s, pairs, ref + r_lo, qer + q_lo, n, c);
        if (r != 1) return r;
        c.mode = kStageNibble;              // 1: too many exception bytes -> nibbles below
    }
    const StageLayout l = c.lay = stage_layout(c.mode, (size_t)n, c.rb, c.qb, 0);
    BSW_TRY(s.h_stage.grow(l.bytes));
    uint8_t *h = s.h_stage;
    SeqPair *sp = (SeqPair *)(h + l.pair_off);
    if (bulk) {
        // records + both packs as one pool job list (pieces of ~2 MB)
        const size_t pb = (size_t)n * sizeof(SeqPair);
        const int np = (int)std::max<size_t>(1, pb >> 21), nr = (int)std::max<size_t>(1, c.rb >> 22),
                  nq = (int)std::max<size_t>(1, c.qb >> 22);
        auto even = [](size_t total, int k, int parts) {
            return k == parts ? total : (total * (size_t)k / (size_t)parts) & ~(size_t)31;
        };
        HostPool::get().parallel_for(np + nr + nq, [&](int t) {
            if (t < np) {
                const size_t a0 = pb * t / np, a1 = pb * (t + 1) / np;
                memcpy((char *)sp + a0, (const char *)pairs + a0, a1 - a0);
            } else if (t < np + nr) {
                const size_t a0 = even(c.rb, t - np, nr), a1 = even(c.rb, t - np + 1, nr);
                pack_nibbles(h + l.ref_off + a0 / 2, ref + r_lo + a0, a1 - a0);
            } else {
                const size_t a0 = even(c.qb, t - np - nr, nq), a1 = even(c.qb, t - np - nr + 1, nq);
                pack_nibbles(h + l.qer_off + a0 / 2, qer + q_lo + a0, a1 - a0);
            }
        });
    } else {
        par_memcpy(sp, pairs, (size_t)n * sizeof(SeqPair));
        int64_t ro = 0, qo = 0;
        for (int32_t i = 0; i < n; ++i) {
            SeqPair &p = sp[i];
            if (p.len1 > 0) { memcpy(h + l.ref_off + ro, ref + p.idr, (size_t)p.len1); p.idr = (int32_t)ro; ro += p.len1; }
            else p.idr = 0;
            if (p.len2 > 0) { memcpy(h + l.qer_off + qo, qer + p.idq, (size_t)p.len2); p.idq = (int32_t)qo; qo += p.len2; }
            else p.idq = 0;
        }
    }
    memset(h + l.ref_off + l.ref_len, 0, 4);
    memset(h + l.qer_off + l.qer_len, 0, 4);
    return BSW_OK;
}

// outputs of a finished chunk -> the caller's records: 24 B per pair (2-bit), whole records
// (nibbles: they carry the caller's own input fields) or the output fields of the staged records
// (gathered: their offsets were rewritten)
static void unstage_outputs(const Slot &s, SeqPair *pairs, int32_t n, int mode)
{
    if (mode == kStageNibble) {
        par_memcpy(pairs, s.h_stage.p, (size_t)n * sizeof(SeqPair));
        return;
    }
    const int32_t *o = (const int32_t *)s.h_stage.p;
    if (mode == kStageGather) {
        for (int32_t i = 0; i < n; ++i) put_outputs(pairs[i], o + BSW_SP_WORDS * (int64_t)i + BSW_SP_SCORE / 4);
        return;
    }
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(HostPool::workers() + 1, n >> 15));
    HostPool::get().parallel_for(nt, [&](int t) {
        for (int32_t i = (int32_t)((int64_t)n * t / nt); i < (int32_t)((int64_t)n * (t + 1) / nt); ++i)
            put_outputs(pairs[i], o + 6 * (int64_t)i);
    });
}

// The largest buffers any chunk of a host-buffer call needs, in the staging form stage_chunk will
// pick for it first (a 2-bit chunk that falls back to nibbles -- more than 1/32 non-ACGT bytes --
// grows its slot as before): reserve_slot grows a slot to them before its first chunk.
struct SlotReserve {
    int32_t m = 0;                      // pairs
    size_t rb = 0, qb = 0, stage = 0;   // unpacked ref / qer bytes, pinned / device staging bytes
    void add(int32_t mc, const BlkStat *b, int32_t nb, bool two_bit)
    {
        size_t r, q;
        const StageMode mode = stage_mode(merge_blocks(b, nb), two_bit, &r, &q);
        m = std::max(m, mc);
        rb = std::max(rb, r);
        qb = std::max(qb, q);
        stage = std::max(stage, stage_layout(mode, (size_t)mc, r, q, mode == kStage2bit ? exc_cap(r, q) : 0).bytes);
    }
};

static int reserve_slot(Slot &s, const SlotReserve &r)
{
    if (r.m <= 0) return BSW_OK;
    BSW_TRY(hipSetDevice(s.device));
    // the helper stream now, on the calling thread: created lazily by the enqueuer thread it cost
    // ~10 ms per slot (hipStreamCreateWithPriority) in the middle of a call's pipeline, stalling
    // every chunk queued behind it (HIP API trace, profiles/r06/hostpath_first_calls_api.txt)
    if (int e = ensure_pstream(s)) return e;
    if (r.stage > s.h_stage.cap) BSW_TRY(s.h_stage.reserve_exact(r.stage + r.stage / 4));
    BSW_TRY(s.d_stage.grow(r.stage));
    BSW_TRY(s.d_ref.grow(r.rb + 16));
    BSW_TRY(s.d_qer.grow(r.qb + 16));
    BSW_TRY(s.d_pairs.grow((size_t)r.m));
    BSW_TRY(s.d_bkt.grow(exc_buckets((int64_t)r.rb, (int64_t)r.qb).total()));
    BSW_TRY(grow_sort(s, r.m));
    BSW_TRY(sort_order(s, r.m, kKeyBits, (hipStream_t)0, false));     // (d_tmp only)
    return BSW_OK;
}

// Copy-engine warm-up, once per device context, on its first multi-chunk host call: H2D and D2H
// copies in flight at once on every slot's helper and DP streams, large and small, as the
// pipeline issues them.  Without it one hipMemcpyAsync in each of a context's first two calls
// blocked for 7.6-9.6 ms with the GPU idle (HIP API trace, profiles/r06/hostpath_first_calls_api.txt);
// with SDMA disabled (HSA_ENABLE_SDMA=0, blit-kernel copies) the stall was gone, so the first
// copies that land on a not yet used DMA engine pay its set-up.
static int prime_copies(Slot *const *slots, int ns)
{
    for (size_t want : {(size_t)1 << 62, (size_t)4 << 20, (size_t)64 << 10}) {
        for (int k = 0; k < ns; ++k) {
            Slot &s = *slots[k];
            const size_t half = std::min(s.h_stage.cap, s.d_stage.cap) / 2, sz = std::min(want, half);
            if (sz == 0) continue;
            uint8_t *h = s.h_stage;
            BSW_TRY(hipMemcpyAsync(s.d_stage, h, sz, hipMemcpyHostToDevice, s.pstream));
            BSW_TRY(hipMemcpyAsync(h + half, s.d_stage + half, sz, hipMemcpyDeviceToHost, s.stream));
        }
        for (int k = 0; k < ns; ++k) {
            BSW_TRY(hipStreamSynchronize(slots[k]->pstream));
            BSW_TRY(hipStreamSynchronize(slots[k]->stream));
        }
    }
    return BSW_OK;
}

// One device's share of a host-buffer call: a pipeline of chunks over the device's slots.
// Per chunk: stage into the slot's pinned buffer (host pool) -> one H2D -> unpack -> plan / sort
// -> DP kernels -> D2H of the outputs.  The calling thread only stages; a launcher thread enqueues
// each chunk's DP kernels and output readback as soon as that chunk's class counts are back, so
// the GPU never waits for the host to finish staging the next chunk (round 1's single-thread loop
// launched chunk k's kernels only after chunk k + 1 was staged: ~1.4 ms of idle GPU per chunk in
// the rocprofv3 timeline).  Calls of several chunks hand each staged chunk to an enqueuer thread,
// so the calling thread stages the next chunk at once: the enqueue of a chunk (H2D, unpack, plan,
// sort -- ~0.9 ms of runtime calls per 256K-pair chunk in the kernel + copy trace) otherwise sat
// between two stagings and made the next chunk's DP start after the current one had drained
// (profiles/r04/hostpath_trace_*.txt).  One-chunk calls -- up to 128K pairs, kt_for-sized batches
// -- run on one slot and enqueue inline (no thread hand-off).  Outputs are identical to one
// unchunked call (pairs are independent).
//
// Errors: a chunk whose enqueue failed still goes to the launcher, which skips the DP of every
// chunk once the call has an error and releases finish(k) with the first one.  The enqueuer is
// stopped before the launcher, and each handles every queued job first.
struct ShardCall {
    static constexpr int kSlots = BSW_HP_SLOTS;
    const KParams &kp;
    DeviceCtx &dc;
    SeqPair *pairs;
    const uint8_t *ref, *qer;
    int32_t n, w;
    int cell_bits;
    bool two_bit;

    std::unique_ptr<Slot> slots[kSlots];    // taken as chunks start (a one-chunk call takes one)
    struct Pending { int32_t at = 0, n = 0, seq = -1; int mode = kStageGather; } pend[kSlots];  // chunk in flight
    bsw_stats_t agg{};
    double stage_ms = 0;

    // what finish(k) waits on, under mu: the call's first error and per slot the seq (chunks are
    // numbered in order) of the last chunk the launcher is through with
    std::mutex mu;
    std::condition_variable cv;
    int err = BSW_OK;
    int32_t launched[kSlots];

    struct LaunchJob { int k; int32_t seq; int mode; };
    struct EnqJob { int k; int32_t seq; StagedChunk c; };
    bool launcher_dev_ok = false, enqueuer_dev_ok = false;  // hipSetDevice on each thread
    bool async = false;
    Worker<LaunchJob> launcher;             // (the workers go first: members above outlive them)
    Worker<EnqJob> enqueuer;

    ShardCall(const KParams &kp_, DeviceCtx &dc_, SeqPair *pairs_, const uint8_t *ref_, const uint8_t *qer_,
              int32_t n_, int32_t w_, int cell_bits_, bool two_bit_)
        : kp(kp_), dc(dc_), pairs(pairs_), ref(ref_), qer(qer_), n(n_), w(w_), cell_bits(cell_bits_), two_bit(two_bit_)
    {
        std::fill(launched, launched + kSlots, -1);
    }

    // the launcher always, the enqueuer for a call of several chunks
    void start(bool several)
    {
        launcher.start([this](LaunchJob &j) { launch(j); },
                       [this] { launcher_dev_ok = hipSetDevice(dc.device) == hipSuccess; });
        async = several;
        if (!async) return;
        enqueuer.start(
            [this](EnqJob &j) {
                if (enqueuer_dev_ok) (void)enqueue(j.k, j.seq, j.c);
                else to_launcher(j.k, j.seq, j.c.mode, BSW_E_HIP);
            },
            [this] { enqueuer_dev_ok = hipSetDevice(dc.device) == hipSuccess; });
    }

    // slot k's chunk, enqueued with status r, to the launcher
    void to_launcher(int k, int32_t seq, int mode, int r)
    {
        {
            std::lock_guard<std::mutex> g(mu);
            if (r && !err) err = r;
        }
        launcher.push(LaunchJob{k, seq, mode});
    }

    int take_slot(int k, const SlotReserve &res)
    {
        if (slots[k]) return BSW_OK;
        int r = BSW_OK;
        slots[k] = dc.acquire(r);
        if (r) return r;
        // every buffer of the slot at the call's largest chunk at once: chunks rotate over the
        // slots, so sizing by the chunk at hand regrew a slot (hipFree waits for the device) on
        // the first calls of a context as its chunks got larger
        return reserve_slot(*slots[k], res);
    }

    // the context's first pipelined call: every slot it will use now, then the copy warm-up over
    // all of them at once (prime_copies).  A failure leaves the context cold for the rerun
    int warm_up(const SlotReserve &res, int nchunks)
    {
        bool cold = false;
        if (!dc.copies_warm.compare_exchange_strong(cold, true)) return BSW_OK;
        const int ns = std::min<int>(kSlots, nchunks);
        Slot *sp[kSlots] = {slots[0].get()};
        int r = BSW_OK;
        for (int j = 1; j < ns && !r; ++j)
            if (!(r = take_slot(j, res))) sp[j] = slots[j].get();
        if (!r) r = prime_copies(sp, ns);
        if (r) dc.copies_warm.store(false);
        return r;
    }

    int stage(int k, int32_t seq, const ChunkRange &ch, const BlkStat *bs, StagedChunk &c)
    {
        const int32_t a = ch.b * kStageBlk, m = chunk_pairs(ch, n);
        const auto t0 = std::chrono::steady_clock::now();
        if (int r = stage_chunk(*slots[k], pairs + a, ref, qer, m, bs + ch.b, ch.nb, two_bit, c)) return r;
        stage_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        pend[k] = Pending{a, m, seq, c.mode};
        return BSW_OK;
    }

    // the device side of one staged chunk -- H2D of the slot's staging buffer, unpack kernels,
    // plan / sort -- then its launcher job, whatever the status.  Everything but the DP kernels
    // runs on the slot's high-priority stream: the next chunk's copies, unpack / plan / sort
    // kernels and the outputs' readback are dispatched ahead of the queued DP workgroups
    int enqueue(int k, int32_t seq, const StagedChunk &c)
    {
        const int r = enqueue_device(*slots[k], c);
        to_launcher(k, seq, c.mode, r);
        return r;
    }
    int enqueue_device(Slot &s, const StagedChunk &c)
    {
        if (int e = ensure_pstream(s)) return e;
        hipStream_t hs = s.pstream;
        const StageLayout &l = c.lay;
        BSW_TRY(s.d_stage.grow(l.bytes));
        BSW_TRY(hipMemcpyAsync(s.d_stage, s.h_stage, l.bytes, hipMemcpyHostToDevice, hs));
        const uint8_t *d_r = s.d_stage + l.ref_off, *d_q = s.d_stage + l.qer_off;
        SeqPair *d_p = (SeqPair *)(s.d_stage + l.pair_off);
        if (c.mode == kStage2bit) {     // 2-bit codes -> bytes, exceptions patched, records expanded
            // one launch (stage_in_kernel: both unpacks, the exception patches, the records and
            // the pad zeroing) instead of six: a chunk's enqueue is launch-bound on the host
            // (~60 us per launch while the pool packs the next chunk, HIP API trace
            // profiles/r04/hostpath_api_trace.txt)
            BSW_TRY(s.d_ref.grow(c.rb + 16));
            BSW_TRY(s.d_qer.grow(c.qb + 16));
            BSW_TRY(s.d_pairs.grow((size_t)c.n));
            if (int e = launch_stage_in(s, hs, d_r, (int64_t)c.rb, d_q, (int64_t)c.qb,
                                        (const uint32_t *)(s.d_stage + l.exc_off), c.n_exr, c.n_exr + c.n_exq,
                                        (const PairIn *)(s.d_stage + l.pair_off), c.n, s.d_ref, s.d_qer, s.d_pairs,
                                        nullptr))
                return e;
            d_r = s.d_ref;
            d_q = s.d_qer;
            d_p = s.d_pairs;
        } else if (c.mode == kStageNibble) {    // nibbles -> one byte per base in the slot's buffers
            BSW_TRY(s.d_ref.grow(c.rb + 4));
            BSW_TRY(s.d_qer.grow(c.qb + 4));
            BSW_TRY(hipMemsetAsync(s.d_ref + c.rb, 0, 4, hs));
            BSW_TRY(hipMemsetAsync(s.d_qer + c.qb, 0, 4, hs));
            const int64_t tr = ((int64_t)c.rb + 7) / 8, tq = ((int64_t)c.qb + 7) / 8;
            if (tr > 0)
                hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((tr + 255) / 256)), dim3(256), 0, hs, d_r, s.d_ref,
                                   (int64_t)c.rb);
            if (tq > 0)
                hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, hs, d_q, s.d_qer,
                                   (int64_t)c.qb);
            BSW_TRY(hipGetLastError());
            d_r = s.d_ref;
            d_q = s.d_qer;
        }
        PlanCall pc;
        pc.d_pairs = d_p;
        // kernels index ref / qer by idr / idq: shift the bases so staged byte 0 is r_base / q_base
        pc.d_ref = d_r - c.r_base;
        pc.d_qer = d_q - c.q_base;
        pc.n = c.n; pc.w = w; pc.cell_bits = cell_bits; pc.stream = hs;
        pc.dp_stream = s.stream;
        pc.plan_stream = hs;
        return run_plan(kp, s, pc);
    }

    // launcher thread: a chunk's DP kernels and the readback of its outputs
    void launch(const LaunchJob &job)
    {
        int r = launcher_dev_ok ? BSW_OK : BSW_E_HIP;
        {
            std::lock_guard<std::mutex> g(mu);
            if (err) r = err;
        }
        Slot &p = *slots[job.k];
        if (!r) r = run_dp(kp, p);
        // the outputs' gather and readback go on the high-priority stream once the DP (and its
        // guard readback) is done: on the DP stream they would queue behind the next chunks'
        // DP workgroups (a 1.4 ms copy in the trace)
        hipStream_t os = p.run_stream;
        hipStream_t hs = p.plan.plan_stream;       // the chunk's helper stream
        if (!r && hs && p.run_stream != hs) {
            if (!p.evd && hipEventCreateWithFlags(&p.evd.p, hipEventDisableTiming) != hipSuccess) r = BSW_E_HIP;
            if (!r && (hipEventRecord(p.evd, p.run_stream) != hipSuccess ||
                       hipStreamWaitEvent(hs, p.evd, 0) != hipSuccess))
                r = BSW_E_HIP;
            os = hs;
            p.run_stream = hs;                     // finish_stats waits here: after the DP's stream
        }
        if (!r && job.mode == kStage2bit) {        // outputs only: 24 B per pair
            const int32_t m = p.plan.n;
            if (launch_gather_outputs(p.plan.d_pairs, (int32_t *)p.d_stage.p, m, os) != BSW_OK ||
                hipMemcpyAsync(p.h_stage, p.d_stage, (size_t)m * kOutBytes, hipMemcpyDeviceToHost, os) != hipSuccess)
                r = BSW_E_HIP;
        } else if (!r && hipMemcpyAsync(p.h_stage, p.plan.d_pairs, (size_t)p.plan.n * sizeof(SeqPair),
                                        hipMemcpyDeviceToHost, os) != hipSuccess) {
            r = BSW_E_HIP;
        }
        {
            std::lock_guard<std::mutex> g(mu);
            if (r && !err) err = r;
            launched[job.k] = job.seq;
        }
        cv.notify_all();
    }

    // wait for slot k's chunk, outputs back in the caller's records
    int finish(int k)
    {
        Pending &pd = pend[k];
        if (pd.n == 0) return BSW_OK;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return launched[k] == pd.seq; });
            if (err) return err;
        }
        Slot &s = *slots[k];
        if (int r = finish_stats(s)) return r;          // also BSW_E_RANGE: kernel guard tripped
        unstage_outputs(s, pairs + pd.at, pd.n, pd.mode);
        agg.kernel_ms += s.stats.kernel_ms;
        add_counters(agg, s.stats);
        pd.n = 0;
        return BSW_OK;
    }

    // the chunk loop: chunk j on slot j % kSlots, once that slot's last chunk is finished
    int run(const std::vector<ChunkRange> &chs, const BlkStat *bs, const SlotReserve &res)
    {
        BSW_TRY(hipSetDevice(dc.device));
        if (int r = reserve_slot(*slots[0], res)) return r;     // (slot 0 was taken before the threads started)
        if (chs.size() > 1)
            if (int r = warm_up(res, (int)chs.size())) return r;
        int32_t seq = 0;
        for (const ChunkRange &ch : chs) {
            const int k = seq % kSlots;
            if (int r = finish(k)) return r;
            if (int r = take_slot(k, res)) return r;
            StagedChunk c;
            if (int r = stage(k, seq, ch, bs, c)) return r;
            if (async) enqueuer.push(EnqJob{k, seq, c});
            else if (int r = enqueue(k, seq, c)) return r;
            ++seq;
        }
        for (int k = 0; k < kSlots; ++k)
            if (int r = finish(k)) return r;
        return BSW_OK;
    }
};

int host_shard(const KParams &kp, DeviceCtx &dc, SeqPair *pairs, const uint8_t *ref,
                      const uint8_t *qer, int32_t n, int32_t w, int cell_bits, int32_t chunk, bool two_bit,
                      bsw_stats_t *st)
{
    if (n == 0) return BSW_OK;
    const auto t_start = std::chrono::steady_clock::now();
    // the whole prepass (validation + per-block byte extents) before chunk 0: validating only chunk
    // 0's blocks first and the rest after it started measured no faster
    std::vector<BlkStat> bs;
    if (!prepass(pairs, n, bs)) return BSW_E_RANGE;
    if (chunk <= 0) chunk = n;
    const int32_t nblk = (int32_t)bs.size(), first_blk = first_chunk_blocks(nblk, chunk, BSW_HP_FIRST_BLK);
    const std::vector<ChunkRange> chs = chunk_schedule(bs, chunk, first_blk);
    SlotReserve res{};
    for (const ChunkRange &ch : chs) res.add(chunk_pairs(ch, n), bs.data() + ch.b, ch.nb, two_bit);

    ShardCall call(kp, dc, pairs, ref, qer, n, w, cell_bits, two_bit);
    int rc = BSW_OK;
    call.slots[0] = dc.acquire(rc);
    if (rc) return rc;
    call.start(nblk > first_blk);
    rc = call.run(chs, bs.data(), res);
    call.enqueuer.stop();                               // handles its queue first (every job reaches the launcher)
    call.launcher.stop();
    call.agg.stage_ms = (float)call.stage_ms;
    call.agg.host_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    // give_back(slot, rc) drains a failed call's slots: their stream and pstream, which may hold
    // queued chunks, and also run_stream and the side streams -- idle by now, since the launcher
    // has been joined and run_dp joins its fork before it returns, so the wider drain waits on
    // nothing more
    for (auto &s : call.slots)
        if (s) dc.give_back(std::move(s), rc);
    if (rc == BSW_OK && st) *st = call.agg;
    return rc;
}

// ---------------------------------------------------------------- cross-call coalescing
// Upstream's kt_for workers each hand getScores* a few thousand pairs per call.  Run one by one,
// every such call pays a plan / sort / DP launch sequence whose lane-per-pair waves live ~1 ms
// whatever the batch size, and 8 workers' calls contend for the runtime.  Here a small call
// (<= BSW_OPT_COALESCE pairs) is queued on its device; the first caller that finds fewer than
// agg_leaders_max batches in flight becomes a leader, takes EVERY queued call of the same
// (w, cell_bits, end_bonus) -- its own or others' -- and runs them as one device batch: the
// callers' contiguous byte extents 2-bit-packed side by side in one pinned staging buffer
// (records rebased), one H2D, one plan / sort / DP, 24 B of outputs per pair back, scattered
// to each caller's records.  A lone caller leads its own one-call batch at once (no added
// wait); under load, calls that arrive while a batch is on the GPU form the next one.
// Outputs are identical to separate calls (pairs are independent).
struct AggReq {
    SeqPair *pairs;
    const uint8_t *ref, *qer;
    int32_t n, w;
    int cell_bits;
    int32_t eb;
    int rc = BSW_OK;
    bsw_stats_t st{};
    bool done = false;
};
constexpr int32_t kAggMaxPairs = 262144;        // pairs per coalesced batch
constexpr int64_t kAggLingerPairs = 4096;       // a lingering leader starts once this many are queued

struct AggSeg {                                 // one call inside a coalesced batch
    AggReq *r;
    int64_t r_lo, r_hi, q_lo, q_hi;             // the call's byte extents in its own buffers
    int64_t r_off, q_off;                       // their offsets in the batch's code space
    int32_t p_off;                              // first record in the batch
};

static int run_group_staged(const KParams &kp, DeviceCtx &dc, std::vector<AggSeg> &segs, int32_t N, int64_t r_tot,
                            int64_t q_tot, int32_t w, int cell_bits, bsw_stats_t &st)
{
    return with_slot(dc, [&](Slot &s) -> int {
        const size_t cap = exc_cap((size_t)r_tot, (size_t)q_tot);
        const StageLayout l = stage_layout(kStage2bit, (size_t)N, (size_t)r_tot, (size_t)q_tot, cap);
        const size_t pair_off = l.pair_off, ref_off = l.ref_off, qer_off = l.qer_off, exc_off = l.exc_off;
        BSW_TRY(s.h_stage.grow(l.bytes));
        const auto tg0 = std::chrono::steady_clock::now();
        uint8_t *h = s.h_stage;
        memset(h + ref_off, 0, l.ref_len + 4);          // the padding between calls' extents
        memset(h + qer_off, 0, l.qer_len + 4);
        // tasks: per call its records, and its ref / qer extents in pieces of <= 1 MB cut at
        // multiples of 64 codes (every call's extent starts 64-aligned in the code space)
        struct Task { int seg, kind; int64_t a, b; };
        std::vector<Task> tasks;
        constexpr int64_t kPiece = (int64_t)1 << 20;
        for (int g = 0; g < (int)segs.size(); ++g) {
            tasks.push_back(Task{g, 0, 0, 0});
            for (int kind = 1; kind <= 2; ++kind) {
                const int64_t len = kind == 1 ? segs[g].r_hi - segs[g].r_lo : segs[g].q_hi - segs[g].q_lo;
                for (int64_t a = 0; a < len; a += kPiece) tasks.push_back(Task{g, kind, a, std::min(len, a + kPiece)});
            }
        }
        std::vector<std::vector<uint32_t>> ex(tasks.size());
        // per task: the row-group kernel's contract over its records (max qlen, or -1: a misfit)
        std::vector<int> gq_maxq(tasks.size(), 0), gq_maxt(tasks.size(), 0);
        PairIn *pin = (PairIn *)(h + pair_off);
        HostPool::get().parallel_for((int)tasks.size(), [&](int t) {
            const Task &k = tasks[t];
            const AggSeg &g = segs[k.seg];
            if (k.kind == 0) {
                const SeqPair *p = g.r->pairs;
                int maxq = 0, maxt = 0;
                for (int32_t i = 0; i < g.r->n; ++i) {
                    PairIn &o = pin[g.p_off + i];
                    o.idr = p[i].len1 > 0 ? (int32_t)(p[i].idr - g.r_lo + g.r_off) : 0;
                    o.idq = p[i].len2 > 0 ? (int32_t)(p[i].idq - g.q_lo + g.q_off) : 0;
                    o.len1 = p[i].len1; o.len2 = p[i].len2; o.h0 = p[i].h0;
                    if (maxq >= 0) maxq = gq_pair_ok(kp, p[i].len2, p[i].len1, p[i].h0, 16) ? std::max(maxq, p[i].len2) : -1;
                    maxt = std::max(maxt, p[i].len1);
                }
                gq_maxq[t] = maxq;
                gq_maxt[t] = maxt;
            } else if (k.kind == 1) {
                pack_2bit(h + ref_off + (g.r_off + k.a) / 4, g.r->ref + g.r_lo + k.a, (size_t)(k.b - k.a),
                          (uint32_t)(g.r_off + k.a), ex[t]);
            } else {
                pack_2bit(h + qer_off + (g.q_off + k.a) / 4, g.r->qer + g.q_lo + k.a, (size_t)(k.b - k.a),
                          (uint32_t)(g.q_off + k.a), ex[t]);
            }
        });
        size_t n_r = 0, n_q = 0;
        for (size_t t = 0; t < tasks.size(); ++t) (tasks[t].kind == 1 ? n_r : n_q) += ex[t].size();
        if (n_r + n_q > cap) return 1;                  // too many non-ACGT bytes: caller splits
        uint32_t *exw = (uint32_t *)(h + exc_off);
        size_t o_r = 0, o_q = n_r;
        for (size_t t = 0; t < tasks.size(); ++t) {
            if (ex[t].empty()) continue;
            size_t &o = tasks[t].kind == 1 ? o_r : o_q;
            memcpy(exw + o, ex[t].data(), ex[t].size() * 4);
            o += ex[t].size();
        }
        const size_t up = exc_off + (n_r + n_q) * 4;
        const auto tg1 = std::chrono::steady_clock::now();
        BSW_TRY(s.d_stage.grow(stage_layout(kStage2bit, (size_t)N, (size_t)r_tot, (size_t)q_tot, n_r + n_q).bytes));
        BSW_TRY(hipMemcpyAsync(s.d_stage, s.h_stage, up, hipMemcpyHostToDevice, s.stream));
        BSW_TRY(s.d_ref.grow((size_t)r_tot + 4));
        BSW_TRY(s.d_qer.grow((size_t)q_tot + 4));
        BSW_TRY(s.d_pairs.grow((size_t)N));
        const int32_t ne = (int32_t)(n_r + n_q);
        if (int e = launch_stage_in(s, s.stream, s.d_stage + ref_off, r_tot, s.d_stage + qer_off, q_tot,
                                    (const uint32_t *)(s.d_stage + exc_off), (int32_t)n_r, ne,
                                    (const PairIn *)(s.d_stage + pair_off), N, s.d_ref, s.d_qer, s.d_pairs,
                                    s.d_meta + kMetaErr))
            return e;
        PlanCall pc;
        pc.d_pairs = s.d_pairs; pc.d_ref = s.d_ref; pc.d_qer = s.d_qer;
        pc.n = N; pc.w = w; pc.cell_bits = cell_bits; pc.stream = s.stream;
        int gq_max = 0, gq_mt = 0;
        for (size_t t = 0; t < tasks.size(); ++t)
            if (tasks[t].kind == 0) {
                gq_max = (gq_max < 0 || gq_maxq[t] < 0) ? -1 : std::max(gq_max, gq_maxq[t]);
                gq_mt = std::max(gq_mt, gq_maxt[t]);
            }
        pc.gq_maxq = gq_max;
        pc.gq_maxt = gq_mt;
        // host-checked row-group batch: the kernel writes the 24 output bytes per pair straight
        // into the staging buffer (its inputs were expanded out of it above)
        if (pc.gq_maxq >= 0) pc.d_out24 = (int32_t *)s.d_stage.p;
        int r = run_plan(kp, s, pc);
        if (!r) r = run_dp(kp, s);
        if (r) {
            (void)hipStreamSynchronize(s.stream);
            return r;
        }
        if (!(s.fast == 2 && s.plan.d_out24))
            if (int e = launch_gather_outputs(s.d_pairs, (int32_t *)s.d_stage.p, N, s.stream)) return e;
        BSW_TRY(hipMemcpyAsync(s.h_stage, s.d_stage, (size_t)N * kOutBytes, hipMemcpyDeviceToHost, s.stream));
        // the leader polls its batch (~0.3 ms) instead of the runtime's blocking wait: 8 callers x 1K
        // coalesced 11.4 / 12.4 -> 14.1 / 13.5 M/s (same box, alternating; profiles/r05/slot_ownq_percall.txt)
        if ((r = finish_stats(s, true))) return r;
        const int32_t *out = (const int32_t *)s.h_stage.p;
        auto scatter = [&](int g) {
            SeqPair *p = segs[g].r->pairs;
            const int32_t *q = out + 6 * (int64_t)segs[g].p_off;
            for (int32_t i = 0; i < segs[g].r->n; ++i, q += 6) put_outputs(p[i], q);
        };
        // a few thousand records: on this thread (waking the host pool costs more than the copy)
        if (N <= 16384)
            for (int g = 0; g < (int)segs.size(); ++g) scatter(g);
        else
            HostPool::get().parallel_for((int)segs.size(), scatter);
        st = s.stats;
        st.stage_ms = (float)std::chrono::duration<double, std::milli>(tg1 - tg0).count();
        return BSW_OK;
    });
}

// One coalesced batch: calls that fail validation get BSW_E_RANGE; calls whose buffers are not
// contiguous (scattered idr / idq) and batches with too many non-ACGT bytes run on their own
// through host_shard.
static void run_group(const KParams &kp, DeviceCtx &dc, std::vector<AggReq *> &G, int32_t chunk, bool two_bit)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<AggSeg> segs;
    std::vector<AggReq *> alone;
    int64_t r_tot = 0, q_tot = 0;
    int32_t N = 0;
    for (AggReq *r : G) {
        std::vector<BlkStat> bs;
        if (!prepass(r->pairs, r->n, bs)) { r->rc = BSW_E_RANGE; continue; }
        const BlkStat t = merge_blocks(bs.data(), (int32_t)bs.size());
        const int64_t r_lo = t.r_lo, r_hi = t.r_hi, q_lo = t.q_lo, q_hi = t.q_hi;
        if (!two_bit || !bulk_extents(t)) { alone.push_back(r); continue; }
        segs.push_back(AggSeg{r, r_lo, r_hi, q_lo, q_hi, r_tot, q_tot, N});
        r_tot = (r_tot + (r_hi - r_lo) + 63) & ~(int64_t)63;
        q_tot = (q_tot + (q_hi - q_lo) + 63) & ~(int64_t)63;
        N += r->n;
    }
    if (!segs.empty()) {
        bsw_stats_t st{};
        const int rc = (r_tot < ((int64_t)1 << 30) && q_tot < ((int64_t)1 << 30))
                           ? run_group_staged(kp, dc, segs, N, r_tot, q_tot, segs[0].r->w, segs[0].r->cell_bits, st)
                           : 1;
        if (rc == 1) {
            for (auto &g : segs) alone.push_back(g.r);
        } else {
            st.n_devices = 1;
            st.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            for (auto &g : segs) { g.r->rc = rc; g.r->st = st; }
        }
    }
    for (AggReq *r : alone) {
        bsw_stats_t st{};
        r->rc = host_shard(kp, dc, r->pairs, r->ref, r->qer, r->n, r->w, r->cell_bits, chunk, two_bit, &st);
        st.n_devices = 1;
        r->st = st;
    }
}

int coalesced_call(const KParams &kp, DeviceCtx &dc, SeqPair *pairs, const uint8_t *ref, const uint8_t *qer,
                          int32_t n, int32_t w, int cell_bits, int32_t chunk, bool two_bit, bsw_stats_t *st)
{
    AggReq me{pairs, ref, qer, n, w, cell_bits, kp.end_bonus};
    std::unique_lock<std::mutex> lk(dc.agg_mu);
    dc.agg_q.push_back(&me);
    dc.agg_qn += n;
    ++dc.agg_inside;
    if (dc.agg_lingering > 0) dc.agg_cv.notify_all();      // a lingering leader counts the queue
    while (!me.done) {
        if (dc.agg_leaders < dc.agg_leaders_max && !dc.agg_q.empty()) {
            // lead: every queued call with the front call's (w, cell_bits, end_bonus), FIFO
            // linger only when there are more callers than leader slots (batching is then the only
            // way to serve them all) and two or more batches run: with fewer callers the batches
            // must overlap instead -- a lingering leader serialised 2 callers (1K: 4.0 vs 6.8 M/s)
            // and cost 4 callers a quarter (profiles/r04/percall_linger_r4{q,r}.txt)
            if (dc.agg_inside > dc.agg_leaders_max && dc.agg_nrun >= 2 && dc.agg_linger_us > 0 &&
                dc.agg_qn < kAggLingerPairs) {
                // the device is busy anyway: hold this leader's place until the queue holds
                // kAggLingerPairs pairs (the next calls of the callers whose batches just finished),
                // the device goes idle, or linger_us passes -- a row-group batch costs ~0.3 ms
                // whether it carries 1K or 4K pairs, so fuller batches are the small-call
                // throughput
                ++dc.agg_leaders;
                ++dc.agg_lingering;
                dc.agg_cv.wait_for(lk, std::chrono::microseconds(dc.agg_linger_us), [&] {
                    return me.done || dc.agg_qn >= kAggLingerPairs || dc.agg_nrun < 2;
                });
                --dc.agg_lingering;
                --dc.agg_leaders;
                if (me.done) break;
                if (dc.agg_q.empty()) continue;       // another leader took every queued call
            }
            ++dc.agg_leaders;
            std::vector<AggReq *> G;
            const AggReq *f = dc.agg_q.front();
            const int32_t fw = f->w, feb = f->eb;
            const int fcb = f->cell_bits;
            int64_t tot = 0;
            for (auto it = dc.agg_q.begin(); it != dc.agg_q.end();) {
                AggReq *r = *it;
                if (r->w == fw && r->cell_bits == fcb && r->eb == feb && (G.empty() || tot + r->n <= kAggMaxPairs)) {
                    G.push_back(r);
                    tot += r->n;
                    dc.agg_qn -= r->n;
                    it = dc.agg_q.erase(it);
                } else {
                    ++it;
                }
            }
            dc.agg_run += tot;
            ++dc.agg_nrun;
            lk.unlock();
            KParams gk = kp;
            gk.end_bonus = feb;
            run_group(gk, dc, G, chunk, two_bit);
            lk.lock();
            dc.agg_run -= tot;
            --dc.agg_nrun;
            --dc.agg_leaders;
            for (AggReq *r : G) r->done = true;
            dc.agg_cv.notify_all();
        } else {
            dc.agg_cv.wait(lk);
        }
    }
    --dc.agg_inside;
    if (st) *st = me.st;
    return me.rc;
}

}  // namespace bsw
