// bsw_sort.hip -- sort_order (bsw_sort.h): the stable sort that turns plan keys into order[].
//
// A least-significant-digit radix sort whose digits are taken from the key bits that vary in the batch
// (the key mask of bsw_sort.h), 8 at a time in rank order: npass = ceil(popcount(varying) / 8) <= 4.
// On the C2 key (class, qlen and tlen / 32 constant) that is two passes instead of the library's block
// sort and ten merge rounds (21 dependent launches at 1M pairs).
//
// A pass is three plain kernels, ordered by their kernel boundaries alone -- no workgroup ever waits
// for another one:
//   count   : a tile of kSortTile keys -> its digit histogram -> table[digit][tile]
//   scan    : workgroup d scans row d of the table over the tiles in place, totals[d] = the row's sum
//   scatter : the tile again: offset of digit d = (sum of totals below d) + table[d][tile], plus the
//             key's stable rank inside the tile; the tile is put in order in LDS and stored from there
// A tile is read in the order (wave, round, lane): wave w of the workgroup's 16 owns keys [256 w, 256 w + 256)
// of the tile and walks them 64 at a time, so a wave-private running count per digit ranks them stably.
// (Four rounds per wave, not sixteen: at 1M keys there are only 245 tiles, and a kernel lasts as long as one
// wave's chain of rounds.)
//
// The host enqueues every pass the key width allows without knowing the mask; each kernel derives npass
// and its pass's bits from the mask and returns at once when its pass index is >= npass.  Buffers, with
// I = (d_keys, d_vals), O = (d_keys2, d_order) and T = a pair in d_tmp: pass p writes O when an even
// number of passes follow it and T otherwise, and reads I (p = 0) or what pass p - 1 wrote -- so the
// last pass writes d_order for every npass, and I is never written.  The last pass writes no keys.
// npass = 0 (all keys equal): pass 0's count kernel copies d_vals to d_order.
//
// BSW_SORT=lib in the environment restores the library call (hipCUB DeviceRadixSort) for A/B runs;
// -DBSW_SORT_ONESWEEP builds the library's own radix route (rocPRIM with merge_sort_limit = 0) as the
// comparison arm (profiles/sort_order/ab.txt).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rocprim/rocprim.hpp>
#include <cstdlib>
#include <cstring>
#include "bsw_engine.h"
#include "bsw_sort.h"

namespace bsw {

static_assert(kSortTile % kSortThreads == 0 && kSortThreads % 64 == 0 && kSortThreads >= 256, "whole rounds, whole waves, a thread per digit");
static_assert(kMetaSpread <= 64, "one lane per mask slot");
constexpr int kSortRounds = kSortTile / kSortThreads;
constexpr int kSortWaves = kSortThreads / 64;

struct SortArgs {
    const uint32_t *keys_i;             // I: the caller's pairs (read only)
    const int32_t *vals_i;
    uint32_t *keys_o;                   // O: d_keys2, d_order
    int32_t *vals_o;
    uint32_t *keys_t;                   // T: in d_tmp
    int32_t *vals_t;
    uint32_t *table;                    // [256][nt], digit-major
    uint32_t *totals;                   // [256]
    const int32_t *mask;                // d_meta-shaped key mask, or null
    uint32_t n;
    int32_t nt;
    int32_t key_bits, pass;
};

// The pass's bit mask (its <= 8 bits of the varying set) and the batch's pass count; wave-uniform.
__device__ __forceinline__ uint32_t sort_pass_bits(const SortArgs &a, int &npass)
{
    uint32_t varying = a.key_bits >= 32 ? ~0u : (1u << a.key_bits) - 1u;
    if (a.mask) {
        const int lane = threadIdx.x & 63;
        uint32_t o = 0, no = 0;
        if (lane < kMetaSpread) {
            o = (uint32_t)a.mask[lane * kMetaCounts + kMetaKeyOr];
            no = (uint32_t)a.mask[lane * kMetaCounts + kMetaKeyNor];
        }
        varying &= wave_or(o) & wave_or(no);
        varying = (uint32_t)__builtin_amdgcn_readfirstlane((int)varying);
    }
    npass = (__popc(varying) + 7) >> 3;
    uint32_t v = varying;
    for (int j = 0; j < 8 * a.pass; ++j) v &= v - 1;        // drop the earlier passes' bits
    uint32_t rest = v;
    for (int j = 0; j < 8; ++j) rest &= rest - 1;           // ... and the later passes'
    return v ^ rest;
}

// the key's digit: its bits at the set positions of m, packed in rank order
__device__ __forceinline__ uint32_t sort_digit(uint32_t k, uint32_t m)
{
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (m) {
            d |= ((k >> (__ffs((int)m) - 1)) & 1u) << j;
            m &= m - 1;
        }
    }
    return d;
}

// lanes of the wave that hold a valid key with this lane's digit (nb = the digit's width)
__device__ __forceinline__ unsigned long long sort_peers(uint32_t d, bool valid, int nb)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < nb) {
            const bool bit = (d >> j) & 1u;
            const unsigned long long b = __ballot(bit);
            peers &= bit ? b : ~b;
        }
    }
    return peers;
}

__device__ __forceinline__ bool sort_writes_o(int npass, int pass) { return ((npass - 1 - pass) & 1) == 0; }

__global__ __launch_bounds__(kSortThreads) void sort_count_kernel(const SortArgs a)
{
    int npass;
    const uint32_t m = sort_pass_bits(a, npass);
    const uint32_t tile0 = blockIdx.x * (uint32_t)kSortTile;
    if (a.pass >= npass) {
        if (a.pass == 0)                    // npass == 0, all keys equal: the order is the input's
            for (int j = 0; j < kSortRounds; ++j) {
                const uint32_t i = tile0 + j * kSortThreads + threadIdx.x;
                if (i < a.n) a.vals_o[i] = a.vals_i[i];
            }
        return;
    }
    const uint32_t *keys = a.pass == 0 ? a.keys_i : (sort_writes_o(npass, a.pass - 1) ? a.keys_o : a.keys_t);
    const int nb = __popc(m);
    __shared__ uint32_t hist[256];
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t base = tile0 + (threadIdx.x >> 6) * (kSortTile / kSortWaves) + lane;
    uint32_t k[kSortRounds];
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j) {
        const uint32_t i = base + j * 64;
        k[j] = i < a.n ? keys[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j) {
        const bool valid = base + j * 64 < a.n;
        const uint32_t d = sort_digit(k[j], m);
        const unsigned long long peers = sort_peers(d, valid, nb);
        if (valid && lane == __ffsll((long long)peers) - 1) atomicAdd(&hist[d], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    if (threadIdx.x < 256) a.table[(size_t)threadIdx.x * a.nt + blockIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(kSortScanChunk) void sort_scan_kernel(const SortArgs a)
{
    int npass;
    (void)sort_pass_bits(a, npass);
    if (a.pass >= npass) return;
    using Scan = hipcub::BlockScan<uint32_t, kSortScanChunk>;
    __shared__ typename Scan::TempStorage tmp;
    uint32_t *row = a.table + (size_t)blockIdx.x * a.nt;
    uint32_t carry = 0;
    for (int32_t c = 0; c < a.nt; c += kSortScanChunk) {
        const int32_t i = c + (int32_t)threadIdx.x;
        const uint32_t v = i < a.nt ? row[i] : 0u;
        uint32_t ex, sum;
        Scan(tmp).ExclusiveSum(v, ex, sum);
        if (i < a.nt) row[i] = carry + ex;
        carry += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const SortArgs a)
{
    int npass;
    const uint32_t m = sort_pass_bits(a, npass);
    if (a.pass >= npass) return;
    const bool from_i = a.pass == 0, from_o = !from_i && sort_writes_o(npass, a.pass - 1);
    const uint32_t *keys = from_i ? a.keys_i : from_o ? a.keys_o : a.keys_t;
    const int32_t *vals = from_i ? a.vals_i : from_o ? a.vals_o : a.vals_t;
    const bool to_o = sort_writes_o(npass, a.pass), last = a.pass == npass - 1;
    uint32_t *keys_w = to_o ? a.keys_o : a.keys_t;
    int32_t *vals_w = to_o ? a.vals_o : a.vals_t;
    const int nb = __popc(m);
    __shared__ uint32_t whist[kSortWaves][256];    // per wave and digit: running count, then the place in LDS
    __shared__ uint32_t wsum[4], lsum[4];          // the two scans' sums of waves 0..3
    __shared__ uint32_t gofs[256];                 // per digit: place in the output - place in LDS
    __shared__ uint32_t skey[kSortTile];           // the tile in sorted order
    __shared__ int32_t sval[kSortTile];
    for (int e = threadIdx.x; e < kSortWaves * 256; e += kSortThreads) (&whist[0][0])[e] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t tile0 = blockIdx.x * (uint32_t)kSortTile;
    const uint32_t base = tile0 + wv * (kSortTile / kSortWaves) + lane;
    uint32_t k[kSortRounds], dr[kSortRounds];      // dr: digit << 16 | rank among the wave's keys of that digit
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j) {
        const uint32_t i = base + j * 64;
        k[j] = i < a.n ? keys[i] : 0u;
    }
    int32_t v[kSortRounds];
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j) {
        const uint32_t i = base + j * 64;
        v[j] = i < a.n ? vals[i] : 0;
    }
    volatile uint32_t *wh = whist[wv];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j) {
        const bool valid = base + j * 64 < a.n;
        const uint32_t d = sort_digit(k[j], m);
        const unsigned long long peers = sort_peers(d, valid, nb);
        const uint32_t prior = wh[d];              // every peer reads it before their first lane adds
        __builtin_amdgcn_wave_barrier();
        if (valid && lane == __ffsll((long long)peers) - 1) wh[d] = prior + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        dr[j] = (d << 16) | (prior + (uint32_t)__popcll(peers & below));
    }
    __syncthreads();
    // thread d < 256: where digit d's keys of this tile start in the output (the digits' totals scanned: inside
    // each of the first four waves, then over their sums) and in LDS (the same scan over the tile's own digit
    // counts), then each wave's share of them in turn
    uint32_t inc = 0, tot = 0, linc = 0, cnt = 0;
    if (threadIdx.x < 256) {
        inc = tot = a.totals[threadIdx.x];
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) cnt += whist[w][threadIdx.x];
        linc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= o) inc += up;
            const uint32_t lup = (uint32_t)__shfl_up((int)linc, o);
            if (lane >= o) linc += lup;
        }
        if (lane == 63) {
            wsum[wv] = inc;
            lsum[wv] = linc;
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        uint32_t g = inc - tot + a.table[(size_t)threadIdx.x * a.nt + blockIdx.x];
        for (int w = 0; w < wv; ++w) g += wsum[w];
        uint32_t l = linc - cnt;
        for (int w = 0; w < wv; ++w) l += lsum[w];
        gofs[threadIdx.x] = g - l;
        g = l;
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) {
            const uint32_t c = whist[w][threadIdx.x];
            whist[w][threadIdx.x] = g;
            g += c;
        }
    }
    __syncthreads();
    // through LDS in sorted order, so that neighbouring lanes store to neighbouring places of a digit's run
    // (a tile holds 16 keys per digit on average: stored from registers, every lane of a wave hit another line)
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j)
        if (base + j * 64 < a.n) {
            const uint32_t l = whist[wv][dr[j] >> 16] + (dr[j] & 0xffffu);
            skey[l] = k[j];
            sval[l] = v[j];
        }
    __syncthreads();
    const uint32_t here = min(a.n - tile0, (uint32_t)kSortTile);
#pragma unroll
    for (int j = 0; j < kSortRounds; ++j) {
        const uint32_t l = j * kSortThreads + threadIdx.x;
        if (l < here) {
            const uint32_t key = skey[l], pos = gofs[sort_digit(key, m)] + l;
            vals_w[pos] = sval[l];
            if (!last) keys_w[pos] = key;
        }
    }
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the library routes: hipCUB's DeviceRadixSort (the A/B switch), or rocPRIM's radix_sort_pairs forced
// onto its onesweep path (the comparison arm's build)
static hipError_t lib_sort(void *tmp, size_t &bytes, Slot &s, int32_t n, int key_bits, hipStream_t st)
{
#ifdef BSW_SORT_ONESWEEP
    using Cfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;
    return rocprim::radix_sort_pairs<Cfg>(tmp, bytes, s.d_keys.p, s.d_keys2.p, s.d_vals.p, s.d_order.p, (size_t)n, 0u,
                                          (unsigned)key_bits, st);
#else
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, s.d_keys.p, s.d_keys2.p, s.d_vals.p, s.d_order.p, n, 0,
                                              key_bits, st);
#endif
}

static bool sort_use_lib()
{
#ifdef BSW_SORT_ONESWEEP
    return true;
#else
    static const bool lib = [] {
        const char *e = getenv("BSW_SORT");
        return e && !strcmp(e, "lib");
    }();
    return lib;
#endif
}

hipError_t sort_order(Slot &s, int32_t n, int key_bits, hipStream_t st, bool run, const int32_t *d_mask)
{
    if (n <= 0) return hipSuccess;
    if (sort_use_lib()) {
        size_t tmp_bytes = 0;
        hipError_t e = lib_sort(nullptr, tmp_bytes, s, n, key_bits, st);
        if (e == hipSuccess) e = s.d_tmp.grow(tmp_bytes);
        if (e == hipSuccess && run) e = lib_sort(s.d_tmp, tmp_bytes, s, n, key_bits, st);
        return e;
    }
    const int32_t nt = sort_tiles(n);
    const size_t table_b = align256((size_t)256 * nt * sizeof(uint32_t)), totals_b = 256 * sizeof(uint32_t);
    const size_t col_b = align256((size_t)n * sizeof(uint32_t));
    hipError_t e = s.d_tmp.grow(table_b + totals_b + 2 * col_b);
    if (e != hipSuccess || !run) return e;
    SortArgs a;
    a.keys_i = s.d_keys; a.vals_i = s.d_vals;
    a.keys_o = s.d_keys2; a.vals_o = s.d_order;
    a.table = reinterpret_cast<uint32_t *>(s.d_tmp.p);
    a.totals = reinterpret_cast<uint32_t *>(s.d_tmp.p + table_b);
    a.keys_t = reinterpret_cast<uint32_t *>(s.d_tmp.p + table_b + totals_b);
    a.vals_t = reinterpret_cast<int32_t *>(s.d_tmp.p + table_b + totals_b + col_b);
    a.mask = d_mask;
    a.n = (uint32_t)n; a.nt = nt; a.key_bits = key_bits;
    const int max_pass = (std::min(std::max(key_bits, 1), 32) + 7) / 8;
    for (int p = 0; p < max_pass; ++p) {
        a.pass = p;
        hipLaunchKernelGGL(sort_count_kernel, dim3((unsigned)nt), dim3(kSortThreads), 0, st, a);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(256), dim3(kSortScanChunk), 0, st, a);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)nt), dim3(kSortThreads), 0, st, a);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------- test hook (not part of the ABI)
__global__ void sort_hook_kernel(const uint32_t *__restrict__ keys, int32_t n, int32_t *__restrict__ vals,
                                 int32_t *meta)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    if (valid) vals[i] = i;
    if (!meta) return;
    __shared__ uint32_t s_or[2];
    key_mask_zero(s_or);
    __syncthreads();
    key_mask_add(valid ? keys[i] : 0u, valid, s_or);
    __syncthreads();
    key_mask_flush(s_or, meta);
}

}  // namespace bsw

// sort_order on its own, for tests (beside bsw_pc_stats: no part of the ABI): n keys at d_keys -> a
// slot, values 0..n-1, the key mask by a kernel of its own when use_mask is set, the permutation to
// d_order_out.  Both pointers may be device or host memory.
extern "C" int bsw_sort_order_device(bsw_ctx_t *ctx, const uint32_t *d_keys, int32_t n, int key_bits, int use_mask,
                                     int32_t *d_order_out)
{
    using namespace bsw;
    if (!ctx || n < 0 || key_bits < 1 || key_bits > 32) return BSW_E_INVAL;
    if (n == 0) return BSW_OK;
    if (!d_keys || !d_order_out) return BSW_E_INVAL;
    return with_slot(*ctx->devs[0], [&](Slot &s) -> int {
        hipStream_t st = s.stream;
        BSW_TRY(grow_sort(s, n));
        BSW_TRY(hipMemcpyAsync(s.d_keys, d_keys, (size_t)n * sizeof(uint32_t), hipMemcpyDefault, st));
        BSW_TRY(hipMemsetAsync(s.d_meta, 0, kMetaWords * sizeof(int32_t), st));
        hipLaunchKernelGGL(sort_hook_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.d_keys.p, n,
                           s.d_vals.p, use_mask ? s.d_meta.p : nullptr);
        BSW_TRY(hipGetLastError());
        BSW_TRY(sort_order(s, n, key_bits, st, true, use_mask ? s.d_meta.p : nullptr));
        BSW_TRY(hipMemcpyAsync(d_order_out, s.d_order, (size_t)n * sizeof(int32_t), hipMemcpyDefault, st));
        BSW_TRY(hipStreamSynchronize(st));
        return BSW_OK;
    });
}
