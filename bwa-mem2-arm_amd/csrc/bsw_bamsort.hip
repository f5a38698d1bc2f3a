// bsw_bamsort.hip -- coordinate sort of BAM alignment blocks and the .bai (include/bsw_bamsort.h).
//   the sort   bam_key_kernel      one lane per record: the block checks, a 64-bit key, the value i, the keys' OR / NOR
//              (hipCUB radix sort of (key, i) over the key bits that vary: stable)
//              bam_len_kernel      the sorted lengths (scanned into d_out_off)
//              bam_tile_kernel     each output tile's first record, by a search of d_out_off
//              bam_permute_kernel  the hot path, output stationary: a workgroup owns kPermTile aligned bytes of d_out,
//                                  finds each 16-byte piece's record in its slice of d_out_off (LDS) and puts the piece
//                                  together from five aligned source dwords behind a funnel shift; pieces that straddle
//                                  two records fall back to dwords, dwords that straddle to bytes
//   the index  bai_extent_kernel   one lane per sorted record: checks, extent, bin, the (refID, bin) key
//              bai_window_kernel   order check, the references' first / last records, atomicMin into the flat linear
//                                  index and atomicMax of the last window (a record whose predecessor covers the window
//                                  cannot be the minimum and skips the atomic)
//              bai_fill_kernel     per reference: untouched windows take the next touched one's value (suffix minimum)
//              (hipCUB radix sort of ((refID, bin), i): stable, so a bin's members stay in file order)
//              bai_flag_kernel / scans / bai_compact_kernel / bai_size_kernel   bin and chunk heads, their indices, sizes
//              bai_ref_kernel, bai_bin_kernel                                    the file
// Everything per record is bsw_bamsort_k.h, shared with the serial model tools/bamsort_model.cpp.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include "bsw_bamsort_k.h"
#include "bsw_stage_k.h"

namespace bsw {

using namespace bamsort;

// ---------------------------------------------------------------- the sort
// a little-endian word at any byte p of a 4-byte aligned base, from the two aligned dwords it lies in (both inside the
// record when 8 bytes of it follow p)
__device__ __forceinline__ uint32_t ld32_dwords(const uint8_t *p)
{
    const uint32_t *a = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
    return (uint32_t)(((uint64_t)a[1] << 32 | a[0]) >> (8 * (int)((uintptr_t)p & 3)));
}
// read_fixed's fields of the sort (block_size, refID, pos, flag) by aligned dword loads
__device__ __forceinline__ Fixed read_fixed_sort(const uint8_t *bam, const uint8_t *blk)
{
    if ((uintptr_t)bam & 3) return read_fixed(blk);
    Fixed f{};
    f.block_size = (int32_t)ld32_dwords(blk);
    f.ref_id = (int32_t)ld32_dwords(blk + 4);
    f.pos = (int32_t)ld32_dwords(blk + 8);
    f.flag = ld32_dwords(blk + 16) >> 16;
    return f;
}

__global__ __launch_bounds__(256) void bam_key_kernel(const uint8_t *__restrict__ bam, const int64_t *__restrict__ off,
                                                      int32_t n_rec, int32_t n_ref, uint64_t *__restrict__ key,
                                                      int32_t *__restrict__ val, int32_t *__restrict__ meta)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint64_t k = 0;
    bool ok = false;
    if (i < n_rec) {
        const int64_t o0 = off[i], o1 = off[i + 1];
        if (span_ok(o0, o1) && (i > 0 || o0 == 0)) {
            const Fixed f = read_fixed_sort(bam, bam + o0);
            if (block_ok(f, o1 - o0, n_ref)) {
                ok = true;
                k = sort_key(f, n_ref);
            }
        }
        if (!ok) meta[kBsErr] = 1;
        key[i] = k;
        val[i] = i;
    }
    // OR of the keys and of their complements over the wave, then an atomic per wave and word that still has a bit to add
    uint32_t w[4] = {ok ? (uint32_t)k : 0u, ok ? (uint32_t)(k >> 32) : 0u, ok ? ~(uint32_t)k : 0u, ok ? ~(uint32_t)(k >> 32) : 0u};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] |= (uint32_t)__shfl_xor((int)w[q], o);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (w[q] & ~((volatile uint32_t *)meta)[kBsOr + q]) atomicOr((uint32_t *)meta + kBsOr + q, w[q]);
    }
}

__global__ __launch_bounds__(256) void bam_len_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ perm,
                                                      int32_t n_rec, int64_t *__restrict__ len)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n_rec) return;
    int64_t v = 0;
    if (i < n_rec) {
        const int32_t r = perm[i];
        v = off[r + 1] - off[r];
    }
    len[i] = v;
}

// 16 bytes of the output or of the source, 4-byte aligned, not more
struct __attribute__((packed, aligned(4))) Dwords4 { uint32_t x, y, z, w; };
// a dword of the output from the two aligned source dwords it lies in
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int sh) { return (uint32_t)(((uint64_t)hi << 32 | lo) >> sh); }

// tile_rec[t] = the last record that starts at or before byte t * kPermTile of the output (out_off[0] == 0): one lane per
// tile, so that the searches' dependent loads overlap instead of standing in front of every workgroup of the copy
__global__ __launch_bounds__(256) void bam_tile_kernel(const int64_t *__restrict__ out_off, int32_t n_rec, int32_t n_tiles,
                                                       int32_t *__restrict__ tile_rec)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tiles) return;
    const int64_t tile_beg = (int64_t)t * kPermTile;
    int lo = 0, hi = n_rec;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (out_off[mid] <= tile_beg) lo = mid; else hi = mid;
    }
    tile_rec[t] = lo;
}

__global__ __launch_bounds__(256) void bam_permute_kernel(const uint8_t *__restrict__ bam, const int64_t *__restrict__ off,
                                                          const int32_t *__restrict__ perm,
                                                          const int64_t *__restrict__ out_off,
                                                          const int32_t *__restrict__ tile_rec, int32_t n_rec,
                                                          int64_t n_bytes, uint8_t *__restrict__ out)
{
    __shared__ int32_t s_end[kPermSlice];           // the slice's record ends, from the tile's start; INT32_MAX behind it
    __shared__ int64_t s_delta[kPermSlice];         // source byte - output byte
    const int lane = threadIdx.x;
    const int64_t tile_beg = (int64_t)blockIdx.x * kPermTile;
    const int tile_n = (int)(n_bytes - tile_beg < kPermTile ? n_bytes - tile_beg : kPermTile);
    {
        const int r = tile_rec[blockIdx.x] + lane;
        int32_t e = INT32_MAX;
        int64_t d = 0;
        if (r < n_rec) {
            const int64_t o = out_off[r];
            if (o < tile_beg + tile_n) {
                const int64_t e64 = out_off[r + 1] - tile_beg;
                e = (int32_t)(e64 < kPermTile ? e64 : kPermTile);
                d = off[perm[r]] - o;
            }
        }
        s_end[lane] = e;
        s_delta[lane] = d;
    }
    __syncthreads();
    const uintptr_t in_beg = (uintptr_t)bam, in_end = in_beg + (uint64_t)n_bytes;
    for (int p = 16 * lane; p < tile_n; p += 16 * 256) {
        int k = 0;                                  // the record of byte p: the ends at or below p
#pragma unroll
        for (int step = kPermSlice / 2; step > 0; step >>= 1)
            if (s_end[k + step - 1] <= p) k += step;
        if (p + 16 <= s_end[k]) {
            const uintptr_t src = (uintptr_t)(bam + tile_beg + p + s_delta[k]), a = src & ~(uintptr_t)3;
            if (a >= in_beg && a + 20 <= in_end) {
                const int sh = 8 * (int)(src & 3);
                const Dwords4 v = *(const Dwords4 *)a;      // (one 16-byte load and a dword: the source is dword aligned)
                const uint32_t w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w, w4 = ((const uint32_t *)a)[4];
                *(Dwords4 *)(out + tile_beg + p) = Dwords4{funnel(w0, w1, sh), funnel(w1, w2, sh), funnel(w2, w3, sh),
                                                           funnel(w3, w4, sh)};
                continue;
            }
        }
        for (int q = p; q < p + 16 && q < tile_n; q += 4) {
            while (s_end[k] <= q) ++k;
            if (q + 4 <= s_end[k]) {
                const uintptr_t src = (uintptr_t)(bam + tile_beg + q + s_delta[k]), a = src & ~(uintptr_t)3;
                if (a >= in_beg && a + 8 <= in_end) {
                    const uint32_t *s32 = (const uint32_t *)a;
                    *(uint32_t *)(out + tile_beg + q) = funnel(s32[0], s32[1], 8 * (int)(src & 3));
                    continue;
                }
            }
            int kk = k;
            for (int b = q; b < q + 4 && b < tile_n; ++b) {
                while (s_end[kk] <= b) ++kk;
                out[tile_beg + b] = bam[tile_beg + b + s_delta[kk]];
            }
        }
    }
}

hipError_t launch_bamsort_keys(const uint8_t *bam, const int64_t *off, int32_t n_rec, int32_t n_ref, uint64_t *key,
                               int32_t *val, int32_t *meta, hipStream_t s)
{
    if (n_rec <= 0) return hipSuccess;
    hipLaunchKernelGGL(bam_key_kernel, grid_for(n_rec, 256), dim3(256), 0, s, bam, off, n_rec, n_ref, key, val, meta);
    return hipGetLastError();
}

hipError_t launch_bamsort_pairs(void *tmp, size_t *tmp_bytes, const uint64_t *key_in, uint64_t *key_out, const int32_t *val_in,
                                int32_t *val_out, int32_t n, int lo, int hi, hipStream_t s)
{
    return hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, key_in, key_out, val_in, val_out, n, lo, hi, s);
}

hipError_t launch_bamsort_lens(const int64_t *off, const int32_t *perm, int32_t n_rec, int64_t *len, hipStream_t s)
{
    hipLaunchKernelGGL(bam_len_kernel, grid_for((int64_t)n_rec + 1, 256), dim3(256), 0, s, off, perm, n_rec, len);
    return hipGetLastError();
}

hipError_t launch_bamsort_permute(const uint8_t *bam, const int64_t *off, const int32_t *perm, const int64_t *out_off,
                                  int32_t *tile_rec, int32_t n_rec, int64_t n_bytes, uint8_t *out, hipStream_t s)
{
    if (n_rec <= 0 || n_bytes <= 0) return hipSuccess;
    const int32_t n_tiles = (int32_t)bamsort_tiles(n_bytes);
    hipLaunchKernelGGL(bam_tile_kernel, grid_for(n_tiles, 256), dim3(256), 0, s, out_off, n_rec, n_tiles, tile_rec);
    hipLaunchKernelGGL(bam_permute_kernel, dim3(n_tiles), dim3(256), 0, s, bam, off, perm, out_off, tile_rec, n_rec, n_bytes,
                       out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the index
// per reference, uint32 words (zeroed per call)
constexpr int kRLastWin1 = 0;           // the last touched window + 1: n_intv
constexpr int kRFirst1 = 1, kRLast1 = 2;    // the first and the last record, + 1; 0: the reference has none
constexpr int kRUnmapped = 3;           // records with flag 0x4
constexpr int kRBin0 = 4, kRBin1 = 5;   // the reference's bins [kRBin0, kRBin1) of the global numbering
constexpr int kRChunk0 = 6, kRChunk1 = 7;
static_assert(kRChunk1 + 1 == kBiRefWords, "RefAcc");
// the int32 arrays of BaiArgs::ints, n_rec + 1 entries each
enum { kIRid, kIBeg, kIEnd, kIBinFlag, kIChunkFlag, kIBinIdx, kIChunkIdx, kIChunkJ, kIBinJ, kIBinC, kIChunkBin, kINum };
static_assert(kINum == kBiIntArrays, "the index's int32 scratch");
constexpr uint32_t kUntouched = 0xffffffffu;

__device__ __forceinline__ int32_t *ints_of(const BaiArgs &a, int which) { return a.ints + (size_t)which * ((size_t)a.n_rec + 1); }

__global__ __launch_bounds__(256) void bai_extent_kernel(const BaiArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    int32_t rid = -1, beg = INT32_MAX, end = INT32_MAX;     // (a rejected record takes no part in what follows)
    uint32_t bin = 0;
    bool ok = false;
    const int64_t o0 = a.off[i], o1 = a.off[i + 1];
    if (span_ok(o0, o1) && (i > 0 || o0 == 0)) {
        const uint8_t *blk = a.bam + o0;
        const Fixed f = read_fixed(blk);
        if (block_ok(f, o1 - o0, a.n_ref) && cigar_ok(f)) {
            const int64_t v = a.voff[i];
            ok = v >= 0 && v <= a.end_voff && (i == 0 || a.voff[i - 1] <= v);
            beg = f.pos;
            if (f.ref_id >= 0) {
                const int64_t e = record_end(blk, f);
                if (f.pos < 0 || e > a.ref_len[f.ref_id]) {
                    ok = false;
                } else {
                    rid = f.ref_id;
                    end = (int32_t)e;
                    bin = reg2bin(beg, e);
                    if (f.flag & 4) atomicAdd(&a.ref[(size_t)rid * kBiRefWords + kRUnmapped], 1u);
                }
            }
        }
    }
    if (!ok) a.meta[kBiErr] = 1;
    ints_of(a, kIRid)[i] = rid;
    ints_of(a, kIBeg)[i] = beg;
    ints_of(a, kIEnd)[i] = end;
    a.key[i] = bin_key(rid, bin, a.n_ref);
    a.val[i] = i;
}

__global__ __launch_bounds__(256) void bai_window_kernel(const BaiArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const int32_t *rids = ints_of(a, kIRid), *begs = ints_of(a, kIBeg), *ends = ints_of(a, kIEnd);
    const int32_t rid = rids[i], beg = begs[i];
    const int32_t prid = i > 0 ? rids[i - 1] : 0, pbeg = i > 0 ? begs[i - 1] : -1;
    // (a rejected record has set the error word already: its INT32_MAX takes no part in the comparison)
    if (i > 0 && beg != INT32_MAX && pbeg != INT32_MAX && !order_ok(prid, pbeg, rid, beg, a.n_ref)) a.meta[kBiErr] = 1;
    if (rid < 0) {
        if (i == 0 || prid >= 0) a.meta[kBiNoCoor] = a.n_rec - i;
        return;
    }
    uint32_t *ref = a.ref + (size_t)rid * kBiRefWords;
    const bool has_prev = i > 0 && prid == rid;
    if (!has_prev) ref[kRFirst1] = (uint32_t)i + 1;
    if (i + 1 == a.n_rec || rids[i + 1] != rid) ref[kRLast1] = (uint32_t)i + 1;
    const int w0 = beg >> kLinShift, w1 = (ends[i] - 1) >> kLinShift;
    const int pw0 = has_prev ? pbeg >> kLinShift : 1, pw1 = has_prev ? (ends[i - 1] - 1) >> kLinShift : 0;
    uint32_t *lin = a.lin + a.win_off[rid];
    for (int w = w0; w <= w1; ++w)
        if (w < pw0 || w > pw1) atomicMin(&lin[w], (uint32_t)i);
    if (pw1 < w1 || pw0 > pw1) atomicMax(&ref[kRLastWin1], (uint32_t)w1 + 1);
}

__global__ __launch_bounds__(256) void bai_fill_kernel(const BaiArgs a)
{
    __shared__ uint32_t s[256];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int n = (int)a.ref[(size_t)r * kBiRefWords + kRLastWin1];
    uint32_t *lin = a.lin + a.win_off[r];
    uint32_t carry = kUntouched;
    for (int base = n > 0 ? (n - 1) / 256 * 256 : -1; base >= 0; base -= 256) {
        const int w = base + lane;
        s[lane] = w < n ? lin[w] : kUntouched;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t t = lane + d < 256 ? s[lane + d] : kUntouched;
            __syncthreads();
            if (t < s[lane]) s[lane] = t;
            __syncthreads();
        }
        const uint32_t v = s[lane] < carry ? s[lane] : carry;
        if (w < n) lin[w] = v;
        if (s[0] < carry) carry = s[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void bai_flag_kernel(const BaiArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > a.n_rec) return;
    int bf = 0, cf = 0;
    if (j < a.n_rec) {
        const uint64_t k = a.key2[j];
        if ((int64_t)(k >> 16) < a.n_ref) {
            bf = j == 0 || a.key2[j - 1] != k;
            cf = bf || chunk_head(a.voff[a.val2[j]], vend(a.voff, a.val2[j - 1], a.n_rec, a.end_voff));
        }
    }
    ints_of(a, kIBinFlag)[j] = bf;
    ints_of(a, kIChunkFlag)[j] = cf;
}

__global__ __launch_bounds__(256) void bai_compact_kernel(const BaiArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n_rec) return;
    const uint64_t k = a.key2[j];
    const int64_t rid = (int64_t)(k >> 16);
    if (rid >= a.n_ref) return;
    const int b = ints_of(a, kIBinIdx)[j + 1] - 1, c = ints_of(a, kIChunkIdx)[j + 1] - 1;
    if (ints_of(a, kIChunkFlag)[j]) {
        ints_of(a, kIChunkJ)[c] = j;
        ints_of(a, kIChunkBin)[c] = b;
    }
    if (ints_of(a, kIBinFlag)[j]) {
        ints_of(a, kIBinJ)[b] = j;
        ints_of(a, kIBinC)[b] = c;
    }
    uint32_t *ref = a.ref + (size_t)rid * kBiRefWords;
    if (j == 0 || (int64_t)(a.key2[j - 1] >> 16) != rid) { ref[kRBin0] = (uint32_t)b; ref[kRChunk0] = (uint32_t)c; }
    if (j + 1 == a.n_rec || (int64_t)(a.key2[j + 1] >> 16) != rid) { ref[kRBin1] = (uint32_t)b + 1; ref[kRChunk1] = (uint32_t)c + 1; }
}

__global__ __launch_bounds__(256) void bai_size_kernel(const BaiArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > a.n_ref) return;
    int64_t size = 0;
    if (r < a.n_ref) {
        const uint32_t *ref = a.ref + (size_t)r * kBiRefWords;
        const bool has = ref[kRFirst1] != 0;
        size = ref_bytes(has ? (int64_t)ref[kRBin1] - ref[kRBin0] : 0, has ? (int64_t)ref[kRChunk1] - ref[kRChunk0] : 0, has,
                         ref[kRLastWin1]);
        if (ref[kRLastWin1]) atomicAdd((unsigned long long *)(a.meta + kBiIntv), (unsigned long long)ref[kRLastWin1]);
    }
    a.ref_size[r] = size;
    if (r == 0) {
        a.meta[kBiBins] = a.n_rec > 0 ? ints_of(a, kIBinIdx)[a.n_rec] : 0;
        a.meta[kBiChunks] = a.n_rec > 0 ? ints_of(a, kIChunkIdx)[a.n_rec] : 0;
    }
}

// one workgroup per reference: n_bin, the pseudo-bin, n_intv, the linear index; the file's head and tail
__global__ __launch_bounds__(256) void bai_ref_kernel(const BaiArgs a)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const uint32_t *ref = a.ref + (size_t)r * kBiRefWords;
    const bool has = ref[kRFirst1] != 0;
    const int64_t nb = has ? (int64_t)ref[kRBin1] - ref[kRBin0] : 0, nc = has ? (int64_t)ref[kRChunk1] - ref[kRChunk0] : 0;
    const int n_intv = (int)ref[kRLastWin1];
    const int64_t base = kBaiHead + a.ref_off[r];
    int64_t at = base + 4 + 8 * nb + 16 * nc;
    if (lane == 0) {
        if (r == 0) {
            put32(a.bai, 0, 0x01494142u);           // `BAI\1`
            put32(a.bai, 4, (uint32_t)a.n_ref);
            put64(a.bai, kBaiHead + a.ref_off[a.n_ref], (uint64_t)(uint32_t)a.meta[kBiNoCoor]);
        }
        put32(a.bai, base, (uint32_t)(nb + (has ? 1 : 0)));
        if (has) {
            const int32_t first = (int32_t)ref[kRFirst1] - 1, last = (int32_t)ref[kRLast1] - 1;
            put32(a.bai, at, kPseudoBin);
            put32(a.bai, at + 4, 2);
            put64(a.bai, at + 8, (uint64_t)a.voff[first]);
            put64(a.bai, at + 16, (uint64_t)vend(a.voff, last, a.n_rec, a.end_voff));
            put64(a.bai, at + 24, (uint64_t)(last - first + 1) - ref[kRUnmapped]);
            put64(a.bai, at + 32, ref[kRUnmapped]);
        }
    }
    at += has ? kPseudoBytes : 0;
    if (lane == 0) put32(a.bai, at, (uint32_t)n_intv);
    const uint32_t *lin = a.lin + a.win_off[r];
    for (int w = lane; w < n_intv; w += 256) put64(a.bai, at + 4 + 8 * (int64_t)w, (uint64_t)a.voff[lin[w]]);
}

// where bin b of the global numbering lies in the file
__device__ __forceinline__ int64_t bai_bin_at(const BaiArgs &a, int b)
{
    const uint64_t rid = a.key2[ints_of(a, kIBinJ)[b]] >> 16;
    const uint32_t *ref = a.ref + (size_t)rid * kBiRefWords;
    return kBaiHead + a.ref_off[rid] + 4 + 8 * ((int64_t)b - ref[kRBin0]) + 16 * ((int64_t)ints_of(a, kIBinC)[b] - ref[kRChunk0]);
}

// lane j: bin j of the global numbering, and chunk j
__global__ __launch_bounds__(256) void bai_bin_kernel(const BaiArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int n_bins = ints_of(a, kIBinIdx)[a.n_rec], n_chunks = ints_of(a, kIChunkIdx)[a.n_rec];
    const int32_t *bin_c = ints_of(a, kIBinC), *chunk_j = ints_of(a, kIChunkJ);
    if (j < n_bins) {
        const int64_t at = bai_bin_at(a, j);
        put32(a.bai, at, (uint32_t)(a.key2[ints_of(a, kIBinJ)[j]] & 0xffff));
        put32(a.bai, at + 4, (uint32_t)((j + 1 < n_bins ? bin_c[j + 1] : n_chunks) - bin_c[j]));
    }
    if (j < n_chunks) {
        const int b = ints_of(a, kIChunkBin)[j];
        const int64_t at = bai_bin_at(a, b) + 8 + 16 * (int64_t)(j - bin_c[b]);
        const int n_placed = a.n_rec - a.meta[kBiNoCoor];
        const int j0 = chunk_j[j], j1 = j + 1 < n_chunks ? chunk_j[j + 1] : n_placed;
        put64(a.bai, at, (uint64_t)a.voff[a.val2[j0]]);
        put64(a.bai, at + 8, (uint64_t)vend(a.voff, a.val2[j1 - 1], a.n_rec, a.end_voff));
    }
}

// bits of the (refID, bin) key: 16 of the bin, then what holds n_ref
static int bin_key_bits(int32_t n_ref)
{
    int bits = 16;
    while (bits < 63 && ((uint64_t)n_ref >> (bits - 16)) != 0) ++bits;
    return bits;
}

hipError_t bai_tmp_bytes(int32_t n_rec, int32_t n_ref, size_t *bytes)
{
    size_t b32 = 0, b64 = 0, bs = 0;
    if (hipError_t e = launch_scan32(nullptr, &b32, nullptr, nullptr, n_rec, nullptr)) return e;
    if (hipError_t e = launch_scan64(nullptr, &b64, nullptr, nullptr, n_ref, nullptr)) return e;
    if (n_rec > 0)
        if (hipError_t e = launch_bamsort_pairs(nullptr, &bs, nullptr, nullptr, nullptr, nullptr, n_rec, 0, bin_key_bits(n_ref), nullptr))
            return e;
    *bytes = std::max(std::max(b32, b64), std::max<size_t>(bs, 16));
    return hipSuccess;
}

#define BAI_TRY(x) do { if (hipError_t _e = (x)) return _e; } while (0)

hipError_t launch_bai_plan(const BaiArgs &a, hipStream_t s)
{
    const int n = a.n_rec;
    size_t tb = a.tmp_bytes;
    BAI_TRY(hipMemsetAsync(a.ref, 0, (size_t)a.n_ref * kBiRefWords * sizeof(uint32_t), s));
    if (a.n_win > 0) BAI_TRY(hipMemsetAsync(a.lin, 0xff, (size_t)a.n_win * sizeof(uint32_t), s));
    if (n > 0) {
        hipLaunchKernelGGL(bai_extent_kernel, grid_for(n, 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bai_window_kernel, grid_for(n, 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bai_fill_kernel, dim3(a.n_ref), dim3(256), 0, s, a);
        BAI_TRY(hipGetLastError());
        BAI_TRY(launch_bamsort_pairs(a.tmp, &tb, a.key, a.key2, a.val, a.val2, n, 0, bin_key_bits(a.n_ref), s));
        hipLaunchKernelGGL(bai_flag_kernel, grid_for((int64_t)n + 1, 256), dim3(256), 0, s, a);
        BAI_TRY(hipGetLastError());
        int32_t *ints = a.ints;
        const size_t stride = (size_t)n + 1;
        tb = a.tmp_bytes;
        BAI_TRY(launch_scan32(a.tmp, &tb, ints + kIBinFlag * stride, ints + kIBinIdx * stride, n, s));
        tb = a.tmp_bytes;
        BAI_TRY(launch_scan32(a.tmp, &tb, ints + kIChunkFlag * stride, ints + kIChunkIdx * stride, n, s));
        hipLaunchKernelGGL(bai_compact_kernel, grid_for(n, 256), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(bai_size_kernel, grid_for((int64_t)a.n_ref + 1, 256), dim3(256), 0, s, a);
    BAI_TRY(hipGetLastError());
    tb = a.tmp_bytes;
    return launch_scan64(a.tmp, &tb, a.ref_size, a.ref_off, a.n_ref, s);
}

hipError_t launch_bai_write(const BaiArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(bai_ref_kernel, dim3(a.n_ref), dim3(256), 0, s, a);
    if (a.n_rec > 0) hipLaunchKernelGGL(bai_bin_kernel, grid_for(a.n_rec, 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace bsw
