// bsw_markdup.hip -- duplicate marking on the records of bsw_records* (include/bsw_markdup.h).
//   md_score_kernel      the bandwidth path: kMdScoreGroup lanes per read sum its quals through aligned dwords with head
//                        and tail masks, reduced over the group by shuffles
//   md_end_kernel        one lane per read: the input checks, the candidate test, the end word (rid, u, s); the pair
//                        candidates from the neighbour lane
//   (scans of the candidate flags)
//   md_key_kernel        one lane per read: the compact end keys, per even read the pair's key words; the OR of the key
//                        words and of their complements over the wave, then an atomic per wave and word
//   md_pack_kernel       the varying bits of a key's words in one 64-bit word (the one-pass route)
//   md_gather_kernel     the next word of the key in the order so far (the multi-pass route)
//   (hipCUB radix sorts of (key, index): stable)
//   md_head_kernel       a sorted member starts a set when a key word differs from its predecessor's
//   md_pair_mark_kernel  pairs that are not their set's head
//   md_hpos_kernel, md_end_mark_kernel   every end's set head, behind a scan of the head flags; a fragment's mark
//   md_mark_kernel       one lane per record and per read: the only writer of d_recs and d_dup
// Everything per read and per pair is bsw_markdup_k.h, shared with the serial model tools/markdup_model.cpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "bsw_markdup_k.h"
#include "bsw_stage_k.h"

#ifndef BSW_MD_SCORE_GROUP
#define BSW_MD_SCORE_GROUP kMdScoreGroup
#endif

namespace bsw {

using namespace markdup;

template <int G>
__global__ __launch_bounds__(256) void md_score_kernel(const MdArgs a)
{
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a group is a power of two of lanes inside one wave");
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t / G;
    const int sub = (int)(t % G);
    int64_t sum = 0;
    bool bad = false;
    if (r < a.n_reads) {
        const int64_t off = a.read_off[r], len = a.read_len[r];
        if (!extent_ok(off, len, a.quals_len)) bad = true;
        else sum = score_span(a.quals, a.quals_len, off, off + len, a.min_qual, sub, G);
    }
    uint32_t lo = (uint32_t)sum, hi = (uint32_t)((uint64_t)sum >> 32);   // (a lane's share stays below 2^32 * 94)
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const uint64_t other = (uint64_t)(uint32_t)__shfl_xor((int)hi, o) << 32 | (uint32_t)__shfl_xor((int)lo, o);
        const uint64_t s = ((uint64_t)hi << 32 | lo) + other;
        lo = (uint32_t)s;
        hi = (uint32_t)(s >> 32);
    }
    if (sub == 0 && r < a.n_reads) {
        a.score[r] = bad ? 0 : score_clamp((int64_t)((uint64_t)hi << 32 | lo));
        if (bad) a.meta[kMdErr] = 1;
    }
}

__global__ __launch_bounds__(256) void md_end_kernel(const MdArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool ok = true, cand = false;
    uint64_t e = 0;
    if (i < a.n_reads) {
        const int32_t f0 = a.rec_first[i], f1 = a.rec_first[i + 1];
        if (f0 < 0 || f1 < f0 || f1 > a.n_rec || (i == 0 && f0 != 0) || (i == a.n_reads - 1 && f1 != a.n_rec)) {
            ok = false;
        } else {
            for (int32_t k = f0; k < f1; ++k) {
                const int32_t rd = a.recs[k].read, al = a.recs[k].aln;
                if (rd != i || al < -1 || al >= a.n_aln) ok = false;
            }
            // (a read without a record has no first record: f0 may be n_rec, and d_recs NULL when n_rec is 0)
            if (ok && f1 > f0 && candidate(a.recs[f0].flag)) {
                const int64_t pos = a.recs[f0].pos;
                const int32_t al = a.recs[f0].aln, is_rev = a.recs[f0].is_rev;
                const int32_t nc = al >= 0 ? a.aln[al].n_cigar : 0;
                if (al < 0 || pos < 0 || pos >= a.l_pac || nc <= 0 || nc > a.cigar_stride) {
                    ok = false;
                } else {
                    const int64_t u = unclipped5(pos, is_rev, a.cigar + (int64_t)al * a.cigar_stride, nc);
                    if (!u_ok(u)) {
                        ok = false;
                    } else {
                        e = end_word(a.ctg.off ? contig_rid(a.ctg, pos) : 0, u, is_rev);
                        cand = true;
                    }
                }
            }
        }
        if (!ok) a.meta[kMdErr] = 1;
        a.cflag[i] = cand;
        a.eword[i] = e;
    } else if (i == a.n_reads) {
        a.cflag[i] = 0;
        a.pflag[a.n_pairs] = 0;
    }
    // reads 2p and 2p + 1 sit in neighbouring lanes of one wave
    const int mate = __shfl_xor((int)cand, 1);
    if (a.paired && i < a.n_reads && !(i & 1)) a.pflag[i >> 1] = cand && mate;
}

// w[q] |= over the wave, then one atomic per word that still has a bit to add
template <int N>
__device__ __forceinline__ void wave_or_into(uint32_t (&w)[N], uint32_t *dst)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < N; ++q) w[q] |= (uint32_t)__shfl_xor((int)w[q], o);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (w[q] & ~((volatile uint32_t *)dst)[q]) atomicOr(dst + q, w[q]);
    }
}

__global__ __launch_bounds__(256) void md_key_kernel(const MdArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint64_t ek[2] = {0, 0}, pk[3] = {0, 0, 0};
    bool is_end = false, is_pair = false;
    if (i < a.n_reads && a.cflag[i]) {
        is_end = true;
        const bool in_pair = a.paired && a.pflag[i >> 1];
        const int32_t c = a.cidx[i];
        ek[0] = a.eword[i];
        ek[1] = end_rank(!in_pair, (uint32_t)a.score[i]);
        a.cid[c] = i;
        a.ekey[0][c] = ek[0];
        a.ekey[1][c] = ek[1];
        if (in_pair && !(i & 1)) {
            is_pair = true;
            const int32_t p = i >> 1, c2 = a.pidx[p];
            const uint64_t x = ek[0], y = a.eword[i + 1];
            pk[0] = x < y ? x : y;
            pk[1] = x < y ? y : x;
            pk[2] = score_field((uint32_t)a.score[i] + (uint32_t)a.score[i + 1]);
            a.pid[c2] = p;
#pragma unroll
            for (int q = 0; q < 3; ++q) a.pkey[q][c2] = pk[q];
        }
    }
    // [0, 6) the pair words' OR, [6, 12) their complements' -- kMdOrPair .. kMdNorPair + 6 are contiguous; the ends' likewise
    uint32_t w[12], v[8];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        w[2 * q] = is_pair ? (uint32_t)pk[q] : 0u;
        w[2 * q + 1] = is_pair ? (uint32_t)(pk[q] >> 32) : 0u;
        w[6 + 2 * q] = is_pair ? ~(uint32_t)pk[q] : 0u;
        w[6 + 2 * q + 1] = is_pair ? ~(uint32_t)(pk[q] >> 32) : 0u;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        v[2 * q] = is_end ? (uint32_t)ek[q] : 0u;
        v[2 * q + 1] = is_end ? (uint32_t)(ek[q] >> 32) : 0u;
        v[4 + 2 * q] = is_end ? ~(uint32_t)ek[q] : 0u;
        v[4 + 2 * q + 1] = is_end ? ~(uint32_t)(ek[q] >> 32) : 0u;
    }
    static_assert(kMdNorPair == kMdOrPair + 6 && kMdOrEnd == kMdNorPair + 6, "the pair words of meta");
    static_assert(kMdNorEnd == kMdOrEnd + 6 && kMdNorEnd + 6 <= kMdCounterStride, "the end words of meta");
    wave_or_into(w, (uint32_t *)a.meta + kMdOrPair);
    uint32_t vo[4] = {v[0], v[1], v[2], v[3]}, vn[4] = {v[4], v[5], v[6], v[7]};
    wave_or_into(vo, (uint32_t *)a.meta + kMdOrEnd);
    wave_or_into(vn, (uint32_t *)a.meta + kMdNorEnd);
}

__global__ __launch_bounds__(256) void md_pack_kernel(const MdWords k, int32_t n, uint64_t *__restrict__ out,
                                                      int32_t *__restrict__ val)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    uint64_t key = 0;
    for (int q = 0; q < k.n; ++q) {
        const int bits = bit_count(k.mask[q]);
        if (bits == 0) continue;
        key = (bits < 64 ? key << bits : 0) | pack_bits(k.w[q][j], k.mask[q]);
    }
    out[j] = key;
    val[j] = j;
}

__global__ __launch_bounds__(256) void md_gather_kernel(const uint64_t *__restrict__ word, const int32_t *__restrict__ val,
                                                        int32_t n, uint64_t *__restrict__ out, int32_t *__restrict__ iota)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    out[j] = word[val ? val[j] : j];
    if (!val) iota[j] = j;
}

__global__ __launch_bounds__(256) void md_head_kernel(const MdWords k, const int32_t *__restrict__ perm, int32_t n,
                                                      int32_t *__restrict__ hflag)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    int head = 0;
    if (j < n) {
        head = j == 0;
        if (j > 0) {
            const int32_t c = perm[j], b = perm[j - 1];
            for (int q = 0; q < k.n; ++q) head |= k.w[q][c] != k.w[q][b];
        }
    }
    hflag[j] = head;
}

// the marking kernels count into meta: a lane's count is summed over its wave and lane 0 adds it, each counter on a cache
// line of its own (kMdCounterStride); with at most kMdMarkBlocks workgroups striding over the members that is a few
// thousand atomics per counter, where one per wave of a 2M-record batch serialised on one line for 2 ms
__device__ __forceinline__ void wave_add_into(int v, int32_t *dst)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

__global__ __launch_bounds__(256) void md_pair_mark_kernel(const MdArgs a, const int32_t *__restrict__ perm, int32_t n)
{
    int dups = 0, sets = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int j = (int)base + threadIdx.x;
        if (j >= n) continue;
        if (!a.hflag[j]) {
            const int32_t p = a.pid[perm[j]];
            a.dupr[2 * p] = a.dupr[2 * p + 1] = (uint8_t)kDupPair;
            ++dups;
        } else if (j + 1 < n && !a.hflag[j + 1]) {
            ++sets;
        }
    }
    wave_add_into(dups, a.meta + kMdDupPairs);
    wave_add_into(sets, a.meta + kMdPairSets);
}

__global__ __launch_bounds__(256) void md_hpos_kernel(const MdArgs a, int32_t n)
{
    int sets = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int j = (int)base + threadIdx.x;
        if (j >= n || !a.hflag[j]) continue;
        a.hpos[a.hidx[j]] = j;
        sets += j + 1 < n && !a.hflag[j + 1];
    }
    wave_add_into(sets, a.meta + kMdEndSets);
}

__global__ __launch_bounds__(256) void md_end_mark_kernel(const MdArgs a, const int32_t *__restrict__ perm, int32_t n)
{
    int by_pair = 0, by_frag = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int j = (int)base + threadIdx.x;
        if (j >= n) continue;
        const int32_t c = perm[j];
        if (!(a.ekey[1][c] >> 32)) continue;            // a pair's end: md_pair_mark_kernel decides
        const int32_t h = a.hpos[a.hidx[j + 1] - 1];    // the set's head: the best pair end, or the best fragment
        const bool head_is_pair = !(a.ekey[1][perm[h]] >> 32);
        const int d = head_is_pair ? kDupFragByPair : j != h ? kDupFrag : 0;
        if (d) a.dupr[a.cid[c]] = (uint8_t)d;
        by_pair += d == kDupFragByPair;
        by_frag += d == kDupFrag;
    }
    wave_add_into(by_pair, a.meta + kMdDupFragByPair);
    wave_add_into(by_frag, a.meta + kMdDupFrag);
}

__global__ __launch_bounds__(256) void md_mark_kernel(const MdArgs a)
{
    const int32_t n = a.n_rec > a.n_reads ? a.n_rec : a.n_reads;
    int flagged = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int i = (int)base + threadIdx.x;
        if (i < a.n_reads) a.dup[i] = a.dupr[i];
        if (i < a.n_rec) {
            bsw_rec_t *r = a.recs + i;
            const int32_t f = r->flag;
            const int d = a.dupr[r->read];
            const int32_t nf = marked_flag(f, f, d);
            r->flag = nf;
            r->sam_flag = marked_flag(r->sam_flag, f, d);
            flagged += (nf & 0x400) != 0;
        }
    }
    wave_add_into(flagged, a.meta + kMdFlagged);
}

static inline dim3 mark_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, kMdMarkBlocks)); }

hipError_t launch_md_scores(const MdArgs &a, hipStream_t s)
{
    if (!a.quals) return hipMemsetAsync(a.score, 0, (size_t)a.n_reads * sizeof(int32_t), s);
    hipLaunchKernelGGL(md_score_kernel<BSW_MD_SCORE_GROUP>, grid_for((int64_t)a.n_reads * BSW_MD_SCORE_GROUP, 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_md_ends(const MdArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(md_end_kernel, grid_for((int64_t)a.n_reads + 1, 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_md_keys(const MdArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(md_key_kernel, grid_for(a.n_reads, 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_md_pack(const MdWords &k, int32_t n, uint64_t *out, int32_t *val, hipStream_t s)
{
    hipLaunchKernelGGL(md_pack_kernel, grid_for(n, 256), dim3(256), 0, s, k, n, out, val);
    return hipGetLastError();
}

hipError_t launch_md_gather(const uint64_t *word, const int32_t *val, int32_t n, uint64_t *out, int32_t *iota, hipStream_t s)
{
    hipLaunchKernelGGL(md_gather_kernel, grid_for(n, 256), dim3(256), 0, s, word, val, n, out, iota);
    return hipGetLastError();
}

hipError_t launch_md_heads(const MdWords &k, const int32_t *perm, int32_t n, int32_t *hflag, hipStream_t s)
{
    hipLaunchKernelGGL(md_head_kernel, grid_for((int64_t)n + 1, 256), dim3(256), 0, s, k, perm, n, hflag);
    return hipGetLastError();
}

hipError_t launch_md_pair_marks(const MdArgs &a, const int32_t *perm, int32_t n_pc, hipStream_t s)
{
    hipLaunchKernelGGL(md_pair_mark_kernel, mark_grid(n_pc), dim3(256), 0, s, a, perm, n_pc);
    return hipGetLastError();
}

hipError_t launch_md_end_marks(const MdArgs &a, const int32_t *perm, int32_t n_cand, hipStream_t s)
{
    hipLaunchKernelGGL(md_hpos_kernel, mark_grid(n_cand), dim3(256), 0, s, a, n_cand);
    hipLaunchKernelGGL(md_end_mark_kernel, mark_grid(n_cand), dim3(256), 0, s, a, perm, n_cand);
    return hipGetLastError();
}

hipError_t launch_md_mark(const MdArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(md_mark_kernel, mark_grid(a.n_rec > a.n_reads ? a.n_rec : a.n_reads), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace bsw
