// bsw_markdup_k.h -- everything per read and per pair of the duplicate marking (include/bsw_markdup.h): the candidate
// test, the clip and rlen walk, the unclipped 5' coordinate, the key words, the score of a dword of quals, the packing
// of the varying key bits, the winner rule.  Every function here compiles for the host and for the device:
// bsw_markdup.hip runs them one lane per read / pair / record, tools/markdup_model.cpp runs the same functions serially.
#pragma once
#include <stdint.h>
#include "../../include/bsw_rec.h"
#include "bsw_contig_seg.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MARKDUP_HD __host__ __device__ inline
#else
#define MARKDUP_HD inline
#endif

namespace bsw {
namespace markdup {

constexpr int kDupPair = 1, kDupFrag = 2, kDupFragByPair = 3;
constexpr int64_t kMaxLPac = (int64_t)1 << 39;
constexpr int32_t kMaxContigs = (1 << 23) - 1;
// the end word: rid (23 bits) | u + kUBias (40 bits) | s (1 bit).  A clip is below 2^31 and pos below 2^39, so
// u + kUBias lies in [0, 2^40) and the words compare as the tuples (rid, u, s) do
constexpr int64_t kUBias = (int64_t)1 << 31;
constexpr int kUShift = 1, kRidShift = 41;
constexpr int32_t kScoreMax = INT32_MAX;            // a read's score saturates here

// the first record of a read decides: it is mapped (a read without a record is no candidate, and has no first record
// to read: the caller tests that first)
MARKDUP_HD bool candidate(int32_t first_flag) { return !(first_flag & 4); }

MARKDUP_HD bool is_clip(uint32_t w) { return (w & 15) == 3 || (w & 15) == 4; }
// rlen: the sum of the M (0) and D (2) lengths
MARKDUP_HD int64_t cigar_rlen(const uint32_t *cigar, int32_t n_cigar)
{
    int64_t rlen = 0;
    for (int32_t k = 0; k < n_cigar; ++k) {
        const uint32_t op = cigar[k] & 15;
        if (op == 0 || op == 2) rlen += cigar[k] >> 4;
    }
    return rlen;
}
// u of an end at pos on strand is_rev (n_cigar >= 1)
MARKDUP_HD int64_t unclipped5(int64_t pos, int32_t is_rev, const uint32_t *cigar, int32_t n_cigar)
{
    if (!is_rev) return pos - (is_clip(cigar[0]) ? (int64_t)(cigar[0] >> 4) : 0);
    const uint32_t last = cigar[n_cigar - 1];
    return pos + cigar_rlen(cigar, n_cigar) - 1 + (is_clip(last) ? (int64_t)(last >> 4) : 0);
}
// u fits the end word's 40 bits: pos is below 2^39, so only a CIGAR whose rlen plus clip passes 2^31 can fail this
MARKDUP_HD bool u_ok(int64_t u) { return u >= -kUBias && u < ((int64_t)1 << 40) - kUBias; }
// a read's quals [off, off + len) lie inside quals_len bytes (stated without the sum, which can wrap)
MARKDUP_HD bool extent_ok(int64_t off, int64_t len, int64_t quals_len) { return off >= 0 && len >= 0 && off <= quals_len && len <= quals_len - off; }
MARKDUP_HD uint64_t end_word(int32_t rid, int64_t u, int32_t is_rev)
{
    return (uint64_t)rid << kRidShift | (uint64_t)(u + kUBias) << kUShift | (is_rev ? 1u : 0u);
}

// (q - 33 >= min_qual ? q - 33 : 0) summed over the bytes k of dword w whose bit k of `keep` is set
MARKDUP_HD int32_t score_dword(uint32_t w, uint32_t keep, int32_t min_qual)
{
    int32_t sum = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int32_t v = (int32_t)((w >> (8 * k)) & 0xff) - 33;
        sum += ((keep >> k) & 1) && v >= min_qual ? v : 0;
    }
    return sum;
}
MARKDUP_HD int32_t score_clamp(int64_t sum) { return sum > kScoreMax ? kScoreMax : (int32_t)sum; }
// the bytes [beg, end) of quals (quals_len bytes) through aligned dwords with head and tail masks, dwords first,
// first + step, ... of the read's span (a group of `step` lanes shares a read; the serial model runs first = 0,
// step = 1).  A dword that reaches outside the array is read by its kept bytes
MARKDUP_HD int64_t score_span(const uint8_t *quals, int64_t quals_len, int64_t beg, int64_t end, int32_t min_qual, int first,
                              int step)
{
    const uintptr_t q0 = (uintptr_t)quals, q1 = q0 + (uint64_t)quals_len, b = q0 + (uint64_t)beg, e = q0 + (uint64_t)end;
    int64_t sum = 0;
    for (uintptr_t a = (b & ~(uintptr_t)3) + 4 * (uintptr_t)first; a < e; a += 4 * (uintptr_t)step) {
        uint32_t keep = 0xf;
        if (a < b) keep &= 0xfu << (b - a);
        if (a + 4 > e) keep &= 0xfu >> (a + 4 - e);
        uint32_t w = 0;
        if (a >= q0 && a + 4 <= q1) {
            w = *(const uint32_t *)a;
        } else {
            for (int k = 0; k < 4; ++k)
                if ((keep >> k) & 1) w |= (uint32_t)*(const uint8_t *)(a + k) << (8 * k);
        }
        sum += score_dword(w, keep, min_qual);
    }
    return sum;
}

// the sort's least significant field: a higher score sorts first
MARKDUP_HD uint64_t score_field(uint32_t score) { return (uint64_t)(uint32_t)~score; }
// the end sort's second word: pair ends ahead of fragments, fragments by complemented score
MARKDUP_HD uint64_t end_rank(bool is_frag, uint32_t score) { return is_frag ? (uint64_t)1 << 32 | score_field(score) : 0; }
// the winner rule as a comparison (the sort states it through score_field and its stability): a before b
MARKDUP_HD bool wins(uint32_t score_a, int32_t idx_a, uint32_t score_b, int32_t idx_b)
{
    return score_a > score_b || (score_a == score_b && idx_a < idx_b);
}

// the bits of w that `mask` selects, moved together (keys that agree outside mask keep their order)
MARKDUP_HD uint64_t pack_bits(uint64_t w, uint64_t mask)
{
    uint64_t out = 0;
    int at = 0;
    while (mask) {
        const uint64_t low = mask & (~mask + 1);
        if (w & low) out |= (uint64_t)1 << at;
        ++at;
        mask ^= low;
    }
    return out;
}
MARKDUP_HD int bit_count(uint64_t v)
{
    int n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
}
// the span [lo, hi) of a mask of varying bits; hi == lo: none
MARKDUP_HD void mask_span(uint64_t v, int *lo, int *hi)
{
    *lo = *hi = 0;
    if (!v) return;
    while (!(v >> *lo & 1)) ++*lo;
    *hi = 64;
    while (!(v >> (*hi - 1) & 1)) --*hi;
}

// 0x400 on a record of a read whose mark is `dup`: set on a mapped record of a duplicate, cleared otherwise
MARKDUP_HD int32_t marked_flag(int32_t flag, int32_t rec_flag, int dup)
{
    return dup && !(rec_flag & 4) ? flag | 0x400 : flag & ~0x400;
}

}  // namespace markdup

#if defined(__HIPCC__)
// ---------------------------------------------------------------- launch interface (bsw_markdup.hip)
constexpr int kMdMaxWords = 3;                      // 64-bit words of a sort key, most significant first
// meta words (one int32 array, zeroed per call): the error word, then per sort the OR of the key words and of their
// complements (kMdMaxWords 64-bit words each); behind them the counters, one per 128-byte line
constexpr int kMdErr = 0, kMdOrPair = 2, kMdNorPair = 8, kMdOrEnd = 14, kMdNorEnd = 20;
constexpr int kMdCounterStride = 32;
constexpr int kMdDupPairs = 1 * kMdCounterStride, kMdDupFrag = 2 * kMdCounterStride, kMdDupFragByPair = 3 * kMdCounterStride,
              kMdPairSets = 4 * kMdCounterStride, kMdEndSets = 5 * kMdCounterStride, kMdFlagged = 6 * kMdCounterStride,
              kMdMetaWords = 7 * kMdCounterStride;
constexpr int kMdMarkBlocks = 1024;                 // workgroups of a marking kernel, at most: they stride over the members
constexpr int kMdScoreGroup = 8;                    // lanes per read of the score kernel

struct MdWords {                        // the words of a sort key, most significant first, and their varying bits
    const uint64_t *w[kMdMaxWords];
    uint64_t mask[kMdMaxWords];
    int n;
};

struct MdArgs {                         // one call
    bsw_rec_t *recs;
    const int32_t *rec_first;
    const bsw_aln_t *aln;
    const uint32_t *cigar;
    const int64_t *read_off;
    const int32_t *read_len;
    const uint8_t *quals;               // nullptr: every score is 0
    int64_t quals_len, l_pac;
    int32_t n_rec, n_aln, n_reads, n_pairs, cigar_stride, paired, min_qual;
    ContigView ctg;
    uint8_t *dup;                       // [n_reads] the caller's
    // scratch
    int32_t *score;                     // [n_reads]
    uint64_t *eword;                    // [n_reads] the end words of the candidates
    int32_t *cflag, *cidx;              // [n_reads + 1] candidate flags and their scan
    int32_t *pflag, *pidx;              // [n_pairs + 1] pair candidates likewise
    int32_t *pid, *cid;                 // [n_pairs], [n_reads]: the pair / read of a compact index
    uint64_t *pkey[kMdMaxWords];        // [n_pairs] each: lo end, hi end, score field
    uint64_t *ekey[2];                  // [n_reads] each: end word, end_rank
    int32_t *hflag, *hidx, *hpos;       // [n_reads + 1]: set heads of a sorted list, their scan, the heads' positions
    uint8_t *dupr;                      // [n_reads] the marks before the mark kernel publishes them
    int32_t *meta;
};
// scores (zero without quals)
hipError_t launch_md_scores(const MdArgs &a, hipStream_t s);
// checks, candidates and end words; cflag / pflag (their entry n is zeroed)
hipError_t launch_md_ends(const MdArgs &a, hipStream_t s);
// behind the scans of cflag / pflag: the compact key words, pid / cid, and the words' OR / NOR into meta
hipError_t launch_md_keys(const MdArgs &a, hipStream_t s);
// out[j] = the words' masked bits packed into one word, most significant word first; val[j] = j
hipError_t launch_md_pack(const MdWords &k, int32_t n, uint64_t *out, int32_t *val, hipStream_t s);
// out[j] = word[val[j]];  val == nullptr: out[j] = word[j] and iota[j] = j
hipError_t launch_md_gather(const uint64_t *word, const int32_t *val, int32_t n, uint64_t *out, int32_t *iota, hipStream_t s);
// hflag[j] = the sorted member j starts a set: one of the k.n words differs from its predecessor's (hflag[n] = 0)
hipError_t launch_md_heads(const MdWords &k, const int32_t *perm, int32_t n, int32_t *hflag, hipStream_t s);
// behind the scan of hflag: pairs that are not their set's head into dupr; the sets with more than one member
hipError_t launch_md_pair_marks(const MdArgs &a, const int32_t *perm, int32_t n_pc, hipStream_t s);
// the same for the ends: hpos, then every fragment's mark from its set's head
hipError_t launch_md_end_marks(const MdArgs &a, const int32_t *perm, int32_t n_cand, hipStream_t s);
// the only writer of recs and dup
hipError_t launch_md_mark(const MdArgs &a, hipStream_t s);
#endif

}  // namespace bsw
