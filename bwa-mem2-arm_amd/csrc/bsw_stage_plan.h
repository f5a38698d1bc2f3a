// bsw_stage_plan.h -- the planning of a host-buffer call (bsw_pipeline.hip), host-only and free of
// HIP headers so that g++ and the sanitizer driver (tools/asan) compile it: per-block extents, the
// staging mode of a chunk, THE byte layout of a staged chunk (every buffer that is sized or
// addressed by it -- pinned, device, coalesced batch and the bsw_pack_batch wire form -- calls
// stage_layout) and the chunk schedule of a call.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/bsw_seqpair.h"

namespace bsw {

constexpr int32_t kStageBlk = 4096;         // pairs per staging block (a chunk is whole blocks)
constexpr size_t kPairInBytes = 20;         // sizeof(PairIn), bsw_kernels.h: the five input fields
constexpr size_t kOutBytes = 24;            // the six outputs of a pair (SeqPair bytes 32..55)

// Per-block extents of the byte buffers (the pre-pass of a host-buffer call), from which chunks are
// cut and staged without another pass over the records
struct BlkStat {
    int64_t r_lo, r_hi, q_lo, q_hi, r_sum, q_sum;
    bool bad;
};

// blocks [0, nb) as one: their common extents (none: [0, 0)) and byte sums
inline BlkStat merge_blocks(const BlkStat *b, int32_t nb)
{
    BlkStat t{INT64_MAX, 0, INT64_MAX, 0, 0, 0, false};
    for (int32_t k = 0; k < nb; ++k) {
        t.r_lo = std::min(t.r_lo, b[k].r_lo); t.r_hi = std::max(t.r_hi, b[k].r_hi); t.r_sum += b[k].r_sum;
        t.q_lo = std::min(t.q_lo, b[k].q_lo); t.q_hi = std::max(t.q_hi, b[k].q_hi); t.q_sum += b[k].q_sum;
    }
    if (t.r_lo == INT64_MAX) t.r_lo = t.r_hi = 0;
    if (t.q_lo == INT64_MAX) t.q_lo = t.q_hi = 0;
    return t;
}
// staged in bulk (the whole extents, packed) when they hold little besides the pairs' own bytes;
// else gathered pair by pair
inline bool bulk_extents(const BlkStat &t)
{
    return (t.r_hi - t.r_lo) <= t.r_sum + t.r_sum / 4 + 4096 && (t.q_hi - t.q_lo) <= t.q_sum + t.q_sum / 4 + 4096;
}

// How a chunk is staged.  Contiguous chunks (the upstream layout: each batch's windows
// concatenated in pair order) pack their byte extents into 2-bit codes + exception words, with the
// records cut to their five input fields (20 of 56 B) and only the 24 output bytes coming back --
// or into nibbles with whole records when 2-bit staging is off or the chunk holds too many
// non-ACGT bytes; scattered ones are gathered pair by pair as bytes.
enum StageMode { kStageGather = 0, kStageNibble = 1, kStage2bit = 2 };

// the mode merged blocks `t` are staged in first (a 2-bit chunk with too many exceptions falls
// back to nibbles) and the ref / qer bytes they unpack to: exception positions have 30 bits
inline StageMode stage_mode(const BlkStat &t, bool two_bit, size_t *rb, size_t *qb)
{
    const bool bulk = bulk_extents(t);
    *rb = (size_t)(bulk ? t.r_hi - t.r_lo : t.r_sum);
    *qb = (size_t)(bulk ? t.q_hi - t.q_lo : t.q_sum);
    if (!bulk) return kStageGather;
    return two_bit && *rb < ((size_t)1 << 30) && *qb < ((size_t)1 << 30) ? kStage2bit : kStageNibble;
}

// 2-bit staging is given up past this many exception words (1/32 of the bytes)
inline size_t exc_cap(size_t rb, size_t qb) { return (rb + qb) / 32 + 1024; }

// the exceptions' bucket table (exc_bucket_kernel): one entry per 4096 positions and one past the
// end, ref buckets [0, nbr) then qer buckets [nbr, nbr + nbq)
struct ExcBuckets {
    int64_t nbr, nbq;
    size_t total() const { return (size_t)(nbr + nbq); }
};
inline ExcBuckets exc_buckets(int64_t rb, int64_t qb) { return ExcBuckets{(rb + 4095) / 4096 + 1, (qb + 4095) / 4096 + 1}; }

inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// One staged chunk: [records x n | ref codes + 4 | qer codes + 4 | exception words], every part
// 256-aligned.  Records are PairIn (2-bit) or SeqPair; codes are 4, 2 or 1 per byte (2-bit, nibble,
// gathered); the 4 zero bytes after each code part serve the kernels' aligned dword loads; only
// the 2-bit form has exception words.  The two end rules differ because the first is ABI:
//   wire_bytes = a256(exc_off + 4 n_exc)                  bsw_pack_batch's total_bytes
//   bytes      = max(exc_off + 4 n_exc, 24 n)  (2-bit)    staging: the outputs come back through it
//              = qer_off + qer_len + 4         (others)   (whole records come back in place)
struct StageLayout {
    size_t pair_off = 0, ref_off = 0, qer_off = 0, exc_off = 0;
    size_t ref_len = 0, qer_len = 0;    // staged code bytes (without the 4 pad bytes)
    size_t bytes = 0, wire_bytes = 0;
};
inline StageLayout stage_layout(int mode, size_t n, size_t rb, size_t qb, size_t n_exc)
{
    const size_t per = mode == kStage2bit ? 4 : mode == kStageNibble ? 2 : 1;
    StageLayout l;
    l.ref_len = (rb + per - 1) / per;
    l.qer_len = (qb + per - 1) / per;
    l.ref_off = a256(n * (mode == kStage2bit ? kPairInBytes : sizeof(SeqPair)));
    l.qer_off = a256(l.ref_off + l.ref_len + 4);
    l.exc_off = a256(l.qer_off + l.qer_len + 4);
    l.wire_bytes = a256(l.exc_off + 4 * n_exc);
    l.bytes = mode == kStage2bit ? std::max(l.exc_off + 4 * n_exc, n * kOutBytes) : l.qer_off + l.qer_len + 4;
    return l;
}

// the six outputs of a pair from their 24 staged bytes
inline void put_outputs(SeqPair &p, const int32_t *o)
{
    p.score = o[0]; p.tle = o[1]; p.gtle = o[2]; p.qle = o[3]; p.gscore = o[4]; p.max_off = o[5];
}

// The chunk schedule of a call: blocks [b, b + nb) per chunk.
// The first chunk is first_min blocks (64K pairs at 16) or 1/32 of the call, at most `chunk` pairs;
// a call of up to 32 blocks within `chunk` is one chunk.  The same size decides whether the call
// runs as several chunks.
struct ChunkRange { int32_t b, nb; };
inline int32_t first_chunk_blocks(int32_t nblk, int32_t chunk, int32_t first_min)
{
    return std::min(std::max<int32_t>(1, chunk / kStageBlk), nblk <= 32 ? nblk : std::max<int32_t>(first_min, nblk / 32));
}
// Chunks double from first_blk blocks up to `chunk` pairs, fewer when their sequence bytes pass
// 512 MB (staged offsets stay int32), never less than one block.  (A small remainder stays its own
// chunk: folded into the last full chunk it added a third, nearly empty generation of waves to
// that launch -- 262144 pairs are exactly two generations at two waves per SIMD -- and the call got
// ~1 ms slower; as its own launch it runs beside the last chunk on another queue.  Measured,
// DESIGN.md §6.)
inline std::vector<ChunkRange> chunk_schedule(const std::vector<BlkStat> &bs, int32_t chunk, int32_t first_blk)
{
    std::vector<ChunkRange> chs;
    const int32_t nblk = (int32_t)bs.size(), cap_blk = std::max<int32_t>(1, chunk / kStageBlk);
    for (int32_t b = 0, nb = 0, cur = first_blk; b < nblk; b += nb, cur = std::min(cap_blk, cur * 2)) {
        int64_t bytes = 0;
        for (nb = 0; nb < cur && b + nb < nblk; ++nb) {
            const int64_t x = bs[b + nb].r_sum + bs[b + nb].q_sum;
            if (nb > 0 && bytes + x > ((int64_t)1 << 29)) break;
            bytes += x;
        }
        chs.push_back(ChunkRange{b, nb});
    }
    return chs;
}
// pairs of chunk `c` of a call of n pairs
inline int32_t chunk_pairs(const ChunkRange &c, int32_t n) { return std::min(n, (c.b + c.nb) * kStageBlk) - c.b * kStageBlk; }

}  // namespace bsw
