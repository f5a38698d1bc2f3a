// bsw_bamsort_k.h -- everything per record of the BAM sort and the .bai (include/bsw_bamsort.h): the field reads, the
// block checks, the sort key, rlen over the CIGAR words, reg2bin, the chunk-head test, the index's byte layout.  Every
// function here compiles for the host and for the device: bsw_bamsort.hip runs them one lane per record,
// tools/bamsort_model.cpp runs the same functions serially.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BAMSORT_HD __host__ __device__ inline
#else
#define BAMSORT_HD inline
#endif

namespace bsw {
namespace bamsort {

constexpr int kFixedBytes = 36;                     // block_size and the 32 fixed bytes behind it
constexpr int kMinBlockSize = 32;                   // a block_size below it holds no fixed fields
constexpr int kLinShift = 14;                       // 16,384-base windows
constexpr int kMaxRefLen = 1 << 29;
constexpr uint32_t kPseudoBin = 37450;
constexpr int kPseudoBytes = 8 + 2 * 16;            // bin, n_chunk, two chunks
constexpr int kPermTile = 8192;                     // bytes of d_out that one workgroup of the permute kernel owns
constexpr int kPermSlice = 256;                     // records that can start in or reach into one tile, at most
static_assert(kPermTile / kFixedBytes + 2 <= kPermSlice, "the tile's slice of d_out_off fits the LDS arrays");

// blocks start on any byte
BAMSORT_HD uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
BAMSORT_HD uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

struct Fixed {                                      // what the sort and the index read of a block
    int32_t block_size, ref_id, pos;
    uint32_t l_read_name, n_cigar, flag;
};
BAMSORT_HD Fixed read_fixed(const uint8_t *blk)
{
    Fixed f;
    f.block_size = (int32_t)ld32(blk);
    f.ref_id = (int32_t)ld32(blk + 4);
    f.pos = (int32_t)ld32(blk + 8);
    f.l_read_name = blk[12];
    f.n_cigar = ld16(blk + 16);
    f.flag = ld16(blk + 18);
    return f;
}
// the offsets' part of the block check: a block has room for its fixed bytes (so that read_fixed may run)
BAMSORT_HD bool span_ok(int64_t beg, int64_t end) { return beg >= 0 && end - beg >= kFixedBytes; }
// the fields' part: what the sort rejects in a block of `len` bytes
BAMSORT_HD bool block_ok(const Fixed &f, int64_t len, int32_t n_ref)
{
    return f.block_size >= kMinBlockSize && (int64_t)f.block_size == len - 4 && f.ref_id >= -1 && f.ref_id < n_ref &&
           f.pos >= -1;
}
// the CIGAR words lie inside the block (the index reads them)
BAMSORT_HD bool cigar_ok(const Fixed &f) { return 32 + (int64_t)f.l_read_name + 4 * (int64_t)f.n_cigar <= f.block_size; }

// (refID < 0 ? n_ref : refID, pos + 1, flag & 0x10) in one word: bit 0 the strand, bits 1..32 pos + 1, the rest the rid
BAMSORT_HD uint64_t sort_key(const Fixed &f, int32_t n_ref)
{
    const uint64_t rid = (uint64_t)(f.ref_id < 0 ? n_ref : f.ref_id);
    return rid << 33 | (uint64_t)((int64_t)f.pos + 1) << 1 | ((f.flag >> 4) & 1u);
}
// the radix sort's span: the bits [lo, hi) that are set in some key and clear in another (or_ / nor_: the OR of the
// keys and of their complements); hi == lo: no bit varies
BAMSORT_HD void key_span(uint64_t or_, uint64_t nor_, int *lo, int *hi)
{
    const uint64_t v = or_ & nor_;
    *lo = *hi = 0;
    if (!v) return;
    while (!(v >> *lo & 1)) ++*lo;
    *hi = 64;
    while (!(v >> (*hi - 1) & 1)) --*hi;
}

// the reference bases the CIGAR words cover: M 0, D 2, N 3, = 7, X 8
BAMSORT_HD int64_t cigar_rlen(const uint8_t *cigar, uint32_t n_cigar)
{
    int64_t rlen = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t w = ld32(cigar + 4 * k);
        if ((0x18du >> (w & 15)) & 1) rlen += w >> 4;
    }
    return rlen;
}
// [pos, end) of a block whose checks passed
BAMSORT_HD int64_t record_end(const uint8_t *blk, const Fixed &f)
{
    const int64_t rlen = f.n_cigar ? cigar_rlen(blk + kFixedBytes + f.l_read_name, f.n_cigar) : 0;
    return (int64_t)f.pos + (rlen > 0 ? rlen : 1);
}
// the UCSC binning scheme over [beg, end): 14-bit smallest bin, 5 levels
BAMSORT_HD uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
// the (refID, bin) key of the index's second sort; records with no refID take n_ref and go last
BAMSORT_HD uint64_t bin_key(int32_t ref_id, uint32_t bin, int32_t n_ref)
{
    return (uint64_t)(ref_id < 0 ? n_ref : ref_id) << 16 | (ref_id < 0 ? 0u : bin);
}
// the order of the sort between a record and its predecessor: (rid, pos), refID < 0 last
BAMSORT_HD bool order_ok(int32_t prev_ref, int32_t prev_pos, int32_t ref_id, int32_t pos, int32_t n_ref)
{
    const int32_t a = prev_ref < 0 ? n_ref : prev_ref, b = ref_id < 0 ? n_ref : ref_id;
    return a < b || (a == b && prev_pos <= pos);
}
// vend(i): the virtual offset behind record i
BAMSORT_HD int64_t vend(const int64_t *voff, int32_t i, int32_t n_rec, int64_t end_voff)
{
    return i + 1 < n_rec ? voff[i + 1] : end_voff;
}
// a member of a bin whose predecessor in the bin ends at prev_vend starts a new chunk
BAMSORT_HD bool chunk_head(int64_t voff_i, int64_t prev_vend) { return (voff_i >> 16) > (prev_vend >> 16); }

// ---------------------------------------------------------------- the file's layout (every offset a multiple of 4)
constexpr int kBaiHead = 8;                         // magic, n_ref
BAMSORT_HD int64_t ref_bytes(int64_t n_bins, int64_t n_chunks, bool has_records, int64_t n_intv)
{
    return 4 + 8 * n_bins + 16 * n_chunks + (has_records ? kPseudoBytes : 0) + 4 + 8 * n_intv;
}
BAMSORT_HD void put32(uint8_t *bai, int64_t at, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint32_t *)(bai + at) = v;                    // (d_bai and every offset are 4-byte aligned)
#else
    for (int k = 0; k < 4; ++k) bai[at + k] = (uint8_t)(v >> (8 * k));
#endif
}
BAMSORT_HD void put64(uint8_t *bai, int64_t at, uint64_t v)
{
    put32(bai, at, (uint32_t)v);
    put32(bai, at + 4, (uint32_t)(v >> 32));
}

}  // namespace bamsort

#if defined(__HIPCC__)
// ---------------------------------------------------------------- launch interface (bsw_bamsort.hip)
// meta words of the sort (one int32 array, zeroed per call): the error word, then the OR of the keys and of their
// complements as two 64-bit words
constexpr int kBsErr = 0, kBsOr = 2, kBsNor = 4, kBsMetaWords = 8;
// meta words of the index: the error word, bins, chunks, n_no_coor; two 64-bit words: the file's bytes, the
// linear-index entries
constexpr int kBiErr = 0, kBiBins = 1, kBiChunks = 2, kBiNoCoor = 3, kBiBytes = 4, kBiIntv = 6, kBiMetaWords = 8;
constexpr int kBiRefWords = 8;                      // per reference: the uint32 words of RefAcc
constexpr int kBiIntArrays = 11;                    // int32 arrays of n_rec + 1 entries in the index's scratch

// key[i], val[i] = i and the block checks (meta[kBsErr]); the keys' OR / complement OR into meta
hipError_t launch_bamsort_keys(const uint8_t *bam, const int64_t *off, int32_t n_rec, int32_t n_ref, uint64_t *key,
                               int32_t *val, int32_t *meta, hipStream_t s);
// the radix sort of (key, val) over the key bits [lo, hi), stable; tmp == nullptr only sizes *tmp_bytes
hipError_t launch_bamsort_pairs(void *tmp, size_t *tmp_bytes, const uint64_t *key_in, uint64_t *key_out, const int32_t *val_in,
                                int32_t *val_out, int32_t n, int lo, int hi, hipStream_t s);
// len[i] = off[perm[i] + 1] - off[perm[i]], len[n_rec] = 0
hipError_t launch_bamsort_lens(const int64_t *off, const int32_t *perm, int32_t n_rec, int64_t *len, hipStream_t s);
// out[out_off[i], out_off[i + 1]) = bam[off[perm[i]], ...): out 4-byte aligned, no byte at or behind out + n_bytes;
// tile_rec: scratch of bamsort_tiles(n_bytes) entries
static inline int64_t bamsort_tiles(int64_t n_bytes) { return (n_bytes + bamsort::kPermTile - 1) / bamsort::kPermTile; }
hipError_t launch_bamsort_permute(const uint8_t *bam, const int64_t *off, const int32_t *perm, const int64_t *out_off,
                                  int32_t *tile_rec, int32_t n_rec, int64_t n_bytes, uint8_t *out, hipStream_t s);

struct BaiArgs {                        // one index call
    const uint8_t *bam;
    const int64_t *off, *voff;
    int64_t end_voff;
    int32_t n_rec, n_ref;
    const int32_t *ref_len;             // [n_ref], device
    const int64_t *win_off;             // [n_ref + 1]: the references' first entries in lin
    int64_t n_win;
    uint32_t *lin;                      // [n_win] the flat linear index: the smallest record index per window
    uint32_t *ref;                      // [n_ref * kBiRefWords]
    int64_t *ref_size, *ref_off;        // [n_ref + 1]
    uint64_t *key, *key2;               // [n_rec]
    int32_t *val, *val2;                // [n_rec]
    int32_t *ints;                      // kBiIntArrays arrays of n_rec + 1
    int32_t *meta;
    void *tmp;                          // scans and the sort
    size_t tmp_bytes;
    uint8_t *bai;
};
// scratch of the scans and the sort of an index call over n_rec records
hipError_t bai_tmp_bytes(int32_t n_rec, int32_t n_ref, size_t *bytes);
// extents, windows, fill, bins, chunks, sizes: everything up to the byte count (meta, ref_off[n_ref])
hipError_t launch_bai_plan(const BaiArgs &a, hipStream_t s);
// the file into a.bai
hipError_t launch_bai_write(const BaiArgs &a, hipStream_t s);
#endif

}  // namespace bsw
