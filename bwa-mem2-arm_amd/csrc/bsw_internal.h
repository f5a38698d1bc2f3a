// bsw_internal.h -- engine hooks shared by the C ABI translation units (not installed).
#pragma once
#include "../../include/bsw.h"
#include "../../include/bsw_ext.h"
#include <cstdint>
#include <vector>
#include "bsw_contig_seg.h"

namespace bsw {
// bsw_get_scores with a per-call end_bonus (LEFT uses pen_clip5, RIGHT pen_clip3) and the
// call's stats returned instead of stored.
int scores_eb(bsw_ctx_t *ctx, int32_t end_bonus, SeqPair *pairs, const uint8_t *ref,
              const uint8_t *qer, int32_t n, int32_t w, int cell_bits, bsw_stats_t *st);
void ctx_params(const bsw_ctx_t *ctx, bsw_params_t *out);
int ctx_device(const bsw_ctx_t *ctx);          // HIP device of the context's first device slot pool
int64_t ctx_refres_len(bsw_ctx_t *ctx);        // length of the resident reference (-1: none)
// Per-context pinned host staging buffer `which` (0, 1) of at least `bytes`: DMA-speed H2D for
// the extension pipeline's code buffers.  Returns nullptr when another call holds it (the
// caller then uses pageable memory); release with pinned_release.
void *pinned_acquire(bsw_ctx_t *ctx, int which, size_t bytes);
void pinned_release(bsw_ctx_t *ctx, int which);
void set_ext_stats(bsw_ctx_t *ctx, const bsw_ext_stats_t &s);
int64_t ext_chunk_cap(const bsw_ctx_t *ctx);   // reads per extension chunk (BSW_OPT_EXT_CHUNK)
int get_ext_stats(bsw_ctx_t *ctx, bsw_ext_stats_t *out);
void set_chain_stats(bsw_ctx_t *ctx, const bsw_chain_stats_t &s);
int get_chain_stats(bsw_ctx_t *ctx, bsw_chain_stats_t *out);
// bsw_ext_opt_t / seed checks shared by the host and device extension forms (bsw_ext.cpp)
int ext_opt_check(const bsw_ext_opt_t *opt, int64_t ref_len);
bool ext_seed_ok(const bsw_ext_opt_t *opt, const ContigView &cv, const bsw_seed_t &s, int32_t l, int64_t ref_len);
// The context's contig table (bsw_set_contigs) for an extension call that names l_pac over a reference of
// ref_len bases: BSW_E_INVAL when one is set and does not sum to l_pac (l_pac == 0: to ref_len).  *dev = the
// view with device pointers (off null: no table); *host_off = a copy of the prefix sums (empty: no table).
// Either may be null.
int ctx_contigs(bsw_ctx_t *ctx, int64_t l_pac, int64_t ref_len, ContigView *dev, std::vector<int64_t> *host_off);
// bsw_extend_seeds_device with each job's target window given (d_win[2j], d_win[2j + 1]: the
// chain's window, mem_chain2aln) or computed per seed (d_win == nullptr)
int extend_seeds_device_win(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads,
                            const int64_t *d_read_off, const int32_t *d_read_len, const bsw_seed_t *d_seeds,
                            const int64_t *d_win, int32_t n, bsw_alnreg_t *d_out, void *stream);
// mem_chain2aln rounds with every per-read decision on the GPU (bsw_chain.hip): inputs and
// outputs device-resident on the context's first device
int chain_rounds_device(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads, const int64_t *d_read_off,
                        const int32_t *d_read_len, int32_t n_reads, const bsw_seed_t *d_seeds,
                        const int32_t *d_sr, const int32_t *d_sc, int32_t ns, bsw_alnreg_t *d_out, int32_t *d_ext,
                        bsw_chain_stats_t *cs);
// staging packers (bsw_pack.cpp): nibbles (dst[k] = src[2k] & 15 | (src[2k+1] & 15) << 4) and
// 2-bit codes (src[k] & 3) + one exception word (pos0 + k) << 2 | (src[k] >> 2 & 3) per byte
// outside 0..3, ascending (the staging kernels patch code bits 2-3 from them, bsw_pipeline.hip)
void pack_nibbles(uint8_t *dst, const uint8_t *src, size_t nbytes);
void pack_2bit(uint8_t *dst, const uint8_t *src, size_t nbytes, uint32_t pos0, std::vector<uint32_t> &exc);
// a record bsw_get_scores / bsw_pack_batch accept (else BSW_E_RANGE)
inline bool pair_valid(const SeqPair &p)
{
    return p.len1 >= 0 && p.len2 >= 0 && p.len1 <= BSW_MAX_LEN && p.len2 <= BSW_MAX_LEN && p.idr >= 0 && p.idq >= 0;
}
// a += b over the pair and launch counters of two calls' stats (the *_ms fields are the caller's:
// summed along one device's chunks, maxed over devices)
inline void add_counters(bsw_stats_t &a, const bsw_stats_t &b)
{
    a.n_i16 += b.n_i16; a.n_u8 += b.n_u8; a.n_wide += b.n_wide; a.n_packed += b.n_packed;
    a.n_launches += b.n_launches; a.n_wave += b.n_wave; a.n_group += b.n_group;
}
// Layout of a staged blob (the host-array forms of the stages, bsw_stages.cpp): parts end to end
// in the order added, each starting on a 16-byte boundary; a part of 0 bytes takes no room
struct BlobLayout {
    size_t total = 0;                   // bytes laid out so far = the next part's offset
    size_t add(size_t bytes)            // -> the part's offset
    {
        const size_t at = total;
        total += (bytes + 15) & ~(size_t)15;
        return at;
    }
};
}  // namespace bsw
