// bsw_sort.h -- the batch-order sort (bsw_sort.hip) and the key mask that feeds it.
//
// The planning kernels OR every key, and every key's complement, into two words per d_meta slot
// (words kMetaKeyOr / kMetaKeyNor of the class-count lines, zeroed with them).  A bit varies over the
// batch iff it is set in both ORs; the sort takes its digits from the varying bits alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bsw_engine.h"

namespace bsw {

constexpr int kMetaKeyOr = kMetaCounts - 2;     // per slot: OR of the keys, OR of their complements
constexpr int kMetaKeyNor = kMetaCounts - 1;
constexpr int kSortTile = 4096;                 // keys per workgroup of the count and scatter kernels
constexpr int kSortThreads = 1024;
constexpr int kSortScanChunk = 256;             // table entries per iteration of a scan workgroup

// tiles of n keys
static inline int32_t sort_tiles(int32_t n) { return (int32_t)(((int64_t)n + kSortTile - 1) / kSortTile); }

#ifdef __HIPCC__
// OR over the wave's 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// One key per thread (valid = the thread holds one) into the block's slot of `meta` (a d_meta-shaped
// array of kMetaSpread lines of kMetaCounts words), in three steps a kernel places around its own two
// barriers: s_or (two LDS words) zeroed before the first, the waves' ORs added between them, one
// atomicOr per block and word after the second.
__device__ __forceinline__ void key_mask_zero(uint32_t *s_or)
{
    if (threadIdx.x < 2) s_or[threadIdx.x] = 0;
}
__device__ __forceinline__ void key_mask_add(uint32_t key, bool valid, uint32_t *s_or)
{
    const uint32_t a = wave_or(valid ? key : 0u), b = wave_or(valid ? ~key : 0u);
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&s_or[0], a);
        atomicOr(&s_or[1], b);
    }
}
__device__ __forceinline__ void key_mask_flush(const uint32_t *s_or, int32_t *meta)
{
    if (threadIdx.x < 2 && s_or[threadIdx.x])
        atomicOr(reinterpret_cast<uint32_t *>(meta) + (blockIdx.x % kMetaSpread) * kMetaCounts + kMetaKeyOr +
                     threadIdx.x,
                 s_or[threadIdx.x]);
}
#endif

// Stable sort of the slot's (d_keys, d_vals) by the low key_bits bits -> d_order on `st`; d_keys2 is
// free afterwards.  d_mask: a d_meta-shaped array holding the key mask (above), or null: every bit
// below key_bits counts as varying.  run = false only grows d_tmp.  Nothing waits on the host.
BSW_HIDDEN hipError_t sort_order(Slot &s, int32_t n, int key_bits, hipStream_t st, bool run = true,
                                 const int32_t *d_mask = nullptr);

}  // namespace bsw
