// bsw_bgzf.hip -- BGZF on the GPU (include/bsw_bgzf.h): a byte stream in HBM -> whole BGZF blocks.
//   bgzf_deflate_kernel  one workgroup of 256 lanes per block of <= 0xff00 input bytes, a fixed grid looping
//                        over the blocks: tables -> tokens (lane s: strip s) -> code lengths (one lane) -> the
//                        smallest of stored / fixed / dynamic into the block's 64 KB of staging, its size out
//   bgzf_voff_kernel     the records' virtual offsets from the scanned block starts
//   bgzf_pack_kernel     staging -> the contiguous stream (dword copies behind a funnel shift; the EOF marker)
// Everything per strip and per block is bsw_bgzf_k.h, shared with the serial model tools/bgzf_model.cpp.
// LDS per workgroup: 32 KB seg_last + 8 KB first + 1 KB CRC table + the block's Tables (about 10 KB); the
// input stays in HBM / L2 (a 64 KB chunk beside these tables is more than the 64 KB a workgroup gets here).
#include <hip/hip_runtime.h>
#include "bsw_bgzf_k.h"

namespace bsw {

using namespace bgzf;

__global__ __launch_bounds__(256) void bgzf_deflate_kernel(const uint8_t *__restrict__ in, int64_t n_in, int32_t block_bytes,
                                                           int32_t n_blocks, int32_t level, uint8_t *__restrict__ stage,
                                                           uint16_t *__restrict__ tok_all, int64_t *__restrict__ bsize,
                                                           int32_t *__restrict__ meta)
{
    __shared__ uint32_t seg_words[kNSeg * kSegBuckets / 2];
    __shared__ uint32_t first[kFirstBuckets];
    __shared__ uint32_t crc_tab[256];
    __shared__ Tables T;
    uint16_t *seg_last = (uint16_t *)seg_words;
    const int lane = threadIdx.x;
    crc_tab[lane] = crc_table_entry((uint32_t)lane);
    uint16_t *tok = tok_all + (size_t)blockIdx.x * kTokPerBlock + lane;     // unit k of strip `lane` at tok[k * 256]
    if (blockIdx.x == 0 && lane == 0) bsize[n_blocks] = 0;
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int64_t at = (int64_t)b * block_bytes;
        const uint8_t *src = in + at;
        const int n = (int)(n_in - at < block_bytes ? n_in - at : block_bytes);
        uint8_t *out = stage + (size_t)b * kStageStride;
        const int s0 = lane * kStrip < n ? lane * kStrip : n;
        const int s1 = s0 + kStrip < n ? s0 + kStrip : n;
        __syncthreads();                                // the block before is done with the tables
        for (int i = lane; i < kNSeg * kSegBuckets; i += 256) tables_clear(seg_last, first, i);
        for (int i = lane; i < kNLL; i += 256) tables_clear_hist(T, i);
        if (lane == 0) { T.m_ll = 0; T.m_d = 0; T.crc = 0; }
        __syncthreads();
        int k = 0;
        uint32_t fb = 0;
        if (level != 0) {
            for (int p = lane; p + 3 <= n; p += 256) table_insert(src, n, p, seg_last, first);
            for (int p = lane; p < n; p += 256) hist_add(&T.hbyte[src[p]]);
            __syncthreads();
            T.cost[lane] = T.hbyte[lane] ? (uint8_t)lit_cost8((uint32_t)n, T.hbyte[lane]) : 0;
            __syncthreads();
            k = tokenise_strip(src, n, s0, s1, seg_last, first, T.cost, tok, 256, T.hll, T.hd, &fb);
        }
        T.bits_fix[lane] = fb;
        if (s1 > s0) atomicXor(&T.crc, crc_share(crc_bytes(crc_tab, src + s0, s1 - s0), (uint32_t)(n - s1)));
        __syncthreads();
        uint32_t db = 0;
        if (level != 0) {
            for (int s = lane; s < kLLUsed; s += 256) {
                const uint32_t r = sym_rank(T.hll, kLLUsed, s);
                if (r != kNone) { T.sorted_ll[r] = (uint16_t)s; atomicAdd(&T.m_ll, 1u); }
            }
            if (lane < kNDUsed) {
                const uint32_t r = sym_rank(T.hd, kNDUsed, lane);
                if (r != kNone) { T.sorted_d[r] = (uint16_t)lane; atomicAdd(&T.m_d, 1u); }
            }
            __syncthreads();
            if (lane == 0) plan_codes(T);
            __syncthreads();
            db = strip_bits(T, tok, 256, k);
        }
        T.bits_dyn[lane] = db;
        __syncthreads();
        if (lane == 0) plan_block(T, n, level, out);
        __syncthreads();
        if (T.form == kStored) {
            for (int i = lane; i < n; i += 256) out[kHdrBytes + 5 + i] = src[i];
        } else if (s1 > s0) {
            strip_write(T, tok, 256, k, lane == (n - 1) / kStrip, out, kHdrBytes, T.bits_dyn[lane]);
        }
        if (lane == 0) {
            bsize[b] = block_trailer(T, n, out);
            atomicAdd(&meta[kBgzfStored + T.form], 1);
        }
    }
}

__global__ __launch_bounds__(256) void bgzf_voff_kernel(const int64_t *__restrict__ rec_off, int32_t n_rec, int64_t n_in,
                                                        int32_t block_bytes, const int64_t *__restrict__ blk_off,
                                                        int64_t base, int64_t *__restrict__ voff, int32_t *__restrict__ meta)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rec) return;
    const int64_t r = rec_off[i];
    if (r < 0 || r > n_in) { meta[kBgzfErr] = 1; return; }
    const int64_t b = r / block_bytes;                  // (r == n_in on a cut: the end, blk_off[n_blocks])
    voff[i] = (int64_t)(((uint64_t)(base + blk_off[b]) << 16) | (uint64_t)(r - b * block_bytes));
}

__constant__ uint8_t kEofMarker[kEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0,
                                              0, 0, 0, 0, 0, 0, 0, 0};

// block b of the staging to out + blk_off[b]; the workgroup behind the last block writes the EOF marker.
// Block starts fall on any byte: the bytes up to the first aligned dword and behind the last whole one are
// byte stores (the dwords they lie in belong to the neighbours as well), the rest are dwords put together from
// two of the staging's.  -DBSW_BGZF_PACK_BYTES: byte stores throughout (the A/B of DESIGN.md §4.23)
__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint8_t *__restrict__ stage, const int64_t *__restrict__ blk_off,
                                                        int32_t n_blocks, uint8_t *__restrict__ out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t o = blk_off[b];
    if (b == n_blocks) {
        if (lane < kEofBytes) out[o + lane] = kEofMarker[lane];
        return;
    }
    const int sz = (int)(blk_off[b + 1] - o);
    const uint8_t *src = stage + (size_t)b * kStageStride;
#ifdef BSW_BGZF_PACK_BYTES
    for (int i = lane; i < sz; i += 256) out[o + i] = src[i];
#else
    int head = (int)((4 - (o & 3)) & 3);
    head = head < sz ? head : sz;
    const int nd = (sz - head) >> 2, sh = 8 * head;
    if (lane < head) out[o + lane] = src[lane];
    const uint32_t *s32 = (const uint32_t *)src;        // (the staging's blocks start on 64 KB)
    uint32_t *d32 = (uint32_t *)(out + o + head);
    for (int j = lane; j < nd; j += 256)                // source bytes [head + 4 j, + 4): dword j and, shifted, j + 1
        d32[j] = sh ? (s32[j] >> sh) | (s32[j + 1] << (32 - sh)) : s32[j];
    const int tail = head + 4 * nd;
    if (tail + lane < sz) out[o + tail + lane] = src[tail + lane];
#endif
}

hipError_t launch_bgzf_deflate(const uint8_t *in, int64_t n_in, int32_t block_bytes, int32_t n_blocks, int32_t level,
                               uint8_t *stage, uint16_t *tok, int32_t grid, int64_t *bsize, int32_t *meta, hipStream_t s)
{
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(grid), dim3(256), 0, s, in, n_in, block_bytes, n_blocks, level, stage, tok,
                       bsize, meta);
    return hipGetLastError();
}

hipError_t launch_bgzf_voff(const int64_t *rec_off, int32_t n_rec, int64_t n_in, int32_t block_bytes, const int64_t *blk_off,
                            int64_t base, int64_t *voff, int32_t *meta, hipStream_t s)
{
    if (n_rec <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_voff_kernel, dim3((n_rec + 255) / 256), dim3(256), 0, s, rec_off, n_rec, n_in, block_bytes, blk_off,
                       base, voff, meta);
    return hipGetLastError();
}

hipError_t launch_bgzf_pack(const uint8_t *stage, const int64_t *blk_off, int32_t n_blocks, bool eof, uint8_t *out,
                            hipStream_t s)
{
    const int grid = n_blocks + (eof ? 1 : 0);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_pack_kernel, dim3(grid), dim3(256), 0, s, stage, blk_off, n_blocks, out);
    return hipGetLastError();
}

}  // namespace bsw
