// bsw_sel.hip -- region selection (include/bsw_sel.h: mem_sort_dedup_patch, mem_mark_primary_se,
// mem_approx_mapq_se) between bsw_chain2aln_resident and bsw_reg2aln_resident, every per-read
// step on the GPU:
//   seed runs         : launch_seed_runs (bsw_stage.hip); a read's work list lives in the flat
//                       work[] at its run's first slot (a read has at most one region per slot)
//   sel_gather_kernel : av in upstream's order (chains in order, each by len * a and index
//                       descending), seedcov, csub, validation
//   sel_step_kernel   : one work item per read -- the re sort, the i / j loop of the dedup; a
//                       patch_reg that passes its cheap tests SUSPENDS the read (one DP job,
//                       compacted by a ballot and one atomic per wave) and the next launch resumes
//                       it with the job's score; a read whose loop ends goes on through the drops,
//                       the score sort, the identical-hit rule, the hash sort, primary marking and
//                       MAPQ (double precision).  Reads with at most one region skip all of it.
//   sel_build_kernel  : 16 lanes per job, the patch's span through dp_job_write (bsw_stage_k.h)
//   sel_emit_kernel   : after the scan of the kept counts, the compact output
// The sorts are klib's ks_introsort (w_introsort of bsw_memchain.hip with a comparator), their
// explicit stack in LDS; they, the hash, marking, MAPQ and the dedup loop itself (sel_dedup,
// sel_dedup_drop) are in bsw_sel_dev.h (bsw_pe.hip marks again, bsw_matesw.hip dedups with patch = 0).
// Plain C++ with vector stores only; no private arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bsw_sel_k.h"
#include "bsw_sel_dev.h"
#include "bsw_stage_k.h"
#include "bsw_wave.h"

namespace bsw {

// A read whose dedup loop has ended (dedup: it ran, n > 1 at its start): steps 4..7, primary
// marking and MAPQ; returns the number kept.
__device__ __forceinline__ int sel_finish(const SelParams &p, int r, SelW *W, int n, bool dedup, int *stk, int32_t *Z, float frac_rep,
                          int32_t *meta)
{
    if (dedup) n = sel_dedup_drop(W, n, stk, meta);
    if (n == 0) return 0;
    sel_mark_mapq(p, r, W, n, stk, Z, frac_rep);
    return n;
}

__global__ __launch_bounds__(64) void sel_gather_kernel(
    const SelParams p, const int32_t *__restrict__ sbeg, const int32_t *__restrict__ send,
    const int32_t *__restrict__ read_len, const bsw_seed_t *__restrict__ seeds, const int32_t *__restrict__ sc,
    const bsw_alnreg_t *__restrict__ regs, const int32_t *__restrict__ ext, const int32_t *__restrict__ csub,
    SelW *__restrict__ work, SelRd *__restrict__ st, int32_t *__restrict__ meta)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    int n = 0, err = 0;
    if (r < p.n_reads && meta[kSelErr] == 0) {              // (bad read ids: the runs are not to be trusted)
        const int32_t b = sbeg[r], e = send[r];
        const int l_query = read_len[r];
        SelW *W = work + b;
        for (int32_t c0 = b; c0 < e;) {
            int32_t c1 = c0;
            const int32_t cid = sc[c0];
            while (c1 < e && sc[c1] == cid) ++c1;
            const int n0 = n;
            for (int32_t i = c0; i < c1; ++i) {
                if (ext[i] == 0) continue;
                SelW x;
                x.r = regs[i];
                if (x.r.qe == x.r.qb) continue;
                if (x.r.qb < 0 || x.r.qe > l_query || x.r.qe < x.r.qb || x.r.rb < 0 || x.r.rb > x.r.re ||
                    x.r.re > p.ref_len) {
                    err = 1;
                    continue;
                }
                int cov = 0;
                for (int32_t k = c0; k < c1; ++k) {
                    const bsw_seed_t t = seeds[k];
                    if (t.qbeg >= x.r.qb && t.qbeg + t.len <= x.r.qe && t.rbeg >= x.r.rb && t.rbeg + t.len <= x.r.re)
                        cov += t.len;
                }
                x.seedcov = cov; x.sub = 0; x.csub = csub ? csub[i] : 0; x.sub_n = 0; x.n_comp = 1;
                x.secondary = -1; x.src = i; x.mapq = 0; x.hash = 0;
                // insert into W[n0 .. n): (len * a, slot) descending
                const int64_t ki = (int64_t)seeds[i].len * p.a;
                int j = n;
                while (j > n0) {
                    const int32_t s = W[j - 1].src;
                    const int64_t kx = (int64_t)seeds[s].len * p.a;
                    if (kx > ki || (kx == ki && s > i)) break;
                    sel_copy(W + j, W + j - 1);
                    --j;
                }
                W[j] = x;
                ++n;
            }
            c0 = c1;
        }
        if (n > BSW_SEL_MAX_PER_READ) err = 1;
        SelRd s;
        s.n = n; s.i = 0; s.j = 0; s.w = 0;
        st[r] = s;
    }
    const int tot = wave_sum(n);
    const unsigned long long be = __ballot(err);
    if ((threadIdx.x & 63) == 0) {
        if (tot) atomicAdd(&meta[kSelRegsIn], tot);
        if (be) atomicOr(&meta[kSelErr], 1);
    }
}

__global__ __launch_bounds__(64) void sel_step_kernel(
    const SelParams p, const int32_t *__restrict__ list, int32_t n_items, const SeqPair *__restrict__ pairs,
    const int32_t *__restrict__ sbeg, const uint8_t *__restrict__ reads, const int64_t *__restrict__ read_off,
    const float *__restrict__ frac_rep, const uint8_t *__restrict__ ref, SelW *__restrict__ work,
    SelRd *__restrict__ st, int32_t *__restrict__ zbuf, int32_t *__restrict__ next, int32_t *__restrict__ next_cnt,
    int32_t *__restrict__ kept, int32_t *__restrict__ meta)
{
    __shared__ int s_stk[kSelStack * 3 * 64];
    __shared__ int8_t s_mat[32];
#pragma unroll
    for (int k = 0; k < 25; ++k)
        if (threadIdx.x == k) s_mat[k] = p.mat[k];
    __syncthreads();
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool susp = false;
    int r = 0, lq = 0, rl = 0;
    if (t < n_items && meta[kSelErr] == 0) {
        r = list ? list[t] : t;
        const SelRd s = st[r];
        SelW *W = work + sbeg[r];
        int *stk = s_stk + threadIdx.x;
        const bool dedup = s.n > 1;
        if (dedup) {
            if (!list) sel_introsort(s.n, W, stk, LtRe());
            susp = sel_dedup(p, r, W, s.n, list ? s.i : 1, list ? s.j : -2, s.w, list != nullptr, list ? pairs[t].score : 0,
                             reads + read_off[r], ref, s_mat, st, meta, lq, rl);
        }
        if (!susp)
            kept[r] = sel_finish(p, r, W, s.n, dedup, stk, zbuf + sbeg[r], frac_rep ? frac_rep[r] : 0.f, meta);
    }
    const unsigned long long b = __ballot(susp);
    const int lane = threadIdx.x & 63;
    const int mq = wave_max(lq), mt = wave_max(rl);
    int base = 0;
    if (lane == 0 && b) {
        base = atomicAdd(next_cnt, __popcll(b));
        atomicMax(&meta[kSelMaxQ], mq);
        atomicMax(&meta[kSelMaxT], mt);
    }
    base = __shfl(base, 0);
    if (susp) next[base + __popcll(b & ((1ull << lane) - 1))] = r;
}

__global__ void sel_build_kernel(const SelParams p, const int32_t *__restrict__ list, int32_t nj,
                                 const int32_t *__restrict__ sbeg, const uint8_t *__restrict__ reads,
                                 const int64_t *__restrict__ read_off, const SelW *__restrict__ work,
                                 const SelRd *__restrict__ st, const uint8_t *__restrict__ ref,
                                 SeqPair *__restrict__ pairs, uint8_t *__restrict__ qbuf, uint8_t *__restrict__ tbuf)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(t >> 4), sub = (int)(t & 15);
    if (j >= nj) return;
    const int rd = list[j];
    const SelRd s = st[rd];
    const SelW *W = work + sbeg[rd];                        // patch_reg(a = W[s.j], b = W[s.i]): a's start to b's end
    dp_job_write(p, j, sub, reads + read_off[rd], W[s.j].r.qb, W[s.i].r.qe, ref, W[s.j].r.rb, W[s.i].r.re, s.w, pairs,
                 qbuf, tbuf);
}

__global__ void sel_emit_kernel(const SelParams p, const int32_t *__restrict__ sr, const int32_t *__restrict__ sbeg,
                                const int32_t *__restrict__ kept, const int32_t *__restrict__ first,
                                const SelW *__restrict__ work, const float *__restrict__ frac_rep,
                                bsw_alnreg_t *__restrict__ sel_regs, int32_t *__restrict__ sel_read,
                                bsw_selinfo_t *__restrict__ sel_info)
{
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.n_seeds) return;
    const int32_t r = sr[k], idx = k - sbeg[r];
    if (idx >= kept[r]) return;
    const SelW x = work[k];
    const int32_t o = first[r] + idx;
    sel_regs[o] = x.r;
    sel_read[o] = r;
    sel_info[o] = selw_info(x, frac_rep ? frac_rep[r] : 0.f);
}

hipError_t launch_sel_gather(const SelParams &p, const int32_t *sbeg, const int32_t *send, const int32_t *read_len,
                             const bsw_seed_t *seeds, const int32_t *seed_chain, const bsw_alnreg_t *regs,
                             const int32_t *extended, const int32_t *csub, SelW *work, SelRd *st, int32_t *meta,
                             hipStream_t s)
{
    if (p.n_reads <= 0) return hipSuccess;
    hipLaunchKernelGGL(sel_gather_kernel, grid_for(p.n_reads, 64), dim3(64), 0, s, p, sbeg, send, read_len, seeds,
                       seed_chain, regs, extended, csub, work, st, meta);
    return hipGetLastError();
}

hipError_t launch_sel_step(const SelParams &p, const int32_t *list, int32_t n, const SeqPair *pairs,
                           const int32_t *sbeg, const uint8_t *reads, const int64_t *read_off, const float *frac_rep,
                           const uint8_t *ref, SelW *work, SelRd *st, int32_t *zbuf, int32_t *next,
                           int32_t *next_cnt, int32_t *kept, int32_t *meta, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(sel_step_kernel, grid_for(n, 64), dim3(64), 0, s, p, list, n, pairs, sbeg, reads, read_off,
                       frac_rep, ref, work, st, zbuf, next, next_cnt, kept, meta);
    return hipGetLastError();
}

hipError_t launch_sel_build(const SelParams &p, const int32_t *list, int32_t nj, const int32_t *sbeg,
                            const uint8_t *reads, const int64_t *read_off, const SelW *work, const SelRd *st,
                            const uint8_t *ref, SeqPair *pairs, uint8_t *qbuf, uint8_t *tbuf, hipStream_t s)
{
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(sel_build_kernel, grid_for((int64_t)nj * 16, 256), dim3(256), 0, s, p, list, nj, sbeg, reads,
                       read_off, work, st, ref, pairs, qbuf, tbuf);
    return hipGetLastError();
}

hipError_t launch_sel_emit(const SelParams &p, const int32_t *seed_read, const int32_t *sbeg, const int32_t *kept,
                           const int32_t *first, const SelW *work, const float *frac_rep, bsw_alnreg_t *sel_regs,
                           int32_t *sel_read, bsw_selinfo_t *sel_info, hipStream_t s)
{
    if (p.n_seeds <= 0) return hipSuccess;
    hipLaunchKernelGGL(sel_emit_kernel, grid_for(p.n_seeds, 256), dim3(256), 0, s, p, seed_read, sbeg, kept, first,
                       work, frac_rep, sel_regs, sel_read, sel_info);
    return hipGetLastError();
}

}  // namespace bsw
