// bsw_matesw.hip -- mate rescue (include/bsw_matesw.h: mem_matesw and the rescue block of
// mem_sam_pe) between bsw_pe_stat* and bsw_pe_pair*, in rounds around the batched ksw_align2
// (bsw_mate.hip):
//   msw_count_kernel : one work item per pair -- the offsets and every rb checked, the candidate
//                      counts of both ends, each read's room (its list + 4 per call of its mate)
//   msw_step_kernel  : one work item per pair (a wave per block).  Round 0 copies the pair's lists
//                      into the work lists and its candidates' rb aside; a later round applies the
//                      pending call's results in order -- insert after equal scores, then the dedup
//                      of bsw_sel_dev.h with patch = 0 after every live direction once a job ran.
//                      Then the cursor advances past calls that run no job (all four directions
//                      skipped, or only short windows) to the next call that has one; its jobs (at
//                      most 4, known together because skip[] is fixed at call start) are compacted
//                      by a wave prefix sum and one atomic per wave
//   msw_build_kernel : 16 lanes per job, SeqPair + the query (reverse-complemented in the copy) and
//                      the window of the resident text gathered into per-job strides
//   msw_emit_kernel  : after the scan of the list lengths, the compact output
// The outcome counters are added up per wave into one of 32 slots by block.  Plain C++ with vector
// stores only; no private arrays (skip[] and the call's directions are bit masks).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "bsw_matesw_k.h"
#include "bsw_sel_dev.h"
#include "bsw_stage_k.h"
#include "bsw_wave.h"

namespace bsw {

// direction r's window of the text around an anchor at arb; true when a job runs for it
__device__ __forceinline__ bool msw_window(const MswParams &p, const MswDir &d, int r, int64_t arb, int l_ms,
                                           int64_t &rb, int64_t &re)
{
    const bool is_rev = (r >> 1) != (r & 1), is_larger = !(r >> 1);
    const int64_t lo = d.low, hi = d.high, l_pac = p.s.l_pac;
    if (!is_rev) {
        rb = is_larger ? arb + lo : arb - hi;
        re = (is_larger ? arb + hi : arb - lo) + l_ms;
    } else {
        rb = (is_larger ? arb + lo : arb - hi) - l_ms;
        re = is_larger ? arb + hi : arb - lo;
    }
    rb = max(rb, (int64_t)0);
    re = min(re, l_pac << 1);
    if (rb < re) {
        const int64_t mid = (rb + re) >> 1;
        if (p.ctg.off) {
            // bns_fetch_seq(.., mid, ..): the window is clipped to the segment of its midpoint, and the job
            // exists only when that segment's contig is the anchor's (mem_matesw: a->rid == rid)
            if (contig_clip(p.ctg, mid, rb, re) != contig_rid(p.ctg, arb)) return false;
        } else if (mid < l_pac) {
            re = min(re, l_pac);
        } else {
            rb = max(rb, l_pac);
        }
    }
    return rb < re && re - rb >= p.s.min_seed_len;
}

__global__ __launch_bounds__(256) void msw_count_kernel(const MswParams p, const bsw_alnreg_t *__restrict__ regs,
                                                        const int32_t *__restrict__ first, int32_t *__restrict__ ncand,
                                                        int32_t *__restrict__ capv, int32_t *__restrict__ meta)
{
    const int64_t pr64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pr64 >= p.n_pairs) return;
    const int pr = (int)pr64;
    const int f0 = first[2 * pr], f1 = first[2 * pr + 1], f2 = first[2 * pr + 2];
    if (!(f0 >= 0 && f0 <= f1 && f1 <= f2 && f2 <= p.n_regs)) {
        atomicOr(&meta[kMswErr], 1);
        return;                                             // (ncand and capv stay 0)
    }
    const int64_t two_l = p.s.l_pac << 1;
    bool bad = false;
    int c0 = 0, c1 = 0;
    for (int k = f0; k < f2; ++k) {
        const int64_t rb = regs[k].rb;
        bad |= rb < 0 || rb >= two_l;
        const int thr = regs[k < f1 ? f0 : f1].score - p.pen_unpaired;
        if (regs[k].score >= thr) {
            if (k < f1) ++c0;
            else ++c1;
        }
    }
    if (bad) {
        atomicOr(&meta[kMswErr], 1);
        return;
    }
    c0 = min(c0, p.max_matesw);
    c1 = min(c1, p.max_matesw);
    ncand[2 * pr] = c0;
    ncand[2 * pr + 1] = c1;
    capv[2 * pr] = (f1 - f0) + 4 * c1;
    capv[2 * pr + 1] = (f2 - f1) + 4 * c0;
}

__global__ __launch_bounds__(64) void msw_step_kernel(
    const MswParams p, const int32_t *__restrict__ list, int32_t n_items, const bsw_alnreg_t *__restrict__ regs,
    const bsw_selinfo_t *__restrict__ info, const int32_t *__restrict__ first, const int32_t *__restrict__ read_len,
    const int32_t *__restrict__ ncand, const int32_t *__restrict__ coff, const int32_t *__restrict__ woff,
    int64_t *__restrict__ cand, SelW *__restrict__ work, int32_t *__restrict__ nlist, MswSt *__restrict__ st,
    const bsw_kswr_t *__restrict__ aln, MswJob *__restrict__ jobs, int32_t *__restrict__ next,
    int32_t *__restrict__ meta)
{
    __shared__ int s_stk[kSelStack * 3 * 64];
    __shared__ MswDir s_pes[4];
    if (threadIdx.x < 4) s_pes[threadIdx.x] = p.pes[threadIdx.x];
    __syncthreads();
    int *stk = s_stk + threadIdx.x;
    int32_t *slot = meta + (blockIdx.x % kMswSlots) * kMswMetaWords;
    const int64_t two_l = p.s.l_pac << 1;
    const int32_t t = blockIdx.x * 64 + threadIdx.x;
    const int failed = (s_pes[0].failed ? 1 : 0) | (s_pes[1].failed ? 2 : 0) | (s_pes[2].failed ? 4 : 0) |
                       (s_pes[3].failed ? 8 : 0);
    int c_calls = 0, c_skipped = 0, c_short = 0, c_pushed = 0, c_changed = 0, c_jobs = 0, c_u8 = 0;
    int pr = 0, e = 2, j = 0, chg = 0, jm = 0, live = 0, maxt = 0, l_ms = 0;
    bool err = false;
    if (t < n_items) {
        pr = list ? list[t] : t;
        if (!list) {
            // round 0: the lists into the work lists, the candidates' rb aside
#pragma unroll 1
            for (int en = 0; en < 2; ++en) {
                const int r = 2 * pr + en, fb = first[r], n = first[r + 1] - fb;
                SelW *W = work + woff[r];
                int64_t *C = cand + coff[r];
                const int nc = ncand[r];
                const int thr = n ? regs[fb].score - p.pen_unpaired : 0;
                int c = 0;
                for (int k = 0; k < n; ++k) {
                    // the frac_rep of a region rides in the (here unused) hash word of its work entry
                    const bsw_selinfo_t &f = info[fb + k];
                    SelW x;
                    selw_load(x, regs[fb + k], f, (uint64_t)__float_as_uint(f.frac_rep));
                    W[k] = x;
                    if (c < nc && x.r.score >= thr) C[c++] = x.r.rb;
                }
                nlist[r] = n;
            }
            e = 0;
            j = 0;
        } else {
            // the pending call's results, in the order of its directions
            const MswSt s = st[pr];
            e = s.e;
            j = s.j;
            chg = s.mask & 0x300;
            const int ran = s.mask & 15, lv = (s.mask >> 4) & 15;
            const int ms = 2 * pr + 1 - e;
            const int64_t arb = cand[coff[2 * pr + e] + j];
            SelW *W = work + woff[ms];
            const int room = woff[ms + 1] - woff[ms], lm = read_len[ms];
            int n = nlist[ms], k = s.jbase, nj = 0;
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                if (!(lv >> r & 1)) continue;
                if (ran >> r & 1) {
                    const bsw_kswr_t a = aln[k++];
                    ++nj;
                    if (a.score >= p.s.min_seed_len && a.qb >= 0) {
                        int64_t wb, we;
                        msw_window(p, s_pes[r], r, arb, lm, wb, we);
                        const bool is_rev = (r >> 1) != (r & 1);
                        SelW x{};
                        x.r.qb = is_rev ? lm - (a.qe + 1) : a.qb;
                        x.r.qe = is_rev ? lm - a.qb : a.qe + 1;
                        x.r.rb = is_rev ? two_l - (wb + a.te + 1) : wb + a.tb;
                        x.r.re = is_rev ? two_l - (wb + a.tb) : wb + a.te + 1;
                        x.r.score = a.score;
                        x.csub = a.score2;
                        x.secondary = -1;
                        x.src = -1;
                        x.seedcov = (int)min(x.r.re - x.r.rb, (int64_t)(x.r.qe - x.r.qb)) >> 1;
                        if (n >= room) {                    // (the bound is exact: 4 per call of the mate)
                            err = true;
                        } else {
                            int i = 0;
                            while (i < n && W[i].r.score >= a.score) ++i;
                            for (int m = n; m > i; --m) sel_copy(W + m, W + m - 1);
                            W[i] = x;
                            ++n;
                            ++c_pushed;
                        }
                    }
                }
                if (nj > 0 && n > 1) {
                    int lq, rl;
                    sel_introsort(n, W, stk, LtRe());
                    sel_dedup(p.s, ms, W, n, 1, -2, 0, false, 0, nullptr, nullptr, nullptr, nullptr, slot, lq, rl);
                    n = sel_dedup_drop(W, n, stk, slot);
                }
            }
            nlist[ms] = n;
            const int bit = 0x100 << (1 - e);
            if (!(chg & bit)) ++c_changed;
            chg |= bit;
            ++j;
        }
        // on to the next call that has a job
        while (e < 2) {
            if (j >= ncand[2 * pr + e]) {
                ++e;
                j = 0;
                continue;
            }
            const int ms = 2 * pr + 1 - e;
            const int64_t arb = cand[coff[2 * pr + e] + j];
            const SelW *W = work + woff[ms];
            const int n = nlist[ms];
            l_ms = read_len[ms];
            int skip = failed;
            for (int m = 0; m < n; ++m) {
                int64_t dist;
                const int r = infer_dir(p.s.l_pac, arb, W[m].r.rb, dist);
                if (dist >= s_pes[r].low && dist <= s_pes[r].high) skip |= 1 << r;
            }
            ++c_calls;
            if (skip == 15) {
                ++c_skipped;
                ++j;
                continue;
            }
            jm = 0;
            maxt = 0;
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                if (skip >> r & 1) continue;
                int64_t wb, we;
                if (msw_window(p, s_pes[r], r, arb, l_ms, wb, we)) {
                    jm |= 1 << r;
                    maxt = (int)min(max((int64_t)maxt, we - wb), (int64_t)INT32_MAX);
                } else {
                    ++c_short;
                }
            }
            if (jm == 0) {
                ++j;
                continue;
            }
            live = 15 & ~skip;
            break;
        }
        if (e < 2 && (l_ms < 0 || l_ms > BSW_MATE_MAX_QLEN || maxt > BSW_MAX_LEN)) {
            err = true;
            e = 2;
        }
        if (e >= 2) jm = 0;
    }
    // the wave's jobs and pairs, compact
    const int lane = threadIdx.x & 63;
    const int nj = __popc(jm);
    int incl = nj;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const int total = __shfl(incl, 63);
    const unsigned long long b = __ballot(nj > 0);
    const int mt = wave_max(nj ? maxt : 0), mq = wave_max(nj ? l_ms : 0);
    int jb = 0, lb = 0;
    if (lane == 0 && total) {
        jb = atomicAdd(&meta[kMswNJobs], total);
        lb = atomicAdd(&meta[kMswNext], __popcll(b));
        atomicMax(&meta[kMswMaxT], mt);
        atomicMax(&meta[kMswMaxQ], mq);
    }
    jb = __shfl(jb, 0);
    lb = __shfl(lb, 0);
    if (nj > 0) {
        const int jbase = jb + incl - nj;
        next[lb + __popcll(b & ((1ull << lane) - 1))] = pr;
        const int ms = 2 * pr + 1 - e;
        const int64_t arb = cand[coff[2 * pr + e] + j];
        int k = jbase;
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            if (!(jm >> r & 1)) continue;
            int64_t wb, we;
            msw_window(p, s_pes[r], r, arb, l_ms, wb, we);
            MswJob q;
            q.rb = wb; q.len = (int)(we - wb); q.read = ms; q.rev = (r >> 1) != (r & 1); q.pad = 0;
            jobs[k++] = q;
        }
        MswSt s;
        s.e = e; s.j = j; s.jbase = jbase; s.mask = jm | live << 4 | chg;
        st[pr] = s;
        c_jobs = nj;
        c_u8 = l_ms * p.s.a < 250 ? nj : 0;
    }
    c_calls = wave_sum(c_calls); c_skipped = wave_sum(c_skipped); c_short = wave_sum(c_short);
    c_pushed = wave_sum(c_pushed); c_changed = wave_sum(c_changed); c_jobs = wave_sum(c_jobs); c_u8 = wave_sum(c_u8);
    const unsigned long long be = __ballot(err);
    if (lane == 0) {
        if (c_calls) atomicAdd(&slot[kMswCalls], c_calls);
        if (c_skipped) atomicAdd(&slot[kMswAllSkipped], c_skipped);
        if (c_short) atomicAdd(&slot[kMswShort], c_short);
        if (c_pushed) atomicAdd(&slot[kMswPushed], c_pushed);
        if (c_changed) atomicAdd(&slot[kMswChanged], c_changed);
        if (c_jobs) atomicAdd(&slot[kMswJobs], c_jobs);
        if (c_u8) atomicAdd(&slot[kMswJobsU8], c_u8);
        if (be) atomicOr(&meta[kMswErr], 1);
    }
}

__global__ void msw_build_kernel(const MswParams p, const MswJob *__restrict__ jobs, int32_t nj,
                                 const uint8_t *__restrict__ reads, const int64_t *__restrict__ read_off,
                                 const int32_t *__restrict__ read_len, const uint8_t *__restrict__ ref,
                                 SeqPair *__restrict__ pairs, uint8_t *__restrict__ qbuf, uint8_t *__restrict__ tbuf)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(t >> 4), sub = (int)(t & 15);
    if (j >= nj) return;
    const MswJob q = jobs[j];
    const int lq = read_len[q.read];
    const uint8_t *rd = reads + read_off[q.read];
    uint8_t *qd = qbuf + (int64_t)j * p.qstride;
    if (sub == 0)
        dp_job_header(pairs, j, p.qstride, p.tstride, q.len, lq,
                      BSW_KSW_XSUBO | BSW_KSW_XSTART | (lq * p.s.a < 250 ? BSW_KSW_XBYTE : 0) |
                          (p.s.min_seed_len * p.s.a));
    if (q.rev) {                                            // the reverse complement, not dp_job_copy_rev
        for (int k = sub; k < lq; k += 16) {
            const uint8_t c = rd[lq - 1 - k];
            qd[k] = c < 4 ? 3 - c : 4;
        }
    } else {
        dp_job_copy(qd, rd, 0, lq, sub);
    }
    dp_job_copy(tbuf + (int64_t)j * p.tstride, ref, q.rb, q.len, sub);
}

__global__ void msw_emit_kernel(const MswParams p, const int32_t *__restrict__ woff, const int32_t *__restrict__ nlist,
                                const int32_t *__restrict__ out_first, const SelW *__restrict__ work,
                                bsw_alnreg_t *__restrict__ out_regs, int32_t *__restrict__ out_read,
                                bsw_selinfo_t *__restrict__ out_info)
{
    const int64_t r64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r64 >= 2 * (int64_t)p.n_pairs) return;
    const int r = (int)r64;
    const SelW *W = work + woff[r];
    const int n = nlist[r], o = out_first[r];
    for (int k = 0; k < n; ++k) {
        const SelW x = W[k];
        out_regs[o + k] = x.r;
        out_read[o + k] = r;
        out_info[o + k] = selw_info(x, __uint_as_float((uint32_t)x.hash));     // (frac_rep: see round 0)
    }
}

hipError_t launch_msw_count(const MswParams &p, const bsw_alnreg_t *regs, const int32_t *first, int32_t *ncand,
                            int32_t *capv, int32_t *meta, hipStream_t s)
{
    if (p.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(msw_count_kernel, grid_for(p.n_pairs, 256), dim3(256), 0, s, p, regs, first, ncand, capv, meta);
    return hipGetLastError();
}

hipError_t launch_msw_step(const MswParams &p, const int32_t *list, int32_t n_items, const bsw_alnreg_t *regs,
                           const bsw_selinfo_t *info, const int32_t *first, const int32_t *read_len,
                           const int32_t *ncand, const int32_t *coff, const int32_t *woff, int64_t *cand, SelW *work,
                           int32_t *nlist, MswSt *st, const bsw_kswr_t *aln, MswJob *jobs, int32_t *next,
                           int32_t *meta, hipStream_t s)
{
    if (n_items <= 0) return hipSuccess;
    hipLaunchKernelGGL(msw_step_kernel, grid_for(n_items, 64), dim3(64), 0, s, p, list, n_items, regs, info, first,
                       read_len, ncand, coff, woff, cand, work, nlist, st, aln, jobs, next, meta);
    return hipGetLastError();
}

hipError_t launch_msw_build(const MswParams &p, const MswJob *jobs, int32_t nj, const uint8_t *reads,
                            const int64_t *read_off, const int32_t *read_len, const uint8_t *ref, SeqPair *pairs,
                            uint8_t *qbuf, uint8_t *tbuf, hipStream_t s)
{
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(msw_build_kernel, grid_for((int64_t)nj * 16, 256), dim3(256), 0, s, p, jobs, nj, reads, read_off,
                       read_len, ref, pairs, qbuf, tbuf);
    return hipGetLastError();
}

hipError_t launch_msw_emit(const MswParams &p, const int32_t *woff, const int32_t *nlist, const int32_t *out_first,
                           const SelW *work, bsw_alnreg_t *out_regs, int32_t *out_read, bsw_selinfo_t *out_info,
                           hipStream_t s)
{
    if (p.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(msw_emit_kernel, grid_for(2 * (int64_t)p.n_pairs, 256), dim3(256), 0, s, p, woff, nlist,
                       out_first, work, out_regs, out_read, out_info);
    return hipGetLastError();
}

}  // namespace bsw
