// bsw_stage_k.h -- what the stage kernels share (launchers in bsw_stage.hip): the grid size, each
// read's run of seed slots, the exclusive scans, the device code that writes one DP job.  A new stage
// starts here, in bsw_formulas.h, bsw_wave.h (wave reductions) and bsw_sel_dev.h (lists of regions).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/bsw_seqpair.h"
#include "bsw_formulas.h"

namespace bsw {

static inline dim3 grid_for(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// sbeg[r], send[r] (zeroed first) = read r's run of seed slots; *err_word |= 1 on a bad or unsorted
// read id
hipError_t launch_seed_runs(const int32_t *seed_read, int32_t n_seeds, int32_t n_reads, int32_t *sbeg, int32_t *send,
                            int32_t *err_word, hipStream_t s);
// out[0 .. n] = exclusive scan of in[0 .. n] (in[n] = 0, so out[n] is the total); tmp == nullptr
// only sizes *tmp_bytes
hipError_t launch_scan32(void *tmp, size_t *tmp_bytes, const int32_t *in, int32_t *out, int32_t n, hipStream_t s);
hipError_t launch_scan64(void *tmp, size_t *tmp_bytes, const int64_t *in, int64_t *out, int32_t n, hipStream_t s);

// A DP job is built by 16 lanes (sub = the lane of 16), so one load / store instruction covers 16
// consecutive bytes of 4 jobs.  Job j's codes live at qbuf + j * qstride and tbuf + j * tstride
// (idr is 32 bits, the text is not).
__device__ __forceinline__ void dp_job_header(SeqPair *pairs, int j, int qstride, int tstride, int len1, int len2,
                                              int h0)
{
    SeqPair sp{};
    sp.idr = j * tstride; sp.idq = j * qstride; sp.id = j;
    sp.len1 = len1; sp.len2 = len2; sp.h0 = h0;
    pairs[j] = sp;
}
// dst[0, n) = src[beg, beg + n), or src[end - n, end) reversed; I = the index type (int32 in a
// read, int64 in the text)
template <class I>
__device__ __forceinline__ void dp_job_copy(uint8_t *dst, const uint8_t *src, I beg, int n, int sub)
{
    for (int k = sub; k < n; k += 16) dst[k] = src[beg + k];
}
template <class I>
__device__ __forceinline__ void dp_job_copy_rev(uint8_t *dst, const uint8_t *src, I end, int n, int sub)
{
    for (int k = sub; k < n; k += 16) dst[k] = src[end - 1 - k];
}

// One ksw_global2 job as bwa_gen_cigar2 sets it up: q[qb, qe) against ref[rb, re) under the band of
// w_, both reversed when the span lies on the reverse strand so that indels come out left-aligned.
// P = a stage's params with the scoring fields, l_pac and the job strides.
template <class P>
__device__ __forceinline__ void dp_job_write(const P &p, int j, int sub, const uint8_t *q, int qb, int qe,
                                             const uint8_t *ref, int64_t rb, int64_t re, int w_, SeqPair *pairs,
                                             uint8_t *qbuf, uint8_t *tbuf)
{
    const int lq = qe - qb, rl = (int)(re - rb);
    uint8_t *qd = qbuf + (int64_t)j * p.qstride, *td = tbuf + (int64_t)j * p.tstride;
    if (sub == 0)
        dp_job_header(pairs, j, p.qstride, p.tstride, rl, lq,
                      cigar_band(p.a, p.o_del, p.e_del, p.o_ins, p.e_ins, lq, rl, w_));
    if (p.l_pac > 0 && rb >= p.l_pac) {
        dp_job_copy_rev(qd, q, qe, lq, sub);
        dp_job_copy_rev(td, ref, re, rl, sub);
    } else {
        dp_job_copy(qd, q, qb, lq, sub);
        dp_job_copy(td, ref, rb, rl, sub);
    }
}

}  // namespace bsw
