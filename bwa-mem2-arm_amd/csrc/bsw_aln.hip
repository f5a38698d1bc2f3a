// bsw_aln.hip -- final alignments (include/bsw_aln.h: mem_reg2aln -> bwa_gen_cigar2) around the
// batched ksw_global2 of bsw_global.hip, every per-region step on the GPU against the resident
// reference:
//   aln_plan_kernel    : validation, reject test, infer_bw and the first pass's w_; routes a region
//                        as rejected (finished here), gap-free or DP (appended to a COMPACT job
//                        list: the sparse per-read slots of the extension pipeline would leave most
//                        slots empty, since on real reads the gap-free route is the majority)
//   aln_gapfree_kernel : lq == re - rb with w_ == 0 -- score, NM, MD straight from the read and the
//                        text, 16 lanes per region (one load instruction covers 16 consecutive
//                        bytes of 4 regions, as ext_copy_kernel), mismatch columns by ballot
//   aln_build_kernel   : one region's job through dp_job_write (bsw_stage_k.h): SeqPair (h0 =
//                        bwa_gen_cigar2's band) + query slice / reference span in per-job strides,
//                        reversed on the reverse strand
//   aln_finish_kernel  : one wave per job -- the band loop's decision after the DP; regions that go
//                        round again are compacted into the next pass's list, the others get the
//                        NM / MD walk over the traced CIGAR, the deletion squeeze, clips and pos
// Plain C++ with vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bsw_aln_k.h"
#include "bsw_stage_k.h"
#include "bsw_wave.h"

namespace bsw {

// "ACGTN"[c] on the forward strand, "TGCAN"[c] on the reverse strand
__device__ __forceinline__ uint8_t base_letter(int c, bool rev)
{
    const unsigned long long tab = rev ? 0x4E41434754ull : 0x4E54474341ull;
    return (uint8_t)(tab >> (8 * min(c, 4)));
}

struct MdOut {                          // MD bytes of one region: writes stop at cap, len goes on
    uint8_t *p;
    int cap, len;
    __device__ __forceinline__ void put(uint8_t c)
    {
        if (len < cap) p[len] = c;
        ++len;
    }
    __device__ __forceinline__ void num(int u)
    {
        const int d = u >= 10000 ? 5 : u >= 1000 ? 4 : u >= 100 ? 3 : u >= 10 ? 2 : 1;
        for (int k = d - 1; k >= 0; --k) {
            if (len + k < cap) p[len + k] = (uint8_t)('0' + u % 10);
            u /= 10;
        }
        len += d;
    }
};

// Append the regions flagged `take` to list (count *cnt): one global atomic per BLOCK (the waves'
// counts meet in LDS; one atomic per wave on the single counter was the plan kernel's largest
// cost at millions of regions).  Every thread of a 256-thread block calls it.
__device__ __forceinline__ void list_append(bool take, int32_t item, int32_t *list, int32_t *cnt)
{
    __shared__ int s_n[4], s_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(take);
    if (lane == 0) s_n[wv] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        s_base = tot ? atomicAdd(cnt, tot) : 0;
    }
    __syncthreads();
    int base = s_base;
    for (int k = 0; k < wv; ++k) base += s_n[k];
    if (take) list[base + __popcll(b & ((1ull << lane) - 1))] = item;
}

// The last pass's result of region r -> the caller's arrays: pos, deletion squeeze, clips.
// The DP CIGAR is src[0, nsrc) (nsrc <= 0: more than cigar_stride ops), or the single op op0
// when src is null.
__device__ __forceinline__ void aln_write(const AlnParams &p, const bsw_alnreg_t &r, int l_query,
                                          const uint32_t *src, uint32_t op0, int nsrc, int score, int w, int n_pass,
                                          int nm, const MdOut &mo, int flags, bsw_aln_t *out, uint32_t *dst)
{
    bsw_aln_t o;
    o.score = score; o.w = w; o.n_pass = n_pass;
    bool ok = nsrc > 0;
    if (ok) {
        const bool rev = p.l_pac > 0 && r.rb >= p.l_pac;
        int64_t pos = rev ? 2 * p.l_pac - r.re : r.rb;
        const uint32_t first = src ? src[0] : op0, last = src ? src[nsrc - 1] : op0;
        int a0 = 0, a1 = nsrc;
        if ((first & 15) == 2) { pos += first >> 4; a0 = 1; }
        else if ((last & 15) == 2) a1 = nsrc - 1;
        int clip5 = 0, clip3 = 0;
        if (r.qb != 0 || r.qe != l_query) {
            clip5 = rev ? l_query - r.qe : r.qb;
            clip3 = rev ? r.qb : l_query - r.qe;
        }
        const int nfin = (a1 - a0) + (clip5 > 0) + (clip3 > 0);
        ok = nfin <= p.cigar_stride;
        if (ok) {
            int k = 0;
            if (clip5 > 0) dst[k++] = (uint32_t)clip5 << 4 | 3;
            for (int c = a0; c < a1; ++c) dst[k++] = src ? src[c] : op0;
            if (clip3 > 0) dst[k++] = (uint32_t)clip3 << 4 | 3;
            o.pos = pos; o.is_rev = rev; o.n_cigar = nfin; o.NM = nm;
            o.md_len = mo.p ? (mo.len > mo.cap ? -1 : mo.len) : 0;
            if (o.md_len < 0) flags |= BSW_ALN_OVERFLOW;
        }
    }
    if (!ok) {
        o.pos = -1; o.is_rev = 0; o.n_cigar = -1; o.NM = -1; o.md_len = -1;
        flags |= BSW_ALN_OVERFLOW;
    }
    o.flags = flags;
    *out = o;
}

__global__ void aln_plan_kernel(const AlnParams p, const int32_t *__restrict__ read_len,
                                const bsw_alnreg_t *__restrict__ regs, const int32_t *__restrict__ reg_read, int32_t n,
                                AlnState *__restrict__ st, int32_t *__restrict__ list0, int32_t *__restrict__ cnt,
                                int32_t *__restrict__ meta, bsw_aln_t *__restrict__ aln)
{
    __shared__ int s_m[5];
    if (threadIdx.x < 5) s_m[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int err = 0, rej = 0, gf = 0, dp = 0, lq = 0, rl = 0;
    if (i < n) {
        const bsw_alnreg_t r = regs[i];
        AlnState x;
        x.w2 = 0; x.last_sc = -(1 << 30); x.n_pass = 0; x.kind = kAlnRejected;
        const int64_t lq64 = (int64_t)r.qe - r.qb, rl64 = r.re - r.rb;
        // bns_intv2rid < 0: the region bridges a join of the text -- the contig table's, or with no table
        // the strand boundary alone (its n = 1 case)
        if (r.rb < 0 || r.re < 0 || lq64 <= 0 || r.rb >= r.re ||
            (p.ctg.off ? contig_crosses(p.ctg, r.rb, r.re) : (p.l_pac > 0 && r.rb < p.l_pac && r.re > p.l_pac))) {
            rej = 1;
            bsw_aln_t o;
            o.pos = -1; o.is_rev = 0; o.n_cigar = 0; o.NM = -1; o.score = 0; o.w = 0; o.n_pass = 1; o.md_len = 0;
            o.flags = BSW_ALN_REJECTED;
            aln[i] = o;
        } else {
            const int rd = reg_read[i];
            if (rd < 0 || rd >= p.n_reads || r.qb < 0 || r.qe > read_len[rd] || r.re > p.ref_len ||
                rl64 > BSW_MAX_LEN || lq64 > BSW_MAX_LEN) {
                err = 1;
            } else {
                lq = (int)lq64; rl = (int)rl64;
                int w2 = max(infer_bw(lq, rl, r.truesc, p.a, p.o_del, p.e_del),
                             infer_bw(lq, rl, r.truesc, p.a, p.o_ins, p.e_ins));
                if (w2 > p.W) w2 = min(w2, r.w);
                x.w2 = min(w2, p.W << 2);
                gf = lq == rl && x.w2 == 0;
                dp = !gf;
                x.kind = gf ? kAlnGapFree : kAlnDP;
                if (gf) lq = rl = 0;                        // (the maxima size the DP jobs' strides)
            }
        }
        st[i] = x;
    }
    list_append(dp, i, list0, cnt);
    const int lane = threadIdx.x & 63;
    const int wq = wave_max(lq), wt = wave_max(rl);
    const unsigned long long be = __ballot(err), br = __ballot(rej), bg = __ballot(gf);
    if (lane == 0) {
        if (be) atomicOr(&s_m[0], 1);
        if (br) atomicAdd(&s_m[1], __popcll(br));
        if (bg) atomicAdd(&s_m[2], __popcll(bg));
        atomicMax(&s_m[3], wq);
        atomicMax(&s_m[4], wt);
    }
    __syncthreads();
    int32_t *slot = meta + (blockIdx.x % kAlnMetaSpread) * 16;
    if (threadIdx.x == 0 && s_m[0]) atomicOr(&slot[0], 1);
    if (threadIdx.x == 1 && s_m[1]) atomicAdd(&slot[1], s_m[1]);
    if (threadIdx.x == 2 && s_m[2]) atomicAdd(&slot[2], s_m[2]);
    if (threadIdx.x == 3 && s_m[3]) atomicMax(&slot[3], s_m[3]);
    if (threadIdx.x == 4 && s_m[4]) atomicMax(&slot[4], s_m[4]);
}

// 16 lanes per region stride its columns; on the reverse strand column c is read[qe - 1 - c]
// against T[re - 1 - c] (indexing backwards instead of materialising the reversal).  The group's
// first lane turns each 16-column mismatch mask into MD text.
__global__ void aln_gapfree_kernel(const AlnParams p, const uint8_t *__restrict__ reads,
                                   const int64_t *__restrict__ read_off, const int32_t *__restrict__ read_len,
                                   const bsw_alnreg_t *__restrict__ regs, const int32_t *__restrict__ reg_read,
                                   int32_t n, const AlnState *__restrict__ st, const uint8_t *__restrict__ ref,
                                   bsw_aln_t *__restrict__ aln, uint32_t *__restrict__ cigar, uint8_t *__restrict__ md)
{
    __shared__ int8_t s_mat[32];
#pragma unroll
    for (int k = 0; k < 25; ++k)
        if (threadIdx.x == k) s_mat[k] = p.mat[k];
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t >> 4), sub = (int)(t & 15), grp = (threadIdx.x & 63) >> 4;
    const bool act = i < n && st[i].kind == kAlnGapFree;
    bsw_alnreg_t r;
    r.rb = r.re = 0; r.qb = r.qe = r.score = r.truesc = r.w = r.seedlen0 = 0;
    int lq = 0, l_query = 0;
    bool rev = false;
    const uint8_t *q = reads;
    if (act) {
        r = regs[i];
        const int rd = reg_read[i];
        q = reads + read_off[rd];
        l_query = read_len[rd];
        lq = r.qe - r.qb;
        rev = p.l_pac > 0 && r.rb >= p.l_pac;
    }
    const int lmax = wave_max(lq);
    MdOut mo;
    mo.p = md ? md + (int64_t)i * p.md_stride : nullptr;
    mo.cap = md ? p.md_stride : 0;
    mo.len = 0;
    int sc = 0, last = -1, nmm = 0;
    // four 16-column steps per iteration: their loads are issued together, the masks are taken in
    // column order
    for (int c0 = 0; c0 < lmax; c0 += 64) {
        int qc[4], tc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + 16 * k + sub;
            qc[k] = tc[k] = 0;
            if (c < lq) {
                qc[k] = rev ? q[r.qe - 1 - c] : q[r.qb + c];
                tc[k] = rev ? ref[r.re - 1 - c] : ref[r.rb + c];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool valid = c0 + 16 * k + sub < lq;
            if (valid) sc += s_mat[min(tc[k], 4) * 5 + min(qc[k], 4)];
            unsigned m16 = (unsigned)(__ballot(valid && qc[k] != tc[k]) >> (grp * 16)) & 0xffffu;
            if (sub == 0) {
                nmm += __popc(m16);
                while (m16 && mo.p) {
                    const int cc = c0 + 16 * k + __ffs(m16) - 1;
                    m16 &= m16 - 1;
                    mo.num(cc - last - 1);
                    mo.put(base_letter(rev ? ref[r.re - 1 - cc] : ref[r.rb + cc], rev));
                    last = cc;
                }
            }
        }
    }
    sc += __shfl_xor(sc, 8, 16);
    sc += __shfl_xor(sc, 4, 16);
    sc += __shfl_xor(sc, 2, 16);
    sc += __shfl_xor(sc, 1, 16);
    if (act && sub == 0) {
        if (mo.p) mo.num(lq - last - 1);
        // gen_cigar2 ran once, or twice with the same w_ = 0 (and the same score) when the
        // region's truesc asks for another pass
        const int n_pass = (p.W != 0 && sc < r.truesc - p.a) ? 2 : 1;
        aln_write(p, r, l_query, nullptr, (uint32_t)lq << 4, 1, sc, 0, n_pass, nmm, mo, BSW_ALN_NODP, &aln[i],
                  cigar + (int64_t)i * p.cigar_stride);
    }
}

__global__ void aln_build_kernel(const AlnParams p, const uint8_t *__restrict__ reads,
                                 const int64_t *__restrict__ read_off, const bsw_alnreg_t *__restrict__ regs,
                                 const int32_t *__restrict__ reg_read, const AlnState *__restrict__ st,
                                 const int32_t *__restrict__ list, int32_t nj, const uint8_t *__restrict__ ref,
                                 SeqPair *__restrict__ pairs, uint8_t *__restrict__ qbuf, uint8_t *__restrict__ tbuf)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(t >> 4), sub = (int)(t & 15);
    if (j >= nj) return;
    const int rg = list[j];
    const bsw_alnreg_t r = regs[rg];
    dp_job_write(p, j, sub, reads + read_off[reg_read[rg]], r.qb, r.qe, ref, r.rb, r.re, st[rg].w2, pairs, qbuf,
                 tbuf);
}

// One wave per job: the CIGAR is walked wave-uniformly, an M run is compared 64 columns per step
// (consecutive bytes of the job's own buffers) with the mismatch columns by ballot, lane 0 writes
// the MD text and the outputs.
__global__ void aln_finish_kernel(const AlnParams p, const int32_t *__restrict__ read_len,
                                  const bsw_alnreg_t *__restrict__ regs, const int32_t *__restrict__ reg_read,
                                  AlnState *__restrict__ st, const int32_t *__restrict__ list, int32_t nj,
                                  const SeqPair *__restrict__ pairs, const uint8_t *__restrict__ qbuf,
                                  const uint8_t *__restrict__ tbuf, const uint32_t *__restrict__ jcigar,
                                  const int32_t *__restrict__ jncig, int32_t *__restrict__ next,
                                  int32_t *__restrict__ next_cnt, bsw_aln_t *__restrict__ aln,
                                  uint32_t *__restrict__ cigar, uint8_t *__restrict__ md)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= nj) return;                                    // (whole waves)
    const int rg = list[j];
    const bsw_alnreg_t r = regs[rg];
    AlnState x = st[rg];
    const int score = pairs[j].score, w4 = p.W << 2, n_pass = x.n_pass + 1;
    if (!(score == x.last_sc || x.w2 == w4) && n_pass < 3 && score < r.truesc - p.a) {
        if (lane == 0) {
            x.last_sc = score;
            x.w2 = min(x.w2 * 2, w4);
            x.n_pass = n_pass;
            st[rg] = x;
            next[atomicAdd(next_cnt, 1)] = rg;
        }
        return;
    }
    const bool rev = p.l_pac > 0 && r.rb >= p.l_pac;
    const uint8_t *q = qbuf + (int64_t)j * p.qstride, *t = tbuf + (int64_t)j * p.tstride;
    const uint32_t *cg = jcigar + (int64_t)j * p.cigar_stride;
    const int nc = __builtin_amdgcn_readfirstlane(jncig[j]);
    MdOut mo;
    mo.p = md ? md + (int64_t)rg * p.md_stride : nullptr;
    mo.cap = md ? p.md_stride : 0;
    mo.len = 0;
    int x_ = 0, y = 0, last = -1, col = 0, nmm = 0, ngap = 0;   // col: M columns so far; last: the last
    for (int k = 0; k < nc; ++k) {                                //   mismatch's (u = col - last - 1)
        const uint32_t word = __builtin_amdgcn_readfirstlane(cg[k]);
        const int op = word & 15, len = (int)(word >> 4);
        if (op == 0) {
            for (int c0 = 0; c0 < len; c0 += 64) {
                const int c = c0 + lane;
                int tc = 0;
                bool mm = false;
                if (c < len) {
                    tc = t[y + c];
                    mm = q[x_ + c] != tc;
                }
                unsigned long long m = __ballot(mm);
                nmm += __popcll(m);
                while (m && mo.p) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int tb = __shfl(tc, b);
                    if (lane == 0) {
                        mo.num(col + c0 + b - last - 1);
                        mo.put(base_letter(tb, rev));
                    }
                    last = col + c0 + b;
                }
            }
            x_ += len; y += len; col += len;
        } else if (op == 2) {
            if (k > 0 && k < nc - 1) {
                if (lane == 0 && mo.p) {
                    mo.num(col - last - 1);
                    mo.put('^');
                    for (int c = 0; c < len; ++c) mo.put(base_letter(t[y + c], rev));
                }
                last = col - 1;
                ngap += len;
            }
            y += len;
        } else {
            x_ += len;
            ngap += len;
        }
    }
    if (lane == 0) {
        if (mo.p) mo.num(col - last - 1);
        aln_write(p, r, read_len[reg_read[rg]], cg, 0, nc, score, x.w2, n_pass, nmm + ngap, mo, 0, &aln[rg],
                  cigar + (int64_t)rg * p.cigar_stride);
    }
}

hipError_t launch_aln_plan(const AlnParams &p, const int32_t *read_len, const bsw_alnreg_t *regs,
                           const int32_t *reg_read, int32_t n, AlnState *st, int32_t *list0, int32_t *cnt,
                           int32_t *meta, bsw_aln_t *aln, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(meta, 0, kAlnMetaSpread * 16 * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, kAlnCntWords * sizeof(int32_t), s);
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(aln_plan_kernel, grid_for(n, 256), dim3(256), 0, s, p, read_len, regs, reg_read, n, st, list0,
                       cnt, meta, aln);
    return hipGetLastError();
}

hipError_t launch_aln_gapfree(const AlnParams &p, const uint8_t *reads, const int64_t *read_off,
                              const int32_t *read_len, const bsw_alnreg_t *regs, const int32_t *reg_read, int32_t n,
                              const AlnState *st, const uint8_t *ref, bsw_aln_t *aln, uint32_t *cigar, uint8_t *md,
                              hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(aln_gapfree_kernel, grid_for((int64_t)n * 16, 256), dim3(256), 0, s, p, reads, read_off,
                       read_len, regs, reg_read, n, st, ref, aln, cigar, md);
    return hipGetLastError();
}

hipError_t launch_aln_build(const AlnParams &p, const uint8_t *reads, const int64_t *read_off,
                            const bsw_alnreg_t *regs, const int32_t *reg_read, const AlnState *st,
                            const int32_t *list, int32_t nj, const uint8_t *ref, SeqPair *pairs, uint8_t *qbuf,
                            uint8_t *tbuf, hipStream_t s)
{
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(aln_build_kernel, grid_for((int64_t)nj * 16, 256), dim3(256), 0, s, p, reads, read_off, regs,
                       reg_read, st, list, nj, ref, pairs, qbuf, tbuf);
    return hipGetLastError();
}

hipError_t launch_aln_finish(const AlnParams &p, const int32_t *read_len, const bsw_alnreg_t *regs,
                             const int32_t *reg_read, AlnState *st, const int32_t *list, int32_t nj,
                             const SeqPair *pairs, const uint8_t *qbuf, const uint8_t *tbuf, const uint32_t *jcigar,
                             const int32_t *jncig, int32_t *next, int32_t *next_cnt, bsw_aln_t *aln, uint32_t *cigar,
                             uint8_t *md, hipStream_t s)
{
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL(aln_finish_kernel, grid_for((int64_t)nj * 64, 256), dim3(256), 0, s, p, read_len, regs, reg_read,
                       st, list, nj, pairs, qbuf, tbuf, jcigar, jncig, next, next_cnt, aln, cigar, md);
    return hipGetLastError();
}

}  // namespace bsw
