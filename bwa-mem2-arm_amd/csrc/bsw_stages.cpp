// bsw_stages.cpp -- the stages behind the extension, each in a device-resident form and a
// host-array form behind the C ABI: final alignments (bsw_aln.h), region selection (bsw_sel.h),
// the paired-end stage (bsw_pe.h), mate rescue (bsw_matesw.h), SAM records (bsw_rec.h), BGZF
// (bsw_bgzf.h), the BAM sort and index (bsw_bamsort.h) and duplicate marking (bsw_markdup.h).  Their kernels are in
// bsw_aln.hip, bsw_sel.hip, bsw_pe.hip, bsw_matesw.hip, bsw_rec.hip, bsw_bgzf.hip, bsw_bamsort.hip and bsw_markdup.hip;
// what the calls share is below.
// (Layout of the engine: bsw_engine.h.)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <shared_mutex>
#include <vector>
#include "bsw_engine.h"
#include "bsw_mate_k.h"
#include "bsw_global_k.h"
#include "bsw_aln_k.h"
#include "bsw_sel_k.h"
#include "bsw_pe_k.h"
#include "bsw_matesw_k.h"
#include "bsw_rec_k.h"
#include "bsw_bgzf_k.h"
#include "bsw_bamsort_k.h"
#include "bsw_markdup_k.h"
#include "bsw_stage_k.h"

// ---------------------------------------------------------------- shared by the stages
namespace bsw {

// A host-array call's arrays staged through ONE device blob (the slot's d_aio, BlobLayout).  The
// call declares each array once, before it has a slot -- in: copied in, out: copied back, inout:
// both; n elements each -- and gets a Part that converts to the array's device pointer once grow()
// has run.  An _opt array whose host pointer is null takes no room and converts to nullptr.
// Copies run on the slot's stream in the order of declaration and skip empty parts; the call
// site waits for the stream after its last back().
struct BSW_HIDDEN StagedIo {
    template <class T>
    struct Part {
        const StagedIo *io;
        int k;                          // index into recs, -1: an absent optional array
        operator T *() const { return k < 0 ? nullptr : (T *)(io->base + io->recs[k].at); }
    };
    struct Rec { void *host; size_t bytes, at; bool in; };
    std::vector<Rec> recs;
    BlobLayout lay;
    uint8_t *base = nullptr;
    hipStream_t st = nullptr;

    template <class T>
    Part<T> add(T *host, size_t n, bool in, bool optional = false)
    {
        if (optional && !host) return {this, -1};
        recs.push_back({(void *)host, n * sizeof(T), lay.add(n * sizeof(T)), in});
        return {this, (int)recs.size() - 1};
    }
    template <class T> Part<const T> in(const T *host, size_t n) { return add(host, n, true); }
    template <class T> Part<const T> in_opt(const T *host, size_t n) { return add(host, n, true, true); }
    template <class T> Part<T> inout(T *host, size_t n) { return add(host, n, true); }
    template <class T> Part<T> out(T *host, size_t n) { return add(host, n, false); }
    template <class T> Part<T> out_opt(T *host, size_t n) { return add(host, n, false, true); }

    hipError_t grow(Slot &s)            // the slot's first growth in every host form
    {
        const hipError_t e = s.d_aio.grow(lay.total + 16);
        base = s.d_aio;
        st = s.stream;
        return e;
    }
    hipError_t upload() const
    {
        for (const Rec &r : recs)
            if (r.in && r.bytes)
                if (hipError_t e = hipMemcpyAsync(base + r.at, r.host, r.bytes, hipMemcpyHostToDevice, st)) return e;
        return hipSuccess;
    }
    hipError_t stage(Slot &s) { const hipError_t e = grow(s); return e ? e : upload(); }
    // the part's first n elements (default: all) back into its host array
    template <class T>
    hipError_t back(const Part<T> &p, size_t n = SIZE_MAX) const
    {
        if (p.k < 0) return hipSuccess;
        const size_t bytes = std::min(n, recs[p.k].bytes / sizeof(T)) * sizeof(T);
        return bytes ? hipMemcpyAsync(recs[p.k].host, (T *)p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    }
    // bytes from the part's start to the blob's end (the padding between parts included)
    template <class T>
    size_t bytes_from(const Part<T> &p) const { return lay.total - recs[p.k].at; }
};

// host forms: the bytes of `reads` that the offsets and lengths span
static int reads_extent(const int64_t *read_off, const int32_t *read_len, int32_t n_reads, int64_t *rbytes)
{
    *rbytes = 0;
    for (int32_t i = 0; i < n_reads; ++i) {
        if (read_off[i] < 0 || read_len[i] < 0) return BSW_E_RANGE;
        *rbytes = std::max<int64_t>(*rbytes, read_off[i] + read_len[i]);
    }
    return BSW_OK;
}

// Times a stage's helper kernels on `st` with one event pair of the slot (ev2 / ev3; mate rescue
// evw0 / evw1: its batched ksw_align2 times itself with ev0..ev3).  begin() .. end() bracket a
// region; add() reads it once the stream has been waited for -- it does not wait itself.
struct BSW_HIDDEN HelperTimer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st = nullptr;
    hipError_t init(Event &ea, Event &eb, hipStream_t stream)
    {
        hipError_t e = ea ? hipSuccess : hipEventCreate(&ea.p);
        if (e == hipSuccess && !eb) e = hipEventCreate(&eb.p);
        a = ea; b = eb; st = stream;
        return e;
    }
    hipError_t begin() const { return hipEventRecord(a, st); }
    hipError_t end() const { return hipEventRecord(b, st); }
    hipError_t add(float &total) const
    {
        float ms = 0.f;                 // (stays 0 on an error)
        const hipError_t e = hipEventElapsedTime(&ms, a, b);
        total += ms;
        return e;
    }
};

// The slot's buffers for a round of nj DP jobs of strides qstride / tstride; *chunk = the jobs per batch
static hipError_t dp_job_buffers(Slot &s, int32_t nj, int32_t qstride, int32_t tstride, int32_t *chunk)
{
    // SeqPair idr / idq are int32: chunk so j * stride stays below 2^31
    *chunk = (int32_t)std::min<int64_t>(nj, (int64_t)INT32_MAX / std::max(tstride, qstride) - 1);
    if (hipError_t e = s.d_apairs.grow((size_t)*chunk)) return e;
    if (hipError_t e = s.d_aq.grow((size_t)*chunk * qstride)) return e;
    return s.d_at.grow((size_t)*chunk * tstride);
}

// A batch of n DP jobs (d_apairs / d_at / d_aq) through ksw_global2; its time onto dp_ms, its stats
// published as the context's last global-alignment call (bsw_global_last_stats: the last DP batch)
static int dp_batch(bsw_ctx_t *ctx, const GlobParams &gp, Slot &s, int32_t n, uint32_t *d_cigar, int32_t stride,
                    int32_t *d_ncig, hipStream_t st, float &dp_ms)
{
    bsw_global_stats_t gs;
    if (int r = glob_device(gp, s, s.d_apairs, s.d_at, s.d_aq, n, d_cigar, stride, d_ncig, st, &gs)) return r;
    dp_ms += gs.kernel_ms;
    put_stats(ctx, &bsw_ctx::glob_last, gs);
    return BSW_OK;
}

// the resident reference is the forward + reverse strands of an l_pac-base genome; the caller
// holds dc.refmu shared.  A contig table (bsw_contigs.h) has to sum to that l_pac
static bool ref_ok(const DeviceCtx &dc, int64_t l_pac)
{
    return dc.d_refres && dc.refres_len == 2 * l_pac && dc.ctg_ok(l_pac);
}

}  // namespace bsw

// ---------------------------------------------------------------- final alignments (bsw_aln.h)
namespace bsw {

static_assert(kAlnMetaSpread * 16 <= kMetaMaxq && kMetaMaxq + kAlnCntWords <= kMetaWords, "aln meta fits d_meta");

// plan + gap-free -> per pass: build -> ksw_global2 (glob_device) -> finish.  Everything on `st`;
// the host waits once for the plan's counts and once per pass for the next pass's job count.
static int reg2aln_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_ext_opt_t &opt,
                          const uint8_t *d_reads, const int64_t *d_read_off, const int32_t *d_read_len,
                          int32_t n_reads, const bsw_alnreg_t *d_regs, const int32_t *d_reg_read, int32_t n,
                          bsw_aln_t *d_aln, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                          int32_t md_stride, bsw_aln_stats_t &as)
{
    const bsw_params_t &pr = ctx->params;
    AlnParams p{};
    p.W = opt.w; p.a = pr.mat[0];
    p.o_del = pr.o_del; p.e_del = pr.e_del; p.o_ins = pr.o_ins; p.e_ins = pr.e_ins;
    p.n_reads = n_reads;
    p.cigar_stride = cigar_stride; p.md_stride = md_stride;
    p.ref_len = dc.refres_len; p.l_pac = opt.l_pac;
    p.ctg = dc.ctg_view(opt.l_pac);
    memcpy(p.mat, pr.mat, 25);
    GlobParams gp;
    make_glob_params(pr, ctx->glob_band, gp);
    BSW_TRY(s.d_ast.grow((size_t)n));
    BSW_TRY(s.d_alist.grow(2 * (size_t)n));
    BSW_TRY(s.d_acnt.grow(kAlnCntWords));
    HelperTimer tm;
    BSW_TRY(tm.init(s.ev2, s.ev3, st));
    int32_t *h_cnt = s.h_meta + kMetaMaxq;
    BSW_TRY(tm.begin());
    BSW_TRY(launch_aln_plan(p, d_read_len, d_regs, d_reg_read, n, s.d_ast, s.d_alist, s.d_acnt, s.d_meta, d_aln, st));
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_meta, kAlnMetaSpread * 16 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_cnt, s.d_acnt, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    // (regions the plan found in error are marked rejected: the gap-free kernel skips them)
    BSW_TRY(launch_aln_gapfree(p, d_reads, d_read_off, d_read_len, d_regs, d_reg_read, n, s.d_ast, dc.d_refres, d_aln,
                               d_cigar, d_md, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(as.helper_ms));
    int32_t m[5] = {0, 0, 0, 0, 0};
    for (int sl = 0; sl < kAlnMetaSpread; ++sl) {
        const int32_t *v = s.h_meta + sl * 16;
        m[0] |= v[0]; m[1] += v[1]; m[2] += v[2]; m[3] = std::max(m[3], v[3]); m[4] = std::max(m[4], v[4]);
    }
    if (m[0]) return BSW_E_RANGE;
    as.n_rejected = m[1];
    as.n_gapfree = m[2];
    p.qstride = std::max(m[3], 1);                      // longest DP query / reference span
    p.tstride = std::max(m[4], 1);
    int32_t nj = h_cnt[0];
    for (int pass = 0; pass < 3 && nj > 0; ++pass) {
        as.n_dp[pass] = nj;
        const int32_t *list = s.d_alist + (size_t)(pass & 1) * n;
        int32_t *next = s.d_alist + (size_t)((pass + 1) & 1) * n;
        int32_t chunk;
        BSW_TRY(dp_job_buffers(s, nj, p.qstride, p.tstride, &chunk));
        BSW_TRY(s.d_gcig.grow((size_t)chunk * (size_t)cigar_stride));
        BSW_TRY(s.d_gncig.grow((size_t)chunk));
        for (int32_t a = 0; a < nj; a += chunk) {
            const int32_t b = std::min(nj, a + chunk);
            BSW_TRY(tm.begin());
            BSW_TRY(launch_aln_build(p, d_reads, d_read_off, d_regs, d_reg_read, s.d_ast, list + a, b - a, dc.d_refres,
                                     s.d_apairs, s.d_aq, s.d_at, st));
            BSW_TRY(tm.end());
            if (int r = dp_batch(ctx, gp, s, b - a, s.d_gcig, cigar_stride, s.d_gncig, st, as.dp_ms)) return r;
            BSW_TRY(tm.add(as.helper_ms));              // (the batch waited for the stream)
            BSW_TRY(tm.begin());
            BSW_TRY(launch_aln_finish(p, d_read_len, d_regs, d_reg_read, s.d_ast, list + a, b - a, s.d_apairs, s.d_aq,
                                      s.d_at, s.d_gcig, s.d_gncig, next, s.d_acnt + pass + 1, d_aln, d_cigar, d_md, st));
            BSW_TRY(tm.end());
            BSW_TRY(hipMemcpyAsync(h_cnt, s.d_acnt + pass + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            BSW_TRY(hipStreamSynchronize(st));
            BSW_TRY(tm.add(as.helper_ms));
        }
        nj = pass < 2 ? h_cnt[0] : 0;
    }
    return BSW_OK;
}

// argument checks shared by both forms; the caller holds dc.refmu shared
static int reg2aln_check(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, DeviceCtx &dc, int32_t n_reads, int32_t n_regs,
                         int32_t cigar_stride, const void *md, int32_t md_stride)
{
    if (n_reads < 0 || n_regs < 0 || cigar_stride < 1 || md_stride < 0 || (md == nullptr) != (md_stride == 0))
        return BSW_E_INVAL;
    if (!dc.d_refres) return BSW_E_INVAL;
    if (opt->w < 0 || opt->w > (1 << 28) || opt->l_pac < 0 || (opt->l_pac > 0 && !ref_ok(dc, opt->l_pac)) ||
        !dc.ctg_ok(opt->l_pac))
        return BSW_E_INVAL;
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

int bsw_reg2aln_resident(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *d_reads,
                         const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                         const bsw_alnreg_t *d_regs, const int32_t *d_reg_read, int32_t n_regs,
                         bsw_aln_t *d_aln, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                         int32_t md_stride, void *stream)
{
    if (!ctx || !opt) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (const int rc = bsw::reg2aln_check(ctx, opt, dc, n_reads, n_regs, cigar_stride, d_md, md_stride)) return rc;
    if (n_regs > 0 && (!d_reads || !d_read_off || !d_read_len || !d_regs || !d_reg_read || !d_aln || !d_cigar))
        return BSW_E_INVAL;
    bsw_aln_stats_t as{};
    as.n_regs = n_regs;
    if (n_regs > 0) {
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            hipStream_t st = stream ? (hipStream_t)stream : s.stream;
            return bsw::reg2aln_device(ctx, dc, s, st, *opt, d_reads, d_read_off, d_read_len, n_reads, d_regs,
                                       d_reg_read, n_regs, d_aln, d_cigar, cigar_stride, d_md, md_stride, as);
        });
        if (rc) return rc;
    }
    bsw::put_stats(ctx, &bsw_ctx::aln_last, as);
    return BSW_OK;
}

int bsw_reg2aln(bsw_ctx_t *ctx, const bsw_ext_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *regs, const int32_t *reg_read,
                int32_t n_regs, bsw_aln_t *aln, uint32_t *cigar, int32_t cigar_stride, uint8_t *md,
                int32_t md_stride)
{
    if (!ctx || !opt) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::reg2aln_check(ctx, opt, dc, n_reads, n_regs, cigar_stride, md, md_stride)) return rc;
    if (n_regs > 0 && (!reads || !read_off || !read_len || !regs || !reg_read || !aln || !cigar)) return BSW_E_INVAL;
    bsw_aln_stats_t as{};
    as.n_regs = n_regs;
    if (n_regs > 0) {
        int64_t rbytes;
        if (const int rc = bsw::reads_extent(read_off, read_len, n_reads, &rbytes)) return rc;
        const size_t n = (size_t)n_regs, nr = (size_t)n_reads;
        bsw::StagedIo io;
        const auto d_reads = io.in(reads, (size_t)rbytes);
        const auto d_read_off = io.in(read_off, nr);
        const auto d_read_len = io.in(read_len, nr);
        const auto d_regs = io.in(regs, n);
        const auto d_reg_read = io.in(reg_read, n);
        const auto d_aln = io.out(aln, n);
        const auto d_cigar = io.out(cigar, n * (size_t)cigar_stride);
        const auto d_md = io.out_opt(md, n * (size_t)md_stride);
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            BSW_TRY(io.grow(s));
            // (rows the kernels leave unwritten -- rejected regions, overflows -- read back as zeros:
            // cigar and md, the blob's last two parts)
            BSW_TRY(hipMemsetAsync(d_cigar, 0, io.bytes_from(d_cigar), s.stream));
            BSW_TRY(io.upload());
            if (int r = bsw::reg2aln_device(ctx, dc, s, s.stream, *opt, d_reads, d_read_off, d_read_len, n_reads, d_regs,
                                            d_reg_read, n_regs, d_aln, d_cigar, cigar_stride, d_md, md_stride, as))
                return r;
            BSW_TRY(io.back(d_aln));
            BSW_TRY(io.back(d_cigar));
            BSW_TRY(io.back(d_md));
            BSW_TRY(hipStreamSynchronize(s.stream));
            return BSW_OK;
        });
        if (rc) return rc;
    }
    bsw::put_stats(ctx, &bsw_ctx::aln_last, as);
    return BSW_OK;
}

int bsw_aln_last_stats(bsw_ctx_t *ctx, bsw_aln_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::aln_last, out); }

}  // extern "C"

// ---------------------------------------------------------------- region selection (bsw_sel.h)
namespace bsw {

struct SelIo {                          // device pointers of one call, either form
    const uint8_t *reads;
    const int64_t *read_off;
    const int32_t *read_len;
    const bsw_seed_t *seeds;
    const int32_t *seed_read, *seed_chain;
    const bsw_alnreg_t *regs;
    const int32_t *extended, *csub;
    const float *frac_rep;
    bsw_alnreg_t *sel_regs;
    int32_t *sel_read;
    bsw_selinfo_t *sel_info;
    int32_t *read_first;
};

// runs -> gather -> step; per patch round: build -> score-only ksw_global2 (glob_device) -> step
// over the suspended reads; then scan of the kept counts -> emit.  Everything on `st`; the host
// waits once per round for the next round's job count and once for the total.
static int regs_select_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_sel_opt_t &opt,
                              const SelIo &io, int32_t n_reads, int32_t n_seeds, int32_t sel_cap, int32_t *n_sel,
                              bsw_sel_stats_t &ss)
{
    const bsw_params_t &pr = ctx->params;
    SelParams p{};
    p.W = opt.w; p.a = pr.mat[0]; p.b = opt.b;
    p.o_del = pr.o_del; p.e_del = pr.e_del; p.o_ins = pr.o_ins; p.e_ins = pr.e_ins;
    p.n_reads = n_reads; p.n_seeds = n_seeds;
    p.max_chain_gap = opt.max_chain_gap; p.min_seed_len = opt.min_seed_len;
    p.mapQ_coef_len = opt.mapQ_coef_len; p.mapQ_coef_fac = opt.mapQ_coef_fac; p.patch = opt.patch;
    p.mask_level_redun = opt.mask_level_redun; p.mask_level = opt.mask_level;
    p.ref_len = dc.refres_len; p.l_pac = opt.l_pac; p.id0 = opt.id0;
    p.ctg = dc.ctg_view(opt.l_pac);
    memcpy(p.mat, pr.mat, 25);
    GlobParams gp;
    make_glob_params(pr, ctx->glob_band, gp);
    const size_t nr = (size_t)n_reads, ns = (size_t)n_seeds;
    size_t scan_bytes = 0;
    BSW_TRY(launch_scan32(nullptr, &scan_bytes, nullptr, nullptr, n_reads, st));
    BSW_TRY(s.d_swork.grow(std::max<size_t>(ns, 1)));
    BSW_TRY(s.d_sz.grow(std::max<size_t>(ns, 1)));
    BSW_TRY(s.d_sst.grow(std::max<size_t>(nr, 1)));
    BSW_TRY(s.d_srun.grow(2 * nr + 1));
    BSW_TRY(s.d_skept.grow(nr + 1));
    BSW_TRY(s.d_slist.grow(2 * nr + 1));
    BSW_TRY(s.d_smeta.grow(kSelMetaWords));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    HelperTimer tm;
    BSW_TRY(tm.init(s.ev2, s.ev3, st));
    int32_t *sbeg = s.d_srun, *send = s.d_srun + nr;
    int32_t *h_meta = s.h_meta;
    BSW_TRY(tm.begin());
    BSW_TRY(hipMemsetAsync(s.d_srun, 0, (2 * nr + 1) * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_skept, 0, (nr + 1) * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_smeta, 0, kSelMetaWords * sizeof(int32_t), st));
    BSW_TRY(launch_seed_runs(io.seed_read, n_seeds, n_reads, sbeg, send, s.d_smeta + kSelErr, st));
    BSW_TRY(launch_sel_gather(p, sbeg, send, io.read_len, io.seeds, io.seed_chain, io.regs, io.extended, io.csub,
                              s.d_swork, s.d_sst, s.d_smeta, st));
    BSW_TRY(launch_sel_step(p, nullptr, n_reads, nullptr, sbeg, io.reads, io.read_off, io.frac_rep, dc.d_refres,
                            s.d_swork, s.d_sst, s.d_sz, s.d_slist, s.d_smeta + kSelCnt, s.d_skept, s.d_smeta, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_smeta, kSelMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(ss.helper_ms));
    if (h_meta[kSelErr]) return BSW_E_RANGE;
    int32_t nj = h_meta[kSelCnt];
    for (int round = 0; nj > 0; ++round) {
        ss.rounds++;
        ss.n_dp += nj;
        const int cur = round & 1, nxt = cur ^ 1;
        const int32_t *list = s.d_slist + (size_t)cur * nr;
        int32_t *next = s.d_slist + (size_t)nxt * nr;
        p.qstride = std::max(h_meta[kSelMaxQ], 1);          // longest patch query / reference span so far
        p.tstride = std::max(h_meta[kSelMaxT], 1);
        int32_t chunk;
        BSW_TRY(dp_job_buffers(s, nj, p.qstride, p.tstride, &chunk));
        BSW_TRY(hipMemsetAsync(s.d_smeta + kSelCnt + nxt, 0, sizeof(int32_t), st));
        for (int32_t a = 0; a < nj; a += chunk) {
            const int32_t b = std::min(nj, a + chunk);
            BSW_TRY(tm.begin());
            BSW_TRY(launch_sel_build(p, list + a, b - a, sbeg, io.reads, io.read_off, s.d_swork, s.d_sst, dc.d_refres,
                                     s.d_apairs, s.d_aq, s.d_at, st));
            BSW_TRY(tm.end());
            if (int r = dp_batch(ctx, gp, s, b - a, nullptr, 0, nullptr, st, ss.dp_ms)) return r;
            BSW_TRY(tm.add(ss.helper_ms));              // (the batch waited for the stream)
            BSW_TRY(tm.begin());
            BSW_TRY(launch_sel_step(p, list + a, b - a, s.d_apairs, sbeg, io.reads, io.read_off, io.frac_rep,
                                    dc.d_refres, s.d_swork, s.d_sst, s.d_sz, next, s.d_smeta + kSelCnt + nxt, s.d_skept,
                                    s.d_smeta, st));
            BSW_TRY(tm.end());
            BSW_TRY(hipMemcpyAsync(h_meta, s.d_smeta, kSelMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            BSW_TRY(hipStreamSynchronize(st));
            BSW_TRY(tm.add(ss.helper_ms));
            if (h_meta[kSelErr]) return BSW_E_RANGE;
        }
        nj = h_meta[kSelCnt + nxt];
    }
    ss.n_regs_in = h_meta[kSelRegsIn];
    ss.n_redundant = h_meta[kSelRedundant];
    ss.n_identical = h_meta[kSelIdentical];
    ss.n_patch_tried = h_meta[kSelTried];
    ss.n_patch_ok = h_meta[kSelOk];
    ss.n_patch_ratio = h_meta[kSelRatio];
    BSW_TRY(tm.begin());
    BSW_TRY(launch_scan32(s.d_tmp, &scan_bytes, s.d_skept, io.read_first, n_reads, st));
    BSW_TRY(hipMemcpyAsync(h_meta, io.read_first + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    *n_sel = ss.n_sel = h_meta[0];
    if (h_meta[0] > sel_cap) return BSW_E_RANGE;
    BSW_TRY(launch_sel_emit(p, io.seed_read, sbeg, s.d_skept, io.read_first, s.d_swork, io.frac_rep, io.sel_regs,
                            io.sel_read, io.sel_info, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(ss.helper_ms));
    return BSW_OK;
}

// argument checks shared by both forms; the caller holds dc.refmu shared
static int regs_select_check(const bsw_sel_opt_t *opt, DeviceCtx &dc, int32_t n_reads, int32_t n_seeds,
                             int32_t sel_cap)
{
    if (n_reads < 0 || n_seeds < 0 || sel_cap < 0) return BSW_E_INVAL;
    if (!dc.d_refres) return BSW_E_INVAL;
    if (opt->w < 0 || opt->w > (1 << 28) || opt->l_pac < 0 || (opt->l_pac > 0 && !ref_ok(dc, opt->l_pac)) ||
        !dc.ctg_ok(opt->l_pac))
        return BSW_E_INVAL;
    if (opt->max_chain_gap < 0 || opt->mapQ_coef_len < 0 || opt->b < 0 || opt->min_seed_len < 0) return BSW_E_INVAL;
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

void bsw_sel_opt_default(bsw_sel_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->w = 100;
    opt->max_chain_gap = 10000;
    opt->l_pac = 0;
    opt->mask_level_redun = 0.95f;
    opt->mask_level = 0.5f;
    opt->min_seed_len = 19;
    opt->b = 4;
    opt->mapQ_coef_len = 50;
    opt->mapQ_coef_fac = 3;
    opt->patch = 1;
    opt->id0 = 0;
}

int bsw_regs_select_resident(bsw_ctx_t *ctx, const bsw_sel_opt_t *opt, const uint8_t *d_reads,
                             const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                             const bsw_seed_t *d_seeds, const int32_t *d_seed_read, const int32_t *d_seed_chain,
                             const bsw_alnreg_t *d_regs, const int32_t *d_extended, int32_t n_seeds,
                             const int32_t *d_csub, const float *d_frac_rep, bsw_alnreg_t *d_sel_regs,
                             int32_t *d_sel_read, bsw_selinfo_t *d_sel_info, int32_t *d_read_first,
                             int32_t sel_cap, int32_t *n_sel, void *stream)
{
    if (!ctx || !opt || !n_sel) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (const int rc = bsw::regs_select_check(opt, dc, n_reads, n_seeds, sel_cap)) return rc;
    if (!d_read_first || (n_reads > 0 && (!d_read_off || !d_read_len)) ||
        (n_seeds > 0 && (!d_reads || !d_seeds || !d_seed_read || !d_seed_chain || !d_regs || !d_extended)) ||
        (sel_cap > 0 && (!d_sel_regs || !d_sel_read || !d_sel_info)))
        return BSW_E_INVAL;
    bsw_sel_stats_t ss{};
    ss.n_reads = n_reads;
    const bsw::SelIo io = {d_reads, d_read_off, d_read_len, d_seeds, d_seed_read, d_seed_chain, d_regs, d_extended,
                           d_csub, d_frac_rep, d_sel_regs, d_sel_read, d_sel_info, d_read_first};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::regs_select_device(ctx, dc, s, st, *opt, io, n_reads, n_seeds, sel_cap, n_sel, ss);
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::sel_last, ss);
    return BSW_OK;
}

int bsw_regs_select(bsw_ctx_t *ctx, const bsw_sel_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                    const int32_t *read_len, int32_t n_reads, const bsw_seed_t *seeds, const int32_t *seed_read,
                    const int32_t *seed_chain, const bsw_alnreg_t *regs, const int32_t *extended, int32_t n_seeds,
                    const int32_t *csub, const float *frac_rep, bsw_alnreg_t *sel_regs, int32_t *sel_read,
                    bsw_selinfo_t *sel_info, int32_t *read_first, int32_t sel_cap, int32_t *n_sel)
{
    if (!ctx || !opt || !n_sel) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::regs_select_check(opt, dc, n_reads, n_seeds, sel_cap)) return rc;
    if (!read_first || (n_reads > 0 && (!read_off || !read_len)) ||
        (n_seeds > 0 && (!reads || !seeds || !seed_read || !seed_chain || !regs || !extended)) ||
        (sel_cap > 0 && (!sel_regs || !sel_read || !sel_info)))
        return BSW_E_INVAL;
    int64_t rbytes;
    if (const int rc = bsw::reads_extent(read_off, read_len, n_reads, &rbytes)) return rc;
    bsw_sel_stats_t ss{};
    ss.n_reads = n_reads;
    const size_t ns = (size_t)n_seeds, nr = (size_t)n_reads, nc = (size_t)sel_cap;
    bsw::StagedIo io;
    const auto d_reads = io.in(reads, (size_t)rbytes);
    const auto d_read_off = io.in(read_off, nr);
    const auto d_read_len = io.in(read_len, nr);
    const auto d_seeds = io.in(seeds, ns);
    const auto d_seed_read = io.in(seed_read, ns);
    const auto d_seed_chain = io.in(seed_chain, ns);
    const auto d_regs = io.in(regs, ns);
    const auto d_extended = io.in(extended, ns);
    const auto d_csub = io.in_opt(csub, ns);
    const auto d_frac_rep = io.in_opt(frac_rep, nr);
    const auto d_sel_regs = io.out(sel_regs, nc);
    const auto d_sel_read = io.out(sel_read, nc);
    const auto d_sel_info = io.out(sel_info, nc);
    const auto d_read_first = io.out(read_first, nr + 1);
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        const bsw::SelIo dio = {d_reads, d_read_off, d_read_len, d_seeds, d_seed_read, d_seed_chain, d_regs, d_extended,
                                d_csub, d_frac_rep, d_sel_regs, d_sel_read, d_sel_info, d_read_first};
        if (int r = bsw::regs_select_device(ctx, dc, s, s.stream, *opt, dio, n_reads, n_seeds, sel_cap, n_sel, ss))
            return r;
        BSW_TRY(io.back(d_sel_regs, (size_t)*n_sel));   // (the rows emitted, not sel_cap of them)
        BSW_TRY(io.back(d_sel_read, (size_t)*n_sel));
        BSW_TRY(io.back(d_sel_info, (size_t)*n_sel));
        BSW_TRY(io.back(d_read_first));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::sel_last, ss);
    return BSW_OK;
}

int bsw_sel_last_stats(bsw_ctx_t *ctx, bsw_sel_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::sel_last, out); }

}  // extern "C"

// ---------------------------------------------------------------- paired-end stage (bsw_pe.h)
namespace bsw {

// argument checks of both calls and both forms, before anything touches a device
static int pe_check_args(const bsw_pe_opt_t *opt, int32_t n_reads, int32_t n_regs)
{
    if (!opt || n_reads < 0 || (n_reads & 1) || n_regs < 0) return BSW_E_INVAL;
    if (opt->l_pac <= 0 || (opt->id0 & 1) || opt->max_ins < 1 || opt->max_ins > BSW_PE_MAX_INS) return BSW_E_INVAL;
    if (opt->min_seed_len < 0 || opt->b < 0 || opt->mapQ_coef_len < 0) return BSW_E_INVAL;
    return BSW_OK;
}

static int pe_check_pes(const bsw_pestat_t *pes)
{
    if (!pes) return BSW_E_INVAL;
    for (int d = 0; d < 4; ++d)
        if (!pes[d].failed && !(std::isfinite(pes[d].std) && pes[d].std > 0 && std::isfinite(pes[d].avg)))
            return BSW_E_INVAL;
    return BSW_OK;
}

// the stage reads no reference; one that is resident has to be the l_pac the call names
static int pe_check_ref(const bsw_pe_opt_t &opt, DeviceCtx &dc)
{
    return dc.ctg_ok(opt.l_pac) && (!dc.d_refres || ref_ok(dc, opt.l_pac)) ? BSW_OK : BSW_E_INVAL;
}

static void make_pe_params(const bsw_ctx_t *ctx, const bsw_pe_opt_t &opt, int32_t n_reads, int32_t n_regs, PeParams &p)
{
    const bsw_params_t &pr = ctx->params;
    memset(&p, 0, sizeof(p));
    p.s.a = pr.mat[0]; p.s.b = opt.b;
    p.s.o_del = pr.o_del; p.s.e_del = pr.e_del; p.s.o_ins = pr.o_ins; p.s.e_ins = pr.e_ins;
    p.s.n_reads = n_reads;
    p.s.min_seed_len = opt.min_seed_len; p.s.mapQ_coef_len = opt.mapQ_coef_len; p.s.mapQ_coef_fac = opt.mapQ_coef_fac;
    p.s.mask_level = opt.mask_level;
    p.s.l_pac = opt.l_pac; p.s.id0 = opt.id0;
    p.n_pairs = n_reads / 2; p.n_regs = n_regs;
    p.max_ins = opt.max_ins; p.T = opt.T; p.pen_unpaired = opt.pen_unpaired;
    p.ctg = ctx->devs[0]->ctg_view(opt.l_pac);              // (the stage's device; the caller holds its refmu shared)
}

// mem_pestat's per-direction arithmetic over the counts c[v] of insert size v (bsw_pe.h)
static void pestat_of_counts(const int32_t *hist, int bins, bsw_pestat_t *pes)
{
    int64_t nmax = 0;
    for (int d = 0; d < 4; ++d) {
        const int32_t *c = hist + (size_t)d * bins;
        int64_t n = 0;
        for (int v = 0; v < bins; ++v) n += c[v];
        bsw_pestat_t r{};
        r.n = (int32_t)n;
        nmax = std::max(nmax, n);
        if (n < 10) {
            r.failed = 1;
            pes[d] = r;
            continue;
        }
        auto at = [&](int k) {                      // the k-th smallest value
            int64_t acc = 0;
            for (int v = 0; v < bins; ++v) {
                acc += c[v];
                if (acc > k) return v;
            }
            return bins - 1;
        };
        const int p25 = at((int)(.25 * n + .499)), p75 = at((int)(.75 * n + .499));
        r.low = (int)(p25 - 2.0 * (p75 - p25) + .499);
        if (r.low < 1) r.low = 1;
        r.high = (int)(p75 + 2.0 * (p75 - p25) + .499);
        int64_t x = 0;
        const int v0 = std::max(r.low, 0), v1 = std::min(r.high, bins - 1);
        for (int v = v0; v <= v1; ++v) {
            r.avg += (double)c[v] * v;              // (sums of integers: exact in any order)
            x += c[v];
        }
        r.avg /= x;
        for (int v = v0; v <= v1; ++v) r.std += (double)c[v] * ((v - r.avg) * (v - r.avg));
        r.std = sqrt(r.std / x);
        r.low = (int)(p25 - 3.0 * (p75 - p25) + .499);
        r.high = (int)(p75 + 3.0 * (p75 - p25) + .499);
        if (r.low > r.avg - 4.0 * r.std) r.low = (int)(r.avg - 4.0 * r.std + .499);
        if (r.high < r.avg + 4.0 * r.std) r.high = (int)(r.avg + 4.0 * r.std + .499);
        if (r.low < 1) r.low = 1;
        pes[d] = r;
    }
    for (int d = 0; d < 4; ++d)
        if (pes[d].failed == 0 && pes[d].n < nmax * 0.05) pes[d].failed = 1;
}

// count kernel -> the four count arrays and the error word back -> the statistics on the host
static int pe_stat_device(bsw_ctx_t *ctx, Slot &s, hipStream_t st, const bsw_pe_opt_t &opt, const bsw_alnreg_t *regs,
                          const int32_t *first, int32_t n_reads, int32_t n_regs, bsw_pestat_t *pes, bsw_pe_stats_t &ps)
{
    PeParams p;
    make_pe_params(ctx, opt, n_reads, n_regs, p);
    const int bins = opt.max_ins + 1;
    BSW_TRY(s.d_phist.grow((size_t)4 * bins));
    BSW_TRY(s.d_pmeta.grow(kPeSlots * kPeMetaWords));
    HelperTimer tm;
    BSW_TRY(tm.init(s.ev2, s.ev3, st));
    std::vector<int32_t> h((size_t)4 * bins);
    int32_t *h_meta = s.h_meta;
    BSW_TRY(hipMemsetAsync(s.d_phist, 0, h.size() * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_pmeta, 0, kPeSlots * kPeMetaWords * sizeof(int32_t), st));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_pe_stat(p, regs, first, s.d_phist, s.d_pmeta, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_pmeta, kPeSlots * kPeMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h.data(), s.d_phist, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(ps.kernel_ms));
    if (h_meta[kPeErr]) return BSW_E_RANGE;
    pestat_of_counts(h.data(), bins, pes);
    for (int d = 0; d < 4; ++d) ps.n_cand[d] = pes[d].n;
    return BSW_OK;
}

// fast kernel over every pair -> general kernel over the pairs it listed (their count stays on
// the device) -> the counters back
static int pe_pair_device(bsw_ctx_t *ctx, Slot &s, hipStream_t st, const bsw_pe_opt_t &opt, const bsw_pestat_t *pes,
                          bsw_alnreg_t *regs, bsw_selinfo_t *info, const int32_t *first, int32_t n_reads,
                          int32_t n_regs, bsw_pair_t *pairs, bsw_pe_stats_t &ps)
{
    PeParams p;
    make_pe_params(ctx, opt, n_reads, n_regs, p);
    for (int d = 0; d < 4; ++d) {
        p.pes[d].avg = pes[d].avg; p.pes[d].std = pes[d].std;
        p.pes[d].low = pes[d].low; p.pes[d].high = pes[d].high; p.pes[d].failed = pes[d].failed != 0;
    }
    const size_t ng = std::max<size_t>((size_t)n_regs, 1);
    BSW_TRY(s.d_swork.grow(ng));
    BSW_TRY(s.d_sz.grow(ng));
    BSW_TRY(s.d_pv.grow(ng));
    BSW_TRY(s.d_plist.grow(std::max<size_t>((size_t)p.n_pairs, 1)));
    BSW_TRY(s.d_pmeta.grow(kPeSlots * kPeMetaWords));
    HelperTimer tm;
    BSW_TRY(tm.init(s.ev2, s.ev3, st));
    int32_t *h_meta = s.h_meta;
    BSW_TRY(hipMemsetAsync(s.d_pmeta, 0, kPeSlots * kPeMetaWords * sizeof(int32_t), st));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_pe_pair_fast(p, regs, info, first, pairs, s.d_plist, s.d_pmeta, st));
    BSW_TRY(launch_pe_pair_general(p, regs, info, first, pairs, s.d_plist, s.d_swork, s.d_sz, s.d_pv, s.d_pmeta, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_pmeta, kPeSlots * kPeMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(ps.kernel_ms));
    if (h_meta[kPeErr]) return BSW_E_RANGE;
    static_assert(kPeSlots * kPeMetaWords <= kMetaWords, "the slot's pinned mirror holds the pair counters");
    for (int k = 0; k < kPeSlots; ++k) {
        const int32_t *m = h_meta + k * kPeMetaWords;
        int64_t nu;
        memcpy(&nu, m + kPeNu, sizeof(nu));
        ps.n_pairing_tried += m[kPeTried];
        ps.n_paired += m[kPePaired];
        ps.n_multi += m[kPeMulti];
        ps.n_unpaired_preferred += m[kPeUnpaired];
        ps.n_proper += m[kPeProper];
        ps.n_u += nu;
    }
    return BSW_OK;
}

// host forms: read_first as the device will check it, so the staged sizes can be trusted
static int pe_host_first(const int32_t *read_first, int32_t n_reads, int32_t &n_regs)
{
    if (!read_first) return BSW_E_INVAL;
    if (read_first[0] < 0) return BSW_E_RANGE;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_first[r + 1] < read_first[r]) return BSW_E_RANGE;
    n_regs = read_first[n_reads];
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

void bsw_pe_opt_default(bsw_pe_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->max_ins = 10000;
    opt->min_seed_len = 19;
    opt->b = 4;
    opt->T = 30;
    opt->pen_unpaired = 17;
    opt->mapQ_coef_len = 50;
    opt->mapQ_coef_fac = 3;
    opt->mask_level = 0.5f;
}

int bsw_pe_stat_resident(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_alnreg_t *d_sel_regs,
                         const bsw_selinfo_t *d_sel_info, const int32_t *d_read_first, int32_t n_reads,
                         int32_t n_regs, bsw_pestat_t *pes, void *stream)
{
    (void)d_sel_info;                   // (the statistics read the regions alone)
    if (const int rc = bsw::pe_check_args(opt, n_reads, n_regs)) return rc;
    if (!ctx || !pes || !d_read_first || (n_regs > 0 && !d_sel_regs)) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::pe_stat_device(ctx, s, st, *opt, d_sel_regs, d_read_first, n_reads, n_regs, pes, ps);
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::pe_last, ps);
    return BSW_OK;
}

int bsw_pe_stat(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_alnreg_t *sel_regs, const bsw_selinfo_t *sel_info,
                const int32_t *read_first, int32_t n_reads, bsw_pestat_t *pes)
{
    (void)sel_info;
    if (const int rc = bsw::pe_check_args(opt, n_reads, 0)) return rc;
    if (!ctx || !pes) return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && !sel_regs) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    bsw::StagedIo io;
    const auto d_sel_regs = io.in(sel_regs, (size_t)n_regs);
    const auto d_read_first = io.in(read_first, (size_t)n_reads + 1);
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        return bsw::pe_stat_device(ctx, s, s.stream, *opt, d_sel_regs, d_read_first, n_reads, n_regs, pes, ps);
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::pe_last, ps);
    return BSW_OK;
}

int bsw_pe_pair_resident(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_pestat_t *pes, bsw_alnreg_t *d_sel_regs,
                         bsw_selinfo_t *d_sel_info, const int32_t *d_read_first, int32_t n_reads, int32_t n_regs,
                         bsw_pair_t *d_pairs, void *stream)
{
    if (const int rc = bsw::pe_check_args(opt, n_reads, n_regs)) return rc;
    if (const int rc = bsw::pe_check_pes(pes)) return rc;
    if (!ctx || !d_read_first || (n_regs > 0 && (!d_sel_regs || !d_sel_info)) || (n_reads > 0 && !d_pairs))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::pe_pair_device(ctx, s, st, *opt, pes, d_sel_regs, d_sel_info, d_read_first, n_reads, n_regs, d_pairs,
                                   ps);
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::pe_last, ps);
    return BSW_OK;
}

int bsw_pe_pair(bsw_ctx_t *ctx, const bsw_pe_opt_t *opt, const bsw_pestat_t *pes, bsw_alnreg_t *sel_regs,
                bsw_selinfo_t *sel_info, const int32_t *read_first, int32_t n_reads, bsw_pair_t *pairs)
{
    if (const int rc = bsw::pe_check_args(opt, n_reads, 0)) return rc;
    if (const int rc = bsw::pe_check_pes(pes)) return rc;
    if (!ctx || (n_reads > 0 && !pairs)) return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && (!sel_regs || !sel_info)) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (const int rc = bsw::pe_check_ref(*opt, dc)) return rc;
    bsw_pe_stats_t ps{};
    ps.n_pairs = n_reads / 2;
    bsw::StagedIo io;
    const auto d_sel_regs = io.inout(sel_regs, (size_t)n_regs);     // (marked and re-scored in place)
    const auto d_sel_info = io.inout(sel_info, (size_t)n_regs);
    const auto d_read_first = io.in(read_first, (size_t)n_reads + 1);
    const auto d_pairs = io.out(pairs, (size_t)(n_reads / 2));
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        if (int r = bsw::pe_pair_device(ctx, s, s.stream, *opt, pes, d_sel_regs, d_sel_info, d_read_first, n_reads, n_regs,
                                        d_pairs, ps))
            return r;
        BSW_TRY(io.back(d_sel_regs));
        BSW_TRY(io.back(d_sel_info));
        BSW_TRY(io.back(d_pairs));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::pe_last, ps);
    return BSW_OK;
}

int bsw_pe_last_stats(bsw_ctx_t *ctx, bsw_pe_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::pe_last, out); }

}  // extern "C"

// ---------------------------------------------------------------- mate rescue stage (bsw_matesw.h)
namespace bsw {

// argument checks of both forms, before anything touches a device
static int matesw_check_args(const bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes,
                             int32_t n_reads, int32_t n_regs, int32_t out_cap)
{
    if (!opt || !pes || n_reads < 0 || (n_reads & 1) || n_regs < 0 || out_cap < 0) return BSW_E_INVAL;
    if (opt->l_pac <= 0 || opt->max_matesw < 0 || opt->min_seed_len <= 0 || opt->max_chain_gap < 0) return BSW_E_INVAL;
    for (int d = 0; d < 4; ++d)
        if (!pes[d].failed && pes[d].low > pes[d].high) return BSW_E_INVAL;
    if (!ctx) return BSW_E_INVAL;
    return mate_params_ok(ctx->params) ? BSW_OK : BSW_E_INVAL;
}

struct MswIo {
    const uint8_t *reads;
    const int64_t *read_off;
    const int32_t *read_len;
    const bsw_alnreg_t *regs;
    const bsw_selinfo_t *info;
    const int32_t *first;
    bsw_alnreg_t *out_regs;
    int32_t *out_read;
    bsw_selinfo_t *out_info;
    int32_t *out_first;
};

// count + scans -> round 0's step -> per round: one readback of the job count, build, the batched
// ksw_align2, the next step -> the scan of the list lengths -> emit.  The caller holds dc.refmu shared.
static int matesw_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_matesw_opt_t &opt,
                         const bsw_pestat_t *pes, const MswIo &io, int32_t n_reads, int32_t n_regs, int32_t out_cap,
                         int32_t *n_out, bsw_matesw_stats_t &ws)
{
    *n_out = 0;
    const bsw_params_t &pr = ctx->params;
    MswParams p;
    memset(&p, 0, sizeof(p));
    p.s.a = pr.mat[0];
    p.s.max_chain_gap = opt.max_chain_gap; p.s.min_seed_len = opt.min_seed_len; p.s.patch = 0;
    p.s.mask_level_redun = opt.mask_level_redun;
    p.s.l_pac = opt.l_pac; p.s.n_reads = n_reads;
    p.n_pairs = n_reads / 2; p.n_regs = n_regs;
    p.max_matesw = opt.max_matesw; p.pen_unpaired = opt.pen_unpaired;
    p.ctg = p.s.ctg = dc.ctg_view(opt.l_pac);               // (the windows, and the dedup behind every call)
    for (int d = 0; d < 4; ++d) {
        p.pes[d].low = pes[d].low; p.pes[d].high = pes[d].high; p.pes[d].failed = pes[d].failed != 0;
    }
    MateParams mp;
    make_mate_params(pr, mp);
    if ((int64_t)n_regs * 5 > INT32_MAX) return BSW_E_RANGE;        // the work lists' offsets are int32
    const size_t nr = (size_t)n_reads, np = nr / 2, n1 = nr + 1;
    size_t scan_bytes = 0;
    BSW_TRY(launch_scan32(nullptr, &scan_bytes, nullptr, nullptr, n_reads, st));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    BSW_TRY(s.d_wint.grow(5 * n1 + 2 * np + 1));
    BSW_TRY(s.d_wmeta.grow(kMswSlots * kMswMetaWords));
    BSW_TRY(s.d_wst.grow(std::max<size_t>(np, 1)));
    BSW_TRY(s.d_wjobs.grow(std::max<size_t>(4 * np, 1)));
    BSW_TRY(s.d_maln.grow(std::max<size_t>(4 * np, 1)));
    HelperTimer tm;
    BSW_TRY(tm.init(s.evw0, s.evw1, st));
    static_assert(kMswSlots * kMswMetaWords <= kMetaWords, "the slot's pinned mirror holds the stage's counters");
    int32_t *ncand = s.d_wint, *capv = ncand + n1, *coff = capv + n1, *woff = coff + n1, *nlist = woff + n1;
    int32_t *lists = nlist + n1;
    int32_t *h_meta = s.h_meta;
    constexpr size_t kMetaBytes = kMswSlots * kMswMetaWords * sizeof(int32_t);
    BSW_TRY(hipMemsetAsync(s.d_wint, 0, (5 * n1) * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(s.d_wmeta, 0, kMetaBytes, st));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_msw_count(p, io.regs, io.first, ncand, capv, s.d_wmeta, st));
    BSW_TRY(launch_scan32(s.d_tmp, &scan_bytes, ncand, coff, n_reads, st));
    BSW_TRY(launch_scan32(s.d_tmp, &scan_bytes, capv, woff, n_reads, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_wmeta, kMswMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_meta + kMswMetaWords, coff + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_meta + kMswMetaWords + 1, woff + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(ws.helper_ms));
    if (h_meta[kMswErr]) return BSW_E_RANGE;
    const size_t n_cand = (size_t)h_meta[kMswMetaWords], n_work = (size_t)h_meta[kMswMetaWords + 1];
    BSW_TRY(s.d_wcand.grow(std::max<size_t>(n_cand, 1)));
    BSW_TRY(s.d_swork.grow(std::max<size_t>(n_work, 1)));
    int32_t n_items = p.n_pairs;
    const int32_t *list = nullptr;
    for (int round = 0;; ++round) {
        int32_t *next = lists + (size_t)(round & 1) * np;
        BSW_TRY(tm.begin());
        BSW_TRY(launch_msw_step(p, list, n_items, io.regs, io.info, io.first, io.read_len, ncand, coff, woff, s.d_wcand,
                                s.d_swork, nlist, s.d_wst, s.d_maln, s.d_wjobs, next, s.d_wmeta, st));
        BSW_TRY(tm.end());
        BSW_TRY(hipMemcpyAsync(h_meta, s.d_wmeta, kMetaBytes, hipMemcpyDeviceToHost, st));
        BSW_TRY(hipStreamSynchronize(st));
        BSW_TRY(tm.add(ws.helper_ms));
        if (h_meta[kMswErr]) return BSW_E_RANGE;
        const int32_t nj = h_meta[kMswNJobs];
        if (nj == 0) break;
        ++ws.rounds;
        n_items = h_meta[kMswNext];
        list = next;
        p.qstride = std::max(h_meta[kMswMaxQ], 1);
        p.tstride = std::max(h_meta[kMswMaxT], 1);
        int32_t chunk;
        BSW_TRY(dp_job_buffers(s, nj, p.qstride, p.tstride, &chunk));
        BSW_TRY(hipMemsetAsync(s.d_wmeta + kMswNext, 0, 4 * sizeof(int32_t), st));      // the round's words
        for (int32_t a = 0; a < nj; a += chunk) {
            const int32_t b = std::min(nj, a + chunk);
            BSW_TRY(tm.begin());
            BSW_TRY(launch_msw_build(p, s.d_wjobs + a, b - a, io.reads, io.read_off, io.read_len, dc.d_refres, s.d_apairs,
                                     s.d_aq, s.d_at, st));
            BSW_TRY(tm.end());
            bsw_mate_stats_t mst;
            if (int r = mate_device(mp, s, s.d_apairs, s.d_at, s.d_aq, b - a, s.d_maln + a, st, &mst)) return r;
            ws.sw_ms += mst.fwd_ms + mst.rev_ms;
            BSW_TRY(tm.add(ws.helper_ms));          // (the batch waited for the stream)
        }
    }
    for (int k = 0; k < kMswSlots; ++k) {
        const int32_t *m = h_meta + k * kMswMetaWords;
        ws.n_calls += m[kMswCalls];
        ws.n_calls_all_skipped += m[kMswAllSkipped];
        ws.n_jobs += m[kMswJobs];
        ws.n_jobs_u8 += m[kMswJobsU8];
        ws.n_short_window += m[kMswShort];
        ws.n_pushed += m[kMswPushed];
        ws.n_redundant += m[kMswRedundant];
        ws.n_identical += m[kMswIdentical];
        ws.n_lists_changed += m[kMswChanged];
    }
    BSW_TRY(tm.begin());
    BSW_TRY(launch_scan32(s.d_tmp, &scan_bytes, nlist, io.out_first, n_reads, st));
    BSW_TRY(hipMemcpyAsync(h_meta, io.out_first + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    *n_out = ws.n_out = h_meta[0];
    if (h_meta[0] > out_cap) return BSW_E_RANGE;
    BSW_TRY(launch_msw_emit(p, woff, nlist, io.out_first, s.d_swork, io.out_regs, io.out_read, io.out_info, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(ws.helper_ms));
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

void bsw_matesw_opt_default(bsw_matesw_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->max_matesw = 50;
    opt->pen_unpaired = 17;
    opt->min_seed_len = 19;
    opt->max_chain_gap = 10000;
    opt->mask_level_redun = 0.95f;
}

int bsw_matesw_resident(bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes,
                        const uint8_t *d_reads, const int64_t *d_read_off, const int32_t *d_read_len,
                        int32_t n_reads, const bsw_alnreg_t *d_sel_regs, const bsw_selinfo_t *d_sel_info,
                        const int32_t *d_read_first, int32_t n_regs, bsw_alnreg_t *d_out_regs,
                        int32_t *d_out_read, bsw_selinfo_t *d_out_info, int32_t *d_out_first, int32_t out_cap,
                        int32_t *n_out, void *stream)
{
    if (const int rc = bsw::matesw_check_args(ctx, opt, pes, n_reads, n_regs, out_cap)) return rc;
    if (!n_out || !d_read_first || !d_out_first || (n_reads > 0 && (!d_reads || !d_read_off || !d_read_len)) ||
        (n_regs > 0 && (!d_sel_regs || !d_sel_info)) || (out_cap > 0 && (!d_out_regs || !d_out_read || !d_out_info)))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (!bsw::ref_ok(dc, opt->l_pac)) return BSW_E_INVAL;
    bsw_matesw_stats_t ws{};
    ws.n_pairs = n_reads / 2;
    const bsw::MswIo io = {d_reads, d_read_off, d_read_len, d_sel_regs, d_sel_info, d_read_first,
                           d_out_regs, d_out_read, d_out_info, d_out_first};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::matesw_device(ctx, dc, s, st, *opt, pes, io, n_reads, n_regs, out_cap, n_out, ws);
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::matesw_last, ws);
    return BSW_OK;
}

int bsw_matesw(bsw_ctx_t *ctx, const bsw_matesw_opt_t *opt, const bsw_pestat_t *pes, const uint8_t *reads,
               const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *sel_regs,
               const bsw_selinfo_t *sel_info, const int32_t *read_first, bsw_alnreg_t *out_regs,
               int32_t *out_read, bsw_selinfo_t *out_info, int32_t *out_first, int32_t out_cap, int32_t *n_out)
{
    if (const int rc = bsw::matesw_check_args(ctx, opt, pes, n_reads, 0, out_cap)) return rc;
    if (!n_out || !out_first || (n_reads > 0 && (!reads || !read_off || !read_len)) ||
        (out_cap > 0 && (!out_regs || !out_read || !out_info)))
        return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && (!sel_regs || !sel_info)) return BSW_E_INVAL;
    int64_t rbytes;
    if (const int rc = bsw::reads_extent(read_off, read_len, n_reads, &rbytes)) return rc;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (!bsw::ref_ok(dc, opt->l_pac)) return BSW_E_INVAL;
    bsw_matesw_stats_t ws{};
    ws.n_pairs = n_reads / 2;
    const size_t nr = (size_t)n_reads, ng = (size_t)n_regs, nc = (size_t)out_cap;
    bsw::StagedIo io;
    const auto d_reads = io.in(reads, (size_t)rbytes);
    const auto d_read_off = io.in(read_off, nr);
    const auto d_read_len = io.in(read_len, nr);
    const auto d_sel_regs = io.in(sel_regs, ng);
    const auto d_sel_info = io.in(sel_info, ng);
    const auto d_read_first = io.in(read_first, nr + 1);
    const auto d_out_regs = io.out(out_regs, nc);
    const auto d_out_read = io.out(out_read, nc);
    const auto d_out_info = io.out(out_info, nc);
    const auto d_out_first = io.out(out_first, nr + 1);
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        const bsw::MswIo dio = {d_reads, d_read_off, d_read_len, d_sel_regs, d_sel_info, d_read_first,
                                d_out_regs, d_out_read, d_out_info, d_out_first};
        const int r = bsw::matesw_device(ctx, dc, s, s.stream, *opt, pes, dio, n_reads, n_regs, out_cap, n_out, ws);
        if (r == BSW_E_RANGE && *n_out > out_cap) {        // (d_out_first is still written)
            BSW_TRY(io.back(d_out_first));
            BSW_TRY(hipStreamSynchronize(s.stream));
        }
        if (r) return r;
        BSW_TRY(io.back(d_out_regs, (size_t)*n_out));  // (the rows emitted, not out_cap of them)
        BSW_TRY(io.back(d_out_read, (size_t)*n_out));
        BSW_TRY(io.back(d_out_info, (size_t)*n_out));
        BSW_TRY(io.back(d_out_first));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::matesw_last, ws);
    return BSW_OK;
}

int bsw_matesw_last_stats(bsw_ctx_t *ctx, bsw_matesw_stats_t *out)
{
    return bsw::get_stats(ctx, &bsw_ctx::matesw_last, out);
}

}  // extern "C"

// ---------------------------------------------------------------- SAM records (bsw_rec.h)
namespace bsw {

// the options both calls read, before anything touches a device
static int rec_check_opt(const bsw_rec_opt_t *opt)
{
    if (!opt || (opt->flags & ~(BSW_REC_SOFTCLIP | BSW_REC_NO_MULTI | BSW_REC_KEEP_SUPP_MAPQ))) return BSW_E_INVAL;
    const size_t l = strnlen(opt->rname, sizeof(opt->rname));
    return l >= 1 && l <= BSW_REC_MAX_RNAME ? BSW_OK : BSW_E_INVAL;
}

static int records_check_args(const bsw_rec_opt_t *opt, int32_t n_reads, int32_t n_regs, bool paired,
                              int32_t cigar_stride, int32_t md_stride, int32_t rec_cap, int32_t aln_cap)
{
    if (const int rc = rec_check_opt(opt)) return rc;
    if (n_reads < 0 || n_regs < 0 || rec_cap < 0 || aln_cap < 0 || (paired && (n_reads & 1))) return BSW_E_INVAL;
    if (opt->l_pac <= 0 || opt->w < 0 || opt->w > (1 << 28) || opt->max_XA_hits < 0 || !std::isfinite(opt->XA_drop_ratio))
        return BSW_E_INVAL;
    return cigar_stride >= 1 && md_stride >= 1 ? BSW_OK : BSW_E_INVAL;
}

struct RecIo {                          // device pointers of one records call, either form
    const uint8_t *reads;
    const int64_t *read_off;
    const int32_t *read_len;
    RecLists lists;
    bsw_rec_t *recs;
    int32_t *rec_first;
    bsw_aln_t *aln;
    int32_t *aln_reg;
    uint32_t *cigar;
    uint8_t *md;
};

// count -> two scans -> one readback of the totals -> fill (records, the needed regions compact) ->
// reg2aln_device over those on this lease -> finish.  The caller holds dc.refmu shared.
static int records_device(bsw_ctx_t *ctx, DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_rec_opt_t &opt,
                          const RecIo &io, int32_t n_reads, int32_t n_regs, int32_t cigar_stride, int32_t md_stride,
                          int32_t rec_cap, int32_t aln_cap, int32_t *n_rec, int32_t *n_aln, bsw_rec_stats_t &rs)
{
    *n_rec = *n_aln = 0;
    RecParams p{};
    p.n_reads = n_reads; p.n_regs = n_regs;
    p.T = opt.T; p.max_XA_hits = opt.max_XA_hits; p.flags = opt.flags;
    p.mask_level = opt.mask_level; p.xa_ratio = (double)opt.XA_drop_ratio;
    const size_t nr = (size_t)n_reads, n1 = nr + 1;
    size_t scan_bytes = 0;
    BSW_TRY(launch_scan32(nullptr, &scan_bytes, nullptr, nullptr, n_reads, st));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    BSW_TRY(s.d_rcnt.grow(3 * n1));
    BSW_TRY(s.d_rmeta.grow(kRecMetaWords + kRecNameWords));
    HelperTimer tm;
    BSW_TRY(tm.init(s.evw0, s.evw1, st));
    static_assert(kRecMetaWords + 2 <= kMetaWords, "the slot's pinned mirror holds the stage's counters");
    int32_t *nrec = s.d_rcnt, *naln = nrec + n1, *aln_first = naln + n1;
    int32_t *h_meta = s.h_meta;
    BSW_TRY(hipMemsetAsync(s.d_rmeta, 0, kRecMetaWords * sizeof(int32_t), st));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_rec_count(p, io.lists, nrec, naln, s.d_rmeta, st));
    BSW_TRY(launch_scan32(s.d_tmp, &scan_bytes, nrec, io.rec_first, n_reads, st));
    BSW_TRY(launch_scan32(s.d_tmp, &scan_bytes, naln, aln_first, n_reads, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_rmeta, kRecMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_meta + kRecMetaWords, io.rec_first + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_meta + kRecMetaWords + 1, aln_first + nr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(rs.helper_ms));
    if (h_meta[kRecErr]) return BSW_E_RANGE;
    const int32_t nrc = h_meta[kRecMetaWords], na = h_meta[kRecMetaWords + 1];
    *n_rec = rs.n_rec = nrc;
    *n_aln = rs.n_aln = na;
    if (nrc > rec_cap || na > aln_cap) return BSW_E_RANGE;
    BSW_TRY(s.d_rregs.grow(std::max<size_t>((size_t)na, 1)));
    BSW_TRY(s.d_rread.grow(std::max<size_t>((size_t)na, 1)));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_rec_fill(p, io.lists, io.rec_first, aln_first, io.recs, io.aln_reg, s.d_rregs, s.d_rread, st));
    BSW_TRY(tm.end());
    if (na > 0) {
        bsw_ext_opt_t eo;
        bsw_ext_opt_default(&eo);
        eo.w = opt.w; eo.l_pac = opt.l_pac;
        bsw_aln_stats_t as{};
        as.n_regs = na;
        if (int r = reg2aln_device(ctx, dc, s, st, eo, io.reads, io.read_off, io.read_len, n_reads, s.d_rregs, s.d_rread,
                                   na, io.aln, io.cigar, cigar_stride, io.md, md_stride, as))
            return r;
        rs.aln_ms = as.dp_ms + as.helper_ms;    // (bsw_aln_last_stats stays the last bsw_reg2aln* call's)
    } else {
        BSW_TRY(hipStreamSynchronize(st));
    }
    BSW_TRY(tm.add(rs.helper_ms));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_rec_finish(io.lists, dc.ctg_view(opt.l_pac), io.rec_first, io.recs, nrc, io.aln, io.cigar, cigar_stride,
                              na, s.d_rmeta, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(h_meta, s.d_rmeta, kRecMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(rs.helper_ms));
    rs.n_unmapped = h_meta[kRecUnmapped];
    rs.n_supp = h_meta[kRecSupp];
    rs.n_xa = h_meta[kRecXa];
    rs.n_overflow = h_meta[kRecOverflow];
    return h_meta[kRecRejected] || h_meta[kRecOverflow] ? BSW_E_RANGE : BSW_OK;
}

struct OutIo {                          // call 2's outputs, either form: SAM lines or BAM blocks
    uint8_t *out;
    int64_t *off;
};

static int rec_out_check_args(const bsw_rec_opt_t *opt, int32_t n_rec, int32_t n_aln, int32_t n_reads, int32_t paired,
                              int32_t cigar_stride, int32_t md_stride, int64_t out_cap)
{
    if (const int rc = rec_check_opt(opt)) return rc;
    if (n_rec < 0 || n_aln < 0 || n_reads < 0 || out_cap < 0 || cigar_stride < 1 || md_stride < 1) return BSW_E_INVAL;
    return paired && (n_reads & 1) ? BSW_E_INVAL : BSW_OK;
}

// the text calls read no reference; a contig table has to sum to the l_pac they name (the caller
// holds dc.refmu shared, and keeps it while the kernels read the table)
static bool text_ctg_ok(const DeviceCtx &dc, const bsw_rec_opt_t &opt) { return dc.ctg_ok(opt.l_pac); }

static void make_rec_text(const DeviceCtx &dc, const bsw_rec_opt_t &opt, int32_t n_rec, int32_t n_aln, int32_t n_reads,
                          int32_t paired, int32_t cigar_stride, int32_t md_stride, RecText &t)
{
    t.ctg = dc.ctg_view(opt.l_pac);
    t.n_rec = n_rec; t.n_aln = n_aln; t.n_reads = n_reads;
    t.n_names = paired ? n_reads / 2 : n_reads;
    t.cigar_stride = cigar_stride; t.md_stride = md_stride;
    t.paired = paired != 0; t.flags = opt.flags;
    t.rname_len = (int32_t)strnlen(opt.rname, sizeof(opt.rname));
}

// call 2 has two output forms on the same arrays: SAM lines (bsw_rec.h) and BAM alignment blocks (bsw_bam.h)
enum class RecForm { Text, Bam };

// lengths -> scan -> one readback (error word + total) -> write; the time of the first half onto
// len_ms, of the write kernel onto write_ms (the text form reports their sum as text_ms)
static int rec_out_device(RecForm form, Slot &s, hipStream_t st, const bsw_rec_opt_t &opt, RecText &t, const OutIo &io,
                          int64_t out_cap, int64_t *n_bytes, float &len_ms, float &write_ms)
{
    const bool bam = form == RecForm::Bam;
    *n_bytes = 0;
    size_t scan_bytes = 0;
    BSW_TRY(launch_scan64(nullptr, &scan_bytes, nullptr, nullptr, t.n_rec, st));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    BSW_TRY(s.d_rlen.grow((size_t)t.n_rec + 1));
    BSW_TRY(s.d_rmeta.grow(kRecMetaWords + kRecNameWords));
    HelperTimer tm;
    BSW_TRY(tm.init(s.evw0, s.evw1, st));
    static_assert(2 * kRecMetaWords + kRecNameWords <= kMetaWords, "the slot's pinned mirror holds the name");
    int64_t *h_tot = (int64_t *)(s.h_meta + kRecMetaWords);
    int32_t *h_name = s.h_meta + 2 * kRecMetaWords;
    memcpy(h_name, opt.rname, sizeof(opt.rname));
    BSW_TRY(hipMemsetAsync(s.d_rmeta, 0, kRecMetaWords * sizeof(int32_t), st));
    BSW_TRY(hipMemcpyAsync(s.d_rmeta + kRecMetaWords, h_name, sizeof(opt.rname), hipMemcpyHostToDevice, st));
    t.rname = (const uint8_t *)(s.d_rmeta + kRecMetaWords);
    BSW_TRY(tm.begin());
    BSW_TRY(bam ? launch_rec_bam_len(t, s.d_rlen, s.d_rmeta, st) : launch_rec_text_len(t, s.d_rlen, s.d_rmeta, st));
    BSW_TRY(launch_scan64(s.d_tmp, &scan_bytes, s.d_rlen, io.off, t.n_rec, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_rmeta, kRecMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_tot, io.off + t.n_rec, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(len_ms));
    if (s.h_meta[kRecErr]) return BSW_E_RANGE;
    *n_bytes = *h_tot;
    if (*n_bytes > out_cap) return BSW_E_RANGE;
    BSW_TRY(tm.begin());
    BSW_TRY(bam ? launch_rec_bam_write(t, io.off, io.out, st) : launch_rec_text_write(t, io.off, io.out, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(write_ms));
    return BSW_OK;
}

// the text call's counters onto the last stats, whose other fields are the last records call's; the
// BAM call's are a struct of their own
static void put_out_stats(RecForm form, bsw_ctx_t *ctx, int32_t n_rec, int64_t n_bytes, float len_ms, float write_ms)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    if (form == RecForm::Bam) {
        ctx->bam_last = bsw_bam_stats_t{n_rec, 0, n_bytes, len_ms, write_ms};
    } else {
        ctx->rec_last.n_bytes = n_bytes;
        ctx->rec_last.text_ms = len_ms + write_ms;
    }
}

// ---------------------------------------------------------------- BGZF (bsw_bgzf.h)
static int bgzf_check_args(const bsw_bgzf_opt_t *opt, int64_t n_in, int32_t n_rec, int64_t out_cap, int32_t blk_cap)
{
    if (!opt || n_in < 0 || n_rec < 0 || out_cap < 0 || blk_cap < 0) return BSW_E_INVAL;
    if (opt->level < 0 || opt->level > 1 || (opt->flags & ~BSW_BGZF_EOF)) return BSW_E_INVAL;
    if (opt->block_bytes < 1 || opt->block_bytes > BSW_BGZF_MAX_BLOCK) return BSW_E_INVAL;
    return (n_in + opt->block_bytes - 1) / opt->block_bytes > INT32_MAX - 1 ? BSW_E_RANGE : BSW_OK;
}

// clear the staging -> deflate -> sizes scanned into blk_off -> virtual offsets -> one readback (total, error
// word, form counts) -> compaction into out.  bs.n_blocks and bs.n_in are set by the caller
static int bgzf_device(Slot &s, hipStream_t st, const bsw_bgzf_opt_t &opt, const uint8_t *d_in, const int64_t *d_rec_off,
                       int32_t n_rec, uint8_t *d_out, int64_t out_cap, int64_t *d_blk_off, int64_t *d_voff,
                       int64_t *n_bytes, bsw_bgzf_stats_t &bs)
{
    const int32_t nb = bs.n_blocks;
    const bool eof = (opt.flags & BSW_BGZF_EOF) != 0;
    const int32_t grid = std::min<int32_t>(nb, kBgzfGrid);
    *n_bytes = 0;
    size_t scan_bytes = 0;
    BSW_TRY(launch_scan64(nullptr, &scan_bytes, nullptr, nullptr, nb, st));
    BSW_TRY(s.d_tmp.grow(std::max<size_t>(scan_bytes, 16)));
    BSW_TRY(s.d_bsize.grow((size_t)nb + 1));
    BSW_TRY(s.d_bmeta.grow(kBgzfMetaWords));
    BSW_TRY(s.d_bstage.grow(std::max<size_t>((size_t)nb, 1) * bgzf::kStageStride));
    BSW_TRY(s.d_btok.grow(std::max<size_t>((size_t)grid, 1) * bgzf::kTokPerBlock));
    HelperTimer tm;
    BSW_TRY(tm.init(s.evw0, s.evw1, st));
    static_assert(kBgzfMetaWords + 2 <= kMetaWords, "the slot's pinned mirror holds the meta words and the total");
    int64_t *h_tot = (int64_t *)(s.h_meta + kBgzfMetaWords);
    BSW_TRY(hipMemsetAsync(s.d_bmeta, 0, kBgzfMetaWords * sizeof(int32_t), st));
    BSW_TRY(tm.begin());
    if (nb > 0) BSW_TRY(hipMemsetAsync(s.d_bstage, 0, (size_t)nb * bgzf::kStageStride, st));
    BSW_TRY(launch_bgzf_deflate(d_in, bs.n_in, opt.block_bytes, nb, opt.level, s.d_bstage, s.d_btok, grid, s.d_bsize,
                                s.d_bmeta, st));
    if (nb == 0) BSW_TRY(hipMemsetAsync(s.d_bsize, 0, sizeof(int64_t), st));
    BSW_TRY(launch_scan64(s.d_tmp, &scan_bytes, s.d_bsize, d_blk_off, nb, st));
    BSW_TRY(launch_bgzf_voff(d_rec_off, n_rec, bs.n_in, opt.block_bytes, d_blk_off, opt.base_coffset, d_voff, s.d_bmeta, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_bmeta, kBgzfMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_tot, d_blk_off + nb, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(bs.deflate_ms));
    if (s.h_meta[kBgzfErr]) return BSW_E_RANGE;
    bs.n_stored = s.h_meta[kBgzfStored + bgzf::kStored];
    bs.n_fixed = s.h_meta[kBgzfStored + bgzf::kFixed];
    bs.n_dynamic = s.h_meta[kBgzfStored + bgzf::kDynamic];
    *n_bytes = bs.n_out = *h_tot + (eof ? bgzf::kEofBytes : 0);
    if (*n_bytes > out_cap) return BSW_E_RANGE;
    if (nb > 0 || eof) {
        BSW_TRY(tm.begin());
        BSW_TRY(launch_bgzf_pack(s.d_bstage, d_blk_off, nb, eof, d_out, st));
        BSW_TRY(tm.end());
        BSW_TRY(hipStreamSynchronize(st));
        BSW_TRY(tm.add(bs.pack_ms));
    }
    return BSW_OK;
}

// ---------------------------------------------------------------- BAM sort and index (bsw_bamsort.h)
static int bamsort_check_opt(const bsw_bamsort_opt_t *opt)
{
    return !opt || opt->n_ref <= 0 || opt->flags ? BSW_E_INVAL : BSW_OK;
}

static bool ranges_overlap(const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb)
{
    return na > 0 && nb > 0 && (uintptr_t)a < (uintptr_t)b + (uint64_t)nb && (uintptr_t)b < (uintptr_t)a + (uint64_t)na;
}

// keys and checks -> one readback (error word, the keys' OR / NOR, n_bytes) -> radix sort over the bits that vary
// (none: the input order) -> sorted lengths scanned into out_off -> the permute kernel
static int bam_sort_device(Slot &s, hipStream_t st, const bsw_bamsort_opt_t &opt, const uint8_t *d_bam,
                           const int64_t *d_bam_off, int32_t n_rec, uint8_t *d_out, int64_t out_cap, int64_t *d_out_off,
                           int32_t *d_perm, bsw_bamsort_stats_t &qs)
{
    const size_t n = (size_t)n_rec;
    size_t scan_bytes = 0, sort_bytes = 0;
    BSW_TRY(launch_scan64(nullptr, &scan_bytes, nullptr, nullptr, n_rec, st));
    BSW_TRY(launch_bamsort_pairs(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, n_rec, 0, 64, st));
    const size_t tmp_bytes = std::max<size_t>(std::max(scan_bytes, sort_bytes), 16);
    BSW_TRY(s.d_tmp.grow(tmp_bytes));
    BSW_TRY(s.d_qkey.grow(2 * n));
    BSW_TRY(s.d_qval.grow(n));
    BSW_TRY(s.d_rlen.grow(n + 1));
    BSW_TRY(s.d_qmeta.grow(kBsMetaWords));
    HelperTimer tm;
    BSW_TRY(tm.init(s.evw0, s.evw1, st));
    static_assert(kBsMetaWords + 2 <= kMetaWords, "the slot's pinned mirror holds the meta words and the total");
    int64_t *h_tot = (int64_t *)(s.h_meta + kBsMetaWords);
    BSW_TRY(hipMemsetAsync(s.d_qmeta, 0, kBsMetaWords * sizeof(int32_t), st));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_bamsort_keys(d_bam, d_bam_off, n_rec, opt.n_ref, s.d_qkey, s.d_qval, s.d_qmeta, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_qmeta, kBsMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_tot, d_bam_off + n_rec, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(qs.key_ms));
    if (s.h_meta[kBsErr] || *h_tot < 0) return BSW_E_RANGE;
    qs.n_bytes = *h_tot;
    if (qs.n_bytes > out_cap) return BSW_E_RANGE;
    if (ranges_overlap(d_bam, qs.n_bytes, d_out, qs.n_bytes)) return BSW_E_INVAL;
    if (bamsort_tiles(qs.n_bytes) > INT32_MAX) return BSW_E_RANGE;
    BSW_TRY(s.d_qints.grow((size_t)bamsort_tiles(qs.n_bytes) + 1));      // the output tiles' first records
    uint64_t or_, nor_;
    memcpy(&or_, s.h_meta + kBsOr, sizeof or_);
    memcpy(&nor_, s.h_meta + kBsNor, sizeof nor_);
    int lo, hi;
    bamsort::key_span(or_, nor_, &lo, &hi);
    qs.key_bits = hi - lo;
    BSW_TRY(tm.begin());
    if (hi > lo) {
        size_t tb = tmp_bytes;
        BSW_TRY(launch_bamsort_pairs(s.d_tmp, &tb, s.d_qkey, s.d_qkey + n, s.d_qval, d_perm, n_rec, lo, hi, st));
    } else {
        BSW_TRY(hipMemcpyAsync(d_perm, s.d_qval, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(qs.sort_ms));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_bamsort_lens(d_bam_off, d_perm, n_rec, s.d_rlen, st));
    BSW_TRY(launch_scan64(s.d_tmp, &scan_bytes, s.d_rlen, d_out_off, n_rec, st));
    BSW_TRY(launch_bamsort_permute(d_bam, d_bam_off, d_perm, d_out_off, s.d_qints, n_rec, qs.n_bytes, d_out, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(qs.copy_ms));
    return BSW_OK;
}

// the index's host-side plan: the references' first windows in the flat linear index
static int bai_windows(const bsw_bamsort_opt_t &opt, const int32_t *ref_len, std::vector<int64_t> &h64)
{
    const size_t r1 = (size_t)opt.n_ref + 1;
    h64.assign(r1 + (r1 + 1) / 2, 0);               // win_off, then ref_len as int32
    int32_t *h_len = (int32_t *)(h64.data() + r1);
    for (int32_t r = 0; r < opt.n_ref; ++r) {
        if (ref_len[r] < 0 || ref_len[r] > BSW_BAI_MAX_REF_LEN) return BSW_E_RANGE;
        h64[r + 1] = h64[r] + (((int64_t)ref_len[r] + 16383) >> bamsort::kLinShift);
        h_len[r] = ref_len[r];
    }
    return BSW_OK;
}

// plan (extents, windows, bins, chunks, sizes) -> one readback (meta, the references' bytes) -> the file
static int bam_index_device(Slot &s, hipStream_t st, const bsw_bamsort_opt_t &opt, const std::vector<int64_t> &h64,
                            const uint8_t *d_bam, const int64_t *d_bam_off, int32_t n_rec, const int64_t *d_voff,
                            int64_t end_voff, uint8_t *d_bai, int64_t bai_cap, int64_t *n_bytes, bsw_bamsort_stats_t &qs)
{
    const size_t n = (size_t)n_rec, r1 = (size_t)opt.n_ref + 1;
    BaiArgs a{};
    a.n_win = h64[opt.n_ref];
    BSW_TRY(bai_tmp_bytes(n_rec, opt.n_ref, &a.tmp_bytes));
    BSW_TRY(s.d_tmp.grow(a.tmp_bytes));
    BSW_TRY(s.d_qkey.grow(std::max<size_t>(2 * n, 1)));
    BSW_TRY(s.d_qval.grow(std::max<size_t>(2 * n, 1)));
    BSW_TRY(s.d_qints.grow((size_t)kBiIntArrays * (n + 1)));
    BSW_TRY(s.d_qref.grow((size_t)opt.n_ref * kBiRefWords));
    BSW_TRY(s.d_qlin.grow(std::max<size_t>((size_t)a.n_win, 1)));
    BSW_TRY(s.d_qref64.grow(2 * r1 + h64.size()));
    BSW_TRY(s.d_qmeta.grow(kBiMetaWords));
    a.bam = d_bam; a.off = d_bam_off; a.voff = d_voff; a.end_voff = end_voff;
    a.n_rec = n_rec; a.n_ref = opt.n_ref;
    a.ref_size = s.d_qref64; a.ref_off = s.d_qref64 + r1;
    a.win_off = s.d_qref64 + 2 * r1;
    a.ref_len = (const int32_t *)(s.d_qref64 + 3 * r1);
    a.lin = s.d_qlin; a.ref = s.d_qref;
    a.key = s.d_qkey; a.key2 = s.d_qkey + n; a.val = s.d_qval; a.val2 = s.d_qval + n;
    a.ints = s.d_qints; a.meta = s.d_qmeta; a.tmp = s.d_tmp; a.bai = d_bai;
    HelperTimer tm;
    BSW_TRY(tm.init(s.evw0, s.evw1, st));
    static_assert(kBiMetaWords + 2 <= kMetaWords, "the slot's pinned mirror holds the meta words and the total");
    int64_t *h_tot = (int64_t *)(s.h_meta + kBiMetaWords);
    BSW_TRY(hipMemsetAsync(s.d_qmeta, 0, kBiMetaWords * sizeof(int32_t), st));
    BSW_TRY(hipMemcpyAsync(s.d_qref64 + 2 * r1, h64.data(), h64.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    BSW_TRY(tm.begin());
    BSW_TRY(launch_bai_plan(a, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_qmeta, kBiMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(h_tot, a.ref_off + opt.n_ref, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(qs.index_ms));
    if (s.h_meta[kBiErr]) return BSW_E_RANGE;
    qs.n_bins = s.h_meta[kBiBins];
    qs.n_chunks = s.h_meta[kBiChunks];
    qs.n_no_coor = s.h_meta[kBiNoCoor];
    memcpy(&qs.n_intv, s.h_meta + kBiIntv, sizeof qs.n_intv);
    *n_bytes = qs.bai_bytes = bamsort::kBaiHead + *h_tot + 8;
    if (*n_bytes > bai_cap) return BSW_E_RANGE;
    BSW_TRY(tm.begin());
    BSW_TRY(launch_bai_write(a, st));
    BSW_TRY(tm.end());
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(tm.add(qs.index_ms));
    return BSW_OK;
}

// the sort's fields and the index's fields of the last stats are those of the last call of each
static void put_bamsort_stats(bsw_ctx_t *ctx, const bsw_bamsort_stats_t &qs, bool index)
{
    std::lock_guard<std::mutex> g(ctx->stats_mu);
    bsw_bamsort_stats_t &d = ctx->bamsort_last;
    if (index) {
        d.index_ms = qs.index_ms; d.n_bins = qs.n_bins; d.n_chunks = qs.n_chunks; d.n_intv = qs.n_intv;
        d.n_no_coor = qs.n_no_coor; d.bai_bytes = qs.bai_bytes;
    } else {
        d.n_rec = qs.n_rec; d.key_bits = qs.key_bits; d.n_bytes = qs.n_bytes;
        d.key_ms = qs.key_ms; d.sort_ms = qs.sort_ms; d.copy_ms = qs.copy_ms;
    }
}

// ---------------------------------------------------------------- duplicate marking (bsw_markdup.h)
static int markdup_check_args(const bsw_ctx_t *ctx, const bsw_markdup_opt_t *opt, const void *recs, const void *rec_first,
                              int32_t n_rec, const void *aln, const void *cigar, int32_t cigar_stride, int32_t n_aln,
                              const void *read_off, const void *read_len, int32_t n_reads, int64_t quals_len, int32_t paired,
                              const void *dup)
{
    if (!ctx || !opt || opt->l_pac <= 0 || opt->l_pac > markdup::kMaxLPac || opt->min_qual < 0 || opt->flags) return BSW_E_INVAL;
    if (n_rec < 0 || n_aln < 0 || n_reads < 0 || quals_len < 0 || cigar_stride < 1 || (paired && (n_reads & 1))) return BSW_E_INVAL;
    if ((n_reads > 0 && (!rec_first || !read_off || !read_len || !dup)) || (n_rec > 0 && !recs) || (n_aln > 0 && (!aln || !cigar)))
        return BSW_E_INVAL;
    return BSW_OK;
}

static bool markdup_ctg_ok(const DeviceCtx &dc, const bsw_markdup_opt_t &opt)
{
    return dc.ctg_ok(opt.l_pac) && dc.n_ctg <= markdup::kMaxContigs;
}

// The stable sort of n members by the words of k, most significant first: perm[j] = the member at sorted place j.
// Digits come from the varying bits (k.mask) alone.  They fit one word: packed, one radix sort.  Otherwise stable LSD
// passes of the 64-bit sort, the low word first, each over its word's span of varying bits.
static int md_sort(hipStream_t st, const MdWords &k, int32_t n, uint64_t *key_a, uint64_t *key_b, int32_t *val_a,
                   int32_t *perm, void *tmp, size_t tmp_bytes, int32_t *bits, int32_t *route)
{
    int total = 0, passes = 0;
    for (int q = 0; q < k.n; ++q) {
        total += markdup::bit_count(k.mask[q]);
        passes += k.mask[q] != 0;
    }
    *bits = total;
    size_t tb = tmp_bytes;
    if (total == 0) {                               // no bit varies: the input order
        *route = BSW_MARKDUP_ROUTE_NONE;
        BSW_TRY(launch_md_gather(k.w[0], nullptr, n, key_a, perm, st));
    } else if (total <= 64) {
        *route = BSW_MARKDUP_ROUTE_ONE;
        BSW_TRY(launch_md_pack(k, n, key_a, val_a, st));
        BSW_TRY(launch_bamsort_pairs(tmp, &tb, key_a, key_b, val_a, perm, n, 0, total, st));
    } else {
        *route = BSW_MARKDUP_ROUTE_MULTI;
        int32_t *in = nullptr;
        int i = 0;
        for (int q = k.n - 1; q >= 0; --q) {
            if (!k.mask[q]) continue;
            int32_t *out = (passes - 1 - i) & 1 ? val_a : perm;     // (the last pass leaves perm)
            int lo, hi;
            markdup::mask_span(k.mask[q], &lo, &hi);
            if (!in) in = out == perm ? val_a : perm;               // the first pass: the input order
            BSW_TRY(launch_md_gather(k.w[q], i ? in : nullptr, n, key_a, in, st));
            tb = tmp_bytes;
            BSW_TRY(launch_bamsort_pairs(tmp, &tb, key_a, key_b, in, out, n, lo, hi, st));
            in = out;
            ++i;
        }
    }
    return BSW_OK;
}

struct MdIo {                           // device pointers of one call, either form
    bsw_rec_t *recs;
    const int32_t *rec_first;
    const bsw_aln_t *aln;
    const uint32_t *cigar;
    const int64_t *read_off;
    const int32_t *read_len;
    const uint8_t *quals;
    uint8_t *dup;
};

// scores -> ends, candidates, scans, keys -> ONE readback before anything of the caller's is written (error word, the
// counts, the keys' OR / NOR) -> the pair sort and the end sort -> set heads and marks -> the mark kernel -> the counters
static int markdup_device(const DeviceCtx &dc, Slot &s, hipStream_t st, const bsw_markdup_opt_t &opt, const MdIo &io,
                          int32_t n_rec, int32_t n_aln, int32_t cigar_stride, int32_t n_reads, int64_t quals_len,
                          int32_t paired, bsw_markdup_stats_t &ds)
{
    const size_t N = (size_t)n_reads, P = paired ? N / 2 : 0;
    size_t scan_bytes = 0, sort_bytes = 0;
    BSW_TRY(launch_scan32(nullptr, &scan_bytes, nullptr, nullptr, n_reads, st));
    BSW_TRY(launch_bamsort_pairs(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, n_reads, 0, 64, st));
    const size_t tmp_bytes = std::max<size_t>(std::max(scan_bytes, sort_bytes), 16);
    BSW_TRY(s.d_tmp.grow(tmp_bytes));
    BSW_TRY(s.d_dwords.grow(5 * N + 3 * P));
    BSW_TRY(s.d_dints.grow(10 * (N + 1) + 4 * (P + 1) + (N + 3) / 4));
    BSW_TRY(s.d_dmeta.grow(kMdMetaWords));
    MdArgs a{};
    a.recs = io.recs; a.rec_first = io.rec_first; a.aln = io.aln; a.cigar = io.cigar;
    a.read_off = io.read_off; a.read_len = io.read_len; a.quals = io.quals; a.dup = io.dup;
    a.quals_len = quals_len; a.l_pac = opt.l_pac;
    a.n_rec = n_rec; a.n_aln = n_aln; a.n_reads = n_reads; a.n_pairs = (int32_t)P; a.cigar_stride = cigar_stride;
    a.paired = paired != 0; a.min_qual = opt.min_qual;
    a.ctg = dc.ctg_view(opt.l_pac);
    uint64_t *w = s.d_dwords;
    a.eword = w; w += N;
    for (int q = 0; q < 3; ++q) { a.pkey[q] = w; w += P; }
    for (int q = 0; q < 2; ++q) { a.ekey[q] = w; w += N; }
    uint64_t *key_a = w, *key_b = w + N;
    int32_t *v = s.d_dints;
    a.score = v; v += N + 1;
    a.cflag = v; v += N + 1;
    a.cidx = v; v += N + 1;
    a.cid = v; v += N + 1;
    int32_t *val_a = v; v += N + 1;
    int32_t *perm_e = v; v += N + 1;
    a.hflag = v; v += N + 1;
    a.hidx = v; v += N + 1;
    a.hpos = v; v += N + 1;
    a.pflag = v; v += P + 1;
    a.pidx = v; v += P + 1;
    a.pid = v; v += P + 1;
    int32_t *perm_p = v; v += P + 1;
    a.dupr = (uint8_t *)v;                          // the tenth run of N + 1 ints is spare
    a.meta = s.d_dmeta;
    HelperTimer t_score, t_key, t_sort, t_mark;     // one event pair of the slot each
    BSW_TRY(t_score.init(s.ev0, s.ev1, st));
    BSW_TRY(t_key.init(s.ev2, s.ev3, st));
    BSW_TRY(t_sort.init(s.evw0, s.evw1, st));
    BSW_TRY(t_mark.init(s.evq0, s.evq1, st));
    static_assert(kMdMetaWords + 2 <= kMetaWords, "the slot's pinned mirror holds the meta words and the two counts");
    BSW_TRY(hipMemsetAsync(s.d_dmeta, 0, kMdMetaWords * sizeof(int32_t), st));
    BSW_TRY(hipMemsetAsync(a.dupr, 0, N, st));
    BSW_TRY(t_score.begin());
    BSW_TRY(launch_md_scores(a, st));
    BSW_TRY(t_score.end());
    BSW_TRY(t_key.begin());
    BSW_TRY(launch_md_ends(a, st));
    size_t tb = tmp_bytes;
    BSW_TRY(launch_scan32(s.d_tmp, &tb, a.cflag, a.cidx, n_reads, st));
    if (P) {
        tb = tmp_bytes;
        BSW_TRY(launch_scan32(s.d_tmp, &tb, a.pflag, a.pidx, (int32_t)P, st));
    }
    BSW_TRY(launch_md_keys(a, st));
    BSW_TRY(t_key.end());
    s.h_meta[kMdMetaWords + 1] = 0;
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_dmeta, kMdMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipMemcpyAsync(s.h_meta + kMdMetaWords, a.cidx + N, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (P) BSW_TRY(hipMemcpyAsync(s.h_meta + kMdMetaWords + 1, a.pidx + P, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(t_score.add(ds.score_ms));
    BSW_TRY(t_key.add(ds.key_ms));
    if (s.h_meta[kMdErr]) return BSW_E_RANGE;
    const int32_t n_cand = s.h_meta[kMdMetaWords], n_pc = s.h_meta[kMdMetaWords + 1];
    ds.n_cand = n_cand;
    ds.n_pair_cand = n_pc;
    auto words = [&](uint64_t *const *arr, int n, int at_or, int at_nor) {
        MdWords k{};
        k.n = n;
        for (int q = 0; q < n; ++q) {
            uint64_t or_, nor_;
            memcpy(&or_, s.h_meta + at_or + 2 * q, sizeof or_);
            memcpy(&nor_, s.h_meta + at_nor + 2 * q, sizeof nor_);
            k.w[q] = arr[q];
            k.mask[q] = or_ & nor_;
        }
        return k;
    };
    MdWords kp = words(a.pkey, 3, kMdOrPair, kMdNorPair), ke = words(a.ekey, 2, kMdOrEnd, kMdNorEnd);
    BSW_TRY(t_sort.begin());
    if (n_pc > 0)
        if (const int r = md_sort(st, kp, n_pc, key_a, key_b, val_a, perm_p, s.d_tmp, tmp_bytes, &ds.pair_key_bits, &ds.pair_route))
            return r;
    if (n_cand > 0)
        if (const int r = md_sort(st, ke, n_cand, key_a, key_b, val_a, perm_e, s.d_tmp, tmp_bytes, &ds.end_key_bits, &ds.end_route))
            return r;
    BSW_TRY(t_sort.end());
    BSW_TRY(t_mark.begin());
    if (n_pc > 0) {
        kp.n = 2;                                   // a set: equal ends, whatever the score
        BSW_TRY(launch_md_heads(kp, perm_p, n_pc, a.hflag, st));
        BSW_TRY(launch_md_pair_marks(a, perm_p, n_pc, st));
    }
    if (n_cand > 0) {
        ke.n = 1;
        BSW_TRY(launch_md_heads(ke, perm_e, n_cand, a.hflag, st));
        tb = tmp_bytes;
        BSW_TRY(launch_scan32(s.d_tmp, &tb, a.hflag, a.hidx, n_cand, st));
        BSW_TRY(launch_md_end_marks(a, perm_e, n_cand, st));
    }
    BSW_TRY(launch_md_mark(a, st));
    BSW_TRY(t_mark.end());
    BSW_TRY(hipMemcpyAsync(s.h_meta, s.d_dmeta, kMdMetaWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BSW_TRY(hipStreamSynchronize(st));
    BSW_TRY(t_sort.add(ds.sort_ms));
    BSW_TRY(t_mark.add(ds.mark_ms));
    ds.n_dup_pairs = s.h_meta[kMdDupPairs];
    ds.n_dup_frag = s.h_meta[kMdDupFrag];
    ds.n_dup_frag_by_pair = s.h_meta[kMdDupFragByPair];
    ds.n_pair_sets = s.h_meta[kMdPairSets];
    ds.n_end_sets = s.h_meta[kMdEndSets];
    ds.n_flagged = s.h_meta[kMdFlagged];
    return BSW_OK;
}

}  // namespace bsw

extern "C" {

void bsw_rec_opt_default(bsw_rec_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->w = 100;
    opt->T = 30;
    opt->max_XA_hits = 5;
    opt->XA_drop_ratio = 0.8f;
    opt->mask_level = 0.5f;
}

int bsw_records_resident(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const uint8_t *d_reads,
                         const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                         const bsw_alnreg_t *d_sel_regs, const bsw_selinfo_t *d_sel_info,
                         const int32_t *d_read_first, int32_t n_regs, const bsw_pair_t *d_pairs,
                         bsw_rec_t *d_recs, int32_t *d_rec_first, int32_t rec_cap, bsw_aln_t *d_aln,
                         int32_t *d_aln_reg, uint32_t *d_cigar, int32_t cigar_stride, uint8_t *d_md,
                         int32_t md_stride, int32_t aln_cap, int32_t *n_rec, int32_t *n_aln, void *stream)
{
    if (const int rc = bsw::records_check_args(opt, n_reads, n_regs, d_pairs != nullptr, cigar_stride, md_stride, rec_cap,
                                               aln_cap))
        return rc;
    if (!ctx || !n_rec || !n_aln || !d_read_first || !d_rec_first ||
        (n_reads > 0 && (!d_reads || !d_read_off || !d_read_len)) || (n_regs > 0 && (!d_sel_regs || !d_sel_info)) ||
        (rec_cap > 0 && !d_recs) || (aln_cap > 0 && (!d_aln || !d_aln_reg || !d_cigar || !d_md)))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the resident reference stays put
    if (!bsw::ref_ok(dc, opt->l_pac)) return BSW_E_INVAL;
    bsw_rec_stats_t rs{};
    const bsw::RecIo io = {d_reads, d_read_off, d_read_len, {d_sel_regs, d_sel_info, d_read_first, d_pairs},
                           d_recs, d_rec_first, d_aln, d_aln_reg, d_cigar, d_md};
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::records_device(ctx, dc, s, st, *opt, io, n_reads, n_regs, cigar_stride, md_stride, rec_cap, aln_cap,
                                   n_rec, n_aln, rs);
    });
    if (rc != BSW_OK && !(rc == BSW_E_RANGE && rs.n_overflow)) return rc;
    bsw::put_stats(ctx, &bsw_ctx::rec_last, rs);        // (a stride overflow leaves its count in the stats)
    return rc;
}

int bsw_records(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const uint8_t *reads, const int64_t *read_off,
                const int32_t *read_len, int32_t n_reads, const bsw_alnreg_t *sel_regs,
                const bsw_selinfo_t *sel_info, const int32_t *read_first, const bsw_pair_t *pairs,
                bsw_rec_t *recs, int32_t *rec_first, int32_t rec_cap, bsw_aln_t *aln, int32_t *aln_reg,
                uint32_t *cigar, int32_t cigar_stride, uint8_t *md, int32_t md_stride, int32_t aln_cap,
                int32_t *n_rec, int32_t *n_aln)
{
    if (const int rc = bsw::records_check_args(opt, n_reads, 0, pairs != nullptr, cigar_stride, md_stride, rec_cap, aln_cap))
        return rc;
    if (!ctx || !n_rec || !n_aln || !rec_first || (n_reads > 0 && (!reads || !read_off || !read_len)) ||
        (rec_cap > 0 && !recs) || (aln_cap > 0 && (!aln || !aln_reg || !cigar || !md)))
        return BSW_E_INVAL;
    int32_t n_regs = 0;
    if (const int rc = bsw::pe_host_first(read_first, n_reads, n_regs)) return rc;
    if (n_regs > 0 && (!sel_regs || !sel_info)) return BSW_E_INVAL;
    int64_t rbytes;
    if (const int rc = bsw::reads_extent(read_off, read_len, n_reads, &rbytes)) return rc;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (!bsw::ref_ok(dc, opt->l_pac)) return BSW_E_INVAL;
    bsw_rec_stats_t rs{};
    const size_t nr = (size_t)n_reads, ng = (size_t)n_regs, nc = (size_t)rec_cap, na = (size_t)aln_cap;
    bsw::StagedIo io;
    const auto d_reads = io.in(reads, (size_t)rbytes);
    const auto d_read_off = io.in(read_off, nr);
    const auto d_read_len = io.in(read_len, nr);
    const auto d_sel_regs = io.in(sel_regs, ng);
    const auto d_sel_info = io.in(sel_info, ng);
    const auto d_read_first = io.in(read_first, nr + 1);
    const auto d_pairs = io.in_opt(pairs, nr / 2);
    const auto d_recs = io.out(recs, nc);
    const auto d_rec_first = io.out(rec_first, nr + 1);
    const auto d_aln = io.out(aln, na);
    const auto d_aln_reg = io.out(aln_reg, na);
    const auto d_cigar = io.out(cigar, na * (size_t)cigar_stride);
    const auto d_md = io.out(md, na * (size_t)md_stride);
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.grow(s));
        // (what the alignment kernels leave unwritten past a CIGAR or an MD reads back as zeros: cigar and
        // md, the blob's last two parts)
        BSW_TRY(hipMemsetAsync(d_cigar, 0, io.bytes_from(d_cigar), s.stream));
        BSW_TRY(io.upload());
        const bsw::RecIo dio = {d_reads, d_read_off, d_read_len, {d_sel_regs, d_sel_info, d_read_first, d_pairs},
                                d_recs, d_rec_first, d_aln, d_aln_reg, d_cigar, d_md};
        const int r = bsw::records_device(ctx, dc, s, s.stream, *opt, dio, n_reads, n_regs, cigar_stride, md_stride,
                                          rec_cap, aln_cap, n_rec, n_aln, rs);
        if (r == BSW_E_RANGE && (*n_rec > rec_cap || *n_aln > aln_cap)) {   // (d_rec_first is still written)
            BSW_TRY(io.back(d_rec_first));
            BSW_TRY(hipStreamSynchronize(s.stream));
        }
        if (r) return r;
        BSW_TRY(io.back(d_recs, (size_t)*n_rec));           // (the rows written, not the capacities)
        BSW_TRY(io.back(d_rec_first));
        BSW_TRY(io.back(d_aln, (size_t)*n_aln));
        BSW_TRY(io.back(d_aln_reg, (size_t)*n_aln));
        BSW_TRY(io.back(d_cigar, (size_t)*n_aln * (size_t)cigar_stride));
        BSW_TRY(io.back(d_md, (size_t)*n_aln * (size_t)md_stride));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc != BSW_OK && !(rc == BSW_E_RANGE && rs.n_overflow)) return rc;
    bsw::put_stats(ctx, &bsw_ctx::rec_last, rs);
    return rc;
}

// call 2 in either form, every array in HBM
static int rec_out_resident(bsw::RecForm form, bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *d_recs,
                            const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                            const uint32_t *d_cigar, int32_t cigar_stride, const uint8_t *d_md, int32_t md_stride,
                            int32_t n_aln, const uint8_t *d_reads, const int64_t *d_read_off,
                            const int32_t *d_read_len, int32_t n_reads, const uint8_t *d_names,
                            const int64_t *d_name_off, const uint8_t *d_quals, int32_t paired, uint8_t *d_out,
                            int64_t *d_out_off, int64_t out_cap, int64_t *n_bytes, void *stream)
{
    if (const int rc = bsw::rec_out_check_args(opt, n_rec, n_aln, n_reads, paired, cigar_stride, md_stride, out_cap))
        return rc;
    if (!ctx || !n_bytes || !d_out_off || !d_name_off || (n_rec > 0 && (!d_recs || !d_rec_first)) ||
        (n_aln > 0 && (!d_aln || !d_cigar || !d_md)) || (n_reads > 0 && (!d_reads || !d_read_off || !d_read_len || !d_names)) ||
        (out_cap > 0 && !d_out) || ((uintptr_t)d_out & 3))
        return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the contig table stays put
    if (!bsw::text_ctg_ok(dc, *opt)) return BSW_E_INVAL;
    bsw::RecText t{};
    t.recs = d_recs; t.rec_first = d_rec_first; t.aln = d_aln; t.cigar = d_cigar; t.md = d_md;
    t.reads = d_reads; t.names = d_names; t.quals = d_quals;
    t.read_off = d_read_off; t.name_off = d_name_off; t.read_len = d_read_len;
    bsw::make_rec_text(dc, *opt, n_rec, n_aln, n_reads, paired, cigar_stride, md_stride, t);
    float len_ms = 0.f, write_ms = 0.f;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::rec_out_device(form, s, st, *opt, t, {d_out, d_out_off}, out_cap, n_bytes, len_ms, write_ms);
    });
    if (rc) return rc;
    bsw::put_out_stats(form, ctx, n_rec, *n_bytes, len_ms, write_ms);
    return BSW_OK;
}

// the same with host arrays
static int rec_out_host(bsw::RecForm form, bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *recs,
                        const int32_t *rec_first, int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar,
                        int32_t cigar_stride, const uint8_t *md, int32_t md_stride, int32_t n_aln, const uint8_t *reads,
                        const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const uint8_t *names,
                        const int64_t *name_off, const uint8_t *quals, int32_t paired, uint8_t *out, int64_t *out_off,
                        int64_t out_cap, int64_t *n_bytes)
{
    if (const int rc = bsw::rec_out_check_args(opt, n_rec, n_aln, n_reads, paired, cigar_stride, md_stride, out_cap))
        return rc;
    if (!ctx || !n_bytes || !out_off || !name_off || (n_rec > 0 && (!recs || !rec_first)) ||
        (n_aln > 0 && (!aln || !cigar || !md)) || (n_reads > 0 && (!reads || !read_off || !read_len || !names)) ||
        (out_cap > 0 && !out))
        return BSW_E_INVAL;
    int64_t rbytes;
    if (const int rc = bsw::reads_extent(read_off, read_len, n_reads, &rbytes)) return rc;
    const size_t nn = (size_t)(paired ? n_reads / 2 : n_reads);
    for (size_t i = 0; i < nn; ++i)
        if (name_off[i] < 0 || name_off[i + 1] < name_off[i]) return BSW_E_RANGE;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (!bsw::text_ctg_ok(dc, *opt)) return BSW_E_INVAL;
    const size_t nr = (size_t)n_reads, nc = (size_t)n_rec, na = (size_t)n_aln;
    bsw::StagedIo io;
    const auto d_recs = io.in(recs, nc);
    const auto d_rec_first = io.in(rec_first, n_rec > 0 ? nr + 1 : 0);
    const auto d_aln = io.in(aln, na);
    const auto d_cigar = io.in(cigar, na * (size_t)cigar_stride);
    const auto d_md = io.in(md, na * (size_t)md_stride);
    const auto d_reads = io.in(reads, (size_t)rbytes);
    const auto d_read_off = io.in(read_off, nr);
    const auto d_read_len = io.in(read_len, nr);
    const auto d_names = io.in(names, (size_t)name_off[nn]);
    const auto d_name_off = io.in(name_off, nn + 1);
    const auto d_quals = io.in_opt(quals, (size_t)rbytes);
    const auto d_out = io.out(out, (size_t)out_cap);
    const auto d_out_off = io.out(out_off, nc + 1);
    bsw::RecText t{};
    bsw::make_rec_text(dc, *opt, n_rec, n_aln, n_reads, paired, cigar_stride, md_stride, t);
    float len_ms = 0.f, write_ms = 0.f;
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        t.recs = d_recs; t.rec_first = d_rec_first; t.aln = d_aln; t.cigar = d_cigar; t.md = d_md;
        t.reads = d_reads; t.names = d_names; t.quals = d_quals;
        t.read_off = d_read_off; t.name_off = d_name_off; t.read_len = d_read_len;
        const int r = bsw::rec_out_device(form, s, s.stream, *opt, t, {d_out, d_out_off}, out_cap, n_bytes, len_ms,
                                          write_ms);
        if (r == BSW_E_RANGE && *n_bytes > out_cap) {      // (d_out_off is still written)
            BSW_TRY(io.back(d_out_off));
            BSW_TRY(hipStreamSynchronize(s.stream));
        }
        if (r) return r;
        BSW_TRY(io.back(d_out, (size_t)*n_bytes));
        BSW_TRY(io.back(d_out_off));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::put_out_stats(form, ctx, n_rec, *n_bytes, len_ms, write_ms);
    return BSW_OK;
}

int bsw_sam_text_resident(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *d_recs,
                          const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                          const uint32_t *d_cigar, int32_t cigar_stride, const uint8_t *d_md, int32_t md_stride,
                          int32_t n_aln, const uint8_t *d_reads, const int64_t *d_read_off,
                          const int32_t *d_read_len, int32_t n_reads, const uint8_t *d_names,
                          const int64_t *d_name_off, const uint8_t *d_quals, int32_t paired, uint8_t *d_text,
                          int64_t *d_text_off, int64_t text_cap, int64_t *n_bytes, void *stream)
{
    return rec_out_resident(bsw::RecForm::Text, ctx, opt, d_recs, d_rec_first, n_rec, d_aln, d_cigar, cigar_stride, d_md,
                            md_stride, n_aln, d_reads, d_read_off, d_read_len, n_reads, d_names, d_name_off, d_quals, paired,
                            d_text, d_text_off, text_cap, n_bytes, stream);
}

int bsw_sam_text(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *recs, const int32_t *rec_first,
                 int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                 const uint8_t *md, int32_t md_stride, int32_t n_aln, const uint8_t *reads,
                 const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const uint8_t *names,
                 const int64_t *name_off, const uint8_t *quals, int32_t paired, uint8_t *text, int64_t *text_off,
                 int64_t text_cap, int64_t *n_bytes)
{
    return rec_out_host(bsw::RecForm::Text, ctx, opt, recs, rec_first, n_rec, aln, cigar, cigar_stride, md, md_stride, n_aln,
                        reads, read_off, read_len, n_reads, names, name_off, quals, paired, text, text_off, text_cap, n_bytes);
}

int bsw_rec_last_stats(bsw_ctx_t *ctx, bsw_rec_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::rec_last, out); }

// ---------------------------------------------------------------- BAM (include/bsw_bam.h)
int bsw_bam_records_resident(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *d_recs,
                             const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                             const uint32_t *d_cigar, int32_t cigar_stride, const uint8_t *d_md, int32_t md_stride,
                             int32_t n_aln, const uint8_t *d_reads, const int64_t *d_read_off,
                             const int32_t *d_read_len, int32_t n_reads, const uint8_t *d_names,
                             const int64_t *d_name_off, const uint8_t *d_quals, int32_t paired, uint8_t *d_bam,
                             int64_t *d_bam_off, int64_t bam_cap, int64_t *n_bytes, void *stream)
{
    return rec_out_resident(bsw::RecForm::Bam, ctx, opt, d_recs, d_rec_first, n_rec, d_aln, d_cigar, cigar_stride, d_md,
                            md_stride, n_aln, d_reads, d_read_off, d_read_len, n_reads, d_names, d_name_off, d_quals, paired,
                            d_bam, d_bam_off, bam_cap, n_bytes, stream);
}

int bsw_bam_records(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const bsw_rec_t *recs, const int32_t *rec_first,
                    int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                    const uint8_t *md, int32_t md_stride, int32_t n_aln, const uint8_t *reads,
                    const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const uint8_t *names,
                    const int64_t *name_off, const uint8_t *quals, int32_t paired, uint8_t *bam, int64_t *bam_off,
                    int64_t bam_cap, int64_t *n_bytes)
{
    return rec_out_host(bsw::RecForm::Bam, ctx, opt, recs, rec_first, n_rec, aln, cigar, cigar_stride, md, md_stride, n_aln,
                        reads, read_off, read_len, n_reads, names, name_off, quals, paired, bam, bam_off, bam_cap, n_bytes);
}

int bsw_bam_header(bsw_ctx_t *ctx, const bsw_rec_opt_t *opt, const char *sam_text, int32_t l_text, uint8_t *out,
                   int64_t cap, int64_t *n_bytes)
{
    if (const int rc = bsw::rec_check_opt(opt)) return rc;
    if (!ctx || !n_bytes || l_text < 0 || cap < 0 || (l_text > 0 && !sam_text) || (cap > 0 && !out)) return BSW_E_INVAL;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the contig table stays put
    if (!bsw::text_ctg_ok(dc, *opt)) return BSW_E_INVAL;
    const int32_t n_ref = dc.n_ctg > 0 ? dc.n_ctg : 1;
    // one reference: its name's bytes and its length
    auto ref = [&](int32_t k, const uint8_t *&name, int32_t &l_name, int64_t &l_ref) {
        if (dc.n_ctg > 0) {
            name = dc.h_ctg_names.data() + dc.h_ctg_name_off[k];
            l_name = dc.h_ctg_name_off[k + 1] - dc.h_ctg_name_off[k];
            l_ref = dc.h_ctg_off[k + 1] - dc.h_ctg_off[k];
        } else {
            name = (const uint8_t *)opt->rname;
            l_name = (int32_t)strnlen(opt->rname, sizeof(opt->rname));
            l_ref = opt->l_pac;
        }
    };
    int64_t need = 4 + 4 + (int64_t)l_text + 4;
    for (int32_t k = 0; k < n_ref; ++k) {
        const uint8_t *name;
        int32_t l_name;
        int64_t l_ref;
        ref(k, name, l_name, l_ref);
        if (l_ref > INT32_MAX) return BSW_E_RANGE;
        need += 4 + l_name + 1 + 4;
    }
    *n_bytes = need;
    if (cap < need) return BSW_E_RANGE;
    uint8_t *w = out;
    auto put32 = [&](int32_t v) {
        for (int b = 0; b < 4; ++b) *w++ = (uint8_t)((uint32_t)v >> (8 * b));
    };
    memcpy(w, "BAM\1", 4);
    w += 4;
    put32(l_text);
    if (l_text) memcpy(w, sam_text, (size_t)l_text);
    w += l_text;
    put32(n_ref);
    for (int32_t k = 0; k < n_ref; ++k) {
        const uint8_t *name;
        int32_t l_name;
        int64_t l_ref;
        ref(k, name, l_name, l_ref);
        put32(l_name + 1);
        memcpy(w, name, (size_t)l_name);
        w += l_name;
        *w++ = 0;
        put32((int32_t)l_ref);
    }
    return BSW_OK;
}

int bsw_bam_last_stats(bsw_ctx_t *ctx, bsw_bam_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::bam_last, out); }

// ---------------------------------------------------------------- BGZF (include/bsw_bgzf.h)
void bsw_bgzf_opt_default(bsw_bgzf_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->level = 1;
    opt->block_bytes = BSW_BGZF_MAX_BLOCK;
}

int bsw_bgzf_resident(bsw_ctx_t *ctx, const bsw_bgzf_opt_t *opt, const uint8_t *d_in, int64_t n_in,
                      const int64_t *d_rec_off, int32_t n_rec, uint8_t *d_out, int64_t out_cap, int64_t *d_blk_off,
                      int32_t blk_cap, int64_t *d_voff, int32_t *n_blocks, int64_t *n_bytes, void *stream)
{
    if (const int rc = bsw::bgzf_check_args(opt, n_in, n_rec, out_cap, blk_cap)) return rc;
    if (!ctx || !n_blocks || !n_bytes || !d_blk_off || (n_in > 0 && !d_in) || (out_cap > 0 && !d_out) ||
        (n_rec > 0 && (!d_rec_off || !d_voff)) || ((uintptr_t)d_out & 3))
        return BSW_E_INVAL;
    bsw_bgzf_stats_t bs{};
    bs.n_in = n_in;
    *n_blocks = bs.n_blocks = (int32_t)((n_in + opt->block_bytes - 1) / opt->block_bytes);
    *n_bytes = 0;
    if (blk_cap < bs.n_blocks + 1) return BSW_E_RANGE;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::bgzf_device(s, st, *opt, d_in, d_rec_off, n_rec, d_out, out_cap, d_blk_off, d_voff, n_bytes, bs);
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::bgzf_last, bs);
    return BSW_OK;
}

int bsw_bgzf(bsw_ctx_t *ctx, const bsw_bgzf_opt_t *opt, const uint8_t *in, int64_t n_in, const int64_t *rec_off,
             int32_t n_rec, uint8_t *out, int64_t out_cap, int64_t *blk_off, int32_t blk_cap, int64_t *voff,
             int32_t *n_blocks, int64_t *n_bytes)
{
    if (const int rc = bsw::bgzf_check_args(opt, n_in, n_rec, out_cap, blk_cap)) return rc;
    if (!ctx || !n_blocks || !n_bytes || !blk_off || (n_in > 0 && !in) || (out_cap > 0 && !out) ||
        (n_rec > 0 && (!rec_off || !voff)))
        return BSW_E_INVAL;
    bsw_bgzf_stats_t bs{};
    bs.n_in = n_in;
    *n_blocks = bs.n_blocks = (int32_t)((n_in + opt->block_bytes - 1) / opt->block_bytes);
    *n_bytes = 0;
    if (blk_cap < bs.n_blocks + 1) return BSW_E_RANGE;
    const size_t nb1 = (size_t)bs.n_blocks + 1, nr = (size_t)n_rec;
    bsw::StagedIo io;
    const auto d_in = io.in(in, (size_t)n_in);
    const auto d_rec_off = io.in(rec_off, nr ? nr + 1 : 0);
    const auto d_out = io.out(out, (size_t)out_cap);
    const auto d_blk_off = io.out(blk_off, nb1);
    const auto d_voff = io.out(voff, nr);
    bsw::DeviceCtx &dc = *ctx->devs[0];
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        const int r = bsw::bgzf_device(s, s.stream, *opt, d_in, d_rec_off, n_rec, d_out, out_cap, d_blk_off, d_voff, n_bytes,
                                       bs);
        if (r == BSW_E_RANGE && *n_bytes > out_cap) {       // (the block starts and the offsets are still written)
            BSW_TRY(io.back(d_blk_off));
            BSW_TRY(io.back(d_voff));
            BSW_TRY(hipStreamSynchronize(s.stream));
        }
        if (r) return r;
        BSW_TRY(io.back(d_out, (size_t)*n_bytes));
        BSW_TRY(io.back(d_blk_off));
        BSW_TRY(io.back(d_voff));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::put_stats(ctx, &bsw_ctx::bgzf_last, bs);
    return BSW_OK;
}

int bsw_bgzf_last_stats(bsw_ctx_t *ctx, bsw_bgzf_stats_t *out) { return bsw::get_stats(ctx, &bsw_ctx::bgzf_last, out); }

// ---------------------------------------------------------------- BAM sort and index (include/bsw_bamsort.h)
int bsw_bam_sort_resident(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const uint8_t *d_bam,
                          const int64_t *d_bam_off, int32_t n_rec, uint8_t *d_out, int64_t out_cap,
                          int64_t *d_out_off, int32_t *d_perm, void *stream)
{
    if (const int rc = bsw::bamsort_check_opt(opt)) return rc;
    if (!ctx || n_rec < 0 || out_cap < 0 || (out_cap > 0 && !d_out) || ((uintptr_t)d_out & 3) ||
        (n_rec > 0 && (!d_bam || !d_bam_off || !d_out_off || !d_perm)))
        return BSW_E_INVAL;
    if (n_rec > 0 && bsw::ranges_overlap(d_bam, 1, d_out, out_cap)) return BSW_E_INVAL;
    bsw_bamsort_stats_t qs{};
    qs.n_rec = n_rec;
    if (n_rec > 0) {
        bsw::DeviceCtx &dc = *ctx->devs[0];
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            hipStream_t st = stream ? (hipStream_t)stream : s.stream;
            return bsw::bam_sort_device(s, st, *opt, d_bam, d_bam_off, n_rec, d_out, out_cap, d_out_off, d_perm, qs);
        });
        if (rc) return rc;
    }
    bsw::put_bamsort_stats(ctx, qs, false);
    return BSW_OK;
}

int bsw_bam_sort(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const uint8_t *bam, const int64_t *bam_off,
                 int32_t n_rec, uint8_t *out, int64_t out_cap, int64_t *out_off, int32_t *perm)
{
    if (const int rc = bsw::bamsort_check_opt(opt)) return rc;
    if (!ctx || n_rec < 0 || out_cap < 0 || (out_cap > 0 && !out) ||
        (n_rec > 0 && (!bam || !bam_off || !out_off || !perm)))
        return BSW_E_INVAL;
    bsw_bamsort_stats_t qs{};
    qs.n_rec = n_rec;
    if (n_rec > 0) {
        const int64_t n_bytes = bam_off[n_rec];
        if (n_bytes < 0 || n_bytes > out_cap) return BSW_E_RANGE;
        if (bsw::ranges_overlap(bam, n_bytes, out, n_bytes)) return BSW_E_INVAL;
        const size_t nr = (size_t)n_rec;
        bsw::StagedIo io;
        const auto d_bam = io.in(bam, (size_t)n_bytes);
        const auto d_bam_off = io.in(bam_off, nr + 1);
        const auto d_out = io.out(out, (size_t)n_bytes);
        const auto d_out_off = io.out(out_off, nr + 1);
        const auto d_perm = io.out(perm, nr);
        bsw::DeviceCtx &dc = *ctx->devs[0];
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            BSW_TRY(io.stage(s));
            if (const int r = bsw::bam_sort_device(s, s.stream, *opt, d_bam, d_bam_off, n_rec, d_out, n_bytes, d_out_off,
                                                   d_perm, qs))
                return r;
            BSW_TRY(io.back(d_out));
            BSW_TRY(io.back(d_out_off));
            BSW_TRY(io.back(d_perm));
            BSW_TRY(hipStreamSynchronize(s.stream));
            return BSW_OK;
        });
        if (rc) return rc;
    }
    bsw::put_bamsort_stats(ctx, qs, false);
    return BSW_OK;
}

static int bam_index_check(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const int32_t *ref_len, const void *bam,
                           const void *bam_off, int32_t n_rec, const void *voff, int64_t end_voff, const void *bai,
                           int64_t bai_cap, const int64_t *n_bytes)
{
    if (const int rc = bsw::bamsort_check_opt(opt)) return rc;
    if (!ctx || !ref_len || !n_bytes || n_rec < 0 || bai_cap < 0 || end_voff < 0 || (bai_cap > 0 && !bai) ||
        (n_rec > 0 && (!bam || !bam_off || !voff)))
        return BSW_E_INVAL;
    return BSW_OK;
}

int bsw_bam_index_resident(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const int32_t *ref_len, const uint8_t *d_bam,
                           const int64_t *d_bam_off, int32_t n_rec, const int64_t *d_voff, int64_t end_voff,
                           uint8_t *d_bai, int64_t bai_cap, int64_t *n_bytes, void *stream)
{
    if (const int rc = bam_index_check(ctx, opt, ref_len, d_bam, d_bam_off, n_rec, d_voff, end_voff, d_bai, bai_cap, n_bytes))
        return rc;
    if ((uintptr_t)d_bai & 3) return BSW_E_INVAL;
    *n_bytes = 0;
    std::vector<int64_t> h64;
    if (const int rc = bsw::bai_windows(*opt, ref_len, h64)) return rc;
    bsw_bamsort_stats_t qs{};
    bsw::DeviceCtx &dc = *ctx->devs[0];
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        hipStream_t st = stream ? (hipStream_t)stream : s.stream;
        return bsw::bam_index_device(s, st, *opt, h64, d_bam, d_bam_off, n_rec, d_voff, end_voff, d_bai, bai_cap, n_bytes, qs);
    });
    if (rc) return rc;
    bsw::put_bamsort_stats(ctx, qs, true);
    return BSW_OK;
}

int bsw_bam_index(bsw_ctx_t *ctx, const bsw_bamsort_opt_t *opt, const int32_t *ref_len, const uint8_t *bam,
                  const int64_t *bam_off, int32_t n_rec, const int64_t *voff, int64_t end_voff, uint8_t *bai,
                  int64_t bai_cap, int64_t *n_bytes)
{
    if (const int rc = bam_index_check(ctx, opt, ref_len, bam, bam_off, n_rec, voff, end_voff, bai, bai_cap, n_bytes))
        return rc;
    *n_bytes = 0;
    std::vector<int64_t> h64;
    if (const int rc = bsw::bai_windows(*opt, ref_len, h64)) return rc;
    const int64_t bam_bytes = n_rec > 0 ? bam_off[n_rec] : 0;
    if (bam_bytes < 0) return BSW_E_RANGE;
    const size_t nr = (size_t)n_rec;
    bsw::StagedIo io;
    const auto d_bam = io.in(bam, (size_t)bam_bytes);
    const auto d_bam_off = io.in(bam_off, nr ? nr + 1 : 0);
    const auto d_voff = io.in(voff, nr);
    const auto d_bai = io.out(bai, (size_t)bai_cap);
    bsw_bamsort_stats_t qs{};
    bsw::DeviceCtx &dc = *ctx->devs[0];
    const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
        BSW_TRY(io.stage(s));
        if (const int r = bsw::bam_index_device(s, s.stream, *opt, h64, d_bam, d_bam_off, n_rec, d_voff, end_voff, d_bai,
                                                bai_cap, n_bytes, qs))
            return r;
        BSW_TRY(io.back(d_bai, (size_t)*n_bytes));
        BSW_TRY(hipStreamSynchronize(s.stream));
        return BSW_OK;
    });
    if (rc) return rc;
    bsw::put_bamsort_stats(ctx, qs, true);
    return BSW_OK;
}

int bsw_bamsort_last_stats(bsw_ctx_t *ctx, bsw_bamsort_stats_t *out)
{
    return bsw::get_stats(ctx, &bsw_ctx::bamsort_last, out);
}

// ---------------------------------------------------------------- duplicate marking (include/bsw_markdup.h)
void bsw_markdup_opt_default(bsw_markdup_opt_t *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->min_qual = 15;
}

int bsw_mark_duplicates_resident(bsw_ctx_t *ctx, const bsw_markdup_opt_t *opt, bsw_rec_t *d_recs,
                                 const int32_t *d_rec_first, int32_t n_rec, const bsw_aln_t *d_aln,
                                 const uint32_t *d_cigar, int32_t cigar_stride, int32_t n_aln,
                                 const int64_t *d_read_off, const int32_t *d_read_len, int32_t n_reads,
                                 const uint8_t *d_quals, int64_t quals_len, int32_t paired, uint8_t *d_dup, void *stream)
{
    if (const int rc = bsw::markdup_check_args(ctx, opt, d_recs, d_rec_first, n_rec, d_aln, d_cigar, cigar_stride, n_aln,
                                               d_read_off, d_read_len, n_reads, quals_len, paired, d_dup))
        return rc;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);   // the contig table stays put
    if (!bsw::markdup_ctg_ok(dc, *opt)) return BSW_E_INVAL;
    bsw_markdup_stats_t ds{};
    ds.n_reads = n_reads;
    if (n_reads > 0) {
        const bsw::MdIo io{d_recs, d_rec_first, d_aln, d_cigar, d_read_off, d_read_len, d_quals, d_dup};
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            hipStream_t st = stream ? (hipStream_t)stream : s.stream;
            return bsw::markdup_device(dc, s, st, *opt, io, n_rec, n_aln, cigar_stride, n_reads, quals_len, paired, ds);
        });
        if (rc) return rc;
    }
    bsw::put_stats(ctx, &bsw_ctx::markdup_last, ds);
    return BSW_OK;
}

int bsw_mark_duplicates(bsw_ctx_t *ctx, const bsw_markdup_opt_t *opt, bsw_rec_t *recs, const int32_t *rec_first,
                        int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride, int32_t n_aln,
                        const int64_t *read_off, const int32_t *read_len, int32_t n_reads, const uint8_t *quals,
                        int64_t quals_len, int32_t paired, uint8_t *dup)
{
    if (const int rc = bsw::markdup_check_args(ctx, opt, recs, rec_first, n_rec, aln, cigar, cigar_stride, n_aln, read_off,
                                               read_len, n_reads, quals_len, paired, dup))
        return rc;
    bsw::DeviceCtx &dc = *ctx->devs[0];
    std::shared_lock<std::shared_mutex> refg(dc.refmu);
    if (!bsw::markdup_ctg_ok(dc, *opt)) return BSW_E_INVAL;
    bsw_markdup_stats_t ds{};
    ds.n_reads = n_reads;
    if (n_reads > 0) {
        const size_t nr = (size_t)n_reads, nc = (size_t)n_rec, na = (size_t)n_aln;
        bsw::StagedIo io;
        const auto d_recs = io.inout(recs, nc);
        const auto d_rec_first = io.in(rec_first, nr + 1);
        const auto d_aln = io.in(aln, na);
        const auto d_cigar = io.in(cigar, na * (size_t)cigar_stride);
        const auto d_read_off = io.in(read_off, nr);
        const auto d_read_len = io.in(read_len, nr);
        const auto d_quals = io.in_opt(quals, (size_t)quals_len);
        const auto d_dup = io.out(dup, nr);
        const int rc = bsw::with_slot(dc, [&](bsw::Slot &s) -> int {
            BSW_TRY(io.stage(s));
            const bsw::MdIo m{d_recs, d_rec_first, d_aln, d_cigar, d_read_off, d_read_len, d_quals, d_dup};
            if (const int r = bsw::markdup_device(dc, s, s.stream, *opt, m, n_rec, n_aln, cigar_stride, n_reads, quals_len,
                                                  paired, ds))
                return r;
            BSW_TRY(io.back(d_recs));
            BSW_TRY(io.back(d_dup));
            BSW_TRY(hipStreamSynchronize(s.stream));
            return BSW_OK;
        });
        if (rc) return rc;
    }
    bsw::put_stats(ctx, &bsw_ctx::markdup_last, ds);
    return BSW_OK;
}

int bsw_markdup_last_stats(bsw_ctx_t *ctx, bsw_markdup_stats_t *out)
{
    return bsw::get_stats(ctx, &bsw_ctx::markdup_last, out);
}

}  // extern "C"
