// bsw_rec.hip -- kernels of the record stage (include/bsw_rec.h; launch interface bsw_rec_k.h).
//
//   rec_plan_kernel<false>   per read: the number of records and of needed regions (the records'
//                            own and their XA members); validation
//   (two exclusive scans -> rec_first, aln_first; the totals size the caller's buffers)
//   rec_plan_kernel<true>    per read: the records but for the cross-linked fields; the needed
//                            regions compact for reg2aln_device (bsw_stages.cpp)
//   rec_finish_kernel        per record: mem_aln2sam's cross-linking, TLEN, the printed flag; per
//                            alignment: rejected / overflowing rows; the stage's counters
//   rec_text_len_kernel      per record: its line's length      (one scan -> text_off)
//   rec_text_write_kernel    kRecTextGroup lanes per record, kRecTextBlock / kRecTextGroup consecutive
//                            records per block.  A group assembles its line in a window of LDS -- lane 0 the
//                            numbers and literals, all lanes the name, SEQ (complement and reversal in the
//                            copy), QUAL and MD -- and flushes the window's whole dwords with one aligned dword
//                            store per lane and round.  The dword two lines share is put together in LDS
//                            from the tail of one and the head of the other and stored once after the
//                            block's barrier; only the at most three bytes at either end of a BLOCK's
//                            range are byte stores.
//   bam_len_kernel, bam_write_kernel   the same two passes for BAM alignment blocks (include/bsw_bam.h):
//                            kRecBamGroup lanes per record, the text's sinks, window and edge dwords
// Both text kernels run ONE emitter (emit_line) over two sinks, so the lengths are the bytes written;
// both BAM kernels run emit_bam over the same two.
// The lists are short (bsw_pe.hip's general kernel): XA membership is recounted per record instead
// of kept in per-read arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bsw_rec_k.h"
#include "bsw_stage_k.h"

namespace bsw {

namespace {

constexpr int kBlock = 256;

struct ListView {                       // one read's list
    const bsw_alnreg_t *a;
    const bsw_selinfo_t *inf;
    int n;
    float ml;
    double ratio;
    int z, kz;                          // the paired branch's region and its secondary_all before the switch; -1
};

// PRIMARY MARKING step 4's test (bsw_sel.h)
__device__ __forceinline__ bool overlaps(const bsw_alnreg_t &x, const bsw_alnreg_t &y, float ml)
{
    const int b_max = max(x.qb, y.qb), e_min = min(x.qe, y.qe);
    if (e_min <= b_max) return false;
    const int min_l = min(x.qe - x.qb, y.qe - y.qb);
    return (float)(e_min - b_max) >= (float)min_l * ml;
}

__device__ int sec_all(const ListView &v, int i)
{
    const int s = v.inf[i].secondary;
    if (s != -2) return s;
    for (int j = 0; j < i; ++j)
        if (v.inf[j].secondary == -1 && overlaps(v.a[j], v.a[i], v.ml)) return j;
    return -1;
}

// secondary_all after the primary switch
__device__ __forceinline__ int sec_sw(const ListView &v, int i)
{
    if (v.kz < 0) return sec_all(v, i);
    if (i == v.z) return -1;
    const int s = sec_all(v, i);
    return (s == v.kz || i == v.kz) ? v.z : s;
}

__device__ __forceinline__ int xa_pri(const ListView &v, int i)
{
    const int k = sec_sw(v, i);
    return (k >= 0 && (double)v.a[i].score >= (double)v.a[k].score * v.ratio) ? k : -1;
}

// the XA members a record of region r carries
__device__ int xa_count(const ListView &v, int r, int max_hits)
{
    int c = 0;
    for (int i = 0; i < v.n; ++i) c += xa_pri(v, i) == r;
    return c <= max_hits ? c : 0;
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void rec_plan_kernel(RecParams p, RecLists L, int32_t *nrec, int32_t *naln,
                                                          int32_t *meta, const int32_t *rec_first,
                                                          const int32_t *aln_first, bsw_rec_t *recs, int32_t *aln_reg,
                                                          bsw_alnreg_t *creg, int32_t *creg_read)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r > p.n_reads) return;
    if (r == p.n_reads) {
        if (!FILL) nrec[r] = naln[r] = 0;
        return;
    }
    const int f0 = L.first[r], f1 = L.first[r + 1];
    bool bad = f0 < 0 || f1 < f0 || f1 > p.n_regs || f1 - f0 > BSW_SEL_MAX_PER_READ;
    ListView v;
    v.n = bad ? 0 : f1 - f0;
    v.a = L.regs + (bad ? 0 : f0);
    v.inf = L.info + (bad ? 0 : f0);
    v.ml = p.mask_level;
    v.ratio = p.xa_ratio;
    v.z = v.kz = -1;
    for (int i = 0; i < v.n; ++i) {
        const int s = v.inf[i].secondary;
        bad |= s < -2 || s >= v.n;
    }
    const int e = r & 1;
    bsw_pair_t pr{};
    bool paired = false;
    int extra = 0;
    if (L.pairs && !bad) {
        pr = L.pairs[r >> 1];
        paired = pr.paired != 0;
        extra = (e ? 0x81 : 0x41) | (pr.proper ? 0x2 : 0);
        if (paired) {
            v.z = e ? pr.z[1] : pr.z[0];
            if (v.z < 0 || v.z >= v.n) bad = true;
            else v.kz = sec_all(v, v.z);
        }
    }
    if (bad) {
        if (!FILL) {
            atomicOr(meta + kRecErr, 1);
            nrec[r] = naln[r] = 0;
        }
        return;
    }
    int ri = FILL ? rec_first[r] : 0, ai = FILL ? aln_first[r] : 0;
    const int n_list = FILL ? rec_first[r + 1] - ri : 0;
    int l = 0, mapq0 = 0, na = 0;
    // one record: k = its region within the list, or -1
    auto record = [&](int k, int flag, int mapq) {
        const int m = k >= 0 ? xa_count(v, k, p.max_XA_hits) : 0;
        if (FILL) {
            bsw_rec_t o{};
            o.pos = o.mpos = -1;
            o.read = r;
            o.reg = k >= 0 ? f0 + k : -1;
            o.aln = o.m_aln = -1;
            o.which = l;
            o.n_list = n_list;
            o.flag = flag;
            o.mapq = mapq;
            if (k >= 0) {
                o.aln = ai;
                o.score = v.a[k].score;
                o.sub = max(v.inf[k].sub, v.inf[k].csub);
                o.xa_first = ai + 1;
                o.xa_n = m;
                aln_reg[ai] = f0 + k;
                creg[ai] = v.a[k];
                creg_read[ai] = r;
                ++ai;
                for (int i = 0, left = m; left > 0 && i < v.n; ++i)
                    if (xa_pri(v, i) == k) {
                        aln_reg[ai] = f0 + i;
                        creg[ai] = v.a[i];
                        creg_read[ai] = r;
                        ++ai;
                        --left;
                    }
            }
            recs[ri + l] = o;
        }
        na += k >= 0 ? 1 + m : 0;
        ++l;
    };
    if (paired) {
        record(v.z, (0x40 << e) | 0x1 | (pr.proper ? 0x2 : 0), e ? pr.mapq[1] : pr.mapq[0]);
    } else {
        for (int k = 0; k < v.n; ++k) {
            if (v.a[k].score < p.T || v.inf[k].secondary >= 0) continue;
            int flag = extra, mapq = v.inf[k].mapq;
            if (l == 0) mapq0 = mapq;
            else {
                flag |= (p.flags & BSW_REC_NO_MULTI) ? 0x10000 : 0x800;
                if (!(p.flags & BSW_REC_KEEP_SUPP_MAPQ) && mapq > mapq0) mapq = mapq0;
            }
            record(k, flag, mapq);
        }
        if (l == 0) record(-1, extra | 0x4, 0);
    }
    if (!FILL) {
        nrec[r] = l;
        naln[r] = na;
    }
}

__device__ __forceinline__ int64_t cigar_rlen(const uint32_t *cg, int n)
{
    int64_t l = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t op = cg[i] & 15u;
        if (op == 0 || op == 2) l += cg[i] >> 4;
    }
    return l;
}

__global__ __launch_bounds__(kBlock) void rec_finish_kernel(RecLists L, ContigView ctg, const int32_t *rec_first,
                                                            bsw_rec_t *recs, int32_t n_rec, const bsw_aln_t *aln,
                                                            const uint32_t *cigar, int32_t cigar_stride, int32_t n_aln,
                                                            int32_t *meta)
{
    __shared__ int32_t cnt[kRecMetaWords];
    if (threadIdx.x < kRecMetaWords) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_aln) {
        const bsw_aln_t a = aln[i];
        if (a.flags & BSW_ALN_REJECTED) atomicAdd(cnt + kRecRejected, 1);
        else if (a.n_cigar < 0 || a.md_len < 0) atomicAdd(cnt + kRecOverflow, 1);
    }
    if (i < n_rec) {
        bsw_rec_t o = recs[i];
        int flag = o.flag;
        const bool p_map = o.aln >= 0;
        bool p_ok = false;              // p has a CIGAR the kernel may read
        int64_t pos = -1;
        int is_rev = 0;
        if (p_map) {
            const bsw_aln_t a = aln[o.aln];
            pos = a.pos;
            is_rev = a.is_rev;
            p_ok = a.n_cigar > 0 && !(a.flags & BSW_ALN_REJECTED);
        } else {
            flag |= 0x4;
            atomicAdd(cnt + kRecUnmapped, 1);
        }
        if (o.which > 0) atomicAdd(cnt + kRecSupp, 1);
        if (o.xa_n > 0) atomicAdd(cnt + kRecXa, o.xa_n);
        int64_t mpos = -1, tlen = 0;
        int m_rev = 0, m_aln = -1;
        if (L.pairs) {
            flag |= 0x1;
            // the other end's record 0 (list[z], or the unmapped alignment): its aln was written by the fill pass
            const int ma = recs[rec_first[o.read ^ 1]].aln;
            bool m_ok = false;
            if (ma >= 0) {
                const bsw_aln_t b = aln[ma];
                mpos = b.pos;
                m_rev = b.is_rev;
                m_aln = ma;
                m_ok = b.n_cigar > 0 && !(b.flags & BSW_ALN_REJECTED);
            } else {
                flag |= 0x8;
            }
            if (!p_map && ma >= 0) { pos = mpos; is_rev = m_rev; }
            if (ma < 0 && p_map) { mpos = pos; m_rev = is_rev; }
            // (mem_aln2sam: p->rid == m->rid; both positions are forward coordinates)
            if (p_ok && m_ok && (!ctg.off || contig_of(ctg, pos) == contig_of(ctg, mpos))) {
                const int64_t p0 = pos + (is_rev ? cigar_rlen(cigar + (size_t)o.aln * cigar_stride, aln[o.aln].n_cigar) - 1 : 0);
                const int64_t p1 = mpos + (m_rev ? cigar_rlen(cigar + (size_t)ma * cigar_stride, aln[ma].n_cigar) - 1 : 0);
                tlen = -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
            }
        }
        if (is_rev) flag |= 0x10;
        if (m_rev) flag |= 0x20;
        o.pos = pos;
        o.is_rev = is_rev;
        o.mpos = mpos;
        o.m_is_rev = m_rev;
        o.m_aln = m_aln;
        o.tlen = tlen;
        o.flag = flag;
        o.sam_flag = (flag & 0xffff) | ((flag & 0x10000) ? 0x100 : 0);
        // (other records read only .aln of this one, which stays)
        recs[i].pos = o.pos; recs[i].mpos = o.mpos; recs[i].tlen = o.tlen; recs[i].flag = o.flag;
        recs[i].sam_flag = o.sam_flag; recs[i].is_rev = o.is_rev; recs[i].m_is_rev = o.m_is_rev; recs[i].m_aln = o.m_aln;
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < kRecMetaWords && cnt[threadIdx.x]) atomicAdd(meta + threadIdx.x, cnt[threadIdx.x]);
}

// ---------------------------------------------------------------- text
__device__ __forceinline__ int n_digits(uint64_t v)
{
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

struct CountSink {                      // one work item per record: the line's length
    int64_t n = 0;
    __device__ __forceinline__ void ch(char) { ++n; }
    __device__ __forceinline__ void lit(const char *, int k) { n += k; }
    __device__ __forceinline__ void num(int64_t v) { n += (v < 0) + n_digits(v < 0 ? 0 - (uint64_t)v : (uint64_t)v); }
    __device__ __forceinline__ void copy(const uint8_t *, int k) { n += k; }
    __device__ __forceinline__ void seq(const uint8_t *, int qb, int qe, bool) { n += qe - qb; }
    __device__ __forceinline__ void qual(const uint8_t *, int qb, int qe, bool) { n += qe - qb; }
    // (the binary puts of the BAM emitter)
    __device__ __forceinline__ void u8(uint32_t) { ++n; }
    __device__ __forceinline__ void u16(uint32_t) { n += 2; }
    __device__ __forceinline__ void u32(uint32_t) { n += 4; }
    __device__ __forceinline__ void rep(uint8_t, int k) { n += k; }
    __device__ __forceinline__ void seq4(const uint8_t *, int qb, int qe, bool) { n += (qe - qb + 1) >> 1; }
    __device__ __forceinline__ void qual33(const uint8_t *, int qb, int qe, bool) { n += qe - qb; }
};

constexpr int kWin = 512;               // bytes of a group's LDS window

// G lanes of one wave assemble a line (the text kernel: kRecTextGroup; the BAM kernel, a block:
// kRecBamGroup).  win[0] is the byte at global offset gbase (a multiple of 4); fill = the bytes assembled so far, the same on every lane of the group: every
// lane runs every call, lane 0 alone writes what is not a bulk copy.
template <int G>
struct LdsSink {
    uint8_t *win;                       // the group's window, 4-byte aligned
    uint32_t *out;                      // the text, as dwords
    uint8_t *head;                      // edge[local]: this line's head bytes go to [gbase0 & 3 .., 4)
    uint8_t *tail;                      // edge[local + 1]: this line's last (end & 3) bytes
    int64_t gbase;
    int fill, lane;
    int k0;                             // the line's start within its first dword
    bool head_pending;                  // k0 != 0 and that dword has not been set aside yet

    __device__ __forceinline__ void fence() const
    {
        // the group's lanes are lanes of one wave: LDS serves a wave's accesses in order; the fence keeps
        // the compiler from moving them and waits for the counter
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    // the window's whole dwords out, the remainder to its front
    __device__ __forceinline__ void flush()
    {
        fence();
        const int nd = fill >> 2, rem = fill & 3;
        int d0 = 0;
        if (head_pending && nd > 0) {
            if (lane >= k0 && lane < 4) head[lane] = win[lane];     // (the bytes before the line's start are not its own)
            d0 = 1;
            head_pending = false;
        }
        const uint32_t *w = (const uint32_t *)win;
        for (int d = d0 + lane; d < nd; d += G) out[(gbase >> 2) + d] = w[d];
        uint8_t keep = 0;
        if (lane < rem) keep = win[nd * 4 + lane];
        fence();
        if (lane < rem) win[lane] = keep;
        gbase += (int64_t)nd * 4;
        fill = rem;
        fence();
    }
    __device__ __forceinline__ void room(int k) { if (fill + k > kWin) flush(); }
    __device__ __forceinline__ void ch(char c)
    {
        room(1);
        if (lane == 0) win[fill] = (uint8_t)c;
        ++fill;
    }
    __device__ __forceinline__ void lit(const char *s, int k)
    {
        room(k);
        if (lane == 0)
            for (int i = 0; i < k; ++i) win[fill + i] = (uint8_t)s[i];
        fill += k;
    }
    __device__ __forceinline__ void num(int64_t v)
    {
        const bool neg = v < 0;
        const uint64_t u = neg ? 0 - (uint64_t)v : (uint64_t)v;
        const int nd = n_digits(u), k = nd + neg;
        room(k);
        if (lane == 0) {
            if (neg) win[fill] = '-';
            if (u <= 0xffffffffu) {
                uint32_t x = (uint32_t)u;
                for (int i = k - 1; i >= (int)neg; --i) { win[fill + i] = (uint8_t)('0' + x % 10); x /= 10; }
            } else {
                uint64_t x = u;
                for (int i = k - 1; i >= (int)neg; --i) { win[fill + i] = (uint8_t)('0' + x % 10); x /= 10; }
            }
        }
        fill += k;
    }
    // src(t) for t in [0, k), by all lanes, a window at a time
    template <class F>
    __device__ __forceinline__ void bulk(int k, F src)
    {
        int done = 0;
        while (done < k) {
            if (fill == kWin) flush();
            const int c = min(k - done, kWin - fill);
            for (int t = lane; t < c; t += G) win[fill + t] = src(done + t);
            fill += c;
            done += c;
        }
    }
    __device__ __forceinline__ void copy(const uint8_t *s, int k) { bulk(k, [&](int t) { return s[t]; }); }
    __device__ __forceinline__ void seq(const uint8_t *s, int qb, int qe, bool rev)
    {
        bulk(qe - qb, [&](int t) {
            const int c = min((int)s[rev ? qe - 1 - t : qb + t], 4);
            return (uint8_t)(rev ? "TGCAN"[c] : "ACGTN"[c]);
        });
    }
    __device__ __forceinline__ void qual(const uint8_t *s, int qb, int qe, bool rev)
    {
        bulk(qe - qb, [&](int t) { return s[rev ? qe - 1 - t : qb + t]; });
    }
    // the binary puts of the BAM emitter, little-endian: one byte per lane (G >= 4)
    __device__ __forceinline__ void u8(uint32_t v)
    {
        room(1);
        if (lane == 0) win[fill] = (uint8_t)v;
        ++fill;
    }
    __device__ __forceinline__ void u16(uint32_t v)
    {
        room(2);
        if (lane < 2) win[fill + lane] = (uint8_t)(v >> (8 * lane));
        fill += 2;
    }
    __device__ __forceinline__ void u32(uint32_t v)
    {
        room(4);
        if (lane < 4) win[fill + lane] = (uint8_t)(v >> (8 * lane));
        fill += 4;
    }
    __device__ __forceinline__ void rep(uint8_t c, int k) { bulk(k, [&](int) { return c; }); }
    // two bases per byte, the first in the high nibble: A 1, C 2, G 4, T 8, the rest 15
    __device__ __forceinline__ void seq4(const uint8_t *s, int qb, int qe, bool rev)
    {
        const int n = qe - qb;
        auto nib = [&](int j) {
            const int c = s[rev ? qe - 1 - j : qb + j];
            return c >= 4 ? 15u : rev ? 8u >> c : 1u << c;
        };
        bulk((n + 1) >> 1, [&](int t) { return (uint8_t)(nib(2 * t) << 4 | (2 * t + 1 < n ? nib(2 * t + 1) : 0u)); });
    }
    __device__ __forceinline__ void qual33(const uint8_t *s, int qb, int qe, bool rev)
    {
        bulk(qe - qb, [&](int t) { return (uint8_t)(s[rev ? qe - 1 - t : qb + t] - 33); });
    }
    // the last whole dwords out; the line's last (end & 3) bytes to the edge they share with the next line
    __device__ __forceinline__ void finish()
    {
        flush();
        if (lane < fill) tail[lane] = win[lane];
    }
};

template <class S>
__device__ __forceinline__ void put_cigar(S &s, const uint32_t *cg, int n, char clip)
{
    for (int i = 0; i < n; ++i) {
        const uint32_t w = cg[i];
        const int op = min((int)(w & 15u), 4);
        s.num(w >> 4);
        s.ch((op >= 3 && clip) ? clip : "MIDSH"[op]);
    }
}

// what emit_line reads of record i has to lie inside the arrays
__device__ __forceinline__ bool text_record_ok(const RecText &t, int i)
{
    const bsw_rec_t &p = t.recs[i];
    if (p.read < 0 || p.read >= t.n_reads || p.aln < -1 || p.aln >= t.n_aln || p.m_aln < -1 || p.m_aln >= t.n_aln)
        return false;
    if (p.xa_n < 0 || p.xa_first < 0 || (p.xa_n > 0 && (int64_t)p.xa_first + p.xa_n > t.n_aln)) return false;
    const int ni = t.paired ? p.read >> 1 : p.read;
    if (ni >= t.n_names) return false;
    const int64_t nl = t.name_off[ni + 1] - t.name_off[ni];
    if (t.name_off[ni] < 0 || nl < 0 || nl > BSW_REC_MAX_NAME) return false;
    if (t.read_len[p.read] < 0 || t.read_off[p.read] < 0) return false;
    const int f0 = t.rec_first[p.read];
    if (p.which < 0 || p.n_list < 1 || p.which >= p.n_list || f0 < 0 || (int64_t)f0 + p.n_list > t.n_rec || f0 + p.which != i)
        return false;
    auto aln_ok = [&](int a) {
        const bsw_aln_t &x = t.aln[a];
        return x.n_cigar >= 1 && x.n_cigar <= t.cigar_stride && x.md_len >= 0 && x.md_len <= t.md_stride;
    };
    if (p.aln >= 0 && !aln_ok(p.aln)) return false;
    if (p.m_aln >= 0 && !aln_ok(p.m_aln)) return false;
    for (int j = 0; j < p.xa_n; ++j)
        if (!aln_ok(p.xa_first + j)) return false;
    if (p.aln >= 0) {                   // the clips cut from SEQ fit the read
        const uint32_t *cg = t.cigar + (size_t)p.aln * t.cigar_stride;
        const int n = t.aln[p.aln].n_cigar;
        const int64_t c5 = (cg[0] & 15u) >= 3 ? cg[0] >> 4 : 0, c3 = (cg[n - 1] & 15u) >= 3 ? cg[n - 1] >> 4 : 0;
        if (c5 + c3 > t.read_len[p.read]) return false;
    }
    for (int j = 0; j < p.n_list; ++j) {
        const bsw_rec_t &q = t.recs[f0 + j];
        if (j != p.which && !(q.flag & 0x100) && (q.aln < 0 || q.aln >= t.n_aln || !aln_ok(q.aln))) return false;
    }
    return true;
}

// where a forward position prints: its contig's name, the contig's offset and its rid -- with no
// table opt->rname, 0 and 0
struct Place {
    const uint8_t *name;
    int len, rid;
    int64_t base, end;                  // the contig is [base, end)
};

__device__ __forceinline__ Place place_of(const RecText &t, int64_t pos)
{
    if (!t.ctg.off) return {t.rname, t.rname_len, 0, 0, INT64_MAX};
    const int k = contig_of(t.ctg, pos);
    const int o = t.ctg.name_off[k];
    return {t.ctg.names + o, t.ctg.name_off[k + 1] - o, k, t.ctg.off[k], t.ctg.off[k + 1]};
}

// the same for a position that usually lies in the contig already found (the mate, SA and XA entries): no
// second search then
__device__ __forceinline__ Place place_near(const RecText &t, int64_t pos, const Place &near)
{
    return pos >= near.base && pos < near.end ? near : place_of(t, pos);
}

template <class S>
__device__ __forceinline__ void emit_line(S &s, const RecText &t, int i)
{
    const bsw_rec_t p = t.recs[i];
    const int r = p.read, which = p.which;
    const bool soft = t.flags & BSW_REC_SOFTCLIP;
    const char clip = soft ? 0 : (which ? 'H' : 'S');
    const int ni = t.paired ? r >> 1 : r;
    const int64_t n0 = t.name_off[ni];
    s.copy(t.names + n0, (int)(t.name_off[ni + 1] - n0));
    s.ch('\t');
    s.num(p.sam_flag);
    s.ch('\t');
    const int ncig = p.aln >= 0 ? t.aln[p.aln].n_cigar : 0;
    const uint32_t *cg = t.cigar + (size_t)max(p.aln, 0) * t.cigar_stride;
    Place at = {nullptr, 0, t.ctg.off ? -1 : 0, 0, 0};   // (an empty range: nothing is near it)
    if (p.pos >= 0) {
        at = place_of(t, p.pos);
        s.copy(at.name, at.len);
        s.ch('\t');
        s.num(p.pos - at.base + 1);
        s.ch('\t');
        s.num(p.mapq);
        s.ch('\t');
        if (ncig) put_cigar(s, cg, ncig, clip);
        else s.ch('*');
    } else {
        s.lit("*\t0\t0\t*", 7);
    }
    s.ch('\t');
    if (p.mpos >= 0) {
        const Place mt = place_near(t, p.mpos, at);
        if (mt.rid == at.rid) s.ch('=');    // (pos >= 0 whenever mpos is: cross-linking)
        else s.copy(mt.name, mt.len);
        s.ch('\t');
        s.num(p.mpos - mt.base + 1);
        s.ch('\t');
        s.num(p.tlen);
    } else {
        s.lit("*\t0\t0", 5);
    }
    s.ch('\t');
    int qb = 0, qe = t.read_len[r];
    if (ncig && which && !soft) {
        const int c5 = (cg[0] & 15u) >= 3 ? (int)(cg[0] >> 4) : 0, c3 = (cg[ncig - 1] & 15u) >= 3 ? (int)(cg[ncig - 1] >> 4) : 0;
        if (p.is_rev) { qe -= c5; qb += c3; }
        else { qb += c5; qe -= c3; }
    }
    const int64_t ro = t.read_off[r];
    s.seq(t.reads + ro, qb, qe, p.is_rev != 0);
    s.ch('\t');
    if (t.quals) s.qual(t.quals + ro, qb, qe, p.is_rev != 0);
    else s.ch('*');
    if (ncig) {
        s.lit("\tNM:i:", 6);
        s.num(t.aln[p.aln].NM);
        s.lit("\tMD:Z:", 6);
        s.copy(t.md + (size_t)p.aln * t.md_stride, t.aln[p.aln].md_len);
    }
    if (p.m_aln >= 0) {
        s.lit("\tMC:Z:", 6);
        put_cigar(s, t.cigar + (size_t)p.m_aln * t.cigar_stride, t.aln[p.m_aln].n_cigar, clip);
    }
    s.lit("\tAS:i:", 6);
    s.num(p.score);
    if (p.sub >= 0) {
        s.lit("\tXS:i:", 6);
        s.num(p.sub);
    }
    if (!(p.flag & 0x100)) {
        const int f0 = t.rec_first[r];
        bool any = false;
        for (int j = 0; j < p.n_list; ++j) any |= j != which && !(t.recs[f0 + j].flag & 0x100);
        if (any) {
            s.lit("\tSA:Z:", 6);
            for (int j = 0; j < p.n_list; ++j) {
                if (j == which || (t.recs[f0 + j].flag & 0x100)) continue;
                const int qa = t.recs[f0 + j].aln;
                const bsw_aln_t a = t.aln[qa];
                const Place sa = place_near(t, a.pos, at);
                s.copy(sa.name, sa.len);
                s.ch(',');
                s.num(a.pos - sa.base + 1);
                s.ch(',');
                s.ch(a.is_rev ? '-' : '+');
                s.ch(',');
                put_cigar(s, t.cigar + (size_t)qa * t.cigar_stride, a.n_cigar, 0);
                s.ch(',');
                s.num(t.recs[f0 + j].mapq);
                s.ch(',');
                s.num(a.NM);
                s.ch(';');
            }
        }
    }
    if (p.xa_n > 0) {
        s.lit("\tXA:Z:", 6);
        for (int j = p.xa_first; j < p.xa_first + p.xa_n; ++j) {
            const bsw_aln_t a = t.aln[j];
            const Place xa = place_near(t, a.pos, at);
            s.copy(xa.name, xa.len);
            s.ch(',');
            s.ch(a.is_rev ? '-' : '+');
            s.num(a.pos - xa.base + 1);
            s.ch(',');
            put_cigar(s, t.cigar + (size_t)j * t.cigar_stride, a.n_cigar, 0);
            s.ch(',');
            s.num(a.NM);
            s.ch(';');
        }
    }
    s.ch('\n');
}

__global__ __launch_bounds__(kBlock) void rec_text_len_kernel(RecText t, int64_t *len, int32_t *meta)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > t.n_rec) return;
    if (i == t.n_rec) {
        len[i] = 0;
        return;
    }
    if (!text_record_ok(t, i)) {
        atomicOr(meta + kRecErr, 1);
        len[i] = 0;
        return;
    }
    CountSink s;
    emit_line(s, t, i);
    len[i] = s.n;
}

constexpr int kPerBlock = kRecTextBlock / kRecTextGroup;

__global__ __launch_bounds__(kRecTextBlock) void rec_text_write_kernel(RecText t, const int64_t *text_off, uint8_t *text)
{
    __shared__ uint32_t win[kPerBlock][kWin / 4];
    __shared__ uint32_t edge[kPerBlock + 1];
    const int g = threadIdx.x / kRecTextGroup, lane = threadIdx.x % kRecTextGroup;
    const int r0 = blockIdx.x * kPerBlock;
    const int nvalid = min(kPerBlock, t.n_rec - r0);
    if (threadIdx.x <= kPerBlock) edge[threadIdx.x] = 0;
    __syncthreads();
    if (g < nvalid) {
        const int64_t o = text_off[r0 + g];
        LdsSink<kRecTextGroup> s;
        s.win = (uint8_t *)win[g];
        s.out = (uint32_t *)text;
        s.head = (uint8_t *)&edge[g];
        s.tail = (uint8_t *)&edge[g + 1];
        s.gbase = o & ~(int64_t)3;
        s.fill = s.k0 = (int)(o & 3);
        s.lane = lane;
        s.head_pending = s.k0 != 0;
        emit_line(s, t, r0 + g);
        s.finish();
    }
    __syncthreads();
    // the dwords two lines share; the block's own two ends byte by byte
    const int b = threadIdx.x;
    if (b <= nvalid) {
        const int64_t o = text_off[r0 + b];
        const int k = (int)(o & 3);
        if (k) {
            const uint8_t *e = (const uint8_t *)&edge[b];
            uint8_t *at = text + (o & ~(int64_t)3);
            if (b > 0 && b < nvalid) *(uint32_t *)at = edge[b];
            else if (b == 0) for (int j = k; j < 4; ++j) at[j] = e[j];
            else for (int j = 0; j < k; ++j) at[j] = e[j];
        }
    }
}

// ---------------------------------------------------------------- BAM (include/bsw_bam.h)
// the UCSC binning scheme, 14-bit smallest bin, 5 levels; beg = -1, end = 0 gives 4680 (arithmetic shifts)
__device__ __forceinline__ int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// what the binary fields cannot hold, on top of text_record_ok
__device__ __forceinline__ bool bam_record_ok(const RecText &t, int i)
{
    if (!text_record_ok(t, i)) return false;
    const bsw_rec_t &p = t.recs[i];
    const int ni = t.paired ? p.read >> 1 : p.read;
    if (t.name_off[ni + 1] - t.name_off[ni] > BSW_BAM_MAX_NAME) return false;
    if (p.tlen < INT32_MIN || p.tlen > INT32_MAX) return false;
    if (p.pos >= 0 && p.pos - place_of(t, p.pos).base > INT32_MAX) return false;
    if (p.mpos >= 0 && p.mpos - place_of(t, p.mpos).base > INT32_MAX) return false;
    return p.aln < 0 || t.aln[p.aln].n_cigar <= 0xffff;
}

// an integer tag with the smallest type that holds v, as the text parser picks it
template <class S>
__device__ __forceinline__ void put_int_tag(S &s, const char *tag, int32_t v)
{
    s.lit(tag, 2);
    if (v >= 0) {
        if (v <= 0xff) { s.ch('C'); s.u8(v); }
        else if (v <= 0xffff) { s.ch('S'); s.u16(v); }
        else { s.ch('I'); s.u32(v); }
    } else {
        if (v >= -128) { s.ch('c'); s.u8(v); }
        else if (v >= -32768) { s.ch('s'); s.u16(v); }
        else { s.ch('i'); s.u32(v); }
    }
}

// block = the record's bytes behind block_size: the count pass passes 0, the write pass the
// difference of its offsets.  The Z values are emit_line's own calls.
template <class S>
__device__ __forceinline__ void emit_bam(S &s, const RecText &t, int i, uint32_t block)
{
    const bsw_rec_t p = t.recs[i];
    const int r = p.read, which = p.which;
    const bool soft = t.flags & BSW_REC_SOFTCLIP;
    const char clip = soft ? 0 : (which ? 'H' : 'S');
    const int ni = t.paired ? r >> 1 : r;
    const int64_t n0 = t.name_off[ni];
    const int l_name = (int)(t.name_off[ni + 1] - n0);
    const int ncig = p.aln >= 0 ? t.aln[p.aln].n_cigar : 0;
    const uint32_t *cg = t.cigar + (size_t)max(p.aln, 0) * t.cigar_stride;
    Place at = {nullptr, 0, -1, 0, 0};                   // (an empty range: nothing is near it)
    int64_t pos = -1, mpos = -1;
    int mrid = -1;
    if (p.pos >= 0) {
        at = place_of(t, p.pos);
        pos = p.pos - at.base;
    }
    if (p.mpos >= 0) {
        const Place mt = place_near(t, p.mpos, at);
        mrid = mt.rid;
        mpos = p.mpos - mt.base;
    }
    int qb = 0, qe = t.read_len[r];
    if (ncig && which && !soft) {
        const int c5 = (cg[0] & 15u) >= 3 ? (int)(cg[0] >> 4) : 0, c3 = (cg[ncig - 1] & 15u) >= 3 ? (int)(cg[ncig - 1] >> 4) : 0;
        if (p.is_rev) { qe -= c5; qb += c3; }
        else { qb += c5; qe -= c3; }
    }
    const int bin = reg2bin(pos, pos + (ncig ? cigar_rlen(cg, ncig) : 1));
    // the fixed part: nine dwords
    s.u32(block);
    s.u32((uint32_t)at.rid);
    s.u32((uint32_t)pos);
    s.u32((uint32_t)(l_name + 1) | (uint32_t)((p.pos >= 0 ? p.mapq : 0) & 0xff) << 8 | (uint32_t)(bin & 0xffff) << 16);
    s.u32((uint32_t)ncig | (uint32_t)(p.sam_flag & 0xffff) << 16);
    s.u32((uint32_t)(qe - qb));
    s.u32((uint32_t)mrid);
    s.u32((uint32_t)mpos);
    s.u32((uint32_t)p.tlen);
    s.copy(t.names + n0, l_name);
    s.u8(0);
    for (int k = 0; k < ncig; ++k) {
        const uint32_t w = cg[k];
        uint32_t op = w & 15u;
        if (op >= 3) op = clip ? (clip == 'S' ? 4u : 5u) : (op == 3 ? 4u : 5u);
        s.u32((w & ~15u) | op);
    }
    const int64_t ro = t.read_off[r];
    s.seq4(t.reads + ro, qb, qe, p.is_rev != 0);
    if (t.quals) s.qual33(t.quals + ro, qb, qe, p.is_rev != 0);
    else s.rep(0xff, qe - qb);
    if (ncig) {
        put_int_tag(s, "NM", t.aln[p.aln].NM);
        s.lit("MDZ", 3);
        s.copy(t.md + (size_t)p.aln * t.md_stride, t.aln[p.aln].md_len);
        s.u8(0);
    }
    if (p.m_aln >= 0) {
        s.lit("MCZ", 3);
        put_cigar(s, t.cigar + (size_t)p.m_aln * t.cigar_stride, t.aln[p.m_aln].n_cigar, clip);
        s.u8(0);
    }
    put_int_tag(s, "AS", p.score);
    if (p.sub >= 0) put_int_tag(s, "XS", p.sub);
    if (!(p.flag & 0x100)) {
        const int f0 = t.rec_first[r];
        bool any = false;
        for (int j = 0; j < p.n_list; ++j) any |= j != which && !(t.recs[f0 + j].flag & 0x100);
        if (any) {
            s.lit("SAZ", 3);
            for (int j = 0; j < p.n_list; ++j) {
                if (j == which || (t.recs[f0 + j].flag & 0x100)) continue;
                const int qa = t.recs[f0 + j].aln;
                const bsw_aln_t a = t.aln[qa];
                const Place sa = place_near(t, a.pos, at);
                s.copy(sa.name, sa.len);
                s.ch(',');
                s.num(a.pos - sa.base + 1);
                s.ch(',');
                s.ch(a.is_rev ? '-' : '+');
                s.ch(',');
                put_cigar(s, t.cigar + (size_t)qa * t.cigar_stride, a.n_cigar, 0);
                s.ch(',');
                s.num(t.recs[f0 + j].mapq);
                s.ch(',');
                s.num(a.NM);
                s.ch(';');
            }
            s.u8(0);
        }
    }
    if (p.xa_n > 0) {
        s.lit("XAZ", 3);
        for (int j = p.xa_first; j < p.xa_first + p.xa_n; ++j) {
            const bsw_aln_t a = t.aln[j];
            const Place xa = place_near(t, a.pos, at);
            s.copy(xa.name, xa.len);
            s.ch(',');
            s.ch(a.is_rev ? '-' : '+');
            s.num(a.pos - xa.base + 1);
            s.ch(',');
            put_cigar(s, t.cigar + (size_t)j * t.cigar_stride, a.n_cigar, 0);
            s.ch(',');
            s.num(a.NM);
            s.ch(';');
        }
        s.u8(0);
    }
}

__global__ __launch_bounds__(kBlock) void bam_len_kernel(RecText t, int64_t *len, int32_t *meta)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > t.n_rec) return;
    if (i == t.n_rec) {
        len[i] = 0;
        return;
    }
    if (!bam_record_ok(t, i)) {
        atomicOr(meta + kRecErr, 1);
        len[i] = 0;
        return;
    }
    CountSink s;
    emit_bam(s, t, i, 0u);
    len[i] = s.n;
}

constexpr int kBamPerBlock = kRecTextBlock / kRecBamGroup;

// rec_text_write_kernel's shape with kRecBamGroup lanes per record: the blocks are not dword-aligned
// (names vary), so the dword two records share goes through the edge words here too
__global__ __launch_bounds__(kRecTextBlock) void bam_write_kernel(RecText t, const int64_t *bam_off, uint8_t *bam)
{
    __shared__ uint32_t win[kBamPerBlock][kWin / 4];
    __shared__ uint32_t edge[kBamPerBlock + 1];
    const int g = threadIdx.x / kRecBamGroup, lane = threadIdx.x % kRecBamGroup;
    const int r0 = blockIdx.x * kBamPerBlock;
    const int nvalid = min(kBamPerBlock, t.n_rec - r0);
    if (threadIdx.x <= kBamPerBlock) edge[threadIdx.x] = 0;
    __syncthreads();
    if (g < nvalid) {
        const int64_t o = bam_off[r0 + g];
        LdsSink<kRecBamGroup> s;
        s.win = (uint8_t *)win[g];
        s.out = (uint32_t *)bam;
        s.head = (uint8_t *)&edge[g];
        s.tail = (uint8_t *)&edge[g + 1];
        s.gbase = o & ~(int64_t)3;
        s.fill = s.k0 = (int)(o & 3);
        s.lane = lane;
        s.head_pending = s.k0 != 0;
        emit_bam(s, t, r0 + g, (uint32_t)(bam_off[r0 + g + 1] - o - 4));
        s.finish();
    }
    __syncthreads();
    // the dwords two records share; the block's own two ends byte by byte
    const int b = threadIdx.x;
    if (b <= nvalid) {
        const int64_t o = bam_off[r0 + b];
        const int k = (int)(o & 3);
        if (k) {
            const uint8_t *e = (const uint8_t *)&edge[b];
            uint8_t *at = bam + (o & ~(int64_t)3);
            if (b > 0 && b < nvalid) *(uint32_t *)at = edge[b];
            else if (b == 0) for (int j = k; j < 4; ++j) at[j] = e[j];
            else for (int j = 0; j < k; ++j) at[j] = e[j];
        }
    }
}

}  // namespace

hipError_t launch_rec_bam_len(const RecText &t, int64_t *len, int32_t *meta, hipStream_t s)
{
    bam_len_kernel<<<grid_for((int64_t)t.n_rec + 1, kBlock), kBlock, 0, s>>>(t, len, meta);
    return hipGetLastError();
}

hipError_t launch_rec_bam_write(const RecText &t, const int64_t *bam_off, uint8_t *bam, hipStream_t s)
{
    if (t.n_rec == 0) return hipSuccess;
    bam_write_kernel<<<grid_for(t.n_rec, kBamPerBlock), kRecTextBlock, 0, s>>>(t, bam_off, bam);
    return hipGetLastError();
}

hipError_t launch_rec_count(const RecParams &p, const RecLists &l, int32_t *nrec, int32_t *naln, int32_t *meta,
                            hipStream_t s)
{
    rec_plan_kernel<false><<<grid_for((int64_t)p.n_reads + 1, kBlock), kBlock, 0, s>>>(
        p, l, nrec, naln, meta, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_rec_fill(const RecParams &p, const RecLists &l, const int32_t *rec_first, const int32_t *aln_first,
                           bsw_rec_t *recs, int32_t *aln_reg, bsw_alnreg_t *creg, int32_t *creg_read, hipStream_t s)
{
    if (p.n_reads == 0) return hipSuccess;
    rec_plan_kernel<true><<<grid_for(p.n_reads, kBlock), kBlock, 0, s>>>(p, l, nullptr, nullptr, nullptr, rec_first,
                                                                         aln_first, recs, aln_reg, creg, creg_read);
    return hipGetLastError();
}

hipError_t launch_rec_finish(const RecLists &l, const ContigView &ctg, const int32_t *rec_first, bsw_rec_t *recs,
                             int32_t n_rec, const bsw_aln_t *aln, const uint32_t *cigar, int32_t cigar_stride,
                             int32_t n_aln, int32_t *meta, hipStream_t s)
{
    const int64_t n = n_rec > n_aln ? n_rec : n_aln;
    if (n == 0) return hipSuccess;
    rec_finish_kernel<<<grid_for(n, kBlock), kBlock, 0, s>>>(l, ctg, rec_first, recs, n_rec, aln, cigar, cigar_stride,
                                                              n_aln, meta);
    return hipGetLastError();
}

hipError_t launch_rec_text_len(const RecText &t, int64_t *len, int32_t *meta, hipStream_t s)
{
    rec_text_len_kernel<<<grid_for((int64_t)t.n_rec + 1, kBlock), kBlock, 0, s>>>(t, len, meta);
    return hipGetLastError();
}

hipError_t launch_rec_text_write(const RecText &t, const int64_t *text_off, uint8_t *text, hipStream_t s)
{
    if (t.n_rec == 0) return hipSuccess;
    rec_text_write_kernel<<<grid_for(t.n_rec, kPerBlock), kRecTextBlock, 0, s>>>(t, text_off, text);
    return hipGetLastError();
}

}  // namespace bsw
