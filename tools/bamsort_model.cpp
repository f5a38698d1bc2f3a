// bamsort_model.cpp -- the serial model of the BAM sort and index kernels (bwa-mem2-arm_amd/csrc/bsw_bamsort.hip): the
// kernels' own per-record functions (bsw_bamsort_k.h) run one record after the other over files.  No GPU.
//   g++ -O2 -std=c++17 -I bwa-mem2-arm_amd/csrc tools/bamsort_model.cpp -o bamsort_model
//   bamsort_model sort N_REF BAM OFF OUT OUT_OFF PERM           BAM: the blocks; OFF: int64[n_rec + 1]; writes the sorted
//                                                               blocks, their offsets and the permutation (int32)
//   bamsort_model index N_REF BAM OFF VOFF END_VOFF REF_LEN BAI BAM / OFF sorted; VOFF: int64[n_rec]; REF_LEN:
//                                                               int32[N_REF]; writes the .bai; prints
//                                                               "bins B chunks C intv I no_coor N bytes S"
// Exit status 34: what the library answers with BSW_E_RANGE; 2: usage or I/O.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "bsw_bamsort_k.h"

using namespace bsw::bamsort;

template <class T>
static std::vector<T> read_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    if (v.size() % sizeof(T)) { fprintf(stderr, "%s: %zu bytes are no array of %zu-byte items\n", path, v.size(), sizeof(T)); exit(2); }
    std::vector<T> out(v.size() / sizeof(T));
    if (!v.empty()) memcpy(out.data(), v.data(), v.size());
    return out;
}

static void write_file(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes) || fclose(f)) { perror(path); exit(2); }
}

static int range_error(const char *what, long i)
{
    fprintf(stderr, "BSW_E_RANGE: %s at record %ld\n", what, i);
    return 34;
}

// the checks of the key kernel; fills fx
static int check_blocks(const std::vector<uint8_t> &bam, const std::vector<int64_t> &off, int32_t n_ref, std::vector<Fixed> &fx)
{
    const int32_t n = (int32_t)off.size() - 1;
    fx.resize((size_t)std::max(n, 0));
    for (int32_t i = 0; i < n; ++i) {
        if (!span_ok(off[i], off[i + 1]) || (i == 0 && off[0] != 0) || (size_t)off[i + 1] > bam.size()) return range_error("offsets", i);
        fx[i] = read_fixed(bam.data() + off[i]);
        if (!block_ok(fx[i], off[i + 1] - off[i], n_ref)) return range_error("block", i);
    }
    return 0;
}

static int model_sort(int32_t n_ref, char **argv)
{
    const std::vector<uint8_t> bam = read_file<uint8_t>(argv[0]);
    const std::vector<int64_t> off = read_file<int64_t>(argv[1]);
    if (off.empty()) { fprintf(stderr, "OFF holds n_rec + 1 offsets\n"); return 2; }
    std::vector<Fixed> fx;
    if (const int rc = check_blocks(bam, off, n_ref, fx)) return rc;
    const int32_t n = (int32_t)fx.size();
    std::vector<uint64_t> key(n);
    std::vector<int32_t> perm(n);
    uint64_t or_ = 0, nor_ = 0;
    for (int32_t i = 0; i < n; ++i) {
        key[i] = sort_key(fx[i], n_ref);
        perm[i] = i;
        or_ |= key[i];
        nor_ |= ~key[i];
    }
    int lo, hi;
    key_span(or_, nor_, &lo, &hi);                  // the kernel's radix sort sees these bits alone
    const uint64_t mask = hi > lo ? (hi - lo == 64 ? ~0ull : ((1ull << (hi - lo)) - 1) << lo) : 0;
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return (key[a] & mask) < (key[b] & mask); });
    std::vector<uint8_t> out(bam.size());
    std::vector<int64_t> out_off(n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int64_t len = off[perm[i] + 1] - off[perm[i]];
        memcpy(out.data() + out_off[i], bam.data() + off[perm[i]], (size_t)len);
        out_off[i + 1] = out_off[i] + len;
    }
    write_file(argv[2], out.data(), (size_t)out_off[n]);
    write_file(argv[3], out_off.data(), out_off.size() * sizeof(int64_t));
    write_file(argv[4], perm.data(), perm.size() * sizeof(int32_t));
    printf("records %d bytes %lld key_bits %d\n", n, (long long)out_off[n], hi - lo);
    return 0;
}

struct Chunk { int64_t beg, end; };
struct Bin { std::vector<Chunk> chunks; int64_t last_vend = 0; };
struct Ref {
    std::map<uint32_t, Bin> bins;                   // ascending
    std::vector<int64_t> lin;                       // -1: untouched
    int64_t first_voff = 0, last_vend = 0;
    uint64_t n_mapped = 0, n_unmapped = 0;
    bool has = false;
};

static int model_index(int32_t n_ref, char **argv)
{
    const std::vector<uint8_t> bam = read_file<uint8_t>(argv[0]);
    const std::vector<int64_t> off = read_file<int64_t>(argv[1]);
    const std::vector<int64_t> voff = read_file<int64_t>(argv[2]);
    const int64_t end_voff = atoll(argv[3]);
    const std::vector<int32_t> ref_len = read_file<int32_t>(argv[4]);
    if (off.empty() || voff.size() + 1 != off.size() || (int32_t)ref_len.size() != n_ref || end_voff < 0) {
        fprintf(stderr, "OFF holds n_rec + 1 offsets, VOFF n_rec, REF_LEN N_REF lengths\n");
        return 2;
    }
    for (int32_t r = 0; r < n_ref; ++r)
        if (ref_len[r] < 0 || ref_len[r] > kMaxRefLen) return range_error("ref_len of reference", r);
    std::vector<Fixed> fx;
    if (const int rc = check_blocks(bam, off, n_ref, fx)) return rc;
    const int32_t n = (int32_t)fx.size();
    std::vector<Ref> refs(n_ref);
    uint64_t n_no_coor = 0;
    for (int32_t i = 0; i < n; ++i) {
        const Fixed &f = fx[i];
        const uint8_t *blk = bam.data() + off[i];
        if (!cigar_ok(f)) return range_error("CIGAR", i);
        if (voff[i] < 0 || voff[i] > end_voff || (i > 0 && voff[i - 1] > voff[i])) return range_error("voff", i);
        if (i > 0 && !order_ok(fx[i - 1].ref_id, fx[i - 1].pos, f.ref_id, f.pos, n_ref)) return range_error("order", i);
        if (f.ref_id < 0) { ++n_no_coor; continue; }
        const int64_t beg = f.pos, end = record_end(blk, f), ve = vend(voff.data(), i, n, end_voff);
        if (beg < 0 || end > ref_len[f.ref_id]) return range_error("extent", i);
        Ref &R = refs[f.ref_id];
        if (!R.has) { R.has = true; R.first_voff = voff[i]; }
        R.last_vend = ve;
        ++(f.flag & 4 ? R.n_unmapped : R.n_mapped);
        Bin &B = R.bins[reg2bin(beg, end)];
        if (B.chunks.empty() || chunk_head(voff[i], B.last_vend)) B.chunks.push_back({voff[i], ve});
        else B.chunks.back().end = ve;
        B.last_vend = ve;
        const int64_t w1 = (end - 1) >> kLinShift;
        if ((int64_t)R.lin.size() <= w1) R.lin.resize((size_t)w1 + 1, -1);
        for (int64_t w = beg >> kLinShift; w <= w1; ++w)
            if (R.lin[w] < 0 || voff[i] < R.lin[w]) R.lin[w] = voff[i];
    }
    long n_bins = 0, n_chunks = 0, n_intv = 0;
    int64_t total = kBaiHead + 8;
    for (Ref &R : refs) {
        for (size_t w = R.lin.size(); w-- > 1;)     // untouched windows: the next touched one on the right
            if (R.lin[w - 1] < 0) R.lin[w - 1] = R.lin[w];
        int64_t nc = 0;
        for (auto &kv : R.bins) nc += (int64_t)kv.second.chunks.size();
        total += ref_bytes((int64_t)R.bins.size(), nc, R.has, (int64_t)R.lin.size());
        n_bins += (long)R.bins.size(); n_chunks += (long)nc; n_intv += (long)R.lin.size();
    }
    std::vector<uint8_t> bai((size_t)total);
    int64_t at = 0;
    put32(bai.data(), 0, 0x01494142u);
    put32(bai.data(), 4, (uint32_t)n_ref);
    at = kBaiHead;
    for (const Ref &R : refs) {
        put32(bai.data(), at, (uint32_t)(R.bins.size() + (R.has ? 1 : 0))); at += 4;
        for (const auto &kv : R.bins) {
            put32(bai.data(), at, kv.first); put32(bai.data(), at + 4, (uint32_t)kv.second.chunks.size()); at += 8;
            for (const Chunk &c : kv.second.chunks) { put64(bai.data(), at, (uint64_t)c.beg); put64(bai.data(), at + 8, (uint64_t)c.end); at += 16; }
        }
        if (R.has) {
            put32(bai.data(), at, kPseudoBin); put32(bai.data(), at + 4, 2);
            put64(bai.data(), at + 8, (uint64_t)R.first_voff); put64(bai.data(), at + 16, (uint64_t)R.last_vend);
            put64(bai.data(), at + 24, R.n_mapped); put64(bai.data(), at + 32, R.n_unmapped);
            at += kPseudoBytes;
        }
        put32(bai.data(), at, (uint32_t)R.lin.size()); at += 4;
        for (int64_t v : R.lin) { put64(bai.data(), at, (uint64_t)v); at += 8; }
    }
    put64(bai.data(), at, n_no_coor); at += 8;
    if (at != total) { fprintf(stderr, "layout: %lld bytes written, %lld planned\n", (long long)at, (long long)total); return 3; }
    write_file(argv[5], bai.data(), bai.size());
    printf("bins %ld chunks %ld intv %ld no_coor %llu bytes %lld\n", n_bins, n_chunks, n_intv, (unsigned long long)n_no_coor, (long long)total);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 8 && !strcmp(argv[1], "sort") && atoi(argv[2]) > 0) return model_sort(atoi(argv[2]), argv + 3);
    if (argc == 9 && !strcmp(argv[1], "index") && atoi(argv[2]) > 0) return model_index(atoi(argv[2]), argv + 3);
    fprintf(stderr, "usage: bamsort_model sort N_REF BAM OFF OUT OUT_OFF PERM\n"
                    "       bamsort_model index N_REF BAM OFF VOFF END_VOFF REF_LEN BAI\n");
    return 2;
}
