// markdup_model.cpp -- the serial model of the duplicate-marking kernels (bwa-mem2-arm_amd/csrc/bsw_markdup.hip): the
// kernels' own per-read and per-pair functions (bsw_markdup_k.h) run one read after the other over files.  No GPU.
//   g++ -O2 -std=c++17 -I bwa-mem2-arm_amd/csrc tools/markdup_model.cpp -o markdup_model
//   markdup_model N_READS N_REC N_ALN CIGAR_STRIDE PAIRED L_PAC MIN_QUAL FLAGS RECS REC_FIRST ALN CIGAR READ_OFF READ_LEN
//                 QUALS CTG_LEN OUT_RECS OUT_DUP
//     RECS: bsw_rec_t[N_REC]; REC_FIRST: int32[N_READS + 1]; ALN: bsw_aln_t[N_ALN]; CIGAR: uint32[N_ALN * CIGAR_STRIDE];
//     READ_OFF: int64[N_READS]; READ_LEN: int32[N_READS]; QUALS: the bytes, or - for none; CTG_LEN: int64[n_ctg] the
//     contig table's lengths, or - for no table.  Writes the marked records and uint8[N_READS]; prints
//     "cand C pair_cand P dup_pairs D dup_frag F dup_frag_by_pair B pair_sets S end_sets E flagged G pair_bits X
//      end_bits Y pair_route R end_route Q"
// Exit status 34: what the library answers with BSW_E_RANGE; 22: BSW_E_INVAL; 2: usage or I/O.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>
#include "bsw_markdup_k.h"

using namespace bsw::markdup;

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
    fprintf(stderr, "BSW_E_RANGE: %s at read %ld\n", what, i);
    return 34;
}

struct Sorted {                         // one sort of the stage: the order, the varying bits, the route
    std::vector<int32_t> perm;
    int bits = 0, route = 0;
};

// the stable sort of the members by their words, most significant first, by the route the library takes
template <size_t W>
static Sorted sort_words(const std::vector<uint64_t> (&w)[W])
{
    Sorted s;
    const size_t n = w[0].size();
    s.perm.resize(n);
    std::iota(s.perm.begin(), s.perm.end(), 0);
    if (n == 0) return s;
    uint64_t mask[W];
    for (size_t q = 0; q < W; ++q) {
        uint64_t or_ = 0, nor_ = 0;
        for (size_t j = 0; j < n; ++j) { or_ |= w[q][j]; nor_ |= ~w[q][j]; }
        mask[q] = or_ & nor_;
        s.bits += bit_count(mask[q]);
    }
    if (s.bits == 0) return s;
    if (s.bits <= 64) {
        s.route = 1;
        std::vector<uint64_t> key(n, 0);
        for (size_t j = 0; j < n; ++j)
            for (size_t q = 0; q < W; ++q) {
                const int b = bit_count(mask[q]);
                if (b) key[j] = (b < 64 ? key[j] << b : 0) | pack_bits(w[q][j], mask[q]);
            }
        std::stable_sort(s.perm.begin(), s.perm.end(), [&](int32_t x, int32_t y) { return key[x] < key[y]; });
        return s;
    }
    s.route = 2;
    for (size_t q = W; q-- > 0;) {
        if (!mask[q]) continue;
        int lo, hi;
        mask_span(mask[q], &lo, &hi);
        const uint64_t span = (hi - lo < 64 ? ((uint64_t)1 << (hi - lo)) - 1 : ~(uint64_t)0) << lo;
        std::stable_sort(s.perm.begin(), s.perm.end(), [&](int32_t x, int32_t y) { return (w[q][x] & span) < (w[q][y] & span); });
    }
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 19) { fprintf(stderr, "usage: see the head of tools/markdup_model.cpp\n"); return 2; }
    const int32_t n_reads = atoi(argv[1]), n_rec = atoi(argv[2]), n_aln = atoi(argv[3]), stride = atoi(argv[4]), paired = atoi(argv[5]);
    const int64_t l_pac = atoll(argv[6]);
    const int32_t min_qual = atoi(argv[7]);
    const long flags = atol(argv[8]);
    std::vector<bsw_rec_t> recs = read_file<bsw_rec_t>(argv[9]);
    const std::vector<int32_t> rec_first = read_file<int32_t>(argv[10]);
    const std::vector<bsw_aln_t> aln = read_file<bsw_aln_t>(argv[11]);
    const std::vector<uint32_t> cigar = read_file<uint32_t>(argv[12]);
    const std::vector<int64_t> read_off = read_file<int64_t>(argv[13]);
    const std::vector<int32_t> read_len = read_file<int32_t>(argv[14]);
    const bool has_quals = strcmp(argv[15], "-") != 0, has_ctg = strcmp(argv[16], "-") != 0;
    const std::vector<uint8_t> quals = has_quals ? read_file<uint8_t>(argv[15]) : std::vector<uint8_t>();
    std::vector<int64_t> ctg_off(1, 0);
    if (has_ctg)
        for (int64_t len : read_file<int64_t>(argv[16])) ctg_off.push_back(ctg_off.back() + len);
    const int32_t n_ctg = (int32_t)ctg_off.size() - 1;
    if (l_pac <= 0 || l_pac > kMaxLPac || min_qual < 0 || flags || n_rec < 0 || n_aln < 0 || n_reads < 0 || stride < 1 ||
        (paired && (n_reads & 1)) || (has_ctg && (ctg_off.back() != l_pac || n_ctg > kMaxContigs || n_ctg < 1)))
        return 22;
    if (n_reads > 0 && ((int64_t)rec_first.size() != (int64_t)n_reads + 1 || (int32_t)read_off.size() != n_reads ||
                        (int32_t)read_len.size() != n_reads))
        return 2;
    if ((int32_t)recs.size() != n_rec || (int32_t)aln.size() != n_aln || (int64_t)cigar.size() != (int64_t)n_aln * stride) return 2;
    const bsw::ContigView ctg{ctg_off.data(), nullptr, nullptr, n_ctg, l_pac};
    const size_t N = (size_t)n_reads, P = paired ? N / 2 : 0;

    // scores, checks, candidates and end words: md_score_kernel and md_end_kernel
    std::vector<int32_t> score(N, 0);
    std::vector<uint64_t> eword(N, 0);
    std::vector<uint8_t> cand(N, 0);
    for (int32_t i = 0; i < n_reads; ++i) {
        if (has_quals) {
            const int64_t off = read_off[i], len = read_len[i];
            if (!extent_ok(off, len, (int64_t)quals.size())) return range_error("read extent", i);
            score[i] = score_clamp(score_span(quals.data(), (int64_t)quals.size(), off, off + len, min_qual, 0, 1));
        }
        const int32_t f0 = rec_first[i], f1 = rec_first[i + 1];
        if (f0 < 0 || f1 < f0 || f1 > n_rec || (i == 0 && f0 != 0) || (i == n_reads - 1 && f1 != n_rec)) return range_error("rec_first", i);
        for (int32_t k = f0; k < f1; ++k)
            if (recs[k].read != i || recs[k].aln < -1 || recs[k].aln >= n_aln) return range_error("record", i);
        if (f1 == f0 || !candidate(recs[f0].flag)) continue;
        const bsw_rec_t &r = recs[f0];
        const int32_t nc = r.aln >= 0 ? aln[r.aln].n_cigar : 0;
        if (r.aln < 0 || r.pos < 0 || r.pos >= l_pac || nc <= 0 || nc > stride) return range_error("candidate", i);
        const int64_t u = unclipped5(r.pos, r.is_rev, cigar.data() + (size_t)r.aln * stride, nc);
        if (!u_ok(u)) return range_error("u", i);
        eword[i] = end_word(has_ctg ? bsw::contig_rid(ctg, r.pos) : 0, u, r.is_rev);
        cand[i] = 1;
    }

    // the compact key words: md_key_kernel
    std::vector<uint64_t> pkey[3], ekey[2];
    std::vector<int32_t> pid, cid;
    std::vector<uint8_t> in_pair(N, 0);
    for (size_t p = 0; p < P; ++p) {
        if (!cand[2 * p] || !cand[2 * p + 1]) continue;
        in_pair[2 * p] = in_pair[2 * p + 1] = 1;
        const uint64_t x = eword[2 * p], y = eword[2 * p + 1];
        pkey[0].push_back(std::min(x, y));
        pkey[1].push_back(std::max(x, y));
        pkey[2].push_back(score_field((uint32_t)score[2 * p] + (uint32_t)score[2 * p + 1]));
        pid.push_back((int32_t)p);
    }
    for (size_t i = 0; i < N; ++i) {
        if (!cand[i]) continue;
        ekey[0].push_back(eword[i]);
        ekey[1].push_back(end_rank(!in_pair[i], (uint32_t)score[i]));
        cid.push_back((int32_t)i);
    }
    const Sorted sp = sort_words(pkey), se = sort_words(ekey);

    // set heads and marks: md_head_kernel, md_pair_mark_kernel, md_end_mark_kernel
    std::vector<uint8_t> dup(N, 0);
    long dup_pairs = 0, dup_frag = 0, dup_by_pair = 0, pair_sets = 0, end_sets = 0, flagged = 0;
    const size_t n_pc = pid.size(), n_c = cid.size();
    auto pair_head = [&](size_t j) {
        return j == 0 || pkey[0][sp.perm[j]] != pkey[0][sp.perm[j - 1]] || pkey[1][sp.perm[j]] != pkey[1][sp.perm[j - 1]];
    };
    size_t phead = 0;
    for (size_t j = 0; j < n_pc; ++j) {
        if (pair_head(j)) phead = j;
        if (!pair_head(j)) {
            const int32_t p = pid[sp.perm[j]], w = pid[sp.perm[phead]];
            // the sort's order states the winner rule: the head beats every other member
            if (!wins(~(uint32_t)pkey[2][sp.perm[phead]], w, ~(uint32_t)pkey[2][sp.perm[j]], p)) { fprintf(stderr, "winner rule at pair %d\n", p); return 3; }
            dup[2 * p] = dup[2 * p + 1] = kDupPair;
            ++dup_pairs;
        } else if (j + 1 < n_pc && !pair_head(j + 1)) {
            ++pair_sets;
        }
    }
    size_t head = 0;
    for (size_t j = 0; j < n_c; ++j) {
        const int32_t c = se.perm[j];
        if (j == 0 || ekey[0][c] != ekey[0][se.perm[j - 1]]) {
            head = j;
            if (j + 1 < n_c && ekey[0][se.perm[j + 1]] == ekey[0][c]) ++end_sets;
        }
        if (!(ekey[1][c] >> 32)) continue;
        const bool head_is_pair = !(ekey[1][se.perm[head]] >> 32);
        const int d = head_is_pair ? kDupFragByPair : j != head ? kDupFrag : 0;
        if (d == kDupFrag && !wins(~(uint32_t)ekey[1][se.perm[head]], cid[se.perm[head]], ~(uint32_t)ekey[1][c], cid[c])) {
            fprintf(stderr, "winner rule at read %d\n", cid[c]);
            return 3;
        }
        if (d) {
            dup[cid[c]] = (uint8_t)d;
            ++(head_is_pair ? dup_by_pair : dup_frag);
        }
    }
    // md_mark_kernel
    for (bsw_rec_t &r : recs) {
        const int32_t f = r.flag;
        r.flag = marked_flag(f, f, dup[r.read]);
        r.sam_flag = marked_flag(r.sam_flag, f, dup[r.read]);
        flagged += (r.flag & 0x400) != 0;
    }
    write_file(argv[17], recs.data(), recs.size() * sizeof(bsw_rec_t));
    write_file(argv[18], dup.data(), dup.size());
    printf("cand %zu pair_cand %zu dup_pairs %ld dup_frag %ld dup_frag_by_pair %ld pair_sets %ld end_sets %ld flagged %ld "
           "pair_bits %d end_bits %d pair_route %d end_route %d\n",
           n_c, n_pc, dup_pairs, dup_frag, dup_by_pair, pair_sets, end_sets, flagged, sp.bits, se.bits, sp.route, se.route);
    return 0;
}
