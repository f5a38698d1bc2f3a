// bsw_bgzf_k.h -- the BGZF encoder (include/bsw_bgzf.h) but for what needs LDS or a wave: every function here
// compiles for the host and for the device.  bsw_bgzf.hip runs them with 256 lanes per block of input,
// tools/bgzf_model.cpp runs the same functions serially (the kernel's serial model: same tables, same
// tokens, same bytes).
//
// A block of n <= 0xff00 input bytes is 256 strips of 255 bytes; strip s is tokenised front to back on its
// own (lane s), matches end at the strip's end.  Candidates come from two tables that a pass of their own
// fills before any strip is tokenised, each entry an order-free minimum or maximum of positions, so the
// tokens depend on the bytes alone:
//   seg_last[g][h8]  the last position + 1 in segment g (4 strips, 1020 bytes) whose 3 bytes hash to h8
//   first[h11]       the first position in the block whose 3 bytes hash to h11
// A position tries p - 1 (runs), its own and the three segments before it, and `first`; a candidate at
// or behind p, or further back than 32,768, is refused.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BGZF_HD __host__ __device__ inline
#else
#define BGZF_HD inline
#endif

namespace bsw {
namespace bgzf {

constexpr int kStrip = 255, kStrips = 256;
constexpr int kMaxChunk = kStrip * kStrips;         // 0xff00
constexpr int kStageStride = 65536;                 // a block's room in the staging: header + deflate + trailer <= 65,311
constexpr int kHdrBytes = 18, kTrailerBytes = 8, kEofBytes = 28;
constexpr int kSegStrips = 4, kSeg = kStrip * kSegStrips, kNSeg = kStrips / kSegStrips;
constexpr int kSegBits = 8, kSegBuckets = 1 << kSegBits;
constexpr int kFirstBits = 11, kFirstBuckets = 1 << kFirstBits;
constexpr int kProbeSegs = 3;                       // segments before the position's own that are probed
constexpr int kWindow = 32768, kMinMatch = 3, kMaxMatch = 258;
constexpr int kNLL = 288, kLLUsed = 286, kND = 32, kNDUsed = 30, kNCL = 19;
constexpr int kTokPerBlock = kStrip * kStrips;      // 16-bit token units: a literal 1, a match 2 (>= 3 bytes)
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kStored = 0, kFixed = 1, kDynamic = 2;

// ---------------------------------------------------------------- order-free table updates
BGZF_HD void hist_add(uint32_t *p, uint32_t v = 1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BGZF_HD void min_u32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
// tab[idx] = max(tab[idx], v) on 16-bit entries (the device: a compare-and-swap on the entry's dword)
BGZF_HD void max_u16(uint16_t *tab, int idx, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t *w = (uint32_t *)tab + (idx >> 1);
    const int sh = (idx & 1) * 16;
    uint32_t old = *w;
    while (((old >> sh) & 0xffffu) < v) {
        const uint32_t nw = (old & ~(0xffffu << sh)) | (v << sh);
        const uint32_t prev = atomicCAS(w, old, nw);
        if (prev == old) break;
        old = prev;
    }
#else
    if (tab[idx] < v) tab[idx] = (uint16_t)v;
#endif
}
// base[pos] |= v where other writers may OR into the same byte (and store the dword's other bytes)
BGZF_HD void or_byte(uint8_t *base, int64_t pos, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr((unsigned int *)(base + (pos & ~(int64_t)3)), v << (8 * (int)(pos & 3)));   // base is 4-byte aligned
#else
    base[pos] |= (uint8_t)v;
#endif
}

// ---------------------------------------------------------------- CRC-32 (reflected, 0xEDB88320)
constexpr uint32_t kCrcPoly = 0xEDB88320u;
BGZF_HD uint32_t crc_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1) ? kCrcPoly : 0);
    return i;
}
// the CRC of n bytes (conditioned as zlib's crc32: ~0 in, ~0 out); n == 0 gives 0
BGZF_HD uint32_t crc_bytes(const uint32_t *tab, const uint8_t *p, int n)
{
    uint32_t c = 0xffffffffu;
    int i = 0;
    for (; i + 4 <= n; i += 4) {                        // (a word per load: see load32)
        uint32_t w;
        __builtin_memcpy(&w, p + i, 4);
        for (int k = 0; k < 4; ++k, w >>= 8) c = tab[(c ^ w) & 0xff] ^ (c >> 8);
    }
    for (; i < n; ++i) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return ~c;
}
// a * b mod P, polynomials with x^0 at bit 31
BGZF_HD uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? kCrcPoly : 0);
    }
    return p;
}
// x^(8 m) mod P
BGZF_HD uint32_t crc_xpow8(uint32_t m)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;       // x^0, x^8
    for (; m; m >>= 1) {
        if (m & 1) r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}
// the share of a piece's CRC in the CRC of the whole, `after` bytes behind the piece: the whole's CRC is
// the XOR of its pieces' shares
BGZF_HD uint32_t crc_share(uint32_t crc_piece, uint32_t after) { return crc_mul(crc_piece, crc_xpow8(after)); }

// ---------------------------------------------------------------- symbols
BGZF_HD int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }
// match length 3..258 -> literal/length symbol 257..285, its extra bits and their value
BGZF_HD void len_sym(int len, int &sym, int &eb, int &ev)
{
    const int m = len - 3;
    if (len == 258) { sym = 285; eb = 0; ev = 0; return; }
    if (m < 8) { sym = 257 + m; eb = 0; ev = 0; return; }
    eb = ilog2((uint32_t)m) - 2;
    sym = 257 + 4 * (eb + 1) + ((m >> eb) & 3);
    ev = m & ((1 << eb) - 1);
}
// distance 1..32768 -> distance symbol 0..29
BGZF_HD void dist_sym(int dist, int &sym, int &eb, int &ev)
{
    const int d = dist - 1;
    if (d < 4) { sym = d; eb = 0; ev = 0; return; }
    eb = ilog2((uint32_t)d) - 1;
    sym = 2 * (eb + 1) + ((d >> eb) & 1);
    ev = d & ((1 << eb) - 1);
}
BGZF_HD int fixed_ll_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// ---------------------------------------------------------------- tables and tokens
BGZF_HD uint32_t hash3(const uint8_t *p)
{
    return ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16) * 2654435761u;
}
BGZF_HD void tables_clear(uint16_t *seg_last, uint32_t *first, int i)     // entry i of both (i < kNSeg * kSegBuckets)
{
    seg_last[i] = 0;
    if (i < kFirstBuckets) first[i] = kNone;
}
// position p of in[0, n), p + 3 <= n, into both tables.  A position whose neighbour in the same entry
// wins anyway is skipped: runs of one byte would otherwise put every position of a block into one entry
BGZF_HD void table_insert(const uint8_t *in, int n, int p, uint16_t *seg_last, uint32_t *first)
{
    const uint32_t h = hash3(in + p);
    if (!(p > 0 && hash3(in + p - 1) >> (32 - kFirstBits) == h >> (32 - kFirstBits)))
        min_u32(&first[h >> (32 - kFirstBits)], (uint32_t)p);
    const int g = p / kSeg;
    if (p + 4 <= n && (p + 1) / kSeg == g && hash3(in + p + 1) >> (32 - kSegBits) == h >> (32 - kSegBits)) return;
    max_u16(seg_last, g * kSegBuckets + (int)(h >> (32 - kSegBits)), (uint32_t)p + 1);
}

// What a literal costs, in eighths of a bit, when f of the block's n bytes are this byte: 8 log2(n / f) with the
// mantissa taken as linear, at least one bit.  Integers only: the model and the kernel agree.
BGZF_HD uint32_t lit_cost8(uint32_t n, uint32_t f)
{
    const uint32_t q = (n << 8) / f;                    // >= 256
    const int e = ilog2(q);
    const uint32_t c = (uint32_t)(e - 8) * 8 + (((q << 3) >> e) & 7);
    return c < 8 ? 8 : c;
}

// Four bytes at in + i as a little-endian word, whatever the alignment.  Lanes walk strips of their own, so
// every load instruction of a wave touches 64 cache lines: the tokeniser is bound by the number of its loads,
// and reads words where it can.
BGZF_HD uint32_t load32(const uint8_t *in, int i)
{
    uint32_t v;
    __builtin_memcpy(&v, in + i, 4);
    return v;
}
// the same where the block may end inside the word: the bytes behind in[n - 1] read as 0
BGZF_HD uint32_t load32_end(const uint8_t *in, int i, int n)
{
    if (i + 4 <= n) return load32(in, i);
    uint32_t v = 0;
    for (int k = 0; i + k < n; ++k) v |= (uint32_t)in[i + k] << (8 * k);
    return v;
}

// candidate c for position p (wp: the word at p, maxlen >= 3 bytes of it inside the strip): the longer match wins,
// then the nearer.  A candidate with fewer than 3 equal bytes is no match.
BGZF_HD void consider(const uint8_t *in, int p, uint32_t wp, int c, int maxlen, int &best_len, int &best_dist)
{
    if (c < 0 || c >= p || p - c > kWindow) return;
    if ((load32(in, c) ^ wp) & 0xffffffu) return;        // (c + 4 <= p + 3 <= the strip's end)
    if (best_len >= kMinMatch && in[c + best_len - 1] != in[p + best_len - 1]) return;    // cannot be longer
    int l = kMinMatch;
    while (l + 4 <= maxlen) {
        const uint32_t x = load32(in, c + l) ^ load32(in, p + l);
        if (x) { l += __builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    if (l + 4 > maxlen)                                 // (not left through the break: l + 4 <= maxlen there)
        while (l < maxlen && in[c + l] == in[p + l]) ++l;
    if (l > best_len || (l == best_len && p - c < best_dist)) { best_len = l; best_dist = p - c; }
}

// Strip [s0, s1) of in[0, n) into 16-bit units tok[0], tok[stride], ...: a literal is its byte; a match is
// 0x8000 | (len - 3), then dist - 1.  A match is taken when its bytes as literals (cost[]: lit_cost8 of the
// block's byte counts) would cost more than a length code of 8 bits, a distance code of 5 and the extra bits:
// low-entropy bytes (QUAL) keep their short literal codes, and a whole block of one byte still matches.
// Counts the symbols into hll / hd and the bits of the fixed form into *fixed_bits.  Returns the units.
BGZF_HD int tokenise_strip(const uint8_t *in, int n, int s0, int s1, const uint16_t *seg_last, const uint32_t *first,
                           const uint8_t *cost, uint16_t *tok, int stride, uint32_t *hll, uint32_t *hd,
                           uint32_t *fixed_bits)
{
    int p = s0, k = 0;
    uint32_t fb = 0;
    while (p < s1) {
        const int maxlen = s1 - p < kMaxMatch ? s1 - p : kMaxMatch;
        int best_len = 0, best_dist = 0;
        if (maxlen >= kMinMatch) {
            const uint32_t wp = load32_end(in, p, n);
            consider(in, p, wp, p - 1, maxlen, best_len, best_dist);
            const uint32_t h = (wp & 0xffffffu) * 2654435761u;  // hash3(in + p)
            const int g = p / kSeg, b8 = (int)(h >> (32 - kSegBits));
            for (int j = 0; j <= kProbeSegs && j <= g; ++j) {
                const int v = seg_last[(g - j) * kSegBuckets + b8];
                if (v) consider(in, p, wp, v - 1, maxlen, best_len, best_dist);
            }
            const uint32_t f = first[h >> (32 - kFirstBits)];
            if (f != kNone) consider(in, p, wp, (int)f, maxlen, best_len, best_dist);
        }
        int ls = 0, leb = 0, lev = 0, ds = 0, deb = 0, dev = 0;
        bool take = false;
        if (best_len >= kMinMatch) {
            len_sym(best_len, ls, leb, lev);
            dist_sym(best_dist, ds, deb, dev);
            uint32_t lits = 0;
            int i = 0;
            for (; i + 4 <= best_len; i += 4) {
                const uint32_t w = load32(in, p + i);
                lits += cost[w & 0xff] + cost[(w >> 8) & 0xff] + cost[(w >> 16) & 0xff] + cost[w >> 24];
            }
            for (; i < best_len; ++i) lits += cost[in[p + i]];
            take = lits > 8u * (uint32_t)(8 + leb + 5 + deb);
        }
        if (take) {
            tok[(size_t)k * stride] = (uint16_t)(0x8000 | (best_len - kMinMatch));
            tok[(size_t)(k + 1) * stride] = (uint16_t)(best_dist - 1);
            k += 2;
            hist_add(&hll[ls]);
            hist_add(&hd[ds]);
            fb += (uint32_t)(fixed_ll_len(ls) + leb + 5 + deb);
            p += best_len;
        } else {
            const int c = in[p];
            tok[(size_t)k * stride] = (uint16_t)c;
            k += 1;
            hist_add(&hll[c]);
            fb += (uint32_t)fixed_ll_len(c);
            p += 1;
        }
    }
    *fixed_bits = fb;
    return k;
}

// ---------------------------------------------------------------- code lengths
// the place of symbol s among the used symbols in the order (freq, symbol); kNone when unused
BGZF_HD uint32_t sym_rank(const uint32_t *freq, int n, int s)
{
    const uint32_t f = freq[s];
    if (!f) return kNone;
    uint32_t r = 0;
    for (int t = 0; t < n; ++t) {
        const uint32_t ft = freq[t];
        r += ft && (ft < f || (ft == f && t < s));
    }
    return r;
}
// sorted[] by sym_rank, serially; returns the used symbols
BGZF_HD int sort_syms(const uint32_t *freq, int n, uint16_t *sorted)
{
    int m = 0;
    for (int s = 0; s < n; ++s) {
        const uint32_t r = sym_rank(freq, n, s);
        if (r != kNone) { sorted[r] = (uint16_t)s; ++m; }
    }
    return m;
}
// Huffman code lengths <= limit for the m used symbols sorted[0, m) (ascending by frequency) of n, the rest
// 0.  Two queues over the sorted leaves build the tree; while it is deeper than the limit the weights are
// halved (rounded up, at least 1: the order holds) and it is built again -- equal weights end it at depth
// ceil(log2 m).  Every result is a full tree: the Kraft sum is exactly 1.  One used symbol: length 1.
// w, par: 2 m entries each.
BGZF_HD void code_lengths(const uint32_t *freq, const uint16_t *sorted, int m, int n, int limit, uint8_t *len, uint32_t *w,
                          uint16_t *par)
{
    for (int s = 0; s < n; ++s) len[s] = 0;
    if (m == 0) return;
    if (m == 1) { len[sorted[0]] = 1; return; }
    for (int shift = 0;; ++shift) {
        for (int i = 0; i < m; ++i) w[i] = ((freq[sorted[i]] - 1) >> shift) + 1;
        int li = 0, ii = m, ie = m;
        for (int k = 0; k < m - 1; ++k) {
            uint32_t sum = 0;
            for (int t = 0; t < 2; ++t) {
                const int a = (li < m && (ii >= ie || w[li] <= w[ii])) ? li++ : ii++;
                sum += w[a];
                par[a] = (uint16_t)ie;
            }
            w[ie++] = sum;
        }
        const int root = ie - 1;
        par[root] = 0;
        for (int i = root - 1; i >= 0; --i) par[i] = (uint16_t)(par[par[i]] + 1);     // parents lie above: depths now
        int deepest = 0;
        for (int i = 0; i < m; ++i) deepest = par[i] > deepest ? par[i] : deepest;
        if (deepest <= limit) {
            for (int i = 0; i < m; ++i) len[sorted[i]] = (uint8_t)par[i];
            return;
        }
    }
}
BGZF_HD uint32_t bit_reverse(uint32_t v, int n)      // the low n <= 16 bits of v reversed
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}
// canonical codes of the lengths, bit-reversed for the LSB-first stream.  wk: 32 words
BGZF_HD void canon_codes(const uint8_t *len, int n, uint16_t *code, uint32_t *wk)
{
    uint32_t *count = wk, *next = wk + 16;
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int s = 0; s < n; ++s) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)bit_reverse(next[len[s]]++, len[s]) : 0;
}
// the code lengths lens[0, nl) as symbols of the code-length alphabet: out[i] = symbol | extra << 8
// (16: repeat the last 3..6 times, 17: 3..10 zeros, 18: 11..138 zeros); counts them into hcl.  Returns the entries.
BGZF_HD int cl_runs(const uint8_t *lens, int nl, uint16_t *out, uint32_t *hcl)
{
    int i = 0, k = 0;
    while (i < nl) {
        const int v = lens[i];
        int run = 1;
        while (i + run < nl && lens[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                out[k++] = (uint16_t)(18 | (r - 11) << 8); hcl[18]++;
                run -= r;
            }
            if (run >= 3) { out[k++] = (uint16_t)(17 | (run - 3) << 8); hcl[17]++; run = 0; }
        } else {
            out[k++] = (uint16_t)v; hcl[v]++;
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                out[k++] = (uint16_t)(16 | (r - 3) << 8); hcl[16]++;
                run -= r;
            }
        }
        for (; run > 0; --run) { out[k++] = (uint16_t)v; hcl[v]++; }
    }
    return k;
}
BGZF_HD int cl_order(int i)                            // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                        10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}
BGZF_HD int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// ---------------------------------------------------------------- bits
// Writes the bits [bit0, ...) of a stream that starts at base + byte0, LSB first.  Several writers share a
// stream, each with a range of its own: a byte that a range covers whole is stored, the partial byte at
// either end is ORed in (the stream's bytes are zero before).
struct BitW {
    uint8_t *base;
    int64_t pos;
    uint64_t acc;
    int nacc;
    bool partial;
    BGZF_HD void init(uint8_t *b, int64_t byte0, uint32_t bit0)
    {
        base = b; pos = byte0 + (bit0 >> 3); acc = 0; nacc = (int)(bit0 & 7); partial = nacc != 0;
    }
    BGZF_HD void put(uint32_t v, int n)                 // n <= 16
    {
        acc |= (uint64_t)v << nacc;
        nacc += n;
        while (nacc >= 8) {
            if (partial) { or_byte(base, pos, (uint32_t)(acc & 0xff)); partial = false; }
            else base[pos] = (uint8_t)acc;
            ++pos;
            acc >>= 8;
            nacc -= 8;
        }
    }
    BGZF_HD void finish()
    {
        if (nacc > 0 && acc) or_byte(base, pos, (uint32_t)(acc & 0xff));
    }
};

// ---------------------------------------------------------------- a block's tables (the kernel: in LDS)
struct Tables {
    uint32_t hll[kNLL], hd[kND], hcl[20];
    uint32_t hbyte[256];                                // the block's bytes, counted before the tokens
    uint32_t w[2 * kNLL];
    uint32_t wk[32];
    uint32_t bits_fix[kStrips + 1], bits_dyn[kStrips + 1];      // per strip; after plan_block() the bit offsets of the chosen form
    uint32_t crc, m_ll, m_d;
    uint32_t hdr_bits, deflate_bytes;
    int32_t form, hlit, hdist, hclen, n_seq;
    uint16_t ll_code[kNLL], d_code[kND], cl_code[20];
    uint16_t sorted_ll[kNLL], sorted_d[kND], sorted_cl[20];
    uint16_t par[2 * kNLL];
    uint16_t cl_seq[kNLL + kND];
    uint8_t ll_len[kNLL], d_len[kND], cl_len[20];
    uint8_t all_len[kNLL + kND];
    uint8_t cost[256];                                  // lit_cost8 per byte value, 0 for a byte the block lacks
};

BGZF_HD void tables_clear_hist(Tables &t, int i)         // word i of the histograms (i < kNLL); one end-of-block
{
    t.hll[i] = i == 256;
    if (i < 256) t.hbyte[i] = 0;
    if (i < kND) t.hd[i] = 0;
    if (i < 20) t.hcl[i] = 0;
}

// the bits of strip tokens tok[0], tok[stride], ... (k units) under the tables' codes
BGZF_HD uint32_t strip_bits(const Tables &t, const uint16_t *tok, int stride, int k)
{
    uint32_t bits = 0;
    for (int i = 0; i < k; ++i) {
        const int u = tok[(size_t)i * stride];
        if (u & 0x8000) {
            int ls, leb, lev, ds, deb, dev;
            len_sym((u & 0xff) + kMinMatch, ls, leb, lev);
            dist_sym(tok[(size_t)(++i) * stride] + 1, ds, deb, dev);
            bits += (uint32_t)(t.ll_len[ls] + leb + t.d_len[ds] + deb);
        } else {
            bits += t.ll_len[u];
        }
    }
    return bits;
}
// the strip's tokens into the stream; eob: the end-of-block symbol behind them
BGZF_HD void strip_write(const Tables &t, const uint16_t *tok, int stride, int k, bool eob, uint8_t *base, int64_t byte0,
                         uint32_t bit0)
{
    BitW bw;
    bw.init(base, byte0, bit0);
    for (int i = 0; i < k; ++i) {
        const int u = tok[(size_t)i * stride];
        if (u & 0x8000) {
            int ls, leb, lev, ds, deb, dev;
            len_sym((u & 0xff) + kMinMatch, ls, leb, lev);
            dist_sym(tok[(size_t)(++i) * stride] + 1, ds, deb, dev);
            bw.put(t.ll_code[ls], t.ll_len[ls]);
            if (leb) bw.put((uint32_t)lev, leb);
            bw.put(t.d_code[ds], t.d_len[ds]);
            if (deb) bw.put((uint32_t)dev, deb);
        } else {
            bw.put(t.ll_code[u], t.ll_len[u]);
        }
    }
    if (eob) bw.put(t.ll_code[256], t.ll_len[256]);
    bw.finish();
}

// The serial part, step 1 (one lane): the histograms (end-of-block counted here) and their sorted symbols
// (m_ll, m_d) -> the dynamic form's code lengths, the code-length code, the codes, hdr_bits.
BGZF_HD void plan_codes(Tables &t)
{
    code_lengths(t.hll, t.sorted_ll, (int)t.m_ll, kLLUsed, 15, t.ll_len, t.w, t.par);
    code_lengths(t.hd, t.sorted_d, (int)t.m_d, kNDUsed, 15, t.d_len, t.w, t.par);
    for (int s = kLLUsed; s < kNLL; ++s) t.ll_len[s] = 0;
    for (int s = kNDUsed; s < kND; ++s) t.d_len[s] = 0;
    int hlit = 257, hdist = 1;
    for (int s = 257; s < kLLUsed; ++s) if (t.ll_len[s]) hlit = s + 1;
    for (int s = 1; s < kNDUsed; ++s) if (t.d_len[s]) hdist = s + 1;
    t.hlit = hlit; t.hdist = hdist;
    for (int s = 0; s < hlit; ++s) t.all_len[s] = t.ll_len[s];
    for (int s = 0; s < hdist; ++s) t.all_len[hlit + s] = t.d_len[s];
    t.n_seq = cl_runs(t.all_len, hlit + hdist, t.cl_seq, t.hcl);
    int m_cl = sort_syms(t.hcl, kNCL, t.sorted_cl);
    if (m_cl == 1) {                                    // an incomplete code-length code is not legal: a second, unused code
        const int other = t.sorted_cl[0] == 0 ? 1 : 0;
        t.hcl[other] = 1;
        m_cl = sort_syms(t.hcl, kNCL, t.sorted_cl);
    }
    code_lengths(t.hcl, t.sorted_cl, m_cl, kNCL, 7, t.cl_len, t.w, t.par);
    int hclen = 4;
    for (int i = 4; i < kNCL; ++i) if (t.cl_len[cl_order(i)]) hclen = i + 1;
    t.hclen = hclen;
    uint32_t hb = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int i = 0; i < t.n_seq; ++i) hb += (uint32_t)(t.cl_len[t.cl_seq[i] & 0xff] + cl_extra_bits(t.cl_seq[i] & 0xff));
    t.hdr_bits = hb;
    canon_codes(t.ll_len, kNLL, t.ll_code, t.wk);
    canon_codes(t.d_len, kND, t.d_code, t.wk);
    canon_codes(t.cl_len, kNCL, t.cl_code, t.wk);
}

// Step 2 (one lane), with bits_fix[s] / bits_dyn[s] the token bits of strip s (end-of-block not counted):
// the smallest of the three forms, ties to the simpler; level 0: stored.  Leaves form, deflate_bytes, the
// chosen form's codes in ll_* / d_* and hdr_bits, and in bits_dyn[s] the bit offset of strip s's tokens in
// the deflate stream; writes the block's header (the gzip member's 18 bytes and the deflate block's) into out.
BGZF_HD void plan_block(Tables &t, int n, int level, uint8_t *out)
{
    uint32_t tot_fix = 0, tot_dyn = 0;
    for (int s = 0; s < kStrips; ++s) { tot_fix += t.bits_fix[s]; tot_dyn += t.bits_dyn[s]; }
    const uint32_t stored = 5 + (uint32_t)n;
    const uint32_t fixed = (3 + tot_fix + 7 + 7) >> 3;
    const uint32_t dynamic = (t.hdr_bits + tot_dyn + t.ll_len[256] + 7) >> 3;
    int form = kStored;
    uint32_t best = stored;
    if (level != 0) {
        if (fixed < best) { form = kFixed; best = fixed; }
        if (dynamic < best) { form = kDynamic; best = dynamic; }
    }
    t.form = form;
    t.deflate_bytes = best;
    const uint32_t bsize = kHdrBytes + best + kTrailerBytes - 1;
    const uint8_t hdr[kHdrBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    for (int i = 0; i < kHdrBytes; ++i) out[i] = hdr[i];
    if (form == kStored) {
        out[kHdrBytes] = 1;
        out[kHdrBytes + 1] = (uint8_t)n; out[kHdrBytes + 2] = (uint8_t)(n >> 8);
        out[kHdrBytes + 3] = (uint8_t)~n; out[kHdrBytes + 4] = (uint8_t)(~n >> 8);
        return;
    }
    BitW bw;
    bw.init(out, kHdrBytes, 0);
    if (form == kFixed) {
        for (int s = 0; s < kNLL; ++s) t.ll_len[s] = (uint8_t)fixed_ll_len(s);
        for (int s = 0; s < kND; ++s) t.d_len[s] = 5;
        canon_codes(t.ll_len, kNLL, t.ll_code, t.wk);
        canon_codes(t.d_len, kND, t.d_code, t.wk);
        t.hdr_bits = 3;
        bw.put(1 | 1 << 1, 3);
    } else {
        bw.put(1 | 2 << 1, 3);
        bw.put((uint32_t)(t.hlit - 257), 5);
        bw.put((uint32_t)(t.hdist - 1), 5);
        bw.put((uint32_t)(t.hclen - 4), 4);
        for (int i = 0; i < t.hclen; ++i) bw.put(t.cl_len[cl_order(i)], 3);
        for (int i = 0; i < t.n_seq; ++i) {
            const int sym = t.cl_seq[i] & 0xff;
            bw.put(t.cl_code[sym], t.cl_len[sym]);
            if (cl_extra_bits(sym)) bw.put((uint32_t)(t.cl_seq[i] >> 8), cl_extra_bits(sym));
        }
    }
    bw.finish();
    uint32_t off = t.hdr_bits;
    for (int s = 0; s < kStrips; ++s) {
        const uint32_t b = form == kFixed ? t.bits_fix[s] : t.bits_dyn[s];
        t.bits_dyn[s] = off;
        off += b;
    }
}
// the trailer behind the deflate stream; returns the block's bytes
BGZF_HD uint32_t block_trailer(const Tables &t, int n, uint8_t *out)
{
    uint8_t *p = out + kHdrBytes + t.deflate_bytes;
    for (int i = 0; i < 4; ++i) { p[i] = (uint8_t)(t.crc >> (8 * i)); p[4 + i] = (uint8_t)((uint32_t)n >> (8 * i)); }
    return kHdrBytes + t.deflate_bytes + kTrailerBytes;
}

}  // namespace bgzf

#if defined(__HIPCC__)
// ---------------------------------------------------------------- launch interface (bsw_bgzf.hip)
// meta words (one int32 array, zeroed per call): an error word, then the blocks of each form
constexpr int kBgzfErr = 0, kBgzfStored = 1, kBgzfMetaWords = 8;
constexpr int kBgzfGrid = 768;          // workgroups of the deflate kernel: three per CU (what its LDS admits), each with token scratch of its own
// Blocks b < n_blocks of in[0, n_in), cut at block_bytes, into stage + b * kStageStride (zeroed by the caller:
// strips OR their edge bytes in); bsize[b] = the block's bytes (bsize[n_blocks] = 0).  tok: grid *
// bgzf::kTokPerBlock units.
hipError_t launch_bgzf_deflate(const uint8_t *in, int64_t n_in, int32_t block_bytes, int32_t n_blocks, int32_t level,
                               uint8_t *stage, uint16_t *tok, int32_t grid, int64_t *bsize, int32_t *meta, hipStream_t s);
// voff[i] = (base + blk_off[b]) << 16 | rec_off[i] - b * block_bytes; a rec_off outside [0, n_in] sets meta[kBgzfErr]
hipError_t launch_bgzf_voff(const int64_t *rec_off, int32_t n_rec, int64_t n_in, int32_t block_bytes, const int64_t *blk_off,
                            int64_t base, int64_t *voff, int32_t *meta, hipStream_t s);
// the staged blocks to out + blk_off[b] (out 4-byte aligned); eof: the 28-byte marker at blk_off[n_blocks]
hipError_t launch_bgzf_pack(const uint8_t *stage, const int64_t *blk_off, int32_t n_blocks, bool eof, uint8_t *out,
                            hipStream_t s);
#endif

}  // namespace bsw
