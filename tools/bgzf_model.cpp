// bgzf_model.cpp -- the serial model of the BGZF kernel (bwa-mem2-arm_amd/csrc/bsw_bgzf.hip): the kernel's own
// per-strip and per-block functions (bsw_bgzf_k.h) run one after the other over a file.  No GPU.
//   g++ -O2 -std=c++17 -I bwa-mem2-arm_amd/csrc tools/bgzf_model.cpp -o bgzf_model
//   bgzf_model [--block-bytes N] [--level L] [--eof] IN OUT    IN -> the BGZF stream OUT; prints
//                                                              "blocks B stored S fixed F dynamic D in I out O"
//   bgzf_model --lengths LIMIT F0 F1 ...                       the code lengths of these frequencies, one line
//   bgzf_model --crc-split K IN                                the CRC-32 of IN put together from the CRCs of
//                                                              IN[0, K) and IN[K, ...), as 8 hex digits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "bsw_bgzf_k.h"

using namespace bsw::bgzf;

static std::vector<uint8_t> read_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// one block, the kernel's phases in its order; returns the block's bytes in out (kStageStride, zeroed here)
static uint32_t model_block(const uint8_t *src, int n, int level, const uint32_t *crc_tab, uint8_t *out, int *form)
{
    static uint16_t seg_last[kNSeg * kSegBuckets];
    static uint32_t first[kFirstBuckets];
    static uint16_t tok[kTokPerBlock];
    static Tables T;
    int k[kStrips];
    memset(out, 0, kStageStride);
    for (int i = 0; i < kNSeg * kSegBuckets; ++i) tables_clear(seg_last, first, i);
    for (int i = 0; i < kNLL; ++i) tables_clear_hist(T, i);
    T.crc = 0;
    if (level != 0) {
        for (int p = 0; p + 3 <= n; ++p) table_insert(src, n, p, seg_last, first);
        for (int p = 0; p < n; ++p) hist_add(&T.hbyte[src[p]]);
        for (int v = 0; v < 256; ++v) T.cost[v] = T.hbyte[v] ? (uint8_t)lit_cost8((uint32_t)n, T.hbyte[v]) : 0;
    }
    for (int lane = 0; lane < kStrips; ++lane) {
        const int s0 = lane * kStrip < n ? lane * kStrip : n, s1 = s0 + kStrip < n ? s0 + kStrip : n;
        uint32_t fb = 0;
        k[lane] = level != 0 ? tokenise_strip(src, n, s0, s1, seg_last, first, T.cost, tok + lane, kStrips, T.hll, T.hd, &fb) : 0;
        T.bits_fix[lane] = fb;
        if (s1 > s0) T.crc ^= crc_share(crc_bytes(crc_tab, src + s0, s1 - s0), (uint32_t)(n - s1));
    }
    if (level != 0) {
        T.m_ll = (uint32_t)sort_syms(T.hll, kLLUsed, T.sorted_ll);
        T.m_d = (uint32_t)sort_syms(T.hd, kNDUsed, T.sorted_d);
        plan_codes(T);
    }
    for (int lane = 0; lane < kStrips; ++lane) T.bits_dyn[lane] = level != 0 ? strip_bits(T, tok + lane, kStrips, k[lane]) : 0;
    plan_block(T, n, level, out);
    if (T.form == kStored) {
        memcpy(out + kHdrBytes + 5, src, (size_t)n);
    } else {
        for (int lane = 0; lane * kStrip < n; ++lane)
            strip_write(T, tok + lane, kStrips, k[lane], lane == (n - 1) / kStrip, out, kHdrBytes, T.bits_dyn[lane]);
    }
    *form = T.form;
    return block_trailer(T, n, out);
}

int main(int argc, char **argv)
{
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = crc_table_entry(i);
    if (argc >= 3 && !strcmp(argv[1], "--lengths")) {
        const int limit = atoi(argv[2]), n = argc - 3;
        if (n < 1 || n > kNLL || limit < 1 || limit > 15) { fprintf(stderr, "--lengths: 1..%d frequencies, a limit of 1..15\n", kNLL); return 2; }
        std::vector<uint32_t> freq(n), w(2 * n);
        std::vector<uint16_t> sorted(n), par(2 * n);
        std::vector<uint8_t> len(n);
        for (int i = 0; i < n; ++i) freq[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
        const int m = sort_syms(freq.data(), n, sorted.data());
        code_lengths(freq.data(), sorted.data(), m, n, limit, len.data(), w.data(), par.data());
        for (int i = 0; i < n; ++i) printf("%d%c", len[i], i + 1 < n ? ' ' : '\n');
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--crc-split")) {
        const std::vector<uint8_t> in = read_file(argv[3]);
        const long k = atol(argv[2]);
        if (k < 0 || (size_t)k > in.size()) { fprintf(stderr, "--crc-split: K outside the file\n"); return 2; }
        const uint32_t after = (uint32_t)(in.size() - (size_t)k);
        const uint32_t c = crc_share(crc_bytes(crc_tab, in.data(), (int)k), after) ^ crc_bytes(crc_tab, in.data() + k, (int)after);
        printf("%08x\n", c);
        return 0;
    }
    int block_bytes = kMaxChunk, level = 1, eof = 0, a = 1;
    for (; a < argc && argv[a][0] == '-' && argv[a][1] == '-'; ++a) {
        if (!strcmp(argv[a], "--block-bytes") && a + 1 < argc) block_bytes = atoi(argv[++a]);
        else if (!strcmp(argv[a], "--level") && a + 1 < argc) level = atoi(argv[++a]);
        else if (!strcmp(argv[a], "--eof")) eof = 1;
        else break;
    }
    if (argc - a != 2 || block_bytes < 1 || block_bytes > kMaxChunk || level < 0 || level > 1) {
        fprintf(stderr, "usage: bgzf_model [--block-bytes 1..65280] [--level 0|1] [--eof] IN OUT\n");
        return 2;
    }
    const std::vector<uint8_t> in = read_file(argv[a]);
    FILE *f = fopen(argv[a + 1], "wb");
    if (!f) { perror(argv[a + 1]); return 2; }
    std::vector<uint8_t> out(kStageStride);
    long forms[3] = {0, 0, 0}, blocks = 0, total = 0;
    for (size_t at = 0; at < in.size(); at += (size_t)block_bytes) {
        const int n = (int)(in.size() - at < (size_t)block_bytes ? in.size() - at : (size_t)block_bytes);
        int form;
        const uint32_t sz = model_block(in.data() + at, n, level, crc_tab, out.data(), &form);
        fwrite(out.data(), 1, sz, f);
        ++forms[form]; ++blocks; total += sz;
    }
    if (eof) {
        const uint8_t marker[kEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0,
                                           0, 0, 0, 0, 0, 0, 0, 0};
        fwrite(marker, 1, sizeof marker, f);
        total += kEofBytes;
    }
    if (fclose(f)) { perror(argv[a + 1]); return 2; }
    printf("blocks %ld stored %ld fixed %ld dynamic %ld in %zu out %ld\n", blocks, forms[0], forms[1], forms[2], in.size(), total);
    return 0;
}
