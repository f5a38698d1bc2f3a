"""The contig table (include/bsw_contigs.h): bsw_set_contigs, the segment lookup, and the stages that read the
table, from seeds to text -- mem_chain's seed drop and merge test in bsw_mem_chain_device, mem_chain2aln's window
in bsw_chain2aln* (host-built and resident), mem_sort_dedup_patch in bsw_regs_select*, mem_pestat, mem_pair and
the proper flag in bsw_pe_stat* / bsw_pe_pair*, mem_matesw's window in bsw_matesw*, bwa_gen_cigar2's reject in
bsw_reg2aln*, TLEN in bsw_records*, RNAME / POS / RNEXT / PNEXT / SA:Z / XA:Z in bsw_sam_text*.

Reference: four contigs of 5,000 / 100 / 1,200 / 7,777 random codes (one shorter than a read, names of 1 and 63
bytes), a 100-base unit of the first contig copied into the third and, with one substitution, the fourth.

Two sets.  The pipeline set (Pipe): 200 generated fragments of 2 x 150 bp plus the hand-placed pairs of
_pipe_reads, taken through EVERY stage -- the restatement (tests/contigs_py.py; the C extension oracle by
decomposition over segments, whose argument contigs_py.chain2aln states) each stage on the one before, the GPU
device to device, compared after every stage; one contig == no table at every stage; host-built == resident
bsw_chain2aln.  The hand-placed lists of the stages behind selection, as test_rec.py's hand sets, with lines
worked out by pencil, the error returns and the limits of the table.
"""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bsw
import contigs_py as cp
import rec_py as rq
import reg2aln_py as rp
import regsel_py as sp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import (DEFAULT, RECORDS, declared, exported, fetch, got_aln, got_pair, got_text, mat_gaps, revcomp,
                      same_aln, same_msw, same_records, same_sel, same_text)
from test_matesw import MsBatch, reg, rnd
from test_rec import RNAME, _gpu_case, pairs_of, rec_set

LENS = (5000, 100, 1200, 7777)
NAMES = ("1", "chrB_" + "x" * 58, "chrC", "chrD")
TAB = cp.Table(LENS, NAMES)
L = TAB.sum
OA, OB, OC, OD = TAB.off[:4]                                 # 0, 5000, 5100, 6300
_rng = np.random.default_rng(2024)
REF = _rng.integers(0, 4, L).astype(np.uint8)
REF[OC + 300:OC + 400] = REF[1000:1100]                      # the unit of contig 1 again in chrC ..
REF[9000:9100] = REF[1000:1100]                              # .. and in chrD, one substitution
REF[9040] = (REF[9040] + 1) % 4
T2 = np.concatenate([REF, 3 - REF[::-1]]).astype(np.uint8)
MAT, GAPS = mat_gaps(DEFAULT)


def rv(s, e):
    """the reverse-strand read over forward [s, e) and its region's (rb, re)"""
    return revcomp(REF[s:e]), 2 * L - e, 2 * L - s


# ---------------------------------------------------------------- the lookup
def test_table_segments_and_errors_of_the_restatement():
    assert len(NAMES[0]) == 1 and len(NAMES[1]) == 63 and LENS[1] < 150 and L == 14077
    assert TAB.off == [0, 5000, 5100, 6300, 14077]
    assert TAB.bounds() == [0, 5000, 5100, 6300, 14077, 2 * L - 6300, 2 * L - 5100, 2 * L - 5000, 2 * L]
    b = TAB.bounds()
    for x in [0, 1, 4999, 5000, 5099, 5100, 6299, 6300, L - 1, L, L + 1, 2 * L - 6301, 2 * L - 6300, 2 * L - 5001,
              2 * L - 5000, 2 * L - 1]:
        s = TAB.seg(x)
        assert b[s] <= x < b[s + 1], x                       # seg(x) is the interval that holds x
        assert TAB.rid(x) == (s if s < 4 else 7 - s)
        assert TAB.rid(x) == TAB.rid(2 * L - 1 - x) and (TAB.seg(x) == TAB.seg(2 * L - 1 - x)) is False
    assert TAB.crosses(4999, 5001) and not TAB.crosses(5000, 5100) and TAB.crosses(5000, 5101)
    assert TAB.crosses(L - 1, L + 1) and TAB.crosses(2 * L - 5001, 2 * L - 4999) and not TAB.crosses(L, 2 * L - 6300)
    # one contig: the crossing test is the l_pac one
    one = cp.Table([L], ["x"])
    for rb, re_ in ((0, L), (L - 1, L + 1), (L, 2 * L), (10, 20), (L + 10, L + 20), (L - 5, L)):
        assert one.crosses(rb, re_) == (rb < L < re_)
    # a one-strand text
    flat = cp.Table(LENS, NAMES, two_strand=False)
    assert flat.l_pac == 0 and flat.seg(L - 1) == 3 and flat.seg(5000) == 1 and flat.bounds() == TAB.off
    for lens, names in (((0,), ("a",)), ((-1,), ("a",)), ((5,), ("",)), ((5,), ("x" * 64,)), ((5, 5), ("a",))):
        with pytest.raises(ValueError, match="INVAL"):
            cp.Table(lens, names)
    with pytest.raises(ValueError, match="INVAL"):
        TAB.check(L - 1, 2 * L)
    with pytest.raises(ValueError, match="INVAL"):
        flat.check(0, L + 1)
    TAB.check(L, 2 * L)
    flat.check(0, L)


def _cc_lookup(tmp_path):
    """csrc/bsw_contig_seg.h compiled for the host: seg and rid of every listed coordinate"""
    src = tmp_path / "seg.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "bsw_contig_seg.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  static const int64_t off[5] = {0, 5000, 5100, 6300, 14077};\n"
                   "  bsw::ContigView c{off, nullptr, nullptr, 4, atoll(argv[1])};\n"
                   "  for (int i = 2; i < argc; ++i) { long long x = atoll(argv[i]);\n"
                   '    printf("%d %d\\n", bsw::contig_seg(c, x), bsw::contig_rid(c, x)); }\n'
                   "  return 0; }\n")
    exe = tmp_path / "seg"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "bwa-mem2-arm_amd", "csrc"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_shared_lookup_header_is_the_restatement(tmp_path):
    exe = _cc_lookup(tmp_path)
    xs = sorted(set(v + d for v in TAB.bounds() for d in (-2, -1, 0, 1)) | {-5, 2 * L + 9, 777, L + 777})
    for tab, l_pac in ((TAB, L), (cp.Table(LENS, NAMES, two_strand=False), 0)):
        use = [x for x in xs if l_pac or x < L + 3]
        out = subprocess.run([exe, str(l_pac)] + [str(x) for x in use], capture_output=True, text=True).stdout.split("\n")
        for x, line in zip(use, out):
            assert line == f"{tab.seg(x)} {tab.rid(x)}", (l_pac, x, line)   # (out-of-range x: both clamp)


# ---------------------------------------------------------------- the hand set
class Hand:
    """a batch with its pair decisions (None: single-end), names and quals; run(tab) -> the restatement's result
    under the table, or rec_py's own with tab = None"""

    def __init__(self, batch, pairs=None):
        self.batch, self.pairs = batch, pairs
        n = len(batch.reads) // 2 if pairs is not None else len(batch.reads)
        self.names = [f"q{i}".encode() for i in range(n)]
        self.quals = (33 + (np.arange(sum(len(r) for r in batch.reads)) * 5) % 60).astype(np.uint8)
        self._res = {}

    def run(self, tab=TAB, rname=RNAME):
        key = (id(tab), rname)
        if key not in self._res:
            reads, off, lens, regs, info, first = self.batch.arrays(1)
            info["mapq"] = [g.get("mapq", 0) for e in self.batch.ends for g in e]
            opt = rq.rec_opt(l_pac=L, rname=rname, T=30)
            paired = self.pairs is not None
            if tab is None:
                res = rq.records(T2, reads, off, lens, regs, info, first, self.pairs, opt, MAT, GAPS)
                res.text, res.text_off = rq.sam_text(res, reads, off, lens, self.names, self.quals, opt, paired)
            else:
                res = cp.records(tab, T2, reads, off, lens, regs, info, first, self.pairs, opt, MAT, GAPS)
                res.text, res.text_off = cp.sam_text(tab, res, reads, off, lens, self.names, self.quals, opt, paired)
            res.opt, res.arrays = opt, (reads, off, lens, regs, info, first)
            res.lines = res.text.decode("latin-1").split("\n")[:-1]
            self._res[key] = res
        return self._res[key]


def _single():
    b = MsBatch()
    # 0, 1: exact reads whose middle lies on the join of contigs 1 | chrB, forward and reverse: a region on
    # either side (what is left once the bridging SMEM is dropped and nothing is patched across)
    b.reads.append(REF[4950:5050])
    b.ends.append([reg(4950, 50, qb=0, qe=50, mapq=30), reg(5000, 50, qb=50, qe=100, mapq=40)])
    r, rb, re_ = rv(4950, 5050)
    b.reads.append(r)
    b.ends.append([reg(rb, 50, qb=0, qe=50, mapq=30), reg(rb + 50, 50, qb=50, qe=100, mapq=20)])
    # 2: a mismatch exactly at the join (the first base of chrB)
    m = REF[4950:5050].copy()
    m[50] = (m[50] + 1) % 4
    b.reads.append(m)
    b.ends.append([reg(4950, 50, qb=0, qe=50, mapq=30), reg(5000, 45, qb=50, qe=100, mapq=25)])
    # 3: a read longer than chrB: 40 bases of contig 1, all of chrB (POS 1 to its last base), 40 of chrC
    b.reads.append(REF[4960:5140])
    b.ends.append([reg(4960, 40, qb=0, qe=40, mapq=10), reg(5000, 100, qb=40, qe=140, mapq=60),
                   reg(5100, 40, qb=140, qe=180, mapq=5)])
    # 4: the repeat unit: the primary in contig 1, XA members in chrC, chrD and (a reverse hit) contig 1
    r5, rb5, _ = rv(3000, 3100)
    b.reads.append(REF[1000:1100])
    b.ends.append([reg(1000, 100, mapq=0), reg(OC + 300, 100, secondary=0), reg(9000, 95, secondary=0),
                   reg(rb5, 90, qb=0, qe=24, secondary=0)])
    # 5: a chimeric read: 60 bases of contig 1 forward, 40 of chrD reverse
    r2, rb2, _ = rv(12000, 12040)
    b.reads.append(np.concatenate([REF[2000:2060], r2]))
    b.ends.append([reg(2000, 60, qb=0, qe=60, mapq=50), reg(rb2, 40, qb=60, qe=100, mapq=55, sub=20)])
    # 6: unmapped
    b.reads.append(rnd(seed=6))
    b.ends.append([])
    # 7, 8: a read ending on chrD's last base; a reverse read starting on chrD's first
    b.reads.append(REF[L - 100:L])
    b.ends.append([reg(L - 100, 100, mapq=60)])
    r8, rb8, _ = rv(OD, OD + 100)
    b.reads.append(r8)
    b.ends.append([reg(rb8, 100, mapq=60)])
    # 9: a chimeric read inside one contig
    b.reads.append(np.concatenate([REF[2000:2060], REF[3000:3040]]))
    b.ends.append([reg(2000, 60, qb=0, qe=60, mapq=50), reg(3000, 40, qb=60, qe=100, mapq=45)])
    return Hand(b)


def _paired():
    b = MsBatch()
    r, rb, _ = rv(2400, 2500)
    b.add("same", REF[2000:2100], [reg(2000, 100, mapq=60)], r, [reg(rb, 100, mapq=60)])
    # ends on different contigs, the paired branch and no_pairing (end 0 chimeric over two contigs)
    b.add("cross", REF[2000:2100], [reg(2000, 100, mapq=60)], REF[7000:7100], [reg(7000, 100, mapq=60)])
    r2, rb2, _ = rv(12000, 12040)
    b.add("cross_nopair", np.concatenate([REF[2000:2060], r2]),
          [reg(2000, 60, qb=0, qe=60, mapq=50), reg(rb2, 40, qb=60, qe=100, mapq=55)],
          REF[OC + 500:OC + 600], [reg(OC + 510, 90, qb=10, qe=100, mapq=40)])
    r3, rb3, _ = rv(OC + 100, OC + 200)
    b.add("one", r3, [reg(rb3, 100, mapq=33)], rnd(seed=7), [])
    b.add("none", rnd(seed=8), [], rnd(seed=9), [])
    # mates either side of a join: 500 apart on the concatenation, which no contig-aware stage calls a pair
    r4, rb4, _ = rv(OB, OB + 100)
    b.add("join", REF[4600:4700], [reg(4600, 100, mapq=60)], r4, [reg(rb4, 100, mapq=60)])
    pairs = pairs_of((1, 0, 0, 60, 59, 1), (1, 0, 0, 11, 12, 0), (0, 0, 0, 50, 40, 0), (0, 0, -1, 33, 0, 0),
                     (0, -1, -1, 0, 0, 0), (0, 0, 0, 60, 60, 0))
    return Hand(b, pairs)


_hand = {}


def hand(name):
    if name not in _hand:
        _hand[name] = dict(single=_single, paired=_paired)[name]()
    return _hand[name]


def _f(w, i):
    return w.lines[i].split("\t")


def test_single_end_lines_by_contig():
    w = hand("single").run()
    B = NAMES[1]
    assert list(w.rec_first) == [0, 2, 4, 6, 9, 10, 12, 13, 14, 15, 17]
    assert _f(w, 15)[-1] == "SA:Z:1,3001,+,60S40M,45,0;"
    # read 0: contig 1 to its last base, then chrB from POS 1; SA names the other contig
    assert _f(w, 0)[:9] == ["q0", "0", "1", "4951", "30", "50M50S", "*", "0", "0"] and _f(w, 0)[-1] == f"SA:Z:{B},1,+,50S50M,30,0;"
    assert _f(w, 1)[:6] == ["q0", "2048", B, "1", "30", "50H50M"] and _f(w, 1)[-1] == "SA:Z:1,4951,+,50M50S,30,0;"
    # read 1, reverse: its first 50 bases are forward [5000, 5050) = chrB 1..50
    assert _f(w, 2)[:6] == ["q1", "16", B, "1", "30", "50S50M"] and _f(w, 3)[:6] == ["q1", "2064", "1", "4951", "20", "50M50H"]
    # read 2: the mismatch at chrB's first base
    assert _f(w, 5)[:6] == ["q2", "2048", B, "1", "25", "50H50M"] and _f(w, 5)[11:13] == ["NM:i:1", f"MD:Z:0{'ACGT'[REF[5000]]}49"]
    # read 3: three contigs in one read
    assert [_f(w, i)[2:4] for i in (6, 7, 8)] == [["1", "4961"], [B, "1"], ["chrC", "1"]]
    assert _f(w, 7)[5] == "40H100M40H" and _f(w, 6)[-1] == f"SA:Z:{B},1,+,40S100M40S,10,0;chrC,1,+,140S40M,5,0;"
    # read 4: XA members by their own contig, in list order
    xa = _f(w, 9)[-1]
    assert xa.startswith("XA:Z:chrC,+301,100M,0;chrD,+2701,100M,1;1,-") and xa.count(";") == 3
    # read 5: SA into chrD, relative
    assert _f(w, 10)[-1] == f"SA:Z:chrD,{12000 - OD + 1},-,40M60S,50,0;" and _f(w, 11)[2:4] == ["chrD", str(12000 - OD + 1)]
    assert _f(w, 12)[:6] == ["q6", "4", "*", "0", "0", "*"]
    assert _f(w, 13)[2:6] == ["chrD", str(LENS[3] - 99), "60", "100M"] and _f(w, 14)[1:6] == ["16", "chrD", "1", "60", "100M"]
    # positions in the records stay global
    assert list(w.recs["pos"][[0, 1, 7, 13]]) == [4950, 5000, 5000, L - 100]
    # without the table: one name and concatenated coordinates on every mapped line
    n = hand("single").run(None)
    assert all(a != b for a, b in zip(w.lines, n.lines) if a.split("\t")[2] != "*")
    assert _f(n, 1)[2:4] == [RNAME, "5001"] and np.array_equal(n.recs, w.recs)


def test_paired_end_lines_by_contig():
    w = hand("paired").run()
    F = [_f(w, i) for i in range(len(w.lines))]
    assert list(w.rec_first) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13]
    assert F[0][:9] == ["q0", "99", "1", "2001", "60", "100M", "=", "2401", "500"]
    assert F[1][:9] == ["q0", "147", "1", "2401", "59", "100M", "=", "2001", "-500"]
    # different contigs: RNEXT by name, PNEXT relative, TLEN 0, MC stays
    assert F[2][:9] == ["q1", "65", "1", "2001", "11", "100M", "chrD", "701", "0"] and "MC:Z:100M" in F[2]
    assert F[3][:9] == ["q1", "129", "chrD", "701", "12", "100M", "1", "2001", "0"]
    assert F[4][:9] == ["q2", "65", "1", "2001", "50", "60M40S", "chrC", "511", "0"]
    assert F[5][:9] == ["q2", str(0x41 | 0x800 | 0x10), "chrD", str(12000 - OD + 1), "50", "40M60H", "chrC", "511", "0"]
    assert F[6][:9] == ["q2", "129", "chrC", "511", "40", "10S90M", "1", "2001", "0"]
    # one end unmapped: it takes its mate's contig and position
    assert F[7][:9] == ["q3", str(0x41 | 0x8 | 0x10 | 0x20), "chrC", "101", "33", "100M", "=", "101", "0"]
    assert F[8][:9] == ["q3", str(0x81 | 0x4 | 0x10 | 0x20), "chrC", "101", "0", "*", "=", "101", "0"]
    assert F[9][2:9] == ["*", "0", "0", "*", "*", "0", "0"]
    # either side of the join
    assert F[11][:9] == ["q5", str(0x41 | 0x20), "1", "4601", "60", "100M", NAMES[1], "1", "0"]
    assert F[12][:9] == ["q5", str(0x81 | 0x10), NAMES[1], "1", "60", "100M", "1", "4601", "0"]
    n = hand("paired").run(None)
    assert _f(n, 11)[6:9] == ["=", "5001", "500"] and n.recs[11]["tlen"] == 500 and w.recs[11]["tlen"] == 0
    assert list(np.flatnonzero(n.recs["tlen"] != w.recs["tlen"])) == [2, 3, 4, 5, 6, 11, 12]


def _reg2aln_set():
    """one exact read per region: inside a contig, all of chrB, over each kind of join, over the strand boundary"""
    rows = [(4900, 5000), (5000, 5100), (4950, 5050), (5050, 5150), (5000, 5101), (L - 50, L + 50), (L, L + 100),
            (2 * L - 5050, 2 * L - 4950), (2 * L - 5100, 2 * L - 5000), (2 * L - 100, 2 * L), (-1, 99), (OD - 1, OD + 99)]
    regs = np.zeros(len(rows), dtype=bsw.ALNREG_DTYPE)
    reads = []
    for k, (rb, re_) in enumerate(rows):
        regs[k] = (rb, re_, 0, re_ - rb, re_ - rb, re_ - rb, 100, 19)
        reads.append(T2[max(rb, 0):re_])
    lens = np.array([len(r) for r in reads], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return np.concatenate(reads), off, lens, regs, np.arange(len(rows), dtype=np.int32)


def test_every_rid_branch_is_reached():
    tr = sp.Trace()
    reads, off, lens, regs, rr = _reg2aln_set()
    aln, _, _, _ = cp.reg2aln(TAB, T2, reads, off, lens, regs, rr, MAT, GAPS, 100, tr=tr)
    assert list(aln["flags"] & rp.REJECTED) == [0, 0, 1, 1, 1, 1, 0, 1, 0, 0, 1, 1]
    plain, _, _, _ = rp.reg2aln(T2, L, reads, off, lens, regs, rr, MAT, GAPS, 100)
    assert list(plain["flags"] & rp.REJECTED) == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    one, _, _, _ = cp.reg2aln(cp.Table([L], [RNAME]), T2, reads, off, lens, regs, rr, MAT, GAPS, 100)
    assert np.array_equal(one, plain)
    cnt = tr.cnt
    for name in ("single", "paired"):
        cnt.update({k: v for k, v in hand(name).run().tr.cnt.items() if k in cp.BRANCHES})
    for t in (pe_set()["stat"][1], pe_set()["pair"][3], nopair_case()[4], msw_set()["table"][4], pipe().tr, pipe().sel[4]):
        cnt.update({k: v for k, v in t.cnt.items() if k in cp.BRANCHES})
    print("rid branches:", {k: cnt[k] for k in cp.BRANCHES})
    assert all(cnt[k] > 0 for k in cp.BRANCHES), [k for k in cp.BRANCHES if cnt[k] == 0]
    # a needed region over a join fails the records call, as one over l_pac does
    b = MsBatch()
    b.reads, b.ends = [REF[4950:5050]], [[reg(4950, 100)]]
    with pytest.raises(ValueError, match="RANGE"):
        Hand(b).run()
    assert len(Hand(b).run(None).recs) == 1


def test_one_contig_named_like_rname_is_no_table():
    one = cp.Table([L], [RNAME])
    for name in ("single", "paired"):
        h = hand(name)
        a, b = h.run(one), h.run(None)
        assert a.text == b.text and np.array_equal(a.text_off, b.text_off) and np.array_equal(a.recs, b.recs)
        assert h.run(one, rname="ignored").text == b.text     # opt->rname is not read under a table


# ---------------------------------------------------------------- the header and the setter's checks
def test_library_exports_the_contigs_header():
    src = open(os.path.join(ROOT, "include", "bsw_contigs.h")).read()
    assert re.search(r"#define BSW_CONTIGS_API 1\b", src) and re.search(r"#define BSW_CONTIG_MAX_NAME 63\b", src)
    decl = declared("bsw_contigs.h")
    assert decl == set(bsw.CONTIGS_SYMBOLS)
    assert decl <= exported()
    others = (set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS) |
              set(bsw.MATESW_SYMBOLS) | set(bsw.REC_SYMBOLS))
    assert not decl & others and len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8
    for cc, ext in (("gcc", "c"), ("g++", "cpp")):
        r = subprocess.run([cc, "-fsyntax-only", "-x", "c" if ext == "c" else "c++", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "include", "bsw_contigs.h")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _set(ctx, lens, names, n=None):
    lens = np.asarray(lens, dtype=np.int64)
    arr = (ctypes.c_char_p * max(len(names), 1))(*names)
    return bsw.hip_lib().bsw_set_contigs(ctx, len(lens) if n is None else n, bsw._ptr(lens) if len(lens) else None, arr)


def test_invalid_tables_need_no_device():
    fake = ctypes.c_void_p(1)                                # never dereferenced: the checks come first
    assert _set(None, [5], [b"a"]) == -22
    assert _set(fake, [5], [b"a"], n=-1) == -22
    assert _set(fake, [0], [b"a"]) == -22 and _set(fake, [5, -3], [b"a", b"b"]) == -22
    assert _set(fake, [5], [b""]) == -22 and _set(fake, [5], [b"x" * 64]) == -22 and _set(fake, [5], [None]) == -22
    assert _set(fake, [2 ** 62, 2 ** 62], [b"a", b"b"]) == -22
    assert _set(fake, [2 ** 39, 1], [b"a", b"b"]) == -22        # BSW_CONTIG_MAX_SUM
    many = 2 ** 22 + 1                                          # BSW_CONTIG_MAX_N
    assert _set(fake, np.ones(many, np.int64), [b"a"] * many) == -22
    assert bsw.hip_lib().bsw_set_contigs(fake, 1, None, None) == -22
    F = bsw.hip_lib().bsw_fmi_set_contigs
    one = np.array([5], np.int64)
    assert F(None, 1, bsw._ptr(one)) == -22 and F(fake, -1, bsw._ptr(one)) == -22 and F(fake, 1, None) == -22
    assert F(fake, 2 ** 22 + 1, bsw._ptr(one)) == -22
    with pytest.raises(ValueError):
        bsw.set_contigs(None, [5, 6], ["a"])


# ---------------------------------------------------------------- GPU
def _engine():
    eng = bsw.Engine()
    bsw.set_reference(eng, T2)
    return eng


@pytest.mark.gpu
def test_gpu_reg2aln_rejects_over_every_join():
    reads, off, lens, regs, rr = _reg2aln_set()
    ok = regs["rb"] >= 0                                       # (the library answers BSW_E_RANGE for none of these)
    eng = _engine()
    o = bsw.ext_opt(l_pac=L)
    plain = bsw.reg2aln(eng, reads, off, lens, regs, rr, o)
    same_aln(rp.reg2aln(T2, L, reads, off, lens, regs, rr, MAT, GAPS, 100)[:3], plain, "no table")
    bsw.set_contigs(eng, LENS, NAMES)
    got = bsw.reg2aln(eng, reads, off, lens, regs, rr, o)
    same_aln(cp.reg2aln(TAB, T2, reads, off, lens, regs, rr, MAT, GAPS, 100)[:3], got, "table")
    assert list(np.flatnonzero((got[0]["flags"] ^ plain[0]["flags"]) & bsw.ALN_REJECTED)) == [2, 3, 4, 7, 11] and ok.sum() == 11
    assert bsw.aln_last_stats(eng).n_rejected == 7
    # the resident form
    b = ResidentBatch(eng, reads, off, lens)
    b.put(regs=regs, sr=rr)
    b.reg2aln(o)
    res = got_aln(b)
    same_aln(got, res, "resident")
    # one contig == no table; no contigs removes the table
    bsw.set_contigs(eng, [L], [RNAME])
    same_aln(plain, bsw.reg2aln(eng, reads, off, lens, regs, rr, o), "one contig")
    bsw.set_contigs(eng)
    same_aln(plain, bsw.reg2aln(eng, reads, off, lens, regs, rr, o), "table removed")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["single", "paired"])
def test_gpu_hand_set_host_arrays(name):
    h = hand(name)
    w, plain = h.run(), h.run(None)
    eng = _engine()
    _gpu_case(eng, h, plain, f"{name}, no table")
    bsw.set_contigs(eng, LENS, NAMES)
    _gpu_case(eng, h, w, f"{name}, table")
    assert w.text != plain.text                                 # (so a table that is ignored cannot pass)
    bsw.set_contigs(eng, [L], [RNAME])
    _gpu_case(eng, h, plain, f"{name}, one contig")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["single", "paired"])
def test_gpu_hand_set_device_to_device(name):
    """bsw_records_resident -> bsw_sam_text_resident under the table: the arrays one call leaves in HBM are the
    next call's inputs"""
    h = hand(name)
    w = h.run()
    reads, off, lens, regs, info, first = w.arrays
    eng = _engine()
    bsw.set_contigs(eng, LENS, NAMES)
    b = ResidentBatch(eng, reads, off, lens, h.quals)
    b.put(sreg=regs, sinfo=info, sfirst=first, **({} if h.pairs is None else {"pairs": h.pairs}))
    b.records(bsw.rec_opt(**w.opt), paired=h.pairs is not None)
    rec = fetch(b, *RECORDS)
    b.sam_text(bsw.rec_opt(**w.opt), h.names, h.pairs is not None, cap=len(w.text) + 5)
    txt = got_text(b)
    same_records(w, rec, f"{name} resident", bsw.rec_last_stats(eng))
    same_text(w.text, w.text_off, txt, f"{name} resident")
    eng.close()


@pytest.mark.gpu
def test_gpu_one_contig_is_no_table_on_the_pipeline_set():
    """test_rec's pipeline set (stat, rescue, pair behind it), both forms: a table of one contig named like
    opt->rname changes no byte of any output, and opt->rname is then not read"""
    s = rec_set()
    p, a = s.p, s.p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    o = bsw.rec_opt(**s.opt)

    def host(opt):
        got = bsw.records(eng, a["reads"], a["off"], a["lens"], s.regs, s.info, p.mfirst, s.pairs, opt)
        recs, rfirst, aln, aln_reg, cig, md = got
        return got, bsw.sam_text(eng, recs, rfirst, aln, cig, md, a["reads"], a["off"], a["lens"], s.names, s.quals, opt, True)

    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], s.quals)
    b.put(mreg=s.regs, minfo=s.info, mfirst=p.mfirst, pairs=s.pairs)

    def resident(opt):
        b.records(opt)
        rec = fetch(b, *RECORDS)
        b.sam_text(opt, s.names, True, cap=len(s.text) + 5)
        return rec, got_text(b)

    base = host(o), resident(o)
    same_records(s.res, base[0][0], "no table")
    same_text(s.text, s.text_off, base[0][1], "no table")
    bsw.set_contigs(eng, [p.l_pac], [RNAME])
    for opt, tag in ((o, "one contig"), (bsw.rec_opt(**dict(s.opt, rname="unread")), "rname unread")):
        for (rec0, txt0), (rec1, txt1), form in zip(base, (host(opt), resident(opt)), ("host", "resident")):
            for x, y in zip(rec0, rec1):
                assert x.tobytes() == y.tobytes(), (tag, form)
            assert txt0[0] == txt1[0] and np.array_equal(txt0[1], txt1[1]), (tag, form)
    eng.close()


@pytest.mark.gpu
def test_gpu_table_errors():
    h = hand("paired")
    w = h.run()
    reads, off, lens, regs, info, first = w.arrays
    o = bsw.rec_opt(**w.opt)
    eng = _engine()
    bsw.set_contigs(eng, LENS, NAMES)
    got = bsw.records(eng, reads, off, lens, regs, info, first, h.pairs, o)
    recs, rfirst, aln, aln_reg, cig, md = got
    # a table that does not sum to the call's l_pac: every stage behind the extension says so
    bsw.set_contigs(eng, LENS[:3] + (LENS[3] - 1,), NAMES)
    r2 = _reg2aln_set()
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.reg2aln(eng, *r2, bsw.ext_opt(l_pac=L))
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.records(eng, reads, off, lens, regs, info, first, h.pairs, o)
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.sam_text(eng, recs, rfirst, aln, cig, md, reads, off, lens, h.names, h.quals, o, True)
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.pe_stat(eng, regs, info, first, bsw.pe_opt(l_pac=L))
    # a one-strand reference: the sum has to be its length
    bsw.set_reference(eng, REF)
    bsw.set_contigs(eng, LENS, NAMES)
    one = bsw.reg2aln(eng, r2[0], r2[1], r2[2], r2[3][:5], r2[4][:5], bsw.ext_opt(l_pac=0))
    assert list(one[0]["flags"] & bsw.ALN_REJECTED) == [0, 0, 1, 1, 1]
    # (the text calls read no reference: with l_pac == 0 the table has to sum to the resident length too)
    flat = bsw.rec_opt(**dict(w.opt, l_pac=0))
    assert bsw.sam_text(eng, recs, rfirst, aln, cig, md, reads, off, lens, h.names, h.quals, flat, True)[0] == w.text
    bsw.set_contigs(eng, LENS[:3], NAMES[:3])
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.reg2aln(eng, r2[0], r2[1], r2[2], r2[3][:5], r2[4][:5], bsw.ext_opt(l_pac=0))
    # a needed region over a join: BSW_E_RANGE, as over l_pac
    bsw.set_reference(eng, T2)
    bsw.set_contigs(eng, LENS, NAMES)
    b = MsBatch()
    b.reads, b.ends = [REF[4950:5050]], [[reg(4950, 100)]]
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.records(eng, *b.arrays(), None, o)
    # invalid tables leave the one that is set; the calls work again
    for lens_, names_ in (((0,), ("a",)), ((5,), ("",)), ((5,), ("x" * 64,))):
        with pytest.raises(bsw.BswError, match="-22"):
            bsw.set_contigs(eng, lens_, names_)
    _gpu_case(eng, h, w, "after the errors")
    bsw.set_contigs(eng)
    _gpu_case(eng, h, h.run(None), "table removed")
    eng.close()


# ---------------------------------------------------------------- the paired-end stage under the table
def _pe_batch():
    """30 fragments inside chrD (so FR has statistics), then: mates either side of the chrC | chrD join and of the
    1 | chrB join, 500 apart on the concatenation; lists of two regions whose best pair on the concatenation
    bridges a join while a weaker pair lies inside chrC; a pair inside contig 1"""
    b = MsBatch()
    for i in range(30):
        s = 7000 + 150 * i
        r, rb, _ = rv(s + 380 + i, s + 480 + i)
        b.add(f"d{i}", REF[s:s + 100], [reg(s, 100)], r, [reg(rb, 100)])
    for i in range(3):
        r, rb, _ = rv(OD + 100 + i, OD + 200 + i)
        b.add(f"cd{i}", REF[OD - 300:OD - 200], [reg(OD - 300, 100)], r, [reg(rb, 100)])
    r, rb, _ = rv(OB, OB + 100)
    b.add("ab", REF[4600:4700], [reg(4600, 100)], r, [reg(rb, 100)])
    r2, rb2, _ = rv(OC + 600, OC + 700)
    b.add("two", REF[4600:4700], [reg(4600, 100), reg(OC + 200, 90)], r, [reg(rb, 100), reg(rb2, 90)])
    r3, rb3, _ = rv(2400, 2500)
    b.add("same", REF[2000:2100], [reg(2000, 100)], r3, [reg(rb3, 100)])
    return b


_pe = {}


def pe_set():
    if not _pe:
        import pe_py as pp
        reads, off, lens, regs, info, first = _pe_batch().arrays(1)
        o = pp.pe_opt(l_pac=L)
        _pe["arr"], _pe["opt"] = (regs, info, first), o
        _pe["stat"] = cp.pe_stat(TAB, regs, info, first, o, 1)
        _pe["stat_plain"] = pp.pe_stat(regs, info, first, o, 1)
        pes = _pe["stat"][0]
        _pe["pair"] = cp.pe_pair(TAB, pes, regs, info, first, o, MAT, GAPS)
        _pe["pair_plain"] = pp.pe_pair(pes, regs, info, first, o, MAT, GAPS)
    return _pe


def nopair_case():
    """no_pairing's proper flag: FF statistics given from outside with a std so small that every q is 0 -- no
    pair, but the window still names `proper`.  Pair 0 either side of the 1 | chrB join, pair 1 inside contig 1.
    -> (pes, (regs, info, first), pairs on the concatenation, pairs under the table, the table run's Trace)"""
    if "nopair" not in _pe:
        import pe_py as pp
        given = np.zeros(4, dtype=pp.PESTAT_DTYPE)
        for d in range(4):
            given[d] = (300, 700, 1, 20, 500.0, 50.0)
        given[0] = (300, 700, 0, 20, 500.0, 1e-3)
        b = MsBatch()
        b.add("ff", REF[4600:4700], [reg(4600, 100)], REF[OB:OB + 100], [reg(OB, 100)])
        b.add("ff2", REF[2000:2100], [reg(2000, 100)], REF[2501:2601], [reg(2501, 100)])
        arr = b.arrays(1)[3:]
        o = pe_set()["opt"]
        _, _, pl, _ = pp.pe_pair(given, *arr, o, MAT, GAPS)
        _, _, ct, trn = cp.pe_pair(TAB, given, *arr, o, MAT, GAPS)
        _pe["nopair"] = (given, arr, pl, ct, trn)
    return _pe["nopair"]


def test_paired_end_stage_by_contig():
    s = pe_set()
    pes, tr, isize = s["stat"]
    # the three chrC | chrD fragments and the 1 | chrB one give no insert size, on the concatenation they do (the
    # two-region pair is skipped by cal_sub either way)
    assert [len(v) for v in isize] == [0, 31, 0, 0] and [len(v) for v in s["stat_plain"][2]] == [0, 35, 0, 0]
    assert not pes[1]["failed"] and tr.cnt["stat_cross_rid"] == 4 and tr.cnt["stat_same_rid"] == 31
    regs, info, pairs, trp = s["pair"]
    plain = s["pair_plain"][2]
    assert list(pairs["paired"][:30]) == [1] * 30 and list(pairs["proper"][:30]) == [1] * 30
    assert list(plain["paired"][30:34]) == [1] * 4 and list(pairs["paired"][30:34]) == [0] * 4
    assert list(pairs["proper"][30:34]) == [0] * 4 and list(pairs["z"][33]) == [0, 0]
    # two regions per end: the bridge pair (200) wins on the concatenation; under the table the only pair left is
    # the chrC one (180), which loses to the unpaired tops (200 - 17): paired, not proper
    assert (plain["paired"][34], plain["proper"][34]) == (1, 1) and plain["score"][34] > pairs["score"][34] > 0
    assert (pairs["paired"][34], pairs["proper"][34], list(pairs["z"][34])) == (1, 0, [0, 0])
    assert pairs[35:36].tobytes() == plain[35:36].tobytes() and pairs["paired"][35] == 1
    assert trp.cnt["pair_rid_break"] >= 5 and trp.cnt["pair_same_rid"] == 32      # (the 31 pairs and "two"'s chrC pair)
    assert list(np.flatnonzero([a.tobytes() != b_.tobytes() for a, b_ in zip(pairs, plain)])) == [30, 31, 32, 33, 34]
    # the regions come back on the concatenation, permuted within a read at most
    assert sorted(regs["rb"].tolist()) == sorted(s["arr"][0]["rb"].tolist())
    given, arr, pl, ct, trn = nopair_case()
    assert list(pl["paired"]) == [0, 0] and list(pl["proper"]) == [1, 1] and list(ct["proper"]) == [0, 1]
    assert trn.cnt["nopair_cross_rid"] == 1 and trn.cnt["nopair_same_rid"] == 1
    one = cp.Table([L], [RNAME])
    assert all(np.array_equal(x, y) for x, y in zip(cp.pe_pair(one, pes, *s["arr"], s["opt"], MAT, GAPS)[:3], s["pair_plain"][:3]))
    assert np.array_equal(cp.pe_stat(one, *s["arr"], s["opt"], 1)[0], s["stat_plain"][0])


@pytest.mark.gpu
def test_gpu_paired_end_stage_by_contig():
    s = pe_set()
    regs, info, first = s["arr"]
    o = bsw.pe_opt(l_pac=L)
    eng = _engine()

    def run(pes_in=None):
        pes = bsw.pe_stat(eng, regs, info, first, o)
        return pes, bsw.pe_pair(eng, pes if pes_in is None else pes_in, regs, info, first, o)

    def same(got, want_pes, want, tag):
        for f in ("low", "high", "failed", "n"):
            assert np.array_equal(got[0][f], want_pes[f]), (tag, f)
        assert np.allclose(got[0]["avg"], want_pes["avg"], rtol=1e-12) and np.allclose(got[0]["std"], want_pes["std"], rtol=1e-12)
        for x, y, name in zip(got[1], want[:3], ("regs", "info", "pairs")):
            for f in y.dtype.names:
                assert np.array_equal(x[f], y[f]), (tag, name, f)

    plain = run(s["stat"][0])
    same(plain, s["stat_plain"][0], s["pair_plain"], "no table")
    bsw.set_contigs(eng, LENS, NAMES)
    got = run()
    same(got, s["stat"][0], s["pair"], "table")
    assert not np.array_equal(got[1][2]["paired"], plain[1][2]["paired"]) and got[0][1]["n"] == 31 and plain[0][1]["n"] == 35
    # the resident form, in place
    nr = len(first) - 1
    b = ResidentBatch(eng, np.zeros(1, np.uint8), np.zeros(nr, np.int64), np.zeros(nr, np.int32))   # (neither call reads the reads)
    b.put(sreg=regs, sinfo=info, sfirst=first)
    pes = b.pe_stat(o)
    b.pe_pair(pes, o)
    res = got_pair(b)
    same((pes, res), s["stat"][0], s["pair"], "resident")
    # no_pairing's proper flag
    given, (r1, i1, f1), want_plain, want, _ = nopair_case()
    assert bsw.pe_pair(eng, given, r1, i1, f1, o)[2].tobytes() == np.ascontiguousarray(want, dtype=bsw.PAIR_DTYPE).tobytes()
    # one contig == no table
    bsw.set_contigs(eng, [L], [RNAME])
    one = run(s["stat"][0])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one[1], plain[1])) and one[0].tobytes() == plain[0].tobytes()
    bsw.set_contigs(eng)
    assert bsw.pe_pair(eng, given, r1, i1, f1, o)[2].tobytes() == np.ascontiguousarray(want_plain, dtype=bsw.PAIR_DTYPE).tobytes()
    eng.close()


# ---------------------------------------------------------------- mate rescue windows under the table
def _msw_batch():
    """anchors near the 1 | chrB | chrC joins, mates without a region (FR statistics 300..700): A the window ends on
    contig 1's last base; B it is clipped there; C its midpoint lies in chrC: no job; D likewise, though the mate
    lies in contig 1; E a reverse anchor in chrC whose window is clipped at chrC's first base"""
    b = MsBatch()
    for name, a, (ms, me) in (("A", 4300, (4700, 4800)), ("B", 4500, (4850, 4950)), ("C", 4800, (5150, 5250)),
                              ("D", 4650, (4880, 4980))):
        b.add(name, REF[a:a + 100], [reg(a, 100)], rv(ms, me)[0], [])
    r, rb, _ = rv(5600, 5700)
    b.add("E", r, [reg(rb, 100)], REF[5200:5300], [])
    return b


_msw = {}


def msw_set():
    if not _msw:
        import ksw_align_py as kp
        import matesw_py as mp
        from test_matesw import PES_FR
        arr = _msw_batch().arrays(1)
        o = mp.matesw_opt(l_pac=L)
        _msw.update(arr=arr, pes=PES_FR, table=cp.mate_rescue(TAB, PES_FR, T2, *arr, o, MAT, GAPS, kp.ksw_align2),
                    plain=mp.mate_rescue(PES_FR, T2, *arr, o, MAT, GAPS, kp.ksw_align2),
                    one=cp.mate_rescue(cp.Table([L], [RNAME]), PES_FR, T2, *arr, o, MAT, GAPS, kp.ksw_align2))
    return _msw


def _mate_lists(res):
    first = res[3]
    return [int(first[2 * p + 2] - first[2 * p + 1]) for p in range((len(first) - 1) // 2)]


def test_rescue_windows_by_contig():
    s = msw_set()
    assert _mate_lists(s["plain"]) == [1, 1, 1, 1, 1] and _mate_lists(s["table"]) == [1, 1, 0, 0, 1]
    regs, first = s["table"][0], s["table"][3]
    got = [(int(regs[first[2 * p + 1]]["rb"]), int(regs[first[2 * p + 1]]["re"])) for p in (0, 1, 4)]
    assert got == [(2 * L - 4800, 2 * L - 4700), (2 * L - 4950, 2 * L - 4850), (5200, 5300)]
    c = s["table"][4].cnt
    assert (c["msw_whole"], c["msw_clip"], c["msw_other_rid"], c["msw_same_rid"]) == (1, 4, 2, 3), dict(c)
    for x, y in zip(s["one"][:4], s["plain"][:4]):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_gpu_rescue_windows_by_contig():
    s = msw_set()
    o = bsw.matesw_opt(l_pac=L)
    eng = _engine()
    same_msw(s["plain"], bsw.matesw(eng, s["pes"], *s["arr"], o), "no table", bsw.matesw_last_stats(eng))
    bsw.set_contigs(eng, LENS, NAMES)
    got = bsw.matesw(eng, s["pes"], *s["arr"], o)
    same_msw(s["table"], got, "table", bsw.matesw_last_stats(eng))
    assert _mate_lists((0, 0, 0, got[3])) == [1, 1, 0, 0, 1]
    bsw.set_contigs(eng, [L], [RNAME])
    same_msw(s["plain"], bsw.matesw(eng, s["pes"], *s["arr"], o), "one contig", bsw.matesw_last_stats(eng))
    eng.close()


# ---------------------------------------------------------------- the whole chain of stages under the table
def _unseedable(read):
    """a substitution every 13 to 16 bases: no exact 19-mer is left"""
    r = np.array(read, np.uint8)
    k, i = 7, 0
    while k < len(r):
        r[k] = (r[k] + 1) % 4
        k += 13 + i % 4
        i += 1
    return r


def _pipe_reads():
    """about 200 fragments of 2 x 150 drawn inside the contigs that hold one, then the hand-placed pairs:
    1 / 1r an exact read whose middle lies on the 1 | chrB join, forward and reverse; 2 a mismatch on chrB's first
    base; 3 a read ending on contig 1's last base with one starting on chrD's first; 4 ends on different contigs;
    5a / 5b unseedable mates of anchors near contig 1's end (window clipped; midpoint in the neighbour); 6 the
    repeat unit of contigs 1, chrC and chrD; 7 a chimeric read over contigs 1 and chrD; 8 a chimeric read inside contig 1
    (two regions that dedup compares) with a read over the strand boundary"""
    import bench
    parts = []
    for (lo, hi, n, seed) in ((0, OB, 70, 1), (OC, OD, 20, 2), (OD, L, 110, 3)):
        parts.append(bench.pe_reads(REF[lo:hi], n, 150, seed=seed)[0])
    hand = []
    j = REF[4925:5075]
    hand += [j, rv(5150, 5300)[0], rv(4925, 5075)[0], REF[4500:4650]]
    m = j.copy()
    m[75] = (m[75] + 1) % 4
    hand += [m, rv(4300, 4450)[0]]
    hand += [REF[4850:5000], rv(OD, OD + 150)[0]]
    hand += [REF[2000:2150], rv(7000, 7150)[0]]
    hand += [REF[4250:4400], _unseedable(rv(4700, 4850)[0]), REF[4700:4850], _unseedable(rv(5150, 5300)[0])]
    hand += [REF[975:1125], rv(1400, 1550)[0]]
    hand += [np.concatenate([REF[2000:2075], rv(12000, 12075)[0]]), rv(2400, 2550)[0]]
    hand += [np.concatenate([REF[2000:2075], REF[3000:3075]]), T2[L - 75:L + 75]]
    reads = np.concatenate(parts + [np.asarray(h, np.uint8) for h in hand]).astype(np.uint8)
    n = len(reads) // 150
    return reads, np.arange(n, dtype=np.int64) * 150, np.full(n, 150, np.int32), n - len(hand)


class Pipe:
    """the restatement of every stage under the table, each on the one before"""

    def __init__(self, tab=TAB):
        import matesw_py as mp
        import oracle
        import pe_py as pp
        from test_memchain import _copt_dict
        self.reads, self.off, self.lens, self.hand0 = reads, off, lens, hand0 = _pipe_reads()
        f = oracle.FmiRef(REF)
        self.mems, self.cnt = mems, cnt = f.collect_intv(reads, off, lens, cap=256, nthreads=8)
        self.tr = tr = sp.Trace()
        copt = oracle.chain_opt()
        self.seeds, self.sr, self.sc = cp.mem_chain(tab, _copt_dict(copt), f.sa(), lens, mems, cnt, bsw.SEED_DTYPE, tr)
        self.plain_seeds = oracle.mem_chain(f.sa(), L, lens, mems, cnt, copt)
        self.eopt = bsw.ext_opt(l_pac=L)
        self.regs, self.ext = cp.chain2aln(tab, oracle, oracle.make_params(), self.eopt, T2, reads, off, lens, self.seeds,
                                           self.sr, self.sc, tr)
        self.sel = cp.regs_select(tab, T2, reads, off, lens, self.seeds, self.sr, self.sc, self.regs, self.ext, MAT, GAPS,
                                  sp.sel_opt(l_pac=L))
        sregs, _, sinfo, first, _ = self.sel
        self.popt = pp.pe_opt(l_pac=L)
        self.pes, self.tr_stat, _ = cp.pe_stat(tab, sregs, sinfo, first, self.popt, 1)
        self.msw = cp.mate_rescue(tab, self.pes, T2, reads, off, lens, sregs, sinfo, first, mp.matesw_opt(l_pac=L), MAT, GAPS,
                                  oracle.ksw_align2)
        mregs, _, minfo, mfirst, _ = self.msw
        self.paired = cp.pe_pair(tab, self.pes, mregs, minfo, mfirst, self.popt, MAT, GAPS)
        self.ropt = rq.rec_opt(l_pac=L, rname=RNAME)
        self.res = cp.records(tab, T2, reads, off, lens, self.paired[0], self.paired[1], mfirst, self.paired[2], self.ropt,
                              MAT, GAPS)
        self.names = [f"frag{i}".encode() for i in range(len(lens) // 2)]
        self.quals = (33 + (np.arange(len(reads)) * 7) % 41).astype(np.uint8)
        self.text, self.text_off = cp.sam_text(tab, self.res, reads, off, lens, self.names, self.quals, self.ropt, True)
        self.lines = self.text.decode("latin-1").split("\n")[:-1]


_pipe = {}


def pipe():
    if not _pipe:
        _pipe["x"] = Pipe()
    return _pipe["x"]


def test_pipeline_under_the_table_reaches_every_rid_branch():
    import oracle
    p = pipe()
    cnt = sp.Trace().cnt
    for t in (p.tr, p.sel[4], p.tr_stat, p.msw[4], p.paired[3], p.res.tr):
        cnt.update({k: v for k, v in t.cnt.items() if k in cp.BRANCHES})
    print("pipeline rid branches:", {k: cnt[k] for k in cp.BRANCHES})
    front = ("seed_join", "seed_strand", "seed_kept", "merge_other_rid", "merge_same_rid", "dedup_other_rid", "dedup_same_rid")
    assert all(cnt[k] > 0 for k in front), {k: cnt[k] for k in front}
    # the seeds of the table differ from those of the concatenation: the bridging SMEMs of the hand reads are gone
    assert len(p.seeds) != len(p.plain_seeds[0]) or not np.array_equal(p.seeds, p.plain_seeds[0])
    # no region, seed or window over a join anywhere; the records call therefore goes through
    assert not any(TAB.crosses(int(s["rbeg"]), int(s["rbeg"]) + int(s["len"])) for s in p.seeds)
    live = np.flatnonzero(p.ext)
    assert len(live) and not any(TAB.crosses(int(p.regs[k]["rb"]), int(p.regs[k]["re"])) for k in live)
    h = p.hand0                                               # the hand pairs' first read
    sregs, sread, _, first, _ = p.sel
    for r in (h, h + 2, h + 4):                               # cases 1, 1r, 2: a region either side of the join, no patch
        a = sregs[first[r]:first[r + 1]]
        rids = sorted(TAB.rid(int(x["rb"])) for x in a)
        assert rids[:2] == [0, 1], (r, a)
    # case 3: POS 1 and a contig's last base in the text
    f = [x.split("\t") for x in p.lines]
    by = {}
    for x in f:
        by.setdefault(x[0], []).append(x)
    q3 = by[f"frag{(h + 6) // 2}"]
    assert any(x[2] == "1" and x[5] == "150M" and int(x[3]) == 4851 for x in q3) and any(x[2] == "chrD" and x[3] == "1" for x in q3)
    # case 4: mates on different contigs
    q4 = by[f"frag{(h + 8) // 2}"]
    assert q4[0][2] == "1" and q4[0][6] == "chrD" and q4[0][8] == "0" and not int(q4[0][1]) & 2
    # the one-contig decomposition is the plain oracle call
    one = cp.Table([L], [RNAME])
    s1 = p.plain_seeds
    want = oracle.chain2aln(oracle.make_params(), p.eopt, T2, p.reads, p.off, p.lens, *s1)
    got = cp.chain2aln(one, oracle, oracle.make_params(), p.eopt, T2, p.reads, p.off, p.lens, *s1)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


@pytest.mark.gpu
def test_gpu_pipeline_under_the_table():
    """seeding -> chaining -> extension (host-built and resident) -> selection -> statistics -> rescue -> pairing ->
    records -> text, device to device under the table, each stage against the restatement"""
    p = pipe()
    reads, off, lens = p.reads, p.off, p.lens
    nr = len(lens)
    fmi = bsw.Fmi(REF)
    eng = _engine()
    b = ResidentBatch(eng, reads, off, lens, p.quals)
    plain = b.seed_and_chain(fmi)
    for x, y in zip(plain, p.plain_seeds):
        assert np.array_equal(x, y), "no table: seeds"
    # one contig == no table at the front stages too: seeds, regions (resident and host-built), selection
    def front():
        s_, r_, c_ = b.seed_and_chain(fmi)
        b.chain2aln(p.eopt)
        g_, e_ = b.get("regs"), b.get("ext")
        h_ = bsw.chain2aln(eng, T2, reads, off, lens, s_, r_, c_, p.eopt)
        sel_ = bsw.regs_select(eng, reads, off, lens, s_, r_, c_, g_, e_, bsw.sel_opt(l_pac=L))
        return [s_, r_, c_, g_, e_, h_[0], h_[1]] + list(sel_)

    base = front()
    bsw.set_contigs(eng, [L], [RNAME])
    fmi.set_contigs([L])
    for x, y in zip(base, front()):
        assert x.tobytes() == y.tobytes(), "one contig == no table"
    bsw.set_contigs(eng, LENS, NAMES)
    fmi.set_contigs(LENS[:3])
    with pytest.raises(bsw.BswError, match="-22"):
        b.seed_and_chain(fmi)
    with pytest.raises(bsw.BswError, match="-22"):             # the extension calls check the context's table
        bsw.set_contigs(eng, LENS[:3], NAMES[:3])
        bsw.chain2aln(eng, T2, reads, off, lens, plain[0], plain[1], plain[2], p.eopt)
    bsw.set_contigs(eng, LENS, NAMES)
    for bad in ((0,), (-1, 5)):
        with pytest.raises(bsw.BswError, match="-22"):
            fmi.set_contigs(bad)
    fmi.set_contigs(LENS)
    seeds, sr, sc = b.seed_and_chain(fmi)
    assert np.array_equal(seeds, p.seeds) and np.array_equal(sr, p.sr) and np.array_equal(sc, p.sc), "seeds"
    b.chain2aln(p.eopt)
    regs, ext = b.get("regs"), b.get("ext")
    assert np.array_equal(ext, p.ext), np.flatnonzero(ext != p.ext)[:5]
    assert regs.tobytes() == np.ascontiguousarray(p.regs, dtype=bsw.ALNREG_DTYPE).tobytes(), "regions"
    hregs, hext = bsw.chain2aln(eng, T2, reads, off, lens, seeds, sr, sc, p.eopt)     # the host-built form
    assert hregs.tobytes() == regs.tobytes() and np.array_equal(hext, ext), "host-built == resident"
    k = b.select(bsw.sel_opt(l_pac=L))
    assert k == len(p.sel[0])
    same_sel(p.sel, fetch(b, *b.lists[0]), "selection")
    o = bsw.pe_opt(l_pac=L)
    pes = b.pe_stat(o)
    for fl in ("low", "high", "failed", "n"):
        assert np.array_equal(pes[fl], p.pes[fl]), fl
    cap = len(p.msw[0])
    m = b.matesw(pes, bsw.matesw_opt(l_pac=L), cap=cap)
    assert m == cap
    same_msw(p.msw, fetch(b, *b.lists[0]), "rescue", bsw.matesw_last_stats(eng))
    b.pe_pair(pes, o)
    gp = b.get("pairs")
    for fl in bsw.PAIR_DTYPE.names:
        assert np.array_equal(gp[fl], p.paired[2][fl]), fl
    b.records(bsw.rec_opt(**p.ropt))
    rec = fetch(b, *RECORDS)
    b.sam_text(bsw.rec_opt(**p.ropt), p.names, True, cap=len(p.text) + 5)
    same_records(p.res, rec, "pipeline", bsw.rec_last_stats(eng))
    same_text(p.text, p.text_off, got_text(b), "pipeline")
    eng.close()
    fmi.close()
