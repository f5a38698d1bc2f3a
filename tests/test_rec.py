"""SAM records (include/bsw_rec.h): mem_reg2sam, mem_gen_alt, mem_aln2sam and the output block of
mem_sam_pe behind bsw_pe_pair* / bsw_regs_select*.

CPU: hand-built reads and pairs on test_matesw's small random text with answers worked out by pencil
through the Python restatement (tests/rec_py.py), each also mirrored onto the other strand; the
recomputed secondary_all against one carried through the pair call; test_matesw's pipeline set, extended by
the fragments it lacks (chimeric reads, a repeat above max_XA_hits, equal positions), through stat, rescue,
pair and records with every branch of the restatement reached; the header's symbols and
layouts.
GPU: bsw_records* and bsw_sam_text* == the restatement in every record field, alignment, offset,
counter and text byte.  Parity is unpinned by the reference tree (it holds no source of these
functions; bsw_rec.h restates them).
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import bsw
import pe_py as pp
import rec_py as rq
import reg2aln_py as rp
import regsel_py as sp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import (DEFAULT, RECORDS, SCORINGS, declared, engine_of, exported, fetch, got_text, mat_gaps, revcomp,
                      same_records, same_text)
from test_matesw import L, REF, RL, T, T_MIRROR, MsBatch, ms_set, reg, rnd

RNAME = "chrT"
LET = "ACGTN"


def seq_of(codes):
    return "".join(LET[int(c)] for c in codes)


def rv(s, e):
    """the reverse-strand read over forward [s, e) and its region's (rb, re)"""
    return revcomp(REF[s:e]), 2 * L - e, 2 * L - s


def pairs_of(*rows):
    """rows of (paired, z0, z1, mapq0, mapq1, proper)"""
    p = np.zeros(len(rows), dtype=bsw.PAIR_DTYPE)
    for i, (paired, z0, z1, q0, q1, proper) in enumerate(rows):
        p[i]["paired"], p[i]["z"], p[i]["mapq"], p[i]["proper"] = paired, (z0, z1), (q0, q1), proper
    return p


class Case:
    """a batch with its pair decisions (None: single-end), names, quals and options"""

    def __init__(self, batch, pairs=None, quals=None, **optkw):
        self.batch, self.pairs, self.optkw = batch, pairs, optkw
        n = len(batch.reads) // 2 if pairs is not None else len(batch.reads)
        self.names = [f"q{i}".encode() for i in range(n)]
        self.quals = quals

    def run(self, scoring=DEFAULT, mirror=False, cigar_stride=16, md_stride=64, **kw):
        b = self.batch.mirrored() if mirror else self.batch
        mat, gaps = mat_gaps(scoring)
        a = scoring[0]
        reads, off, lens, regs, info, first = b.arrays(a)
        info["mapq"] = [g.get("mapq", 0) for e in b.ends for g in e]
        okw = dict(l_pac=L, rname=RNAME, T=30 * a)
        okw.update(self.optkw)
        okw.update(kw)
        opt = rq.rec_opt(**okw)
        res = rq.records(T_MIRROR if mirror else T, reads, off, lens, regs, info, first, self.pairs, opt, mat, gaps,
                         cigar_stride, md_stride)
        text, toff = rq.sam_text(res, reads, off, lens, self.names, self.quals, opt, self.pairs is not None)
        res.text, res.text_off, res.opt = text, toff, opt
        res.arrays = (reads, off, lens, regs, info, first)
        res.lines = text.decode("latin-1").split("\n")[:-1]
        return res


def _fields(res, i):
    return res.lines[i].split("\t")


def check_mirror(c, **kw):
    """the other strand gives the mirrored answers: strands flipped, pos = l_pac - (pos + rlen), TLEN negated"""
    w, m = c.run(**kw), c.run(mirror=True, **kw)
    assert len(w.recs) == len(m.recs) and np.array_equal(w.rec_first, m.rec_first)
    for p, q in zip(w.recs, m.recs):
        for f in ("read", "reg", "aln", "which", "n_list", "mapq", "score", "sub", "m_aln", "xa_first", "xa_n"):
            assert p[f] == q[f], f
        assert q["tlen"] == -p["tlen"]
        flip = (0x10 if p["pos"] >= 0 else 0) | (0x20 if p["mpos"] >= 0 else 0)
        assert q["flag"] == p["flag"] ^ flip and q["sam_flag"] == p["sam_flag"] ^ flip
        if p["aln"] >= 0:
            rl = rq._rlen(w.cigar[p["aln"], :w.aln[p["aln"]]["n_cigar"]])
            assert q["pos"] == L - (p["pos"] + rl)
            cw, cm = list(w.cigar[p["aln"], :w.aln[p["aln"]]["n_cigar"]]), list(m.cigar[q["aln"], :m.aln[q["aln"]]["n_cigar"]])
            if all((int(x) & 15) in (0, 3) for x in cw):       # (an indel is left-aligned on either strand)
                assert cm == cw[::-1]
            assert rq._rlen(cm) == rl and m.aln[q["aln"]]["NM"] == w.aln[p["aln"]]["NM"]
    return w, m


# ---------------------------------------------------------------- CPU: single-end records
def case_basic():
    b = MsBatch()
    r1, rb1, re1 = rv(2000, 2100)
    b.reads = [REF[1000:1100], r1, REF[3000:3100], REF[3000:3100], rnd(seed=5)]
    b.ends = [[reg(1000, 100, mapq=60)], [reg(rb1, 100, mapq=37, sub=55, csub=61)],
              [reg(3000, 29, qb=0, qe=30, mapq=9)], [reg(3000, 30, qb=0, qe=30, mapq=9)], []]
    quals = np.frombuffer((b"I" * 50 + b"5" * 50) * 5, dtype=np.uint8).copy()
    return Case(b, None, quals)


def test_single_end_forward_reverse_threshold_and_empty_list():
    w = case_basic().run()
    q = "I" * 50 + "5" * 50
    # two complete lines by hand
    assert w.lines[0] == f"q0\t0\tchrT\t1001\t60\t100M\t*\t0\t0\t{seq_of(REF[1000:1100])}\t{q}\tNM:i:0\tMD:Z:100\tAS:i:100\tXS:i:0"
    assert w.lines[1] == f"q1\t16\tchrT\t2001\t37\t100M\t*\t0\t0\t{seq_of(REF[2000:2100])}\t{q[::-1]}\tNM:i:0\tMD:Z:100\tAS:i:100\tXS:i:61"
    assert w.lines[2] == f"q2\t4\t*\t0\t0\t*\t*\t0\t0\t{seq_of(REF[3000:3100])}\t{q}\tAS:i:0\tXS:i:0"     # score == T - 1
    assert _fields(w, 3)[:6] == ["q3", "0", "chrT", "3001", "9", "30M70S"] and _fields(w, 3)[-2:] == ["AS:i:30", "XS:i:0"]
    assert w.lines[4].startswith("q4\t4\t*\t0\t0\t*\t*\t0\t0\t")
    assert list(w.rec_first) == [0, 1, 2, 3, 4, 5] and list(w.recs["aln"]) == [0, 1, -1, 2, -1]
    assert list(w.recs["reg"]) == [0, 1, -1, 3, -1] and list(w.aln_reg) == [0, 1, 3]
    assert rq.stats_of(w) == dict(n_rec=5, n_unmapped=2, n_supp=0, n_xa=0, n_aln=3, n_overflow=0)
    assert len(w.text) == w.text_off[-1] and all(w.text[w.text_off[i + 1] - 1] == 10 for i in range(5))
    nq = Case(case_basic().batch).run()                       # no quals: `*`
    assert _fields(nq, 0)[10] == "*" and _fields(nq, 1)[10] == "*"
    w, m = check_mirror(case_basic())
    assert _fields(m, 0)[1] == "16" and _fields(m, 0)[9] == seq_of(revcomp(REF[1000:1100])) and _fields(m, 1)[1] == "0"


def case_supp(**kw):
    """a chimeric read: [0, 60) forward at 5000, [60, 100) on the reverse strand over forward [9000, 9040)"""
    b = MsBatch()
    r2, rb2, re2 = rv(9000, 9040)
    b.reads = [np.concatenate([REF[5000:5060], r2])]
    b.ends = [[reg(5000, 60, qb=0, qe=60, mapq=50), reg(rb2, 40, qb=60, qe=100, mapq=55, sub=20)]]
    quals = np.frombuffer(bytes(range(33, 133)), dtype=np.uint8).copy()
    return Case(b, None, quals, **kw)


def test_supplementary_records():
    w = case_supp().run()
    read = case_supp().batch.reads[0]
    ql = bytes(range(33, 133)).decode("latin-1")
    f0, f1 = _fields(w, 0), _fields(w, 1)
    assert f0[:6] == ["q0", "0", "chrT", "5001", "50", "60M40S"] and f0[9] == seq_of(read) and f0[10] == ql
    assert f0[11:] == ["NM:i:0", "MD:Z:60", "AS:i:60", "XS:i:0", "SA:Z:chrT,9001,-,40M60S,50,0;"]
    # 0x800 | 0x10, MAPQ 55 lowered to the primary's 50, hard clip, SEQ / QUAL cut to [60, 100) and reversed
    assert f1[:6] == ["q0", "2064", "chrT", "9001", "50", "40M60H"]
    assert f1[9] == seq_of(REF[9000:9040]) and f1[10] == ql[60:100][::-1]
    assert f1[11:] == ["NM:i:0", "MD:Z:40", "AS:i:40", "XS:i:20", "SA:Z:chrT,5001,+,60M40S,50,0;"]
    assert list(w.recs["which"]) == [0, 1] and list(w.recs["n_list"]) == [2, 2] and w.tr.cnt["supp_capped"] == 1
    k = case_supp(flags=rq.KEEP_SUPP_MAPQ).run()                # -q
    assert _fields(k, 1)[4] == "55" and _fields(k, 0)[-1] == "SA:Z:chrT,9001,-,40M60S,55,0;"
    m = case_supp(flags=rq.NO_MULTI).run()                      # -M: printed 0x100, internal 0x10000, SA stays
    assert _fields(m, 1)[1] == str(0x100 | 0x10) and m.recs[1]["flag"] == 0x10010 and _fields(m, 1)[-1].startswith("SA:Z:")
    assert _fields(m, 0)[-1] == "SA:Z:chrT,9001,-,40M60S,50,0;"
    y = case_supp(flags=rq.SOFTCLIP).run()                      # -Y
    assert _fields(y, 1)[5] == "40M60S" and _fields(y, 1)[9] == seq_of(revcomp(read)) and _fields(y, 1)[10] == ql[::-1]
    check_mirror(case_supp())


def case_sa3():
    b = MsBatch()
    b.reads = [np.concatenate([REF[5000:5040], REF[9000:9030], REF[12000:12030]])]
    b.ends = [[reg(5000, 40, qb=0, qe=40, mapq=60), reg(9000, 30, qb=40, qe=70, mapq=20),
               reg(12000, 30, qb=70, qe=100, mapq=30)]]
    return Case(b)


def test_sa_cross_references_among_three_primaries():
    w = case_sa3().run()
    a, b_, c = "chrT,5001,+,40M60S,60,0;", "chrT,9001,+,40S30M30S,20,0;", "chrT,12001,+,70S30M,30,0;"
    assert [_fields(w, i)[-1] for i in range(3)] == ["SA:Z:" + b_ + c, "SA:Z:" + a + c, "SA:Z:" + a + b_]
    assert [_fields(w, i)[5] for i in range(3)] == ["40M60S", "40H30M30H", "70H30M"]
    assert [_fields(w, i)[1] for i in range(3)] == ["0", "2048", "2048"]
    assert _fields(w, 1)[9] == seq_of(REF[9000:9030])
    check_mirror(case_sa3())


# ---------------------------------------------------------------- CPU: XA
def _xa_members(n, score):
    return [reg(7000 + 500 * i, score, qb=0, qe=24, secondary=0) for i in range(n)]


def case_xa():
    b = MsBatch()
    rd = REF[1000:1100]
    b.reads = [rd] * 4
    b.ends = [[reg(1000, 100, mapq=3)] + _xa_members(5, 90),
              [reg(1000, 100, mapq=3)] + _xa_members(6, 90),
              [reg(1000, 100, mapq=3), reg(7000, 82, qb=0, qe=24, secondary=0), reg(7500, 78, qb=0, qe=24, secondary=0)],
              # a primary below T keeps its members unaligned; region 1 is its secondary
              [reg(1000, 100, qb=0, qe=50, mapq=3), reg(1050, 29, qb=50, qe=100, mapq=0), reg(7000, 28, qb=50, qe=74, secondary=1)]]
    return Case(b)


def test_xa_groups_of_five_and_six_the_ratio_and_unrecorded_primaries():
    for sc in (82, 78):                                       # at least one unit from the product, either side
        assert abs(sc - 100 * float(np.float32(0.8))) >= 1
    w = case_xa().run()
    assert list(w.recs["xa_n"]) == [5, 0, 1, 0] and list(w.recs["xa_first"]) == [1, 7, 8, 10]
    assert list(w.aln_reg) == [0, 1, 2, 3, 4, 5, 6, 13, 14, 16]
    assert w.tr.cnt["xa_dropped_many"] == 1 and w.tr.cnt["xa_below_ratio"] == 1
    xa = _fields(w, 0)[-1]
    assert xa.startswith("XA:Z:chrT,+") and xa.count(";") == 5 and all(len(x.split(",")) == 4 for x in xa[5:-1].split(";"))
    assert not any(f.startswith("XA:Z:") for f in _fields(w, 1)) and _fields(w, 2)[-1].count(";") == 1
    assert rq.stats_of(w)["n_xa"] == 6 and rq.stats_of(w)["n_aln"] == 10 < len(w.arrays[3])
    # the member's text is its own alignment's: strand, pos + 1, CIGAR with S clips, NM
    a = w.aln[8]
    assert _fields(w, 2)[-1] == f"XA:Z:chrT,+{a['pos'] + 1},{rp.cigar_str(w.cigar[8, :a['n_cigar']])},{a['NM']};"
    check_mirror(case_xa())


# ---------------------------------------------------------------- CPU: the paired branch
def case_switch():
    """end 0's chosen region is a former secondary (bsw_pe_pair* left secondary = -2): the switch hands it the
    primary's members, the primary itself among them"""
    b = MsBatch()
    r1, rb1, re1 = rv(20400, 20500)
    b.add("p", REF[20000:20100],
          [reg(1000, 100, qb=0, qe=30, mapq=0), reg(20000, 95, secondary=-2, sub=100, mapq=0), reg(7000, 90, qb=0, qe=24, secondary=0)],
          r1, [reg(rb1, 100, mapq=60)])
    return Case(b, pairs_of((1, 1, 0, 17, 60, 1)))


def test_paired_branch_switches_primary_and_secondary():
    c = case_switch()
    w = c.run()
    assert list(w.recs["reg"]) == [1, 3] and list(w.aln_reg) == [1, 0, 2, 3]
    assert (w.recs[0]["xa_n"], w.recs[0]["xa_first"], w.recs[0]["which"], w.recs[0]["n_list"]) == (2, 1, 0, 1)
    assert w.tr.cnt["recomputed"] == 1 and w.tr.cnt["switch"] == 1
    f0, f1 = _fields(w, 0), _fields(w, 1)
    assert f0[:9] == ["q0", str(0x40 | 0x1 | 0x2 | 0x20), "chrT", "20001", "17", "100M", "=", "20401", "500"]
    assert f1[:9] == ["q0", str(0x80 | 0x1 | 0x2 | 0x10), "chrT", "20401", "60", "100M", "=", "20001", "-500"]
    assert f0[11:15] == ["NM:i:0", "MD:Z:100", "MC:Z:100M", "AS:i:95"] and f0[15] == "XS:i:100" and f0[16].count(";") == 2
    # without the recomputation z's secondary_all would read -1: no switch, no members
    lists = pp.lists_of(dict(l_pac=L), *c.run().arrays[3:6])
    assert rq.secondary_all(w.opt, lists[0]) == [-1, 0, 0] and [x["secondary"] for x in lists[0]] == [-1, -2, 0]
    check_mirror(c)


def case_pe():
    """pair 0 proper (paired branch, FR), pair 1 improper (paired branch, z = {0, 0}), pair 2 no_pairing with two
    records on end 0 and a clipped mate, pair 3 one end unmapped, pair 4 both unmapped, pair 5 RF with a deletion
    and an insertion, pair 6 equal positions"""
    b = MsBatch()
    r, rb, re_ = rv(1400, 1500)
    b.add("proper", REF[1000:1100], [reg(1000, 100, mapq=60)], r, [reg(rb, 100, mapq=60)])
    b.add("improper", REF[1000:1100], [reg(1000, 100, mapq=60)], REF[25000:25100], [reg(25000, 100, mapq=60)])
    r2, rb2, re2 = rv(9000, 9040)
    b.add("nopair", np.concatenate([REF[5000:5060], r2]),
          [reg(5000, 60, qb=0, qe=60, mapq=50), reg(rb2, 40, qb=60, qe=100, mapq=55)],
          REF[5300:5400], [reg(5310, 90, qb=10, qe=100, mapq=40)])
    r3, rb3, re3 = rv(1400, 1500)
    b.add("one", r3, [reg(rb3, 100, mapq=33)], rnd(seed=6), [])
    b.add("none", rnd(seed=7), [], rnd(seed=8), [reg(100, 20, qb=0, qe=20)])
    dele = np.concatenate([REF[1000:1050], REF[1053:1103]])
    ins = np.concatenate([REF[1300:1350], (REF[1350:1353] + 1) % 4, REF[1350:1397]])
    b.add("rf", revcomp(dele), [reg(2 * L - 1103, 91, re=2 * L - 1000, mapq=60)], ins, [reg(1300, 88, re=1397, mapq=60)])
    b.add("equal", REF[1000:1100], [reg(1000, 100, mapq=60)], REF[1000:1100], [reg(1000, 100, mapq=60)])
    pairs = pairs_of((1, 0, 0, 60, 59, 1), (1, 0, 0, 11, 12, 0), (0, 0, 0, 50, 40, 1), (0, 0, -1, 33, 0, 0),
                     (0, -1, -1, 0, 0, 0), (1, 0, 0, 60, 60, 1), (1, 0, 0, 60, 60, 0))
    return Case(b, pairs)


def test_paired_end_flags_mates_tlen_and_mc():
    w = case_pe().run()
    F = [_fields(w, i) for i in range(len(w.lines))]
    assert list(w.rec_first) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    # proper FR
    assert F[0][:9] == ["q0", "99", "chrT", "1001", "60", "100M", "=", "1401", "500"]
    assert F[1][:9] == ["q0", "147", "chrT", "1401", "59", "100M", "=", "1001", "-500"]
    assert F[0][11:] == ["NM:i:0", "MD:Z:100", "MC:Z:100M", "AS:i:100", "XS:i:0"]
    # improper, FF
    assert F[2][:9] == ["q1", "65", "chrT", "1001", "11", "100M", "=", "25001", "24001"]
    assert F[3][:9] == ["q1", "129", "chrT", "25001", "12", "100M", "=", "1001", "-24001"]
    # no_pairing: every record of end 0 carries 0x41 | 0x2 and the mate's record 0; MC is the mate's CIGAR with
    # THIS record's clip letter
    assert F[4][:9] == ["q2", "67", "chrT", "5001", "50", "60M40S", "=", "5311", "311"]
    assert F[5][:9] == ["q2", str(0x43 | 0x800 | 0x10), "chrT", "9001", "50", "40M60H", "=", "5311", "-3730"]
    assert F[4][13] == "MC:Z:10S90M" and F[5][13] == "MC:Z:10H90M"
    assert F[6][:9] == ["q2", "131", "chrT", "5311", "40", "10S90M", "=", "5001", "-311"] and F[6][13] == "MC:Z:60M40S"
    # one end unmapped: the mapped end's mate fields are its own position and strand, no MC, TLEN 0; the unmapped
    # end is placed there, printed on that strand, with MC and without NM / MD
    assert F[7][:9] == ["q3", str(0x41 | 0x8 | 0x10 | 0x20), "chrT", "1401", "33", "100M", "=", "1401", "0"]
    assert F[7][11:] == ["NM:i:0", "MD:Z:100", "AS:i:100", "XS:i:0"]
    assert F[8][:9] == ["q3", str(0x81 | 0x4 | 0x10 | 0x20), "chrT", "1401", "0", "*", "=", "1401", "0"]
    assert F[8][9] == seq_of(revcomp(rnd(seed=6))) and F[8][11:] == ["MC:Z:100M", "AS:i:0", "XS:i:0"]
    # both unmapped (end 1's only region is below T)
    assert F[9][:9] == ["q4", "77", "*", "0", "0", "*", "*", "0", "0"] and F[10][:9] == ["q4", "141", "*", "0", "0", "*", "*", "0", "0"]
    assert F[9][11:] == ["AS:i:0", "XS:i:0"]
    # RF over a deletion (rlen 103) and an insertion (rlen 97)
    ins = case_pe().batch.reads[11]
    s = 0                                                      # indels come out left-aligned: the insertion slides
    while ins[49 - s] == ins[52 - s]:                          # left over bases equal to its own end
        s += 1
    icig = f"{50 - s}M3I{47 + s}M"
    assert F[11][:9] == ["q5", str(0x43 | 0x10), "chrT", "1001", "60", "50M3D50M", "=", "1301", "199"]
    assert F[12][:9] == ["q5", str(0x83 | 0x20), "chrT", "1301", "60", icig, "=", "1001", "-199"]
    assert F[11][13] == "MC:Z:" + icig and F[12][11] == "NM:i:3"
    assert F[11][12] == "MD:Z:50^" + seq_of(REF[1050:1053]) + "50"
    # equal positions
    assert F[13][:9] == ["q6", "65", "chrT", "1001", "60", "100M", "=", "1001", "0"] and F[14][8] == "0"
    assert list(w.recs["m_aln"][:9]) == [1, 0, 3, 2, 6, 6, 4, -1, 7]
    assert rq.stats_of(w) == dict(n_rec=15, n_unmapped=3, n_supp=1, n_xa=0, n_aln=12, n_overflow=0)
    check_mirror(case_pe())


def test_errors_of_the_restatement():
    c = case_pe()
    with pytest.raises(ValueError, match="INVAL"):
        Case(c.batch, c.pairs, rname="").run()
    b = MsBatch()
    b.reads = [REF[1000:1100]] * 3
    b.ends = [[reg(1000, 100)], [], []]
    with pytest.raises(ValueError, match="INVAL"):              # an odd n_reads with pairs
        Case(b, pairs_of((0, 0, -1, 0, 0, 0))).run()
    with pytest.raises(ValueError, match="RANGE"):              # a stride overflow
        case_sa3().run(cigar_stride=2)
    with pytest.raises(ValueError, match="RANGE"):
        case_pe().run(md_stride=4)
    b = MsBatch()
    b.reads = [REF[1000:1100]]
    b.ends = [[reg(L - 50, 100)]]                               # spans the strands: rejected, yet needed
    with pytest.raises(ValueError, match="RANGE"):
        Case(b).run()
    b = MsBatch()
    b.add("z", REF[1000:1100], [reg(1000, 100)], REF[1000:1100], [reg(1000, 100)])
    with pytest.raises(ValueError, match="RANGE"):              # z outside its list
        Case(b, pairs_of((1, 0, 1, 0, 0, 0))).run()


HAND = dict(basic=case_basic, supp=case_supp, sa3=case_sa3, xa=case_xa, switch=case_switch, pe=case_pe)


# ---------------------------------------------------------------- CPU: the pipeline set
def _rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


class ExtSet:
    """test_matesw's 1,500 fragments on their reference extended by a tail that holds what that set lacks, plus
    the fragments that use it -- through the same oracle front end, regsel_py, pe_py, matesw_py, pe_py:
      a 150-base unit in 7 copies, six of them with one substitution (an XA group above max_XA_hits),
      a 90-base unit in 2 exact copies and a unique stretch (a chimeric read: its larger part a MAPQ-0 primary,
      its smaller part a supplementary whose MAPQ is capped),
      a fragment whose ends are the same forward read (equal positions: TLEN 0)"""

    def __init__(self):
        import bench
        import matesw_py as mp
        import oracle
        from test_memchain import _oracle_front, _two_strand
        from test_regsel import _select
        base = ms_set()
        ref0 = bench.seeding_reference(300_000, seed=3)
        assert np.array_equal(_two_strand(ref0), base.T)
        rng = np.random.default_rng(77)
        tail = rng.integers(0, 4, 20_000).astype(np.uint8)
        unit = rng.integers(0, 4, 150).astype(np.uint8)
        for i in range(7):                                     # copy i at 1000 + 1500 i; copies 1..6 one substitution each
            c = unit.copy()
            if i:
                c[20 * i + 5] = (c[20 * i + 5] + 1) % 4
            tail[1000 + 1500 * i:1150 + 1500 * i] = c
        u2 = rng.integers(0, 4, 90).astype(np.uint8)
        tail[12000:12090] = u2
        tail[14000:14090] = u2
        ref = np.concatenate([ref0, tail])
        o = len(ref0)
        extra = []
        for rep in range(3):                                   # a few of each, at shifted mates
            extra += [(tail[1000:1150], _rc(tail[1400 + rep:1550 + rep])),
                      (np.concatenate([u2, tail[17000 + rep:17060 + rep]]), _rc(tail[12400 + rep:12550 + rep])),
                      (tail[18000 + rep:18150 + rep], tail[18000 + rep:18150 + rep])]
        a0 = base.arr
        reads = np.concatenate([a0["reads"]] + [np.concatenate(p) for p in extra]).astype(np.uint8)
        n = len(reads) // 150
        off, lens = np.arange(n, dtype=np.int64) * 150, np.full(n, 150, np.int32)
        self.n_pairs = n // 2
        self.T = Tt = _two_strand(ref)
        self.l_pac = len(ref)
        f, mems, cnt, seeds, sr, sc = _oracle_front(ref, reads, off, lens, cap=256)
        self.eopt = bsw.ext_opt(l_pac=len(ref))
        regs, ext = oracle.chain2aln(oracle.make_params(), self.eopt, Tt, reads, off, lens, seeds, sr, sc)
        self.arr = dict(reads=reads, off=off, lens=lens, seeds=seeds, sr=sr, sc=sc, regs=regs, ext=ext)
        self.sopt = sp.sel_opt(l_pac=self.l_pac)
        self.regs, _, self.info, self.first, _ = _select(Tt, self.arr, opt=self.sopt)
        self.opt = pp.pe_opt(l_pac=self.l_pac)
        self.mat, self.gaps = mat_gaps(DEFAULT)
        self.pes, _, _ = pp.pe_stat(self.regs, self.info, self.first, self.opt, 1)
        self.mregs, self.mread, self.minfo, self.mfirst, self.tr = mp.mate_rescue(
            self.pes, Tt, reads, off, lens, self.regs, self.info, self.first, mp.matesw_opt(l_pac=self.l_pac), self.mat,
            self.gaps, oracle.ksw_align2)
        self.paired = pp.pe_pair(self.pes, self.mregs, self.minfo, self.mfirst, self.opt, self.mat, self.gaps)


_xset = {}


def ext_set():
    if not _xset:
        _xset["x"] = ExtSet()
    return _xset["x"]


class RecSet:
    """the extended pipeline set after stat, rescue and pair, through records and text"""

    def __init__(self):
        p = self.p = ext_set()
        self.regs, self.info, self.pairs, _ = p.paired
        a = p.arr
        self.opt = rq.rec_opt(l_pac=p.l_pac, rname=RNAME)
        self.res = rq.records(p.T, a["reads"], a["off"], a["lens"], self.regs, self.info, p.mfirst, self.pairs, self.opt,
                              p.mat, p.gaps)
        self.names = [f"frag{i}".encode() for i in range(p.n_pairs)]
        self.quals = (33 + (np.arange(len(a["reads"])) * 7) % 41).astype(np.uint8)
        self.text, self.text_off = rq.sam_text(self.res, a["reads"], a["off"], a["lens"], self.names, self.quals, self.opt,
                                               True)


_rset = {}


def rec_set():
    if not _rset:
        _rset["x"] = RecSet()
    return _rset["x"]


def test_pipeline_set_reaches_every_branch():
    s = rec_set()
    c = s.res.tr.cnt
    print("rec set:", dict(c), rq.stats_of(s.res), "bytes", len(s.text))
    assert all(c[k] > 0 for k in rq.BRANCHES), {k: c[k] for k in rq.BRANCHES if c[k] == 0}
    st = rq.stats_of(s.res)
    assert st["n_supp"] > 0 and st["n_aln"] < len(s.regs) and st["n_aln"] == st["n_rec"] - st["n_unmapped"] + st["n_xa"]
    lines = s.text.decode("latin-1").split("\n")[:-1]
    assert len(lines) == st["n_rec"] and all(len(x.split("\t")) >= 13 for x in lines)


def test_recomputed_secondary_all_is_the_carried_one():
    """every list of the pipeline set: secondary_all recomputed from what bsw_pe_pair* left == the one a pair
    call carries along (the marking's own secondary, before the chosen region's is overwritten)"""
    s = rec_set()
    p = s.p
    carried = rq.carried_secondary_all(p.opt, p.mregs, p.minfo, p.mfirst, p.mat, p.gaps)
    lists = pp.lists_of(dict(l_pac=p.l_pac), s.regs, s.info, p.mfirst)
    got = [v for a in lists for v in rq.secondary_all(s.opt, a)]
    assert got == carried
    n2 = int((s.info["secondary"] == -2).sum())
    assert n2 > 0 and sum(1 for g, i in zip(got, s.info) if i["secondary"] == -2 and g >= 0) == n2


# ---------------------------------------------------------------- CPU: the header
def test_library_exports_the_rec_header():
    assert declared("bsw_rec.h") == set(bsw.REC_SYMBOLS)
    assert declared("bsw_rec.h") <= exported(), declared("bsw_rec.h") - exported()
    others = (set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS) |
              set(bsw.MATESW_SYMBOLS))
    assert not set(bsw.REC_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_rec_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_rec.h"\n'
                   f"{sa}(sizeof(bsw_rec_opt_t) == 96 && offsetof(bsw_rec_opt_t, max_XA_hits) == 16 && offsetof(bsw_rec_opt_t, rname) == 32, \"opt\");\n"
                   f"{sa}(sizeof(bsw_rec_t) == 88 && offsetof(bsw_rec_t, tlen) == 16 && offsetof(bsw_rec_t, read) == 24 && offsetof(bsw_rec_t, sam_flag) == 48 && offsetof(bsw_rec_t, m_aln) == 72 && offsetof(bsw_rec_t, xa_n) == 80, \"rec\");\n"
                   f"{sa}(sizeof(bsw_rec_stats_t) == 48 && offsetof(bsw_rec_stats_t, n_bytes) == 24 && offsetof(bsw_rec_stats_t, text_ms) == 40, \"stats\");\n"
                   f"{sa}(BSW_REC_API == 1 && BSW_ABI_VERSION == 8, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.RecOpt) == 96 and bsw.RecOpt.max_XA_hits.offset == 16 and bsw.RecOpt.rname.offset == 32
    assert ctypes.sizeof(bsw.RecStats) == 48 and bsw.RecStats.n_bytes.offset == 24 and bsw.RecStats.text_ms.offset == 40
    assert bsw.REC_DTYPE.itemsize == 88 and bsw.REC_DTYPE.fields["sam_flag"][1] == 48 and bsw.REC_DTYPE.fields["xa_n"][1] == 80
    assert bsw.REC_DTYPE == rq.REC_DTYPE


def _lib_calls(ctx, o, n_reads=2, pairs=True, cs=16, ms=64, text_cap=8, calls=3):
    Lb = bsw.hip_lib()
    regs, info = np.zeros(1, dtype=bsw.ALNREG_DTYPE), np.zeros(1, dtype=bsw.SELINFO_DTYPE)
    first, reads = np.zeros(n_reads + 2, dtype=np.int32), np.zeros(8, np.uint8)
    off, lens = np.zeros(max(n_reads, 1), np.int64), np.zeros(max(n_reads, 1), np.int32)
    pr, recs = np.zeros(2, dtype=bsw.PAIR_DTYPE), np.zeros(4, dtype=bsw.REC_DTYPE)
    aln, areg = np.zeros(4, dtype=bsw.ALN_DTYPE), np.zeros(4, np.int32)
    cig, md = np.zeros(64, np.uint32), np.zeros(256, np.uint8)
    noff, toff, text = np.zeros(4, np.int64), np.zeros(8, np.int64), np.zeros(8, np.uint8)
    nr, na, nb = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    P, B = bsw._ptr, ctypes.byref
    pp_ = P(pr) if pairs else None
    rec = () if not calls & 1 else (
            Lb.bsw_records(ctx, B(o), P(reads), P(off), P(lens), n_reads, P(regs), P(info), P(first), pp_, P(recs),
                           P(first), 4, P(aln), P(areg), P(cig), cs, P(md), ms, 4, B(nr), B(na)),
            Lb.bsw_records_resident(ctx, B(o), P(reads), P(off), P(lens), n_reads, P(regs), P(info), P(first), 0, pp_,
                                    P(recs), P(first), 4, P(aln), P(areg), P(cig), cs, P(md), ms, 4, B(nr), B(na), None))
    return rec if not calls & 2 else rec + (
            Lb.bsw_sam_text(ctx, B(o), P(recs), P(first), 0, P(aln), P(cig), cs, P(md), ms, 0, P(reads), P(off), P(lens),
                            n_reads, P(reads), P(noff), None, int(pairs), P(text), P(toff), text_cap, B(nb)),
            Lb.bsw_sam_text_resident(ctx, B(o), P(recs), P(first), 0, P(aln), P(cig), cs, P(md), ms, 0, P(reads), P(off),
                                     P(lens), n_reads, P(reads), P(noff), None, int(pairs), P(text), P(toff), text_cap,
                                     B(nb), None))


def test_defaults_and_invalid_arguments_need_no_device():
    o = bsw.rec_opt()
    got = {f: getattr(o, f) for f, _ in o._fields_}
    got["rname"] = got["rname"].decode()
    want = dict(rq.DEFAULT_OPT, rname="")
    assert {k: (round(v, 6) if isinstance(v, float) else v) for k, v in got.items()} == want
    Lb = bsw.hip_lib()
    assert Lb.bsw_rec_last_stats(None, None) == -22
    fake = ctypes.c_void_p(1)                                # never dereferenced: the checks come first
    inval = (-22, -22, -22, -22)
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L)) == inval                        # no rname
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname="x" * 64)) == inval        # unterminated
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname=RNAME, flags=8)) == inval
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname=RNAME), n_reads=3) == inval          # odd with pairs
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname=RNAME), cs=0) == inval
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname=RNAME), ms=0) == inval
    assert _lib_calls(None, bsw.rec_opt(l_pac=L, rname=RNAME)) == inval
    for kw in (dict(l_pac=0), dict(l_pac=-1), dict(l_pac=L, w=-1), dict(l_pac=L, max_XA_hits=-1)):
        assert _lib_calls(fake, bsw.rec_opt(rname=RNAME, **kw), calls=1) == (-22, -22), kw
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname=RNAME), text_cap=-1, calls=2) == (-22, -22)
    with pytest.raises(ValueError, match="INVAL"):
        rq.check_opt(rq.rec_opt(l_pac=L, rname="x" * 64), 2, True)


# ---------------------------------------------------------------- GPU
def _bopt(o):
    return bsw.rec_opt(**o)


def _gpu_case(eng, c, w, tag, cigar_stride=16, md_stride=64):
    """both calls through the host forms against the restatement's result w"""
    reads, off, lens, regs, info, first = w.arrays
    o = _bopt(w.opt)
    got = bsw.records(eng, reads, off, lens, regs, info, first, c.pairs, o, cigar_stride, md_stride)
    st = bsw.rec_last_stats(eng)
    same_records(w, got, tag, st)
    assert (st.aln_ms > 0) == (len(w.aln) > 0) and st.helper_ms > 0, tag
    recs, rfirst, aln, aln_reg, cig, md = got
    same_text(w.text, w.text_off, bsw.sam_text(eng, recs, rfirst, aln, cig, md, reads, off, lens, c.names, c.quals, o,
                                                c.pairs is not None), tag)
    st = bsw.rec_last_stats(eng)
    assert st.n_bytes == len(w.text) and st.text_ms > 0 and st.n_rec == len(w.recs), tag


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", SCORINGS)
def test_gpu_hand_sets(scoring):
    eng = engine_of(scoring)
    for mirror in (False, True):
        bsw.set_reference(eng, T_MIRROR if mirror else T)
        for name, mk in HAND.items():
            c = mk()
            _gpu_case(eng, c, c.run(scoring, mirror), f"hand {name} {scoring} {mirror}")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [rq.SOFTCLIP, rq.NO_MULTI, rq.KEEP_SUPP_MAPQ, 7])
def test_gpu_option_flags(flags):
    eng = engine_of()
    bsw.set_reference(eng, T)
    for name in ("supp", "sa3", "pe"):
        c = HAND[name]()
        _gpu_case(eng, c, c.run(flags=flags), f"{name} flags {flags}")
    c = HAND["xa"]()
    _gpu_case(eng, c, c.run(max_XA_hits=6, XA_drop_ratio=0.75), "xa options")
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_host_arrays():
    s = rec_set()
    p, a = s.p, s.p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    o = _bopt(s.opt)
    got = bsw.records(eng, a["reads"], a["off"], a["lens"], s.regs, s.info, p.mfirst, s.pairs, o)
    st = bsw.rec_last_stats(eng)
    same_records(s.res, got, "pipeline set", st)
    # only the needed regions are aligned
    assert st.n_aln == rq.stats_of(s.res)["n_aln"] < len(s.regs)
    recs, rfirst, aln, aln_reg, cig, md = got
    same_text(s.text, s.text_off, bsw.sam_text(eng, recs, rfirst, aln, cig, md, a["reads"], a["off"], a["lens"], s.names,
                                                s.quals, o, True), "pipeline set")
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_device_to_device():
    """bsw_pe_pair_resident -> bsw_records_resident -> bsw_sam_text_resident: the arrays one call leaves in HBM
    are the next call's inputs"""
    s = rec_set()
    p, a = s.p, s.p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], s.quals)
    b.put(mreg=p.mregs, minfo=p.minfo, mfirst=p.mfirst)
    b.pe_pair(p.pes, bsw.pe_opt(l_pac=p.l_pac))
    b.records(_bopt(s.opt))
    rec = fetch(b, *RECORDS)
    b.sam_text(_bopt(s.opt), s.names, True, cap=len(s.text) + 5)
    same_records(s.res, rec, "device to device", bsw.rec_last_stats(eng))
    same_text(s.text, s.text_off, got_text(b), "device to device")
    eng.close()


@pytest.mark.gpu
def test_gpu_single_end_from_regs_select_resident():
    p = ext_set()
    a = p.arr
    nr_all = len(a["lens"])
    opt = rq.rec_opt(l_pac=p.l_pac, rname=RNAME)
    s = RecSet.__new__(RecSet)
    s.res = rq.records(p.T, a["reads"], a["off"], a["lens"], p.regs, p.info, p.first, None, opt, p.mat, p.gaps)
    names = [f"r{i}".encode() for i in range(nr_all)]
    quals = (40 + np.arange(len(a["reads"])) % 30).astype(np.uint8)
    s.text, s.text_off = rq.sam_text(s.res, a["reads"], a["off"], a["lens"], names, quals, opt, False)
    c = s.res.tr.cnt
    assert c["rec_supp"] > 0 and c["supp_capped"] > 0 and c["xa_member"] > 0 and c["xa_dropped_many"] > 0 and c["rec_unmapped"] > 0
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], quals)
    b.put(seeds=a["seeds"], sr=a["sr"], sc=a["sc"])
    b.chain2aln(p.eopt)
    k = b.select(bsw.sel_opt(l_pac=p.l_pac))
    assert k == len(p.regs)
    b.records(_bopt(opt), paired=False)
    rec = fetch(b, *RECORDS)
    b.sam_text(_bopt(opt), names, False, cap=len(s.text) + 5)
    same_records(s.res, rec, "single-end", bsw.rec_last_stats(eng))
    same_text(s.text, s.text_off, got_text(b), "single-end")
    eng.close()


@pytest.mark.gpu
def test_gpu_batch_sizes():
    s = rec_set()
    p, a = s.p, s.p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    o = _bopt(s.opt)
    w = s.res
    for npairs in (0, 1, 63, 64, 65, 257):
        nr = 2 * npairs
        k, nrec = p.mfirst[nr], w.rec_first[nr]
        nal = int(max((w.recs["aln"][:nrec] + 1 + w.recs["xa_n"][:nrec]).max(initial=0), 0))
        got = bsw.records(eng, a["reads"][:nr * 150], a["off"][:nr], a["lens"][:nr], s.regs[:k], s.info[:k],
                          p.mfirst[:nr + 1], s.pairs[:npairs], o)
        sub = rq.Result()
        sub.recs, sub.rec_first, sub.aln, sub.aln_reg = w.recs[:nrec], w.rec_first[:nr + 1], w.aln[:nal], w.aln_reg[:nal]
        sub.cigar, sub.md = w.cigar[:nal], w.md[:nal]
        same_records(sub, got, f"{npairs} pairs", bsw.rec_last_stats(eng))
        recs, rfirst, aln, aln_reg, cig, md = got
        nb = int(s.text_off[nrec])
        same_text(s.text[:nb], s.text_off[:nrec + 1],
                   bsw.sam_text(eng, recs, rfirst, aln, cig, md, a["reads"][:nr * 150], a["off"][:nr], a["lens"][:nr],
                                s.names[:npairs], s.quals[:nr * 150], o, True), f"{npairs} pairs")
    eng.close()


def case_lists(n, xa):
    """a pair whose end 0 has n regions: non-overlapping primaries of 2 bases each past the first, which carries
    xa members; end 1 one region"""
    b = MsBatch()
    e0 = []
    if n:
        e0.append(reg(1000, 100, qb=0, qe=8, mapq=20))
        e0 += _xa_members(min(xa, n - 1), 90)
        for e in e0[1:]:
            e.update(qb=0, qe=8, re=e["rb"] + 8)
        for j in range(len(e0), n):
            q = 8 + 2 * (j - len(e0))
            e0.append(reg(1000 + q, 100 - j, qb=q, qe=q + 2, mapq=j))
    b.add("l", REF[1000:1100], e0, REF[1300:1400], [reg(1300, 100, mapq=60)])
    return Case(b, pairs_of((0, 0 if n else -1, 0, 20, 60, 0)))


@pytest.mark.gpu
def test_gpu_list_lengths():
    eng = engine_of()
    bsw.set_reference(eng, T)
    for n, xa in ((0, 0), (1, 0), (2, 1), (17, 5), (17, 6), (46, 5), (46, 6)):
        c = case_lists(n, xa)
        w = c.run(cigar_stride=4)
        assert w.rec_first[1] == max(n - min(xa, max(n - 1, 0)), 1) and w.recs[0]["xa_n"] == (xa if xa <= 5 and n > 1 else 0)
        _gpu_case(eng, c, w, f"list of {n}, xa {xa}", cigar_stride=4)
    eng.close()


@pytest.mark.gpu
def test_gpu_read_and_name_lengths():
    """the copy loop's edges: reads of 1, 31, 32, 33 and 151 bases on both strands, mapped and not, with and
    without quals; names of 1 and 255 bytes"""
    eng = engine_of()
    bsw.set_reference(eng, T)
    for quals in (True, False):
        b = MsBatch()
        for n in (1, 31, 32, 33, 151):
            r, rb, re_ = rv(4000, 4000 + n)
            b.reads += [REF[3000:3000 + n], r, rnd(n, seed=n)]
            b.ends += [[reg(3000, 40, qb=0, qe=n, mapq=n)], [reg(rb, 40, qb=0, qe=n, mapq=n)], []]
        c = Case(b, None, (33 + np.arange(sum(len(r) for r in b.reads)) % 90).astype(np.uint8) if quals else None)
        c.names = [(b"n" if i % 2 else b"N" * 255) for i in range(len(b.reads))]
        w = c.run()
        assert len(w.recs) == 15 and (w.recs["aln"] >= 0).sum() == 10
        _gpu_case(eng, c, w, f"lengths quals={quals}")
    eng.close()


@pytest.mark.gpu
def test_gpu_errors_and_recovery():
    c = case_pe()
    w = c.run()
    reads, off, lens, regs, info, first = w.arrays
    o = _bopt(w.opt)
    eng = bsw.Engine()
    with pytest.raises(bsw.BswError, match="-22"):            # no resident reference
        bsw.records(eng, reads, off, lens, regs, info, first, c.pairs, o)
    bsw.set_reference(eng, np.zeros(2 * L - 2, np.uint8))     # one that does not fit l_pac
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.records(eng, reads, off, lens, regs, info, first, c.pairs, o)
    bsw.set_reference(eng, T)
    nrec, naln = len(w.recs), len(w.aln)
    for kw in (dict(rec_cap=nrec - 1), dict(aln_cap=naln - 1), dict(rec_cap=0, aln_cap=0)):
        with pytest.raises(bsw.BswError, match="-34") as ei:
            bsw.records(eng, reads, off, lens, regs, info, first, c.pairs, o, **kw)
        assert ei.value.needed == (nrec, naln) and np.array_equal(ei.value.rec_first, w.rec_first), kw
    got = bsw.records(eng, reads, off, lens, regs, info, first, c.pairs, o, rec_cap=nrec, aln_cap=naln)
    same_records(w, got, "exact capacities", bsw.rec_last_stats(eng))
    recs, rfirst, aln, aln_reg, cig, md = got
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.sam_text(eng, recs, rfirst, aln, cig, md, reads, off, lens, c.names, None, o, True, text_cap=len(w.text) - 1)
    assert ei.value.needed == len(w.text) and np.array_equal(ei.value.text_off, w.text_off)
    same_text(w.text, w.text_off, bsw.sam_text(eng, recs, rfirst, aln, cig, md, reads, off, lens, c.names, None, o, True,
                                                text_cap=len(w.text)), "exact text capacity")
    long_names = [b"x" * 256] + c.names[1:]
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.sam_text(eng, recs, rfirst, aln, cig, md, reads, off, lens, long_names, None, o, True)
    bad = recs.copy()
    bad[0]["aln"] = naln
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.sam_text(eng, bad, rfirst, aln, cig, md, reads, off, lens, c.names, None, o, True)
    # a stride overflow: BSW_E_RANGE with the count in the stats
    s3 = case_sa3()
    w3 = s3.run()
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.records(eng, *w3.arrays, None, _bopt(w3.opt), cigar_stride=2)
    assert bsw.rec_last_stats(eng).n_overflow == 1     # 40S30M30S alone has more than two ops
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.records(eng, reads, off, lens, regs, info, first, c.pairs, o, md_stride=4)
    assert bsw.rec_last_stats(eng).n_overflow >= 1
    # a rejected region that a record needs
    b = MsBatch()
    b.reads = [REF[1000:1100]]
    b.ends = [[reg(L - 50, 100)]]
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.records(eng, *b.arrays(), None, o)
    # z outside its list; a decreasing read_first; odd n_reads with pairs
    pz = c.pairs.copy()
    pz[0]["z"] = (0, 1)
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.records(eng, reads, off, lens, regs, info, first, pz, o)
    dec = first.copy()
    dec[3] = dec[2] - 1
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.records(eng, reads, off, lens, regs, info, dec, c.pairs, o)
    P, B = bsw._ptr, ctypes.byref
    nr, na = ctypes.c_int32(0), ctypes.c_int32(0)
    assert bsw.hip_lib().bsw_records(eng._ctx, B(o), P(reads), P(off), P(lens), 3, P(regs), P(info), P(first), P(c.pairs),
                                     P(got[0].copy()), P(first.copy()), 4, P(aln.copy()), P(aln_reg.copy()), P(cig.copy()), 16,
                                     P(md.copy()), 64, 4, B(nr), B(na)) == -22
    _gpu_case(eng, c, w, "after the errors")
    eng.close()
