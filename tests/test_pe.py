"""The paired-end stage (include/bsw_pe.h): mem_pestat, mem_pair and the decision block of
mem_sam_pe behind bsw_regs_select*.

CPU: infer_dir, the statistics and hand-built pairs with known answers through the Python
restatement (tests/pe_py.py), a pipeline set of paired reads through the oracle and regsel_py, the
conditions the GPU comparison rests on (every branch reached, every truncation away from its
boundary), the header's symbols and layouts.
GPU: bsw_pe_stat* and bsw_pe_pair* == the restatement in every output field and counter.  Parity
is unpinned by the reference tree (it holds no source of these functions; bsw_pe.h restates them).
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import bsw
import hiprt
import oracle
import pe_py as pp
import reg2aln_py as rp
import regsel_py as sp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import (DEFAULT, SCORINGS, declared, engine_of, exported, got_aln, got_pair, mat_gaps, same_aln,
                      same_pair, same_pes)
from test_regsel import _select

L = 100_000                                                  # l_pac of the hand-built pairs
RL = 100                                                     # their read length


def _pes(**dirs):
    """pes with every direction failed but the named ones: FR=(low, high, avg, std)"""
    pes = np.zeros(4, dtype=pp.PESTAT_DTYPE)
    pes["failed"] = 1
    for name, (low, high, avg, std) in dirs.items():
        d = ("FF", "FR", "RF", "RR").index(name)
        pes[d] = (low, high, 0, 100, avg, std)
    return pes


PES_FR = _pes(FR=(300, 700, 500.0, 50.0))
PES_WIDE = _pes(FR=(100, 900, 500.0, 50.0))
PES_ALL = _pes(FF=(300, 700, 500.0, 50.0), FR=(300, 700, 500.0, 50.0), RF=(300, 700, 500.0, 50.0),
               RR=(300, 700, 500.0, 50.0))


def reg(rb, score, qb=0, qe=RL, **info):
    return dict(rb=rb, re=rb + (qe - qb), qb=qb, qe=qe, score=score, **info)


def fwd(x, score, **kw):
    """a forward-strand region whose mem_pair coordinate is x"""
    return reg(x, score, **kw)


def rev(x, score, **kw):
    """a reverse-strand region whose mem_pair coordinate (2 l_pac - 1 - rb) is x"""
    return reg(2 * L - 1 - x, score, **kw)


def _shift(g):
    """the other-strand mirror: the doubled text reflected, rb -> (rb + l_pac) mod 2 l_pac.  It is
    what test_regsel._mirror does to a region's strand, with the region's place reflected too, so a
    pair keeps its orientation and its distance"""
    rb = (g["rb"] + L) % (2 * L)
    return dict(g, rb=rb, re=rb + g["re"] - g["rb"])


class PeBatch:
    def __init__(self):
        self.names, self.ends = [], []

    def add(self, name, end0, end1, mirror=True):
        self.names.append(name)
        self.ends += [list(end0), list(end1)]
        if mirror:
            self.names.append(name + "~")
            self.ends += [[_shift(g) for g in end0], [_shift(g) for g in end1]]

    def arrays(self, scale=1):
        """-> (sel_regs, sel_info, read_first); scores (and csub) in units of a"""
        n = sum(len(e) for e in self.ends)
        regs, info = np.zeros(n, dtype=bsw.ALNREG_DTYPE), np.zeros(n, dtype=bsw.SELINFO_DTYPE)
        first, k = [0], 0
        for e in self.ends:
            for g in e:
                regs[k] = (g["rb"], g["re"], g["qb"], g["qe"], g["score"] * scale, g["score"] * scale, 100, 19)
                info[k] = (g.get("seedcov", g["qe"] - g["qb"]), g.get("sub", 0) * scale, g.get("csub", 0) * scale,
                           g.get("sub_n", 0), 1, g.get("secondary", -1), 0, k, g.get("frac_rep", 0.0))
                k += 1
            first.append(k)
        return regs, info, np.array(first, dtype=np.int32)


def _run(batch, pes, scoring=DEFAULT, **optkw):
    mat, gaps = mat_gaps(scoring)
    regs, info, first = batch.arrays(scoring[0])
    opt = pp.pe_opt(l_pac=L, b=scoring[1], **optkw)
    return pp.pe_pair(pes, regs, info, first, opt, mat, gaps)


def _one(name, end0, end1, pes=PES_FR, **kw):
    b = PeBatch()
    b.add(name, end0, end1)
    regs, info, pairs, tr = _run(b, pes, **kw)
    return pairs[0], pairs[1], b, (regs, info), tr


def _fields(p):
    return (int(p["paired"]), list(p["z"]), list(p["mapq"]), int(p["proper"]), int(p["score"]), int(p["sub"]),
            int(p["n_sub"]), int(p["q_pe"]))


# ---------------------------------------------------------------- CPU: infer_dir
def test_infer_dir_four_orientations_on_both_strands():
    R = lambda x: 2 * L - 1 - x                              # noqa: E731  (a reverse-strand rb at place x)
    assert pp.infer_dir(L, 1000, 1500) == (0, 500)           # FF: same strand, the mate ahead
    assert pp.infer_dir(L, 1500, 1000) == (3, 500)           # RR: same strand, the mate behind
    assert pp.infer_dir(L, 1000, R(1500)) == (1, 500)        # FR: p2 = 1500 > 1000
    assert pp.infer_dir(L, 1500, R(1000)) == (2, 500)        # RF: p2 = 1000 < 1500 -> 1 ^ 3
    # the first read on the reverse strand: p2 = 2L - 1 - b2 is compared with the reverse b1
    assert pp.infer_dir(L, R(1500), 1000) == (1, 500)        # FR: p2 = R(1000) > R(1500)
    assert pp.infer_dir(L, R(1000), 1500) == (2, 500)
    assert pp.infer_dir(L, R(1500), R(1000)) == (0, 500)
    assert pp.infer_dir(L, R(1000), R(1500)) == (3, 500)
    assert pp.infer_dir(L, 1000, R(1000)) == (1 ^ 3, 0)      # the same place: p2 == b1 is "not ahead"


# ---------------------------------------------------------------- CPU: statistics
Q12 = [380, 390, 400, 410, 420, 430, 440, 450, 460, 470, 480, 900]


def test_statistics_of_twelve_values_by_pencil():
    tr = sp.Trace()
    # indices (int)(3.499), (int)(9.499): p25 = 410, p75 = 470; first bounds 410 - 120 = 290, 470 + 120 = 590:
    # 900 is outside, the other 11 average 430; their deviations -50 .. 50: sum of squares 11000, / 11 = 1000
    r = pp.pestat_of(Q12, tr)
    assert (r["failed"], r["n"], r["avg"]) == (0, 12, 430.0) and abs(r["std"] - 1000 ** .5) < 1e-12
    # final bounds 410 - 180 = 230 and 470 + 180 = 650; avg -+ 4 std = 303.5, 556.5 lie inside: no widening
    assert (r["low"], r["high"]) == (230, 650) and tr.cnt["dir_widen_low"] + tr.cnt["dir_widen_high"] == 0
    assert pp.pestat_of(Q12[:9], tr)["failed"] == 1 and tr.cnt["dir_few"] == 1
    assert pp.pestat_of(Q12[:9], tr) == dict(low=0, high=0, failed=1, n=9, avg=0.0, std=0.0)


def test_statistics_low_clamp_and_widening():
    tr = sp.Trace()
    # 10 .. 120: p25 = 40, p75 = 100; 40 - 180 < 1 -> 1; 100 + 180 = 280; avg 65, std sqrt(14300 / 12) = 34.5
    r = pp.pestat_of(list(range(10, 130, 10)), tr)
    assert (r["low"], r["high"], r["avg"]) == (1, 280, 65.0) and tr.cnt["dir_low_clamp"] == 1
    # quartiles 480 / 520 (IQR 40), tails at exactly 480 - 80 and 520 + 80 stay in the first bounds:
    # avg = 5920 / 12 = 493.33, std = sqrt(50866.67 / 12) = 65.107; the final 360 and 640 are inside
    # avg -+ 4 std = 232.9, 753.8, so both bounds widen: (int)(232.905 + .499), (int)(753.762 + .499)
    q = [400, 400, 400, 480, 490, 500, 500, 510, 520, 520, 600, 600]
    r = pp.pestat_of(q, tr)
    assert abs(r["avg"] - 5920 / 12) < 1e-9 and abs(r["std"] - (50866.0 / 12 + 2 / 36) ** .5) < 1e-6
    assert (r["low"], r["high"]) == (233, 754) and tr.cnt["dir_widen_low"] == 1 and tr.cnt["dir_widen_high"] == 1


def test_direction_below_five_percent_of_the_largest_fails():
    tr = sp.Trace()
    big = [450 + (k % 100) for k in range(400)]
    pes = pp.pestat_of_dirs([Q12, big, Q12 + Q12[:8], []], tr)
    # 12 < 0.05 * 400 = 20 fails (its bounds stay), 20 does not, 0 failed already
    assert list(pes["failed"]) == [1, 0, 0, 1] and list(pes["n"]) == [12, 400, 20, 0]
    assert (pes[0]["low"], pes[0]["high"]) == (230, 650) and tr.cnt["dir_minor_failed"] == 1


# ---------------------------------------------------------------- CPU: mem_pair by hand
def test_fr_pair_at_the_average_distance():
    # erfc(0) = 1: the term is .721 * log(2) = 0.49976 at a = 1, q = (int)(190 + 0.49976 + .499) = 190
    # score_un = 173 < 190: q_pe = (int)(6.02 * 17 + .499) = 102 -> 60; both MAPQ rules give 60
    p, m, b, _, tr = _one("avg", [fwd(1000, 100)], [rev(1500, 90)])
    assert _fields(p) == (1, [0, 0], [60, 60], 1, 190, 0, 0, 60) == _fields(m)
    assert tr.cnt["u_push"] == 2 and tr.cnt["fast_path"] == 2


@pytest.mark.parametrize("dist,paired", [(299, 0), (300, 1), (700, 1), (701, 0)])
def test_distance_bounds_one_base_either_side(dist, paired):
    p, m, b, _, tr = _one("bound", [fwd(1000, 100)], [rev(1000 + dist, 90)])
    assert p["paired"] == m["paired"] == paired and p["proper"] == paired
    assert tr.cnt["dist_skip"] == 2 * (dist == 299) and tr.cnt["dist_break"] == 2 * (dist == 701)
    if paired:
        # |ns| = 4: .721 * log(2 erfc(2.828)) = -6.47: q = (int)(190 - 6.47 + .499) = 184
        assert (p["score"], p["q_pe"]) == (184, 60)
    else:
        assert _fields(p) == (0, [0, 0], [60, 60], 0, 0, 0, 0, 0)      # no_pairing, outside [low, high]


def test_failed_direction_and_same_position():
    p, m, b, _, tr = _one("ff", [fwd(1000, 100)], [fwd(1500, 90)])
    assert _fields(p) == (0, [0, 0], [60, 60], 0, 0, 0, 0, 0) and tr.cnt["dir_failed_skip"] > 0 and tr.cnt["u_empty"] == 2
    p, m, b, _, tr = _one("ff", [fwd(1000, 100)], [fwd(1500, 90)], pes=PES_ALL)
    assert _fields(p)[:5] == (1, [0, 0], [60, 60], 1, 190)
    # both ends at one place, opposite strands: dist = 0 < low, whichever sorts first
    p, m, b, _, tr = _one("same", [fwd(1000, 100)], [rev(1000, 90)], pes=PES_ALL)
    assert p["paired"] == m["paired"] == 0 and tr.cnt["dist_skip"] >= 2


def test_z_points_at_a_secondary_and_q_pe_lifts_by_forty():
    # end 0: X (100, far away) and Y (95, at the mate) overlap on the read: Y is X's secondary.  Only Y
    # pairs: q = 195, score_un = 183, q_pe = (int)(6.02 * 12 + .499) = 72 -> 60.  Y takes sub = 100 from X:
    # its own MAPQ is 0 and becomes min(60, 0 + 40)
    p, m, b, (regs, info), tr = _one("sec", [fwd(60000, 100), fwd(1000, 95)], [rev(1500, 100)])
    assert _fields(p) == (1, [1, 0], [40, 60], 1, 195, 0, 0, 60) == _fields(m)
    assert list(regs["score"][:2]) == [100, 95] and list(info["secondary"][:2]) == [-1, -2]
    # X: 6.02 * (100 - 95) * 0.4244 = 12.77 -> 13, less (int)(4.343 * log(2) + .499) = 3 for sub_n = 1
    assert list(info["sub"][:2]) == [95, 100] and list(info["sub_n"][:2]) == [1, 0] and list(info["mapq"][:2]) == [10, 0]
    assert tr.cnt["chosen_secondary"] == 2 and tr.cnt["lift40"] == 2 and tr.cnt["z_nonzero"] == 2


def test_runner_up_counts_itself_and_the_hash_breaks_the_tie():
    # two mates 20 either side of the average: equal q = (int)(190 + .721 * log(2 erfc(.2828)) + .499) = 190
    end1 = [rev(1480, 90), rev(1520, 90)]
    p, m, b, _, tr = _one("tie", [fwd(1000, 100)], end1)
    assert (p["score"], p["sub"], p["n_sub"]) == (190, 190, 1) and p["paired"] == 1
    # o - subo = 0 and n_sub = 1: q_pe = 0 - (int)(4.343 * log(2) + .499) = -3 -> 0
    assert p["q_pe"] == 0 and tr.cnt["n_sub"] == 2
    # v sorted by x: end 0 (index 0), then the mates; u's y = k << 32 | i with k = 0; t = pair index << 8
    # which list position each x holds after the second marking (equal scores: the hash sort decides)
    x_of = [2 * L - 1 - int(_[0]["rb"][k]) for k in (1, 2)]
    h = [sp.hash_64((0 << 32 | i) ^ (0 << 8)) & 0xffffffff for i in (1, 2)]     # pair 0: t = 0
    winner_x = (1480, 1520)[int(np.argmax(h))]
    assert int(p["z"][1]) == x_of.index(winner_x)


def test_second_marking_accumulates_sub_n_and_resorts_equal_scores():
    # as bsw_regs_select leaves it: X already carries sub_n = 1 from the first marking
    end0 = [fwd(1000, 100, sub=95, sub_n=1), fwd(1300, 95, secondary=0)]
    p, m, b, (regs, info), tr = _one("again", end0, [])
    assert list(info["sub_n"][:2]) == [2, 0] and list(info["sub"][:2]) == [95, 0] and list(info["secondary"][:2]) == [-1, 0]
    # two equal scores: position i gets hash_64(id0 + r + i); reads where h(r) > h(r + 1) swap them
    swaps = 0
    for r in range(0, 16, 2):
        bt = PeBatch()
        for _ in range(r // 2):
            bt.add("pad", [], [], mirror=False)
        bt.add("eq", [fwd(1000, 80), fwd(5000, 80, qb=0, qe=40)], [], mirror=False)
        regs, info, pairs, tr = _run(bt, PES_FR)
        swap = sp.hash_64(r) > sp.hash_64(r + 1)
        assert list(info["src"]) == ([1, 0] if swap else [0, 1]) and tr.cnt["remark_reorder"] == int(swap)
        swaps += swap
    assert 0 < swaps < 8


# ---------------------------------------------------------------- CPU: mem_sam_pe's branches
def test_multi_on_either_end_goes_unpaired_but_proper():
    halves = [fwd(1000, 50, qb=0, qe=50), fwd(70000, 45, qb=50, qe=100)]
    for e0, e1 in ((halves, [rev(1500, 90)]), ([fwd(1000, 90)], [rev(1500, 50, qb=0, qe=50), rev(70000, 45, qb=50, qe=100)])):
        p, m, b, _, tr = _one("multi", e0, e1)
        assert tr.cnt["multi"] == 2 and (p["paired"], p["proper"], list(p["z"])) == (0, 1, [0, 0]) == (m["paired"], m["proper"], list(m["z"]))
        assert p["score"] > 0 and p["q_pe"] == 0 and tr.cnt["nopair_proper"] == 2
    # a second primary below T is not multi
    p, m, b, _, tr = _one("multi", [fwd(1000, 50, qb=0, qe=50), fwd(70000, 29, qb=50, qe=100)], [rev(1500, 90)])
    assert tr.cnt["multi"] == 0 and p["paired"] == 1


def test_pair_no_better_than_unpaired():
    # dist 150 under the wide bounds: |ns| = 7, .721 * log(2 erfc(4.95)) = -18.7: q = 171 <= 173 = score_un
    p, m, b, _, tr = _one("un", [fwd(1000, 100)], [rev(1150, 90)], pes=PES_WIDE)
    assert _fields(p) == (1, [0, 0], [60, 60], 0, 171, 0, 0, 0) == _fields(m) and tr.cnt["unpaired_preferred"] == 2


def test_csub_cap_and_frac_rep():
    # csub 95 of 100: the MAPQ rule gives 13, q_pe lifts it to min(60, 53), raw(5) = (int)(30.1 + .499) caps it
    p, m, b, _, tr = _one("csub", [fwd(1000, 100, csub=95)], [rev(1500, 90)])
    assert list(p["mapq"]) == [30, 60] and tr.cnt["csub_cap"] == 2
    # frac_rep .5 on end 0: q_pe = (int)(60 * .75 + .499) = 45; end 0's rule gives 30 -> min(45, 70); end 1 keeps 60
    p, m, b, _, tr = _one("frac", [fwd(1000, 100, frac_rep=0.5)], [rev(1500, 90)])
    assert (p["q_pe"], list(p["mapq"])) == (45, [45, 60]) and tr.cnt["frac_rep_pe"] == 2


def test_no_pairing_without_a_reportable_end_and_empty_lists():
    p, m, b, _, tr = _one("low", [fwd(1000, 25)], [fwd(1500, 90)])
    assert _fields(p) == (0, [-1, 0], [0, 60], 0, 0, 0, 0, 0) == _fields(m)
    p, m, b, _, tr = _one("low2", [fwd(1000, 25)], [fwd(1500, 20)])
    assert (p["paired"], list(p["z"]), list(p["mapq"]), p["proper"]) == (0, [-1, -1], [0, 0], 0) and tr.cnt["nopair_none"] == 4
    for e0, e1, z in (([], [rev(1500, 90)], [-1, 0]), ([fwd(1000, 90)], [], [0, -1]), ([], [], [-1, -1])):
        p, m, b, _, tr = _one("empty", e0, e1)
        assert (p["paired"], list(p["z"]), p["proper"], p["score"]) == (0, z, 0, 0) and tr.cnt["empty_end"] == 2
        assert list(p["mapq"]) == [60 if v == 0 else 0 for v in z] == list(m["mapq"])


# ---------------------------------------------------------------- the sets
def hand_batch():
    b = PeBatch()
    halves = [fwd(1000, 50, qb=0, qe=50), fwd(70000, 45, qb=50, qe=100)]
    b.add("avg", [fwd(1000, 100)], [rev(1500, 90)])
    for d in (299, 300, 700, 701, 150, 0):
        b.add(f"d{d}", [fwd(2000, 100)], [rev(2000 + d, 90)])
    b.add("ff", [fwd(1000, 100)], [fwd(1500, 90)])
    b.add("rr", [fwd(1500, 100)], [fwd(1000, 90)])
    b.add("rf", [fwd(1500, 100)], [rev(1000, 90)])
    b.add("sec", [fwd(60000, 100), fwd(1000, 95)], [rev(1500, 100)])
    b.add("tie", [fwd(1000, 100)], [rev(1480, 90), rev(1520, 90)])
    b.add("again", [fwd(1000, 100, sub=95, sub_n=1), fwd(1300, 95, secondary=0)], [])
    b.add("eq", [fwd(1000, 80), fwd(5000, 80, qb=0, qe=40)], [rev(1500, 80), rev(5500, 80, qb=60, qe=100)])
    b.add("multi0", halves, [rev(1500, 90)])
    b.add("multi1", [fwd(1000, 90)], [rev(1500, 50, qb=0, qe=50), rev(70000, 45, qb=50, qe=100)])
    b.add("notmulti", [fwd(1000, 50, qb=0, qe=50), fwd(70000, 29, qb=50, qe=100)], [rev(1500, 90)])
    b.add("csub", [fwd(1000, 100, csub=95)], [rev(1500, 90)])
    b.add("frac", [fwd(1000, 100, frac_rep=0.5)], [rev(1500, 90, frac_rep=0.25)])
    b.add("low", [fwd(1000, 25)], [fwd(1500, 90)])
    b.add("low2", [fwd(1000, 25)], [fwd(1500, 20)])
    b.add("lowfr", [fwd(1000, 25)], [rev(1500, 20)])          # pairs all the same: q = 45 > 28
    b.add("clamp", [fwd(1000, 5)], [rev(1150, 5)])            # wide bounds: 10 - 18.7 < 0 -> q = 0, o = 0
    b.add("e0", [], [rev(1500, 90)])
    b.add("e1", [fwd(1000, 90)], [])
    b.add("e01", [], [])
    # three candidates of different q and a far one: n_sub < u.n - 1
    b.add("many", [fwd(1000, 100), fwd(1040, 60)], [rev(1500, 90), rev(1330, 70), rev(1690, 50), rev(9000, 40)])
    return b


_hand = {}


def hand_want(scoring=DEFAULT, pes="fr"):
    key = (scoring, pes)
    if key not in _hand:
        b = hand_batch()
        P = dict(fr=PES_FR, wide=PES_WIDE, all=PES_ALL)[pes]
        _hand[key] = (b, P, _run(b, P, scoring))
    return _hand[key]


def fuzz_batch(seed=5):
    """list lengths 0, 1, 2, 16, 17, 46 per end in every combination of two, random overlapping
    regions within [low, high] of one another, and every hit at one place"""
    rng = np.random.default_rng(seed)
    b = PeBatch()

    def end(n, x0, rv, spread=200):
        out = []
        for _ in range(n):
            qb = int(rng.integers(0, 60))
            qe = int(rng.integers(qb + 30, RL + 1))
            x = x0 + int(rng.integers(0, spread + 1))
            out.append((rev if rv else fwd)(x, int(rng.integers(20, qe - qb + 1)), qb=qb, qe=qe,
                                            csub=int(rng.choice([0, 0, 25])), sub_n=int(rng.integers(0, 3))))
        return out

    lens = (0, 1, 2, 16, 17, 46)
    for n0 in lens:
        for n1 in lens:
            b.add(f"f{n0}x{n1}", end(n0, 3000, False), end(n1, 3500, True), mirror=(n0 + n1) % 2 == 0)
    b.add("spot", end(46, 3000, False, 0), end(46, 3500, True, 0))
    b.add("spot0", end(17, 3000, False, 0), end(17, 3000, True, 0))
    return b


_fuzz = {}


def fuzz_want():
    if not _fuzz:
        b = fuzz_batch()
        _fuzz["x"] = (b, _run(b, PES_ALL))
    return _fuzz["x"]


class PeSet:
    """about 1,500 fragments (insert 400-600) from a 300 kb reference with dispersed repeat copies,
    through the oracle front end and regsel_py"""

    def __init__(self):
        import bench
        from test_memchain import _oracle_front, _two_strand
        ref = bench.seeding_reference(300_000, seed=3)
        reads, off, lens = bench.pe_reads(ref, 1500, 150, seed=9)
        self.T = T = _two_strand(ref)
        self.l_pac = len(ref)
        f, mems, cnt, seeds, sr, sc = _oracle_front(ref, reads, off, lens, cap=256)
        self.eopt = bsw.ext_opt(l_pac=len(ref))
        regs, ext = oracle.chain2aln(oracle.make_params(), self.eopt, T, reads, off, lens, seeds, sr, sc)
        self.arr = dict(reads=reads, off=off, lens=lens, seeds=seeds, sr=sr, sc=sc, regs=regs, ext=ext)
        rng = np.random.default_rng(5)
        self.frac_rep = (rng.integers(0, 4, len(lens)) * 0.25 * (rng.random(len(lens)) < 0.2)).astype(np.float32)
        self.csub = (np.arange(len(sr)) % 7 == 0).astype(np.int32) * 30
        self.sopt = sp.sel_opt(l_pac=self.l_pac)
        self.sel = _select(T, self.arr, opt=self.sopt, csub=self.csub, frac_rep=self.frac_rep)
        self.regs, _, self.info, self.first, _ = self.sel
        self.opt = pp.pe_opt(l_pac=self.l_pac)
        self.mat, self.gaps = mat_gaps(DEFAULT)
        self.pes, self.tr_stat, self.isize = pp.pe_stat(self.regs, self.info, self.first, self.opt, 1)
        self.want = pp.pe_pair(self.pes, self.regs, self.info, self.first, self.opt, self.mat, self.gaps)


_set = {}


def pe_set():
    if not _set:
        _set["x"] = PeSet()
    return _set["x"]


def stat_batch():
    """single-region pairs that put chosen insert sizes under each direction: 400 FR, 20 RF, 12 FF
    (below 5% of the largest), 9 RR, one at distance 0, one too far, an empty end, a pair whose
    second hit scores above 0.8 of the first"""
    b = PeBatch()
    rng = np.random.default_rng(3)
    for k in range(400):
        b.add("fr", [fwd(1000 + k, 100)], [rev(1000 + k + 450 + int(rng.integers(0, 100)), 100)], mirror=k % 2 == 0)
    for k in range(20):
        b.add("rf", [fwd(9000 + k, 100)], [rev(9000 + k - Q12[k % 12], 100)], mirror=False)
    for k in range(12):
        b.add("ff", [fwd(1000, 100)], [fwd(1000 + Q12[k], 100)], mirror=False)
    for k in range(9):
        b.add("rr", [fwd(5000, 100)], [fwd(5000 - Q12[k], 100)], mirror=False)
    b.add("zero", [fwd(1000, 100)], [rev(1000, 100)])
    b.add("far", [fwd(1000, 100)], [rev(1000 + 10001, 100)])
    b.add("empty", [fwd(1000, 100)], [])
    b.add("sub", [fwd(1000, 100), fwd(8000, 90)], [rev(1500, 100)])
    b.add("subok", [fwd(1000, 100), fwd(8000, 80)], [rev(1500, 100)])
    return b


def test_statistics_from_pairs():
    regs, info, first = stat_batch().arrays()
    pes, tr, isize = pp.pe_stat(regs, info, first, pp.pe_opt(l_pac=L), 1)
    assert list(pes["n"]) == [12, 602, 20, 9] and list(pes["failed"]) == [1, 0, 1, 1]
    assert (pes[0]["low"], pes[0]["high"]) == (230, 650) and sorted(isize[3]) == Q12[:9]
    assert tr.cnt["stat_is_zero"] == 2 and tr.cnt["stat_far"] == 2 and tr.cnt["stat_empty"] == 2 and tr.cnt["stat_sub_skip"] == 2
    with pytest.raises(ValueError, match="RANGE"):
        pp.pe_stat(regs, info, first[::-1].copy(), pp.pe_opt(l_pac=L), 1)
    with pytest.raises(ValueError, match="INVAL"):
        pp.pe_stat(regs, info, first[:-1], pp.pe_opt(l_pac=L), 1)


def test_pipeline_set():
    p = pe_set()
    regs, info, pairs, tr = p.want
    print("pe set:", dict(tr.cnt), "margin", tr.margin, "stat", dict(p.tr_stat.cnt), p.tr_stat.margin, "pes", p.pes)
    assert len(pairs) == 1500 and p.pes[1]["failed"] == 0 and 450 <= p.pes[1]["avg"] <= 550     # dist = insert - 1
    assert p.pes[1]["n"] > 1000 and tr.cnt["paired"] > 1000 and tr.cnt["general_path"] > 20
    assert tr.margin >= 1e-6 and p.tr_stat.margin >= 1e-6


def _all_branches():
    tot, margin = sp.Counter(), 1.0
    runs = [pe_set().want[3], pe_set().tr_stat, fuzz_want()[1][3]]
    runs += [hand_want(DEFAULT, k)[2][3] for k in ("fr", "wide", "all")]
    regs, info, first = stat_batch().arrays()
    runs.append(pp.pe_stat(regs, info, first, pp.pe_opt(l_pac=L), 1)[1])
    tr = sp.Trace()
    pp.pestat_of(list(range(10, 130, 10)), tr)
    pp.pestat_of([400, 400, 400, 480, 490, 500, 500, 510, 520, 520, 600, 600], tr)
    runs.append(tr)
    for t in runs:
        tot.update(t.cnt)
        margin = min(margin, t.margin)
    return tot, margin


def test_combined_sets_reach_every_branch_with_margin():
    tot, margin = _all_branches()
    print("branches:", {k: tot[k] for k in pp.BRANCHES}, "margin", margin)
    assert all(tot[k] > 0 for k in pp.BRANCHES), {k: tot[k] for k in pp.BRANCHES if tot[k] == 0}
    assert margin >= 1e-6


# ---------------------------------------------------------------- CPU: the header
def test_library_exports_the_pe_header():
    assert declared("bsw_pe.h") == set(bsw.PE_SYMBOLS)
    assert declared("bsw_pe.h") <= exported(), declared("bsw_pe.h") - exported()
    others = set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS)
    assert not set(bsw.PE_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_pe_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_pe.h"\n'
                   f"{sa}(sizeof(bsw_pestat_t) == 32 && offsetof(bsw_pestat_t, n) == 12 && offsetof(bsw_pestat_t, std) == 24, \"pes\");\n"
                   f"{sa}(sizeof(bsw_pe_opt_t) == 48 && offsetof(bsw_pe_opt_t, max_ins) == 16 && offsetof(bsw_pe_opt_t, mask_level) == 44, \"opt\");\n"
                   f"{sa}(sizeof(bsw_pair_t) == 40 && offsetof(bsw_pair_t, mapq) == 12 && offsetof(bsw_pair_t, q_pe) == 36, \"pair\");\n"
                   f"{sa}(sizeof(bsw_pe_stats_t) == 56 && offsetof(bsw_pe_stats_t, n_u) == 40 && offsetof(bsw_pe_stats_t, kernel_ms) == 48, \"stats\");\n"
                   f"{sa}(BSW_PE_API == 1 && BSW_ABI_VERSION == 8 && BSW_PE_MAX_INS == 65536, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.PeOpt) == 48 and bsw.PeOpt.max_ins.offset == 16 and bsw.PeOpt.mask_level.offset == 44
    assert ctypes.sizeof(bsw.PeStats) == 56 and bsw.PeStats.n_u.offset == 40 and bsw.PeStats.kernel_ms.offset == 48
    assert bsw.PESTAT_DTYPE == pp.PESTAT_DTYPE and bsw.PAIR_DTYPE == pp.PAIR_DTYPE
    assert bsw.PAIR_DTYPE.fields["mapq"][1] == 12 and bsw.PAIR_DTYPE.fields["q_pe"][1] == 36
    assert bsw.PESTAT_DTYPE.fields["n"][1] == 12 and bsw.PESTAT_DTYPE.fields["std"][1] == 24


def _lib_calls(ctx, o, pes, n_reads=2, stat=True):
    """the four calls (stat=False: the two pair calls) with placeholder arrays -> their return codes"""
    Lb = bsw.hip_lib()
    regs, info = np.zeros(1, dtype=bsw.ALNREG_DTYPE), np.zeros(1, dtype=bsw.SELINFO_DTYPE)
    first, pairs = np.zeros(n_reads + 1, dtype=np.int32), np.zeros(max(n_reads // 2, 1), dtype=bsw.PAIR_DTYPE)
    out = np.zeros(4, dtype=bsw.PESTAT_DTYPE)
    P, B = bsw._ptr, ctypes.byref
    rc = ()
    if stat:
        rc = (Lb.bsw_pe_stat(ctx, B(o), P(regs), P(info), P(first), n_reads, P(out)),
              Lb.bsw_pe_stat_resident(ctx, B(o), P(regs), P(info), P(first), n_reads, 0, P(out), None))
    return rc + (Lb.bsw_pe_pair(ctx, B(o), P(pes), P(regs), P(info), P(first), n_reads, P(pairs)),
                 Lb.bsw_pe_pair_resident(ctx, B(o), P(pes), P(regs), P(info), P(first), n_reads, 0, P(pairs), None))


def test_defaults_and_invalid_arguments_need_no_device():
    o = bsw.pe_opt()
    got = {f: getattr(o, f) for f, _ in o._fields_}
    assert {k: (round(v, 6) if isinstance(v, float) else v) for k, v in got.items()} == pp.DEFAULT_OPT
    Lb = bsw.hip_lib()
    assert Lb.bsw_pe_last_stats(None, None) == -22
    # a context that is never dereferenced: every argument check comes before the first use of it
    fake = ctypes.c_void_p(1)
    good = PES_FR.copy()
    for kw in (dict(l_pac=0), dict(l_pac=L, id0=3), dict(l_pac=L, max_ins=0), dict(l_pac=L, max_ins=bsw.PE_MAX_INS + 1)):
        assert _lib_calls(fake, bsw.pe_opt(**kw), good) == (-22,) * 4, kw
    assert _lib_calls(fake, bsw.pe_opt(l_pac=L), good, n_reads=3) == (-22,) * 4
    for std in (0.0, -1.0, float("nan"), float("inf")):
        bad = good.copy()
        bad[1]["std"] = std
        assert _lib_calls(fake, bsw.pe_opt(l_pac=L), bad, stat=False) == (-22, -22), std
    assert _lib_calls(None, bsw.pe_opt(l_pac=L), good) == (-22,) * 4


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_gpu_statistics_match_the_restatement():
    eng = bsw.Engine()
    regs, info, first = stat_batch().arrays()
    want, tr, _ = pp.pe_stat(regs, info, first, pp.pe_opt(l_pac=L), 1)
    same_pes(want, bsw.pe_stat(eng, regs, info, first, bsw.pe_opt(l_pac=L)), "hand-built")
    st = bsw.pe_last_stats(eng)
    assert list(st.n_cand) == list(want["n"]) and st.n_pairs == len(first) // 2 and st.kernel_ms > 0
    p = pe_set()
    same_pes(p.pes, bsw.pe_stat(eng, p.regs, p.info, p.first, bsw.pe_opt(l_pac=p.l_pac)), "pipeline set")
    b = ResidentBatch(eng, p.arr["reads"], p.arr["off"], p.arr["lens"])
    b.put(sreg=p.regs, sinfo=p.info, sfirst=p.first)
    got = b.pe_stat(bsw.pe_opt(l_pac=p.l_pac))
    same_pes(p.pes, got, "pipeline set, resident")
    for mi in (300, 520):                                   # a max_ins inside the data
        o = pp.pe_opt(l_pac=p.l_pac, max_ins=mi)
        same_pes(pp.pe_stat(p.regs, p.info, p.first, o, 1)[0],
                  bsw.pe_stat(eng, p.regs, p.info, p.first, bsw.pe_opt(l_pac=p.l_pac, max_ins=mi)), f"max_ins {mi}")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", SCORINGS)
def test_gpu_hand_built_pairs(scoring):
    eng = engine_of(scoring)
    for which in ("fr", "wide", "all"):
        b, P, want = hand_want(scoring, which)
        regs, info, first = b.arrays(scoring[0])
        got = bsw.pe_pair(eng, P, regs, info, first, bsw.pe_opt(l_pac=L, b=scoring[1]))
        same_pair(want, got, f"hand-built {scoring} {which}", bsw.pe_last_stats(eng))
    if scoring == DEFAULT:
        b = hand_batch()
        regs, info, first = b.arrays()
        mat, gaps = mat_gaps(DEFAULT)
        for kw in (dict(id0=1 << 40), dict(T=60, pen_unpaired=5), dict(mapQ_coef_len=0), dict(mask_level=0.9)):
            want = pp.pe_pair(PES_ALL, regs, info, first, pp.pe_opt(l_pac=L, **kw), mat, gaps)
            same_pair(want, bsw.pe_pair(eng, PES_ALL, regs, info, first, bsw.pe_opt(l_pac=L, **kw)), f"hand-built {kw}",
                       bsw.pe_last_stats(eng))
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_host_arrays_and_end_to_end():
    p = pe_set()
    eng = bsw.Engine()
    o = bsw.pe_opt(l_pac=p.l_pac)
    same_pair(p.want, bsw.pe_pair(eng, p.pes, p.regs, p.info, p.first, o), "pipeline set", bsw.pe_last_stats(eng))
    pes = bsw.pe_stat(eng, p.regs, p.info, p.first, o)      # the GPU's statistics into the GPU's pairing
    want = pp.pe_pair(pes, p.regs, p.info, p.first, p.opt, p.mat, p.gaps)
    same_pair(want, bsw.pe_pair(eng, pes, p.regs, p.info, p.first, o), "end to end", bsw.pe_last_stats(eng))
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_device_to_device():
    """bsw_regs_select_resident's buffers -> bsw_pe_stat_resident -> bsw_pe_pair_resident ->
    bsw_reg2aln_resident"""
    p = pe_set()
    a = p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"])
    b.put(seeds=a["seeds"], sr=a["sr"], sc=a["sc"])
    b.chain2aln(p.eopt)
    k = b.select(bsw.sel_opt(l_pac=p.l_pac), csub=p.csub, frac_rep=p.frac_rep)
    assert k == len(p.regs)
    o = bsw.pe_opt(l_pac=p.l_pac)
    pes = b.pe_stat(o)
    same_pes(p.pes, pes, "device to device")
    b.pe_pair(pes, o)
    st = bsw.pe_last_stats(eng)
    same_pair(p.want, got_pair(b), "device to device", st)
    assert np.array_equal(b.get("sread"), p.sel[1])          # d_sel_read stays valid
    b.reg2aln(p.eopt)
    aln = got_aln(b)
    sel = np.zeros(k, dtype=bsw.ALNREG_DTYPE)
    for f in sp.ALNREG_FIELDS:
        sel[f] = p.want[0][f]
    same_aln(rp.reg2aln(p.T, p.l_pac, a["reads"], a["off"], a["lens"], sel, p.sel[1], p.mat, p.gaps, p.eopt.w), aln,
             "alignments of the paired regions")
    eng.close()


@pytest.mark.gpu
def test_gpu_batch_sizes():
    p = pe_set()
    eng = bsw.Engine()
    wr, wi, wp, tr = p.want
    o = bsw.pe_opt(l_pac=p.l_pac)
    for npairs in (0, 1, 63, 64, 65, 257):
        k = p.first[2 * npairs]
        f = p.first[:2 * npairs + 1]
        got = bsw.pe_pair(eng, p.pes, p.regs[:k], p.info[:k], f, o)
        same_pair((wr[:k], wi[:k], wp[:npairs], tr), got, f"{npairs} pairs")
        assert bsw.pe_last_stats(eng).n_pairs == npairs
        want = pp.pe_stat(p.regs[:k], p.info[:k], f, p.opt, 1)[0]
        same_pes(want, bsw.pe_stat(eng, p.regs[:k], p.info[:k], f, o), f"{npairs} pairs")
    eng.close()


@pytest.mark.gpu
def test_gpu_list_lengths():
    b, want = fuzz_want()
    c = want[3].cnt
    assert c["n_u"] > 4000 and c["u_many"] > 20 and c["general_path"] > 30 and want[3].margin >= 1e-6, (c, want[3].margin)
    eng = bsw.Engine()
    regs, info, first = b.arrays()
    same_pair(want, bsw.pe_pair(eng, PES_ALL, regs, info, first, bsw.pe_opt(l_pac=L)), "list lengths", bsw.pe_last_stats(eng))
    sw = pp.pe_stat(regs, info, first, pp.pe_opt(l_pac=L), 1)[0]
    same_pes(sw, bsw.pe_stat(eng, regs, info, first, bsw.pe_opt(l_pac=L)), "list lengths")
    eng.close()


@pytest.mark.gpu
def test_gpu_errors_and_recovery():
    b, P, want = hand_want()
    regs, info, first = b.arrays()
    o = bsw.pe_opt(l_pac=L)
    eng = bsw.Engine()
    for kw in (dict(l_pac=0), dict(l_pac=L, id0=1), dict(l_pac=L, max_ins=0), dict(l_pac=L, max_ins=bsw.PE_MAX_INS + 1)):
        with pytest.raises(bsw.BswError, match="-22"):
            bsw.pe_pair(eng, P, regs, info, first, bsw.pe_opt(**kw))
        with pytest.raises(bsw.BswError, match="-22"):
            bsw.pe_stat(eng, regs, info, first, bsw.pe_opt(**kw))
    with pytest.raises(bsw.BswError, match="-22"):            # an odd number of reads
        bsw.pe_pair(eng, P, regs[:first[-2]], info[:first[-2]], first[:-1], o)
    bad = P.copy()
    bad[1]["std"] = 0.0
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.pe_pair(eng, bad, regs, info, first, o)
    bsw.set_reference(eng, np.zeros(2 * L - 2, np.uint8))     # a resident text that does not fit l_pac
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.pe_pair(eng, P, regs, info, first, o)
    bsw.set_reference(eng, np.zeros(2 * L, np.uint8))
    for field, v in (("rb", -1), ("rb", 2 * L)):
        r2 = regs.copy()
        r2[0][field] = v
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.pe_pair(eng, P, r2, info, first, o)
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.pe_stat(eng, r2, info, first, o)
    r2 = regs.copy()
    r2[int(first[b.names.index("many") * 2]) + 1]["rb"] = 2 * L + 5          # inside a general-path pair
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.pe_pair(eng, P, r2, info, first, o)
    dec = first.copy()
    dec[3] = dec[2] - 1
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.pe_pair(eng, P, regs, info, dec, o)
    d = [hiprt.DeviceBuffer.from_array(np.ascontiguousarray(x)) for x in (regs, info, dec)]
    d_pairs = hiprt.DeviceBuffer((len(first) // 2) * bsw.PAIR_DTYPE.itemsize)
    with pytest.raises(bsw.BswError, match="-34"):            # the device's own check of the offsets
        bsw.pe_pair_resident(eng, P, d[0].ptr, d[1].ptr, d[2].ptr, len(first) - 1, len(regs), d_pairs.ptr, o)
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.pe_stat_resident(eng, d[0].ptr, d[1].ptr, d[2].ptr, len(first) - 1, len(regs), o)
    d_first = hiprt.DeviceBuffer.from_array(first)
    with pytest.raises(bsw.BswError, match="-34"):            # offsets past n_regs
        bsw.pe_pair_resident(eng, P, d[0].ptr, d[1].ptr, d_first.ptr, len(first) - 1, len(regs) - 1, d_pairs.ptr, o)
    same_pair(want, bsw.pe_pair(eng, P, regs, info, first, o), "after the errors", bsw.pe_last_stats(eng))
    eng.close()
    eng = bsw.Engine()                                        # fresh slots: the first growth is this call's
    try:
        eng.set_option("test_fail_alloc", 1)
        with pytest.raises(bsw.BswError, match="-12"):
            bsw.pe_pair(eng, P, regs, info, first, o)
        eng.set_option("test_fail_alloc", 1)
        with pytest.raises(bsw.BswError, match="-12"):
            bsw.pe_stat(eng, regs, info, first, o)
    finally:
        eng.set_option("test_fail_alloc", 0)
    same_pair(want, bsw.pe_pair(eng, P, regs, info, first, o), "after a failed growth", bsw.pe_last_stats(eng))
    eng.close()
