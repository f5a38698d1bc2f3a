"""Mate rescue (include/bsw_matesw.h): mem_matesw and the rescue block of mem_sam_pe between
bsw_pe_stat* and bsw_pe_pair*.

CPU: hand-built pairs on a small random text with known answers through the Python restatement
(tests/matesw_py.py), each also mirrored onto the other strand; a pipeline set of paired reads with
unseedable mates through the oracle front end, regsel_py, pe_py and reg2aln_py; the conditions the
GPU comparison rests on (every branch reached, the jobs of both ksw_align2 formulations agree); the
header's symbols and layouts.
GPU: bsw_matesw* == the restatement in every output field and counter, n_jobs and rounds included.
Parity is unpinned by the reference tree (it holds no source of these functions; bsw_matesw.h
restates them).
"""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bsw
import hiprt
import ksw_align_py as kp
import matesw_py as mp
import oracle
import pe_py as pp
import reg2aln_py as rp
import regsel_py as sp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import (DEFAULT, SCORINGS, declared, engine_of, exported, fetch, got_aln, got_pair, mat_gaps, revcomp,
                      same_aln, same_msw, same_pair, same_pes)
from test_pe import _pes
from test_regsel import _select

L = 30_000                                                   # l_pac of the hand text
RL = 100
_rng = np.random.default_rng(11)
REF = _rng.integers(0, 4, L).astype(np.uint8)
T = np.concatenate([REF, 3 - REF[::-1]]).astype(np.uint8)

PES_FR = _pes(FR=(300, 700, 500.0, 50.0))
PES_ALL = _pes(FF=(300, 700, 500.0, 50.0), FR=(300, 700, 500.0, 50.0), RF=(300, 700, 500.0, 50.0),
               RR=(300, 700, 500.0, 50.0))


def reg(rb, score, qb=0, qe=RL, re=None, **info):
    return dict(rb=rb, re=rb + (qe - qb) if re is None else re, qb=qb, qe=qe, score=score, **info)


def rev_at(s, n=RL):
    """the read of the reverse strand that covers forward [s, s + n), and its rb"""
    return revcomp(REF[s:s + n]), 2 * L - (s + n)


def mutate(read, every=16, start=8):
    r = np.array(read, dtype=np.uint8)
    r[start::every] = (r[start::every] + 1) % 4
    return r


def rnd(n=RL, seed=1):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


T_MIRROR = np.roll(T, L)                                     # revcomp(REF) + REF: the other strand first


def _shift(g):
    """the other-strand mirror, as test_pe._shift: rb -> (rb + l_pac) mod 2 l_pac.  Against T_MIRROR the same
    reads align there, so a pair keeps its orientation and its distance"""
    rb = (g["rb"] + L) % (2 * L)
    return dict(g, rb=rb, re=rb + g["re"] - g["rb"])


class MsBatch:
    """pairs of reads with their lists"""

    def __init__(self):
        self.names, self.reads, self.ends = [], [], []

    def add(self, name, read0, end0, read1, end1):
        self.names.append(name)
        self.reads += [np.asarray(read0, np.uint8), np.asarray(read1, np.uint8)]
        self.ends += [list(end0), list(end1)]

    def mirrored(self):
        """the same pairs on the other strand: to be run against T_MIRROR"""
        m = MsBatch()
        m.names, m.reads = list(self.names), list(self.reads)
        m.ends = [[_shift(g) for g in e] for e in self.ends]
        return m

    def arrays(self, scale=1):
        """-> (reads, off, lens, sel_regs, sel_info, read_first); scores in units of a"""
        lens = np.array([len(r) for r in self.reads], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
        reads = np.concatenate(self.reads).astype(np.uint8) if self.reads else np.zeros(0, np.uint8)
        n = sum(len(e) for e in self.ends)
        regs, info = np.zeros(n, dtype=bsw.ALNREG_DTYPE), np.zeros(n, dtype=bsw.SELINFO_DTYPE)
        first, k = [0], 0
        for e in self.ends:
            for g in e:
                regs[k] = (g["rb"], g["re"], g["qb"], g["qe"], g["score"] * scale, g["score"] * scale, 100, 19)
                info[k] = (g.get("seedcov", g["qe"] - g["qb"]), g.get("sub", 0) * scale, g.get("csub", 0) * scale,
                           g.get("sub_n", 0), 1, g.get("secondary", -1), g.get("mapq", 0), k, g.get("frac_rep", 0.0))
                k += 1
            first.append(k)
        return reads, off, lens, regs, info, np.array(first, dtype=np.int32)


def _run(batch, pes, scoring=DEFAULT, ksw=kp.ksw_align2, jobs=None, text=T, **optkw):
    mat, gaps = mat_gaps(scoring)
    reads, off, lens, regs, info, first = batch.arrays(scoring[0])
    return mp.mate_rescue(pes, text, reads, off, lens, regs, info, first, mp.matesw_opt(l_pac=L, **optkw), mat, gaps,
                          ksw, jobs=jobs)


def _one(read0, end0, read1, end1, pes=PES_FR, **kw):
    b = MsBatch()
    b.add("x", read0, end0, read1, end1)
    regs, rd, info, first, tr = _run(b, pes, **kw)
    return regs, info, first, tr


A0 = 1000                                                    # the anchor of most cases: T[1000, 1100) forward
ANCHOR = [reg(A0, 100)]
# every candidate of either end has a hit of the other at distance 500: equal scores in an order the dedup
# would change (rb descending), a third region below the candidate threshold
CONS = ([reg(9000, 80, sub_n=2, mapq=7), reg(A0, 80), reg(15000, 60, secondary=0)],
        [reg(2 * L - 1501, 90), reg(2 * L - 9501, 90, csub=30), reg(20000, 70, secondary=1)])


def _fields(g):
    return tuple(int(g[f]) for f in ("rb", "re", "qb", "qe", "score"))


# ---------------------------------------------------------------- CPU: rescue by pencil
def test_basic_fr_rescue():
    # FR, dist = p2 - b1 with p2 = 2L - 1 - rb: the mate at the mean distance 500 covers forward [1401, 1501).
    # r = 1: is_rev, is_larger: window [1000 + 300 - 100, 1000 + 700) = [1200, 1700), query = revcomp(mate) =
    # forward [1401, 1501) with the 6 substitutions of mate positions 8, 24, .. 88 at 91, 75, .. 11: 11 matches
    # before the first and 8 after the last keep both ends (11 - 4 > 0, 8 - 4 > 0): score 94 - 24 = 70,
    # tb = 201, te = 300, qb = 0, qe = 99 -> rb = 2L - 1501, re = 2L - 1401, [qb, qe) = [0, 100)
    mate, rb = rev_at(1401)
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, mutate(mate), [])
    assert list(first) == [0, 1, 2] and _fields(regs[1]) == (rb, rb + 100, 0, 100, 70) and rb == 2 * L - 1501
    # csub = score2, the best row maximum >= 19 outside te -+ 70 rows: chance similarity in a 500-base window
    # (the C oracle on the same job says which)
    mat, gaps = mat_gaps(DEFAULT)
    q = [int(c) for c in REF[1401:1501]]
    for k in (11, 27, 43, 59, 75, 91):
        q[k] = 3 - ((3 - q[k] + 1) % 4)
    want = oracle.ksw_align2(q, T[1200:1700], mat, *gaps, mp.KSW_XSUBO | mp.KSW_XSTART | mp.KSW_XBYTE | 19)
    assert want[:3] == [70, 300, 99] and want[5:] == [201, 0] and -1 <= want[3] < 40
    assert (info[1]["csub"], info[1]["seedcov"], info[1]["secondary"], info[1]["src"]) == (want[3], 50, -1, -1)
    assert all(info[1][f] == 0 for f in ("sub", "sub_n", "n_comp", "mapq", "frac_rep")) and regs[1]["truesc"] == 0
    assert _fields(regs[0]) == (A0, A0 + RL, 0, RL, 100)
    # the call of end 1 (anchor = nothing: its list was empty before any rescue) does not exist; end 0's one
    # call ran one job (FR alone is live), u8 (100 * 1 < 250)
    c = tr.cnt
    assert (c["calls"], c["jobs"], c["jobs_u8"], c["pushed"], c["job_rev"], tr.rounds) == (1, 1, 1, 1, 1, 1)


def test_rescue_with_clipped_ends_and_a_deletion():
    # 10 random bases at either end of the mate: the local alignment keeps mate [10, 90): qb = 10, qe = 90
    mate, rb = rev_at(1401)
    m = np.array(mate)
    m[:10], m[90:] = (m[:10] + 2) % 4, (m[90:] + 2) % 4                     # every base wrong: nothing to extend
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, m, [])
    assert _fields(regs[1]) == (rb + 10, rb + 90, 10, 90, 80) and info[1]["seedcov"] == 40
    # a 3-base deletion in the read (forward [1451, 1454) missing): 50 + 50 matches, gap 6 + 3 = 9: 91 >
    # either half alone; the reference span is 103
    s = 1401
    m = revcomp(np.concatenate([REF[s:s + 50], REF[s + 53:s + 103]]))
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, m, [])
    rb = 2 * L - (s + 103)
    assert _fields(regs[1]) == (rb, rb + 103, 0, 100, 91) and info[1]["seedcov"] == 50


def test_consistent_hit_runs_no_job_and_returns_the_lists_as_they_were():
    mate, rb = rev_at(1401)
    b = MsBatch()
    b.add("cons", REF[A0:A0 + RL], CONS[0], mutate(mate), CONS[1])
    want = b.arrays()
    regs, rd, info, first, tr = _run(b, PES_FR)
    assert tr.cnt["jobs"] == 0 and tr.rounds == 0 and tr.cnt["all_skipped"] == tr.cnt["calls"] > 0
    assert regs.tobytes() == want[3].astype(regs.dtype).tobytes() and info.tobytes() == want[4].tobytes()
    assert np.array_equal(first, want[5]) and tr.cnt["lists_changed"] == 0


def test_all_four_directions_live_insertion_order_and_dedup_after_each():
    # no hit on the mate: FF, FR, RF, RR all run in one call.  The mate's list holds two far-away hits of the
    # rescued score 70 (hash order: the larger rb first): the rescued one lands after them, then the dedup's
    # score sort puts the three in (rb, qb) order
    mate, rb = rev_at(1401)
    e1 = [reg(25000, 70), reg(22000, 70)]
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, mutate(mate), e1, pes=PES_ALL)
    c = tr.cnt
    # call 0 (anchor of end 0): 4 jobs; r = 0 finds nothing, yet the dedup runs and reorders; r = 1 pushes after
    # the ties.  Then end 1's three candidates (copied before: the two of 70) call into end 0's list
    assert c["jobs"] >= 4 and c["push_tie"] == 1 and c["dedup_run"] >= 4 and c["aln_low"] >= 3
    got = [_fields(regs[k]) for k in range(first[1], first[2])]
    assert [g[0] for g in got] == [22000, 25000, rb] and got[2][4] == 70
    assert c["job_fwd"] > 0 and c["job_rev"] > 0


def test_random_mate_pushes_nothing_yet_the_dedup_reorders():
    e1 = [reg(25000, 60), reg(22000, 60)]
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, rnd(seed=3), e1)
    c = tr.cnt
    assert c["jobs"] >= 1 and c["pushed"] == 0 and c["aln_low"] == c["jobs"] and c["dedup_run"] >= 1
    assert [int(regs[k]["rb"]) for k in range(first[1], first[2])] == [22000, 25000] and c["lists_changed"] >= 1
    assert list(info["src"][first[1]:first[2]]) == [2, 1]                   # the info fields travel along


def test_windows():
    rd = rnd(seed=4)
    # RF (r = 2: is_rev, not larger): [a - 700 - 100, a - 300): a = 310 leaves [0, 10), shorter than 19;
    # a = 250 leaves re = -50 <= rb = 0
    for a, key in ((310, "short_window"), (250, "empty_window")):
        regs, info, first, tr = _one(T[a:a + RL], [reg(a, 100)], rd, [], pes=_pes(RF=(300, 700, 500.0, 50.0)))
        assert tr.cnt[key] == 1 and tr.cnt["jobs"] == 0 and tr.cnt["clamp0"] == 1 and tr.cnt["call_no_job"] == 1
    # FF (r = 0): [a + 300, a + 800).  a = 2L - 500 clamps at 2L; a = L - 500: [L - 200, L + 300), mid = L + 50:
    # cut to [L, L + 300); a = L - 600: [L - 300, L + 200), mid = L - 50: cut to [L - 300, L)
    ff = _pes(FF=(300, 700, 500.0, 50.0))
    for a, key in ((2 * L - 500, "clamp_end"), (L - 500, "cut_right"), (L - 600, "cut_left")):
        jobs = []
        b = MsBatch()
        b.add("w", T[a:a + RL], [reg(a, 100)], rd, [])
        tr = _run(b, ff, jobs=jobs)[4]
        assert tr.cnt[key] == 1 and tr.cnt["jobs"] == 1 and len(jobs[0][1]) == {"clamp_end": 200, "cut_right": 300, "cut_left": 300}[key]
        lo = {"clamp_end": 2 * L - 200, "cut_right": L, "cut_left": L - 300}[key]
        assert jobs[0][1] == [int(c) for c in T[lo:lo + len(jobs[0][1])]]


def test_min_seed_len_quirk_and_byte_switch():
    # a = 2: the threshold in xtra is 38 but the push test is score >= 19: a hit of 15 matching bases (the
    # rest of the mate is N, -1 against anything) scores 30: ksw_align2 skips the reverse pass (30 < 38), qb
    # stays -1 and nothing is pushed
    sc = SCORINGS[2]
    assert sc[0] == 2
    mate = np.array(rev_at(1401)[0])
    mate[:40], mate[55:] = 4, 4
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, mate, [], scoring=sc)
    assert tr.cnt["aln_noqb"] == 1 and tr.cnt["pushed"] == 0 and tr.cnt["aln_low"] == 0
    # l_ms * a < 250: 124 bases at a = 2 are bytes, 125 are not
    for n, key in ((124, "jobs_u8"), (125, "jobs_i16")):
        m, rb = rev_at(1401, n)
        tr = _one(REF[A0:A0 + RL], ANCHOR, mutate(m), [], scoring=sc)[3]
        assert tr.cnt[key] == 1 and tr.cnt["jobs"] == 1 and tr.cnt["pushed"] == 1


def test_redundant_and_identical():
    # the mate's own hit lies 3 past `high` (dist 703: forward [1604, 1704)); the window ends at 1700, so the
    # rescue finds its first 96 bases: 96 of 96 overlap the listed hit -> redundant, the lower score goes.
    # Phase e = 1 mirrors it: the listed hit as anchor finds 96 bases of read 0 beside read 0's own hit
    mate, rb = rev_at(A0 + 604)
    for listed, kept in ((100, 100), (50, 96)):
        regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, mate, [reg(rb, listed)])
        assert tr.cnt["pushed"] == 2 and tr.cnt["drop_p"] + tr.cnt["drop_q"] == 2 and list(first) == [0, 1, 2]
        assert regs[1]["score"] == kept and (regs[1]["qb"], regs[1]["qe"]) == ((0, 100) if kept == 100 else (4, 100))
        assert _fields(regs[0]) == (A0, A0 + RL, 0, RL, 100)
    # identical (score, rb, qb) is always redundant below mask_level_redun = 1; at 1.0 the redundancy test
    # (strictly greater) fails and the identical rule drops the second.  A listed hit 3 short of `low` (dist
    # 297: forward [1198, 1298)): the window starts at 1200 and the rescue finds forward [1200, 1298): the
    # same rb = 2L - 1298, qb = 0, score 98 as the listed [0, 98)
    mate, rb = rev_at(A0 + 198)
    regs, info, first, tr = _one(REF[A0:A0 + RL], ANCHOR, mate, [reg(rb, 98, qb=0, qe=98)], mask_level_redun=1.0)
    assert tr.cnt["identical"] >= 1 and first[2] - first[1] == 1 and _fields(regs[first[1]]) == (rb, rb + 98, 0, 98, 98)


def test_candidate_selection():
    mate = mutate(rev_at(1401)[0])
    for second, calls in ((83, 2), (82, 1)):                 # 100 - 17 = 83 is a candidate, 82 is not
        tr = _one(REF[A0:A0 + RL], [reg(A0, 100), reg(12000, second)], rnd(seed=5), [])[3]
        assert tr.cnt["calls"] == calls and tr.cnt["cand_below"] == 2 - calls
    e0 = [reg(A0, 100), reg(12000, 95), reg(14000, 90)]
    tr = _one(REF[A0:A0 + RL], e0, rnd(seed=5), [], max_matesw=2)[3]
    assert tr.cnt["calls"] == 2 and tr.cnt["cand_cut"] == 1
    regs, info, first, tr = _one(REF[A0:A0 + RL], e0, mate, [], max_matesw=0)
    assert tr.cnt["calls"] == 0 and list(first) == [0, 3, 3]


def _stale():
    # anchors A0 and A1 = A0 + 5.  The mate list: X (score 60, dist 704 from A0 = 699 from A1: in range of A1
    # only) and Y (score 70, 3 bases on: 707 and 702, in range of neither), overlapping 97 of 100.  The mate is random: call 0
    # runs a job, pushes nothing, and its dedup drops X (redundant, lower).  Call 1, which the original lists
    # would have skipped, must run a job
    a1 = A0 + 5
    x = 2 * L - 1 - (A0 + 704)
    e1 = [reg(x - 3, 70), reg(x, 60)]
    return REF[A0:A0 + RL], [reg(A0, 100), reg(a1, 100)], rnd(seed=6), e1


def test_stale_plan_and_vanished_anchor():
    regs, info, first, tr = _one(*_stale())
    c = tr.cnt
    assert c["replan"] >= 1 and c["jobs"] >= 2 and c["drop_p"] + c["drop_q"] >= 1
    # phase e = 1's anchor X was dropped from its own list by phase e = 0 and is still used
    assert c["anchor_gone"] >= 1


# ---------------------------------------------------------------- the sets
GROUPS = ("fr", "all", "rf", "m2", "m0", "mlr1")


def hand_batch(group):
    """-> (batch, pes, optkw)"""
    b = MsBatch()
    rd0 = REF[A0:A0 + RL]
    mate, rb = rev_at(1401)
    if group == "fr":
        b.add("basic", rd0, ANCHOR, mutate(mate), [])
        m = np.array(mate)
        m[:10], m[90:] = (m[:10] + 2) % 4, (m[90:] + 2) % 4
        b.add("clip", rd0, ANCHOR, m, [])
        b.add("del3", rd0, ANCHOR, revcomp(np.concatenate([REF[1401:1451], REF[1454:1504]])), [])
        b.add("cons", rd0, CONS[0], mutate(mate), CONS[1])
        b.add("random", rd0, ANCHOR, rnd(seed=3), [reg(25000, 60), reg(22000, 60)])
        far, frb = rev_at(A0 + 604)
        b.add("redun_hi", rd0, ANCHOR, far, [reg(frb, 100)])
        b.add("redun_lo", rd0, ANCHOR, far, [reg(frb, 50, frac_rep=0.25, csub=20)])
        near, nrb = rev_at(A0 + 198)                         # 3 short of `low`: the rescued hit ends first, q is dropped
        b.add("redun_q", rd0, ANCHOR, near, [reg(nrb, 100)])
        nm = np.array(mate)                                  # the a = 2 quirk: 15 bases among N
        nm[:40], nm[55:] = 4, 4
        b.add("quirk", rd0, ANCHOR, nm, [])
        b.add("thr83", rd0, [reg(A0, 100), reg(12000, 83)], rnd(seed=5), [])
        b.add("thr82", rd0, [reg(A0, 100), reg(12000, 82)], rnd(seed=5), [])
        b.add("stale", *_stale())
        b.add("empty", rd0, [], mutate(mate), [])
        b.add("both", rd0, ANCHOR, mutate(mate), [reg(20000, 40)])
        b.add("long", REF[A0:A0 + 151], [reg(A0, 151, qe=151)], mutate(rev_at(1351, 151)[0]), [])
        return b, PES_FR, {}
    if group == "all":
        b.add("four", rd0, ANCHOR, mutate(mate), [reg(25000, 70), reg(22000, 70)])
        rd = rnd(seed=4)
        for a in (2 * L - 500, L - 500, L - 600, 310, 250):
            b.add(f"w{a}", T[a:a + RL], [reg(a, 100)], rd, [])
        b.add("stale", *_stale())
        return b, PES_ALL, {}
    if group == "rf":
        rd = rnd(seed=4)
        for a in (310, 250):
            b.add(f"w{a}", T[a:a + RL], [reg(a, 100)], rd, [])
        return b, _pes(RF=(300, 700, 500.0, 50.0)), {}
    e0 = [reg(A0, 100), reg(12000, 95), reg(14000, 90)]
    if group == "m2":
        b.add("m2", rd0, e0, rnd(seed=5), [])
        return b, PES_FR, dict(max_matesw=2)
    if group == "m0":
        b.add("m0", rd0, e0, mutate(mate), [])
        return b, PES_FR, dict(max_matesw=0)
    near, nrb = rev_at(A0 + 198)
    b.add("ident", rd0, ANCHOR, near, [reg(nrb, 98, qb=0, qe=98)])
    return b, PES_FR, dict(mask_level_redun=1.0)


_hand = {}


def hand_want(group, scoring=DEFAULT, mirror=False):
    """-> (batch, pes, optkw, the restatement's answer, its jobs, the text)"""
    key = (group, scoring, mirror)
    if key not in _hand:
        b, pes, kw = hand_batch(group)
        b, text = (b.mirrored(), T_MIRROR) if mirror else (b, T)
        jobs = []
        _hand[key] = (b, pes, kw, _run(b, pes, scoring, jobs=jobs, text=text, **kw), jobs, text)
    return _hand[key]


def test_mirrored_hand_set_gives_the_mirrored_answers():
    for g in GROUPS:
        w, m = hand_want(g)[3], hand_want(g, mirror=True)[3]
        assert np.array_equal(w[3], m[3]), g                 # (within a read the (rb, qb) sort may order them otherwise)
        for r in range(len(w[3]) - 1):
            got = [sorted(((int(x["rb"]) + sh) % (2 * L), int(x["qb"]), int(x["qe"]), int(x["score"]))
                          for x in v[0][v[3][r]:v[3][r + 1]]) for v, sh in ((w, L), (m, 0))]
            assert got[0] == got[1], (g, r)
        if g not in ("all", "rf"):                           # (their window cases sit at the text's own ends)
            assert mp.stats_of(w[4], 0, 0) == mp.stats_of(m[4], 0, 0), g


def long_lists(seed=7):
    """lists of 0, 1, 2, 17 and 46 regions per end, every one a candidate, every direction live and no
    consistent hit (the ends are 5,000 apart): 4 jobs per call.  pes with high - low = 3 keeps the windows
    at about the read length"""
    rng = np.random.default_rng(seed)
    b = MsBatch()
    lens = (0, 1, 2, 17, 46)
    for k, n0 in enumerate(lens):
        n1 = lens[(k + 2) % len(lens)]
        x0 = 3000 + 2000 * k
        # odd k: the mate read lies 45 past the first anchor, so nearly every call of end 0 finds it again:
        # pushed, then dropped by the dedup (the list grows into its room and shrinks back); even k: random
        rd0, rd1 = REF[x0:x0 + 60], (REF[x0 + 45:x0 + 105] if k % 2 else rnd(60, seed=20 + k))
        e0 = [reg(x0 + 3 * j, 55 + int(rng.integers(0, 3)), qe=60) for j in range(n0)]
        e1 = [reg(x0 + 5000 + 70 * j, 50 + int(rng.integers(0, 10)), qe=60) for j in range(n1)]
        b.add(f"l{n0}x{n1}", rd0, e0, rd1, e1)
    pes = _pes(FF=(40, 43, 41.0, 1.0), FR=(40, 43, 41.0, 1.0), RF=(40, 43, 41.0, 1.0), RR=(40, 43, 41.0, 1.0))
    return b, pes


_long = {}


def long_want():
    if not _long:
        b, pes = long_lists()
        _long["x"] = (b, pes, _run(b, pes, ksw=oracle.ksw_align2))
    return _long["x"]


def test_both_ksw_formulations_agree_on_every_hand_job():
    n = 0
    for g in GROUPS:
        for sc, mir in ((DEFAULT, False), (SCORINGS[2], True)):
            b, pes, kw, want, jobs, text = hand_want(g, sc, mir)
            mat, gaps = mat_gaps(sc)
            for q, t, xtra in jobs:
                assert kp.ksw_align2(q, t, mat, *gaps, xtra) == oracle.ksw_align2(q, t, mat, *gaps, xtra)
                n += 1
    assert n > 60


class MsSet:
    """about 1,500 fragments (insert 400-600, 150 bp) from a 300 kb reference; 30% of the mates made
    unseedable (a substitution every 13 to 16 bases: no exact 19-mer), 5% of those with a 2-4 base indel
    besides, 5% of them random sequence; through the oracle front end, regsel_py, pe_py, matesw_py, pe_py
    and reg2aln_py"""

    def __init__(self):
        import bench
        from test_memchain import _oracle_front, _two_strand
        ref = bench.seeding_reference(300_000, seed=3)
        reads, off, lens = bench.pe_reads(ref, 1500, 150, seed=9)
        rng = np.random.default_rng(21)
        R = reads.reshape(-1, 150)
        self.kind = np.zeros(1500, np.int8)
        for p in range(1500):
            if rng.random() >= 0.30:
                continue
            m = R[2 * p + int(rng.integers(0, 2))]
            u = rng.random()
            if u < 0.05:
                m[:] = rng.integers(0, 4, 150)
                self.kind[p] = 3
                continue
            if u < 0.10:                                     # a deletion from the read: shift left, random tail
                d, at = int(rng.integers(2, 5)), int(rng.integers(40, 110))
                m[at:150 - d] = m[at + d:].copy()
                m[150 - d:] = rng.integers(0, 4, d)
                self.kind[p] = 2
            else:
                self.kind[p] = 1
            pos = int(rng.integers(0, 13))
            while pos < 150:
                m[pos] = (m[pos] + int(rng.integers(1, 4))) % 4 if m[pos] < 4 else int(rng.integers(0, 4))
                pos += int(rng.integers(13, 17))
        self.T = Tt = _two_strand(ref)
        self.l_pac = len(ref)
        f, mems, cnt, seeds, sr, sc = _oracle_front(ref, reads, off, lens, cap=256)
        self.eopt = bsw.ext_opt(l_pac=len(ref))
        regs, ext = oracle.chain2aln(oracle.make_params(), self.eopt, Tt, reads, off, lens, seeds, sr, sc)
        self.arr = dict(reads=reads, off=off, lens=lens, seeds=seeds, sr=sr, sc=sc, regs=regs, ext=ext)
        self.sopt = sp.sel_opt(l_pac=self.l_pac)
        self.sel = _select(Tt, self.arr, opt=self.sopt)
        self.regs, _, self.info, self.first, _ = self.sel
        self.opt = pp.pe_opt(l_pac=self.l_pac)
        self.mopt = mp.matesw_opt(l_pac=self.l_pac)
        self.mat, self.gaps = mat_gaps(DEFAULT)
        self.pes, self.tr_stat, _ = pp.pe_stat(self.regs, self.info, self.first, self.opt, 1)
        self.want = mp.mate_rescue(self.pes, Tt, reads, off, lens, self.regs, self.info, self.first, self.mopt,
                                   self.mat, self.gaps, oracle.ksw_align2)
        self.mregs, self.mread, self.minfo, self.mfirst, self.tr = self.want
        self.paired = pp.pe_pair(self.pes, self.mregs, self.minfo, self.mfirst, self.opt, self.mat, self.gaps)


_set = {}


def ms_set():
    if not _set:
        _set["x"] = MsSet()
    return _set["x"]


def test_pipeline_set():
    p = ms_set()
    regs, info, pairs, tr = p.paired
    c = p.tr.cnt
    print("matesw set:", dict(c), "rounds", p.tr.rounds, "pes", p.pes, "pair", dict(tr.cnt), tr.margin)
    assert p.pes[1]["failed"] == 0
    rescued = 0
    for k in range(1500):
        z = pairs[k]["z"]
        rescued += any(pairs[k]["paired"] and pairs[k]["proper"] and z[e] >= 0 and
                       info[p.mfirst[2 * k + e] + z[e]]["src"] == -1 for e in (0, 1))
    assert rescued >= 200, rescued
    assert sum(1 for j, g in p.tr.per_pair if j > 0 and g == 0) >= 20
    assert sum(1 for j, g in p.tr.per_pair if j == 0) >= 1000
    assert tr.margin >= 1e-6 and c["jobs"] > 400 and p.tr.rounds >= 1


def test_combined_sets_reach_every_branch():
    tot = sp.Counter()
    for g in GROUPS:
        tot.update(hand_want(g)[3][4].cnt)
    tot.update(hand_want("fr", SCORINGS[2], True)[3][4].cnt)
    tot.update(long_want()[2][4].cnt)
    tot.update(ms_set().tr.cnt)
    m, rb = rev_at(1401, 125)
    tot.update(_one(REF[A0:A0 + RL], ANCHOR, mutate(m), [], scoring=SCORINGS[2])[3].cnt)
    print("branches:", {k: tot[k] for k in mp.BRANCHES})
    assert all(tot[k] > 0 for k in mp.BRANCHES), {k: tot[k] for k in mp.BRANCHES if tot[k] == 0}


# ---------------------------------------------------------------- CPU: the header
def test_library_exports_the_matesw_header():
    assert declared("bsw_matesw.h") == set(bsw.MATESW_SYMBOLS)
    assert declared("bsw_matesw.h") <= exported(), declared("bsw_matesw.h") - exported()
    others = set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS)
    assert not set(bsw.MATESW_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_matesw_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_matesw.h"\n'
                   f"{sa}(sizeof(bsw_matesw_opt_t) == 32 && offsetof(bsw_matesw_opt_t, max_matesw) == 8 && offsetof(bsw_matesw_opt_t, mask_level_redun) == 24, \"opt\");\n"
                   f"{sa}(sizeof(bsw_matesw_stats_t) == 56 && offsetof(bsw_matesw_stats_t, rounds) == 40 && offsetof(bsw_matesw_stats_t, helper_ms) == 52, \"stats\");\n"
                   f"{sa}(BSW_MATESW_API == 1 && BSW_ABI_VERSION == 8, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.MateswOpt) == 32 and bsw.MateswOpt.max_matesw.offset == 8
    assert bsw.MateswOpt.mask_level_redun.offset == 24
    assert ctypes.sizeof(bsw.MateswStats) == 56 and bsw.MateswStats.rounds.offset == 40
    assert bsw.MateswStats.helper_ms.offset == 52


def _lib_calls(ctx, o, pes, n_reads=2):
    Lb = bsw.hip_lib()
    regs, info = np.zeros(1, dtype=bsw.ALNREG_DTYPE), np.zeros(1, dtype=bsw.SELINFO_DTYPE)
    first, rd = np.zeros(n_reads + 1, dtype=np.int32), np.zeros(4, np.int32)
    reads, off, lens = np.zeros(8, np.uint8), np.zeros(max(n_reads, 1), np.int64), np.zeros(max(n_reads, 1), np.int32)
    n_out = ctypes.c_int32(0)
    P, B = bsw._ptr, ctypes.byref
    return (Lb.bsw_matesw(ctx, B(o), P(pes), P(reads), P(off), P(lens), n_reads, P(regs), P(info), P(first), P(regs),
                          P(rd), P(info), P(first), 1, B(n_out)),
            Lb.bsw_matesw_resident(ctx, B(o), P(pes), P(reads), P(off), P(lens), n_reads, P(regs), P(info), P(first), 0,
                                   P(regs), P(rd), P(info), P(first), 1, B(n_out), None))


def test_defaults_and_invalid_arguments_need_no_device():
    o = bsw.matesw_opt()
    got = {f: getattr(o, f) for f, _ in o._fields_}
    assert {k: (round(v, 6) if isinstance(v, float) else v) for k, v in got.items()} == mp.DEFAULT_OPT
    Lb = bsw.hip_lib()
    assert Lb.bsw_matesw_last_stats(None, None) == -22
    fake = ctypes.c_void_p(1)                                # never dereferenced: the checks come first
    good = PES_FR.copy()
    for kw in (dict(l_pac=0), dict(l_pac=-5), dict(l_pac=L, max_matesw=-1), dict(l_pac=L, min_seed_len=0)):
        assert _lib_calls(fake, bsw.matesw_opt(**kw), good) == (-22, -22), kw
    assert _lib_calls(fake, bsw.matesw_opt(l_pac=L), good, n_reads=3) == (-22, -22)
    bad = good.copy()
    bad[1]["low"], bad[1]["high"] = 700, 300
    assert _lib_calls(fake, bsw.matesw_opt(l_pac=L), bad) == (-22, -22)
    assert _lib_calls(None, bsw.matesw_opt(l_pac=L), good) == (-22, -22)
    with pytest.raises(ValueError, match="INVAL"):
        mp.check_opt(mp.matesw_opt(l_pac=L), [dict(low=700, high=300, failed=0)] * 4, 2)


# ---------------------------------------------------------------- GPU
def _gpu(eng, batch, pes, scoring=DEFAULT, **kw):
    reads, off, lens, regs, info, first = batch.arrays(scoring[0])
    return bsw.matesw(eng, pes, reads, off, lens, regs, info, first, bsw.matesw_opt(l_pac=L, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", SCORINGS)
def test_gpu_hand_set(scoring):
    eng = engine_of(scoring)
    bsw.set_reference(eng, T)
    for mirror in (False, True):
        bsw.set_reference(eng, T_MIRROR if mirror else T)
        for g in GROUPS:
            b, pes, kw, want, jobs, text = hand_want(g, scoring, mirror)
            same_msw(want, _gpu(eng, b, pes, scoring, **kw), f"hand {g} {scoring} {mirror}", bsw.matesw_last_stats(eng))
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_host_arrays():
    p = ms_set()
    a = p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    got = bsw.matesw(eng, p.pes, a["reads"], a["off"], a["lens"], p.regs, p.info, p.first, bsw.matesw_opt(l_pac=p.l_pac))
    same_msw(p.want, got, "pipeline set", bsw.matesw_last_stats(eng))
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_device_to_device():
    """bsw_regs_select_resident -> bsw_pe_stat_resident -> bsw_matesw_resident -> bsw_pe_pair_resident ->
    bsw_reg2aln_resident"""
    p = ms_set()
    a = p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"])
    b.put(seeds=a["seeds"], sr=a["sr"], sc=a["sc"])
    b.chain2aln(p.eopt)
    k = b.select(bsw.sel_opt(l_pac=p.l_pac))
    assert k == len(p.regs)
    o = bsw.pe_opt(l_pac=p.l_pac)
    pes = b.pe_stat(o)
    same_pes(p.pes, pes, "device to device")
    cap = len(p.mregs)
    m = b.matesw(pes, bsw.matesw_opt(l_pac=p.l_pac), cap=cap)
    assert m == cap
    same_msw(p.want, fetch(b, *b.lists[0]), "device to device", bsw.matesw_last_stats(eng))
    b.pe_pair(pes, o)
    same_pair(p.paired, got_pair(b), "device to device, paired", bsw.pe_last_stats(eng))
    b.reg2aln(p.eopt)
    aln = got_aln(b)
    sel = np.zeros(m, dtype=bsw.ALNREG_DTYPE)
    for f in sp.ALNREG_FIELDS:
        sel[f] = p.paired[0][f]
    same_aln(rp.reg2aln(p.T, p.l_pac, a["reads"], a["off"], a["lens"], sel, p.mread, p.mat, p.gaps, p.eopt.w), aln,
             "alignments of the rescued regions")
    eng.close()


@pytest.mark.gpu
def test_gpu_batch_sizes():
    p = ms_set()
    a = p.arr
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    wr, wd, wi, wf, tr = p.want
    for npairs in (0, 1, 63, 64, 65, 257):
        k, m = p.first[2 * npairs], wf[2 * npairs]
        got = bsw.matesw(eng, p.pes, a["reads"][:npairs * 300], a["off"][:2 * npairs], a["lens"][:2 * npairs],
                         p.regs[:k], p.info[:k], p.first[:2 * npairs + 1], bsw.matesw_opt(l_pac=p.l_pac))
        same_msw((wr[:m], wd[:m], wi[:m], wf[:2 * npairs + 1], tr), got, f"{npairs} pairs")
        assert bsw.matesw_last_stats(eng).n_pairs == npairs
    eng.close()


@pytest.mark.gpu
def test_gpu_list_lengths():
    b, pes, want = long_want()
    tr = want[4]
    assert tr.rounds >= 40 and tr.cnt["jobs"] > 400 and tr.cnt["pushed"] >= 10 and tr.cnt["drop_p"] + tr.cnt["drop_q"] >= 10
    eng = bsw.Engine()
    bsw.set_reference(eng, T)
    same_msw(want, _gpu(eng, b, pes), "list lengths", bsw.matesw_last_stats(eng))
    eng.close()


@pytest.mark.gpu
def test_gpu_consistent_batch_runs_no_dp():
    b = MsBatch()
    mate, rb = rev_at(1401)
    for k in range(70):
        b.add(f"c{k}", REF[A0:A0 + RL], [reg(A0, 100 - k % 3), reg(9000, 70)], mutate(mate), [reg(rb, 90), reg(rb - 3000, 60)])
    reads, off, lens, regs, info, first = b.arrays()
    eng = bsw.Engine()
    bsw.set_reference(eng, T)
    gr, gd, gi, gf = bsw.matesw(eng, PES_FR, reads, off, lens, regs, info, first, bsw.matesw_opt(l_pac=L))
    st = bsw.matesw_last_stats(eng)
    assert (st.n_jobs, st.rounds, st.sw_ms, st.n_lists_changed) == (0, 0, 0.0, 0) and st.n_calls == st.n_calls_all_skipped > 0
    assert gr.tobytes() == regs.tobytes() and gi.tobytes() == info.tobytes() and np.array_equal(gf, first)
    assert np.array_equal(gd, np.repeat(np.arange(len(first) - 1), np.diff(first)))
    eng.close()


@pytest.mark.gpu
def test_gpu_errors_and_recovery():
    b, pes, kw, want, jobs, text = hand_want("fr")
    reads, off, lens, regs, info, first = b.arrays()
    o = bsw.matesw_opt(l_pac=L)
    eng = bsw.Engine()
    with pytest.raises(bsw.BswError, match="-22"):            # no resident reference
        bsw.matesw(eng, pes, reads, off, lens, regs, info, first, o)
    bsw.set_reference(eng, np.zeros(2 * L - 2, np.uint8))     # one that does not fit l_pac
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.matesw(eng, pes, reads, off, lens, regs, info, first, o)
    bsw.set_reference(eng, T)
    need = len(want[0])
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.matesw(eng, pes, reads, off, lens, regs, info, first, o, out_cap=need - 1)
    assert ei.value.needed == need and np.array_equal(ei.value.first, want[3])
    same_msw(want, bsw.matesw(eng, pes, reads, off, lens, regs, info, first, o, out_cap=need), "exact capacity",
          bsw.matesw_last_stats(eng))
    for v in (-1, 2 * L):
        r2 = regs.copy()
        r2[0]["rb"] = v
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.matesw(eng, pes, reads, off, lens, r2, info, first, o)
    dec = first.copy()
    dec[3] = dec[2] - 1
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.matesw(eng, pes, reads, off, lens, regs, info, dec, o)
    d = [hiprt.DeviceBuffer.from_array(np.ascontiguousarray(x)) for x in (reads, off, lens, regs, info, dec, first)]
    out = [hiprt.DeviceBuffer(need * s) for s in (bsw.ALNREG_DTYPE.itemsize, 4, bsw.SELINFO_DTYPE.itemsize)]
    d_of = hiprt.DeviceBuffer(len(first) * 4)
    nr = len(first) - 1
    with pytest.raises(bsw.BswError, match="-34"):            # the device's own check of the offsets
        bsw.matesw_resident(eng, pes, d[0].ptr, d[1].ptr, d[2].ptr, nr, d[3].ptr, d[4].ptr, d[5].ptr, len(regs),
                            out[0].ptr, out[1].ptr, out[2].ptr, d_of.ptr, need, o)
    with pytest.raises(bsw.BswError, match="-34"):            # offsets past n_regs
        bsw.matesw_resident(eng, pes, d[0].ptr, d[1].ptr, d[2].ptr, nr, d[3].ptr, d[4].ptr, d[6].ptr, len(regs) - 1,
                            out[0].ptr, out[1].ptr, out[2].ptr, d_of.ptr, need, o)
    # a query above BSW_MATE_MAX_QLEN, a window above BSW_MAX_LEN
    bl = MsBatch()
    bl.add("q257", REF[A0:A0 + RL], ANCHOR, rnd(257, seed=8), [])
    with pytest.raises(bsw.BswError, match="-34"):
        _gpu(eng, bl, PES_FR)
    # (a window is cut at l_pac, so one above BSW_MAX_LEN needs a longer text: [101, 36200) of 2 x 40,000)
    bsw.set_reference(eng, np.zeros(80000, np.uint8))
    r1, i1 = np.zeros(1, dtype=bsw.ALNREG_DTYPE), np.zeros(1, dtype=bsw.SELINFO_DTYPE)
    r1[0] = (100, 200, 0, 100, 100, 100, 100, 19)
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.matesw(eng, _pes(FF=(1, 36000, 500.0, 50.0)), reads[:200], off[:2], lens[:2], r1, i1,
                   np.array([0, 1, 1], np.int32), bsw.matesw_opt(l_pac=40000))
    bsw.set_reference(eng, T)
    same_msw(want, bsw.matesw(eng, pes, reads, off, lens, regs, info, first, o), "after the errors", bsw.matesw_last_stats(eng))
    eng.close()
