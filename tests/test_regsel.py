"""Region selection (include/bsw_sel.h): mem_sort_dedup_patch, mem_mark_primary_se and
mem_approx_mapq_se between bsw_chain2aln* and bsw_reg2aln*.

CPU: hand-built reads with known answers through the Python restatement (tests/regsel_py.py), the
sorts' tie order, MAPQ branch by branch, two pipeline sets through the oracle, the conditions the
GPU comparison rests on (every branch reached, every truncation away from its boundary), the
header's symbols and layouts.
GPU: bsw_regs_select / bsw_regs_select_resident == the restatement in every output field, every
read offset, n_sel and the stats counters.  Parity is unpinned by the reference tree (it holds no
source of these functions; bsw_sel.h restates them).
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import bsw
import oracle
import reg2aln_py as rp
import regsel_py as sp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import (DEFAULT, REG_FIELDS, SCORINGS, declared, exported, fetch, got_aln, mat_gaps, revcomp, same_aln,
                      same_sel)


# ---------------------------------------------------------------- batches
class Batch:
    """the arrays of one call; reads are added one at a time with their regions"""

    def __init__(self):
        self.reads, self.lens, self.seeds, self.sr, self.sc, self.regs, self.ext, self.names = [], [], [], [], [], [], [], []

    def add(self, name, read, regions, chains=None, ext=None):
        """regions: (qb, qe, rb, re, score[, w]); each gets a seed slot at its start, in a chain of
        its own unless `chains` names them"""
        r = len(self.lens)
        self.names.append(name)
        self.reads.append(np.asarray(read, dtype=np.uint8))
        self.lens.append(len(read))
        for k, g in enumerate(regions):
            qb, qe, rb, re_, score = (int(v) for v in g[:5])
            w = int(g[5]) if len(g) > 5 else 100
            ln = max(min(19 + 3 * k, qe - qb), 0)
            self.seeds.append((rb, qb, ln))
            self.sr.append(r)
            self.sc.append(chains[k] if chains else k)
            self.regs.append((rb, re_, qb, qe, score, score, w, ln))
            self.ext.append(1 if ext is None else ext[k])

    def arrays(self):
        reads = np.concatenate(self.reads) if self.reads else np.zeros(0, np.uint8)
        lens = np.array(self.lens, dtype=np.int32)
        off = (np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else np.zeros(0)).astype(np.int64)
        seeds = np.array(self.seeds, dtype=[("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")]).view(bsw.SEED_DTYPE)
        regs = np.zeros(len(self.regs), dtype=bsw.ALNREG_DTYPE)
        for k, g in enumerate(self.regs):
            regs[k] = g
        return dict(reads=reads, off=off, lens=lens, seeds=seeds, sr=np.array(self.sr, dtype=np.int32),
                    sc=np.array(self.sc, dtype=np.int32), regs=regs, ext=np.array(self.ext, dtype=np.int32))


assert bsw.ALNREG_DTYPE.names == ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedlen0")


def hand_cases(T, s0=300, step=500):
    """(name, read, regions) on the forward strand of T from s0 on, one every `step` bases"""
    L = len(T) // 2
    R = lambda a, n: T[a:a + n]                                      # noqa: E731
    tail = lambda a: np.array([(int(T[a]) + 1) % 4], dtype=np.uint8)  # noqa: E731
    cat = lambda *p: np.concatenate(p).astype(np.uint8)              # noqa: E731
    c, s = [], s0

    def case(name, read, regs):
        nonlocal s
        assert len(read) == 151, name
        c.append((name, read, regs))
        s += step

    case("patch_del3", cat(R(s, 75), R(s + 78, 75), tail(s + 153)), [(0, 75, s, s + 75, 75), (75, 150, s + 78, s + 153, 75)])
    case("ratio_del6", cat(R(s, 75), R(s + 81, 75), tail(s + 156)), [(0, 75, s, s + 75, 75), (75, 150, s + 81, s + 156, 75)])
    case("strands", R(s, 151), [(0, 75, s, s + 75, 75), (75, 150, L + 100, L + 175, 75)])
    case("not_colinear", R(s, 151), [(75, 150, s, s + 75, 75), (0, 75, s + 80, s + 155, 75)])
    case("past_2w", R(s, 151), [(0, 75, s, s + 75, 75), (75, 150, s + 325, s + 400, 75)])
    case("r_005", cat(R(s, 75), R(s + 85, 75), tail(s + 160)), [(0, 75, s, s + 75, 75), (75, 150, s + 85, s + 160, 75)])
    case("redun_q", R(s, 151), [(0, 150, s, s + 150, 150), (0, 148, s, s + 148, 140)])
    case("redun_p", R(s, 151), [(0, 150, s, s + 150, 150), (0, 148, s, s + 148, 160)])
    case("same", R(s, 151), [(0, 150, s, s + 150, 150), (0, 150, s, s + 150, 150)])
    case("gapfree_patch", R(s, 151), [(0, 75, s, s + 75, 75, 0), (75, 150, s + 75, s + 150, 75, 0)])
    case("three_pieces", cat(R(s, 50), R(s + 51, 50), R(s + 102, 50), tail(s + 152)),
         [(0, 50, s, s + 50, 50), (50, 100, s + 51, s + 101, 50), (100, 150, s + 102, s + 152, 50)])
    case("overlapping", cat(R(s, 75), R(s + 78, 75), tail(s + 153)), [(0, 80, s, s + 80, 80), (70, 150, s + 73, s + 153, 80)])
    case("secondary", R(s, 151), [(0, 150, s, s + 150, 150), (0, 150, s + 200, s + 350, 147)])
    case("lone", R(s, 151), [(0, 151, s, s + 151, 151)])
    case("low_identity", R(s, 151), [(0, 151, s, s + 151, 100)])
    case("empty_span", R(s, 151), [(20, 20, s, s + 100, 60), (0, 100, s, s + 100, 90)])
    return c


def _mirror(read, regs, L):
    n = len(read)
    return revcomp(read), [(n - g[1], n - g[0], 2 * L - g[3], 2 * L - g[2], *g[4:]) for g in regs]


def hand_batch(T, mirrors=True, scale=1, **kw):
    """scale multiplies the recipes' scores (they are in units of a = 1)"""
    b = Batch()
    for name, read, regs in hand_cases(T, **kw):
        regs = [(*g[:4], g[4] * scale, *g[5:]) for g in regs]
        b.add(name, read, regs)
        if mirrors:
            b.add(name + "~", *_mirror(read, regs, len(T) // 2))
    b.add("not_extended", T[100:251], [(0, 151, 100, 251, 151 * scale)], ext=[0])
    return b


def small_text(seed=4, n=9000):
    ref = np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)
    return np.concatenate([ref, revcomp(ref)])


def _select(T, arr, scoring=DEFAULT, opt=None, **kw):
    mat, gaps = mat_gaps(scoring)
    return sp.regs_select(T, arr["reads"], arr["off"], arr["lens"], arr["seeds"], arr["sr"], arr["sc"], arr["regs"],
                          arr["ext"], mat, gaps, opt or sp.sel_opt(l_pac=len(T) // 2, b=scoring[1]), **kw)


_hand = {}


def hand_want(patch=1, scoring=DEFAULT, **optkw):
    key = (patch, scoring, tuple(sorted(optkw.items())))
    if key not in _hand:
        T = small_text()
        b = hand_batch(T, scale=scoring[0])
        arr = b.arrays()
        opt = sp.sel_opt(l_pac=len(T) // 2, patch=patch, b=scoring[1], **optkw)
        _hand[key] = (T, b, arr, opt, _select(T, arr, scoring, opt))
    return _hand[key]


def _of_read(b, want, name):
    r = b.names.index(name)
    regs, rd, info, first, tr = want
    sl = slice(first[r], first[r + 1])
    return regs[sl], info[sl]


# ---------------------------------------------------------------- CPU: known answers
def test_three_base_deletion_is_patched():
    T, b, arr, opt, want = hand_want()
    for name in ("patch_del3", "patch_del3~"):
        regs, info = _of_read(b, want, name)
        assert len(regs) == 1, name
        g = regs[0]
        assert (g["qe"] - g["qb"], g["re"] - g["rb"], g["score"], g["truesc"], g["w"]) == (150, 153, 141, 141, 203)
        assert (info[0]["n_comp"], info[0]["secondary"]) == (3, -1)
    s = 300
    assert (regs[0]["qb"], info[0]["src"]) != (None, None) and _of_read(b, want, "patch_del3")[0][0]["rb"] == s


def test_six_base_deletion_is_refused_by_the_ratio():
    T, b, arr, opt, want = hand_want()
    regs, info = _of_read(b, want, "ratio_del6")
    assert len(regs) == 2 and sorted(regs["score"]) == [75, 75] and list(info["n_comp"]) == [1, 1]
    # 138 / max(150, 156) < 0.90
    one = Batch()
    one.add(*hand_cases(T)[1])
    tr = _select(T, one.arrays(), opt=opt)[4]
    assert tr.cnt["patch_ratio"] == 1 and tr.cnt["patch_dp"] == 1 and tr.cnt["patch_ok"] == 0


@pytest.mark.parametrize("name,branch", [("strands", "patch_strand"), ("not_colinear", "patch_order"),
                                         ("past_2w", "patch_w"), ("r_005", "patch_r")])
def test_patch_refusals(name, branch):
    T = small_text()
    case = [c for c in hand_cases(T) if c[0] == name][0]
    one = Batch()
    one.add(*case)
    regs, rd, info, first, tr = _select(T, one.arrays())
    assert len(regs) == 2 and tr.cnt[branch] == 1 and tr.cnt["patch_tried"] == 0, tr.cnt
    off = _select(T, one.arrays(), opt=sp.sel_opt(l_pac=len(T) // 2, patch=0))[4]
    assert off.cnt["patch_off"] == 1 and off.cnt[branch] == 0


def test_redundant_pair_is_dropped_in_both_score_orders():
    T, b, arr, opt, want = hand_want()
    regs, info = _of_read(b, want, "redun_q")
    assert len(regs) == 1 and (regs[0]["qe"], regs[0]["score"]) == (150, 150)
    regs, info = _of_read(b, want, "redun_p")
    assert len(regs) == 1 and (regs[0]["qe"], regs[0]["score"]) == (148, 160)
    assert want[4].cnt["drop_p"] >= 2 and want[4].cnt["drop_q"] >= 2        # (each with its mirror)


def test_identical_hit_rule_at_mask_level_redun_one():
    T, b, arr, opt, want = hand_want(mask_level_redun=1.0)
    regs, info = _of_read(b, want, "same")
    assert len(regs) == 1 and want[4].cnt["identical"] >= 1
    T, b, arr, opt, want = hand_want()
    assert len(_of_read(b, want, "same")[0]) == 1 and want[4].cnt["identical"] == 0   # (redundant before that)


def test_gap_free_patch_and_two_rounds():
    T, b, arr, opt, want = hand_want()
    regs, info = _of_read(b, want, "gapfree_patch")
    assert len(regs) == 1 and (regs[0]["score"], regs[0]["w"], info[0]["n_comp"]) == (150, 0, 3)
    assert want[4].cnt["patch_gapfree"] >= 1
    regs, info = _of_read(b, want, "three_pieces")
    assert len(regs) == 1 and (regs[0]["qb"], regs[0]["qe"], regs[0]["score"], regs[0]["w"]) == (0, 150, 136, 302)
    assert info[0]["n_comp"] == 5 and want[4].rounds == 2
    regs, info = _of_read(b, want, "overlapping")
    assert len(regs) == 1 and regs[0]["score"] == 141
    regs, info = _of_read(b, want, "empty_span")
    assert len(regs) == 1 and info[0]["src"] == b.sr.index(b.names.index("empty_span")) + 1
    assert len(_of_read(b, want, "not_extended")[0]) == 0


def long_span_batch():
    """a patch candidate whose reference span (33,100) is above BSW_MAX_LEN: two overlapping regions
    with the same overlap share on the read (50 / 150) and on the reference (11,000 / 33,100)"""
    T = small_text(seed=6, n=40000)
    b = Batch()
    b.add("long_span", T[1000:1151], [(0, 100, 1000, 34000, 100), (50, 150, 23000, 34100, 100)])
    return T, b.arrays(), sp.sel_opt(l_pac=len(T) // 2, w=3000)


def test_patch_span_above_max_len_is_an_error():
    T, arr, opt = long_span_batch()
    with pytest.raises(ValueError, match="BSW_MAX_LEN"):
        _select(T, arr, opt=opt)
    tr = _select(T, arr, opt=dict(opt, w=100))[4]              # at w = 100 the band test refuses it first
    assert tr.cnt["patch_w"] == 1 and tr.cnt["patch_tried"] == 0


def test_patch_off_keeps_the_halves():
    T, b, arr, opt, want = hand_want(patch=0)
    assert len(_of_read(b, want, "patch_del3")[0]) == 2 and want[4].cnt["patch_tried"] == 0 and want[4].rounds == 0
    assert want[4].cnt["patch_off"] > 0


# ---------------------------------------------------------------- CPU: sort order
def _tied(n, seed):
    rng = np.random.default_rng(seed)
    s = 2000
    return [(int(q), int(q) + 40, s + 80 - int(d), s + 120, 20 + int(x))
            for q, d, x in zip(rng.permutation(100)[:n], rng.integers(0, 3, n), rng.permutation(n))]


@pytest.mark.parametrize("n", [16, 17])
def test_tied_re_follows_klib(n):
    """tied keys through klib's introsort: its partition swaps equal keys at any n > 2, and what the
    last insertion sort (ranges up to 16) leaves differs between 16 and 17 -- a stable sort is wrong"""
    from memchain_py import introsort
    a = [(5, k) for k in range(n)]
    introsort(a, lambda x, y: x[0] < y[0])
    moved = a != [(5, k) for k in range(n)]
    assert sorted(a) == [(5, k) for k in range(n)] and moved == (n > 2)
    b = [(k % 3, k) for k in range(n)]
    introsort(b, lambda x, y: x[0] < y[0])
    assert [x[0] for x in b] == sorted(k % 3 for k in range(n))
    T = small_text()
    one = Batch()
    one.add("tied", T[2000:2151], _tied(n, 3))
    regs, rd, info, first, tr = _select(T, one.arrays())
    assert first[-1] == len(regs) >= 1


def test_hash_breaks_score_ties():
    assert sp.hash_64(0) == 0x6A396CD39C352659 and len({sp.hash_64(k) for k in range(1000)}) == 1000
    T = small_text()
    one = Batch()
    s = 1000
    one.add("ties", T[s:s + 151], [(0, 50, s, s + 50, 50), (50, 100, s + 3000, s + 3050, 50), (100, 150, s + 6000, s + 6050, 50)])
    orders = set()
    for id0 in (0, 1 << 40, 5, 77):
        regs, rd, info, first, tr = _select(T, one.arrays(), opt=sp.sel_opt(l_pac=len(T) // 2, id0=id0))
        assert len(regs) == 3
        h = [sp.hash_64(id0 + i) for i in range(3)]
        # after step 5 the three are in rb order; the hash sort reorders them by hash
        assert list(info["src"]) == [int(k) for k in np.argsort(h)]
        orders.add(tuple(info["src"]))
    assert len(orders) > 1


# ---------------------------------------------------------------- CPU: MAPQ
def _mq(score=100, sub=0, csub=0, sub_n=0, secondary=-1, seedcov=80, l=100, frac_rep=0.0, **optkw):
    tr = sp.Trace()
    x = dict(score=score, sub=sub, csub=csub, sub_n=sub_n, secondary=secondary, seedcov=seedcov, qb=0, qe=l, rb=0, re=l)
    return sp.approx_mapq(sp.sel_opt(**optkw), x, 1, frac_rep, tr), tr


def test_mapq_branches():
    assert _mq(score=100, sub=100)[0] == 0 and _mq(score=100, sub=120)[1].cnt["mapq_sub_ge"] == 1
    assert _mq(secondary=0)[0] == 0
    # l = 100, exact: t = 3 / log(100); 6.02 * (100 - 19) * t^2 = 206.9 -> 60
    assert _mq()[0] == 60
    # sub 90: 6.02 * 10 * 0.4244 = 25.55 (+ .499) -> 26; the sub_n penalty: 4.343 * log(3) = 4.77 -> 5
    assert _mq(sub=90)[0] == 26 and _mq(sub=90, sub_n=2)[0] == 21
    # csub above sub takes its place: 6.02 * 5 * 0.4244 = 12.77 -> 13
    assert _mq(sub=90, csub=95)[0] == 13 and _mq(sub=90, csub=50)[0] == 26
    assert [_mq(frac_rep=f)[0] for f in (0.0, 0.25, 0.9)] == [60, 45, 6]
    # mapQ_coef_len = 0: 30 * (1 - 19/80) * log(80) = 100.2 -> identity 0.96 leaves it; 0.90 scales it
    m, tr = _mq(score=80, l=100, mapQ_coef_len=0)
    assert tr.cnt["mapq_lowid"] == 0 and tr.cnt["mapq_seedcov"] == 1 and m == 60
    m, tr = _mq(score=60, sub=50, l=100, mapQ_coef_len=0, seedcov=40)
    assert tr.cnt["mapq_lowid"] == 1 and m == int(int(30.0 * (1 - 50 / 60) * np.log(40) + .499) * 0.92 * 0.92 + .499)
    m, tr = _mq(score=99, sub=50, l=100, mapQ_coef_len=0, seedcov=40)
    assert tr.cnt["mapq_lowid"] == 0 and tr.cnt["mapq_seedcov"] == 1 and m == 55     # 30 * (49 / 99) * log(40) = 54.77


def test_secondary_and_sub_n_on_the_hand_batch():
    T, b, arr, opt, want = hand_want()
    regs, info = _of_read(b, want, "secondary")
    assert list(info["secondary"]) == [-1, 0] and list(info["sub"]) == [147, 0] and list(info["sub_n"]) == [1, 0]
    assert list(info["mapq"]) == [3, 0] and list(regs["score"]) == [150, 147]
    regs, info = _of_read(b, want, "lone")
    assert list(info["mapq"]) == [60] and info[0]["seedcov"] == 19


# ---------------------------------------------------------------- pipeline sets
def _with_appended(arr, T, every=25):
    """every 25th extended region twice more in its read, as two further chains: shifted by one
    reference base with score - 1 and with score + 1"""
    L = len(T) // 2
    b = {k: [] for k in ("seeds", "sr", "sc", "regs", "ext")}
    pick = set(int(k) for k in np.flatnonzero(arr["ext"])[::every])
    n, k = len(arr["sr"]), 0
    while k < n:
        e = k
        while e < n and arr["sr"][e] == arr["sr"][k]:
            e += 1
        nxt = int(arr["sc"][k:e].max()) + 1
        rows = [(arr["seeds"][i], arr["sc"][i], arr["regs"][i], arr["ext"][i]) for i in range(k, e)]
        for i in range(k, e):
            g = arr["regs"][i]
            if i in pick and g["re"] + 1 <= len(T) and not (g["rb"] < L <= g["re"]):
                for d in (-1, 1):
                    sd, rg = arr["seeds"][i].copy(), g.copy()
                    sd["rbeg"] += 1; rg["rb"] += 1; rg["re"] += 1; rg["score"] += d
                    rows.append((sd, nxt, rg, 1))
                    nxt += 1
        for sd, c, rg, x in rows:
            b["seeds"].append(sd); b["sr"].append(arr["sr"][k]); b["sc"].append(c); b["regs"].append(rg); b["ext"].append(x)
        k = e
    out = dict(arr)
    out.update(seeds=np.array(b["seeds"], dtype=bsw.SEED_DTYPE), sr=np.array(b["sr"], np.int32),
               sc=np.array(b["sc"], np.int32), regs=np.array(b["regs"], dtype=bsw.ALNREG_DTYPE),
               ext=np.array(b["ext"], np.int32))
    return out


def _join(a, b):
    """batch b's reads after batch a's"""
    out = {}
    for k in ("reads", "lens", "seeds", "sc", "regs", "ext"):
        out[k] = np.concatenate([a[k], b[k]])
    out["off"] = np.concatenate([a["off"], b["off"] + len(a["reads"])]).astype(np.int64)
    out["sr"] = np.concatenate([a["sr"], b["sr"] + len(a["lens"])]).astype(np.int32)
    return out


class PipeSet:
    def __init__(self, which):
        from test_memchain import _oracle_front, _two_strand, dispersed_copies_ref
        if which == "dispersed":
            ref, reads, off, lens = dispersed_copies_ref()
            cap = 2048
        else:
            import bench
            ref = bench.seeding_reference(400_000, seed=3)
            reads, off, lens = bench.seeding_reads(ref, 2000, 151, seed=8)
            cap = 256
        self.T = T = _two_strand(ref)
        self.l_pac = len(ref)
        f, mems, cnt, seeds, sr, sc = _oracle_front(ref, reads, off, lens, cap=cap)
        self.eopt = bsw.ext_opt(l_pac=len(ref))
        regs, ext = oracle.chain2aln(oracle.make_params(), self.eopt, T, reads, off, lens, seeds, sr, sc)
        self.plain = dict(reads=reads, off=off, lens=lens, seeds=seeds, sr=sr, sc=sc, regs=regs, ext=ext)
        self.opt = sp.sel_opt(l_pac=self.l_pac)
        self.want_plain = _select(T, self.plain, opt=self.opt)
        rng = np.random.default_rng(5)
        self.frac_rep = (rng.integers(0, 4, len(lens)) * 0.25 * (rng.random(len(lens)) < 0.3)).astype(np.float32)
        self.full = _join(_with_appended(self.plain, T), hand_batch(T, s0=1300, step=2000).arrays())
        self.full_frac = np.concatenate([self.frac_rep, np.zeros(len(self.full["lens"]) - len(lens), np.float32)])
        self.csub = (np.arange(len(self.full["sr"])) % 7 == 0).astype(np.int32) * 30
        self.want = _select(T, self.full, opt=self.opt, csub=self.csub, frac_rep=self.full_frac)


_sets = {}


def pipe_set(which):
    if which not in _sets:
        _sets[which] = PipeSet(which)
    return _sets[which]


def test_dispersed_copies_set():
    p = pipe_set("dispersed")
    regs, rd, info, first, tr = p.want_plain
    per_read = np.bincount(p.plain["sr"][p.plain["ext"] != 0], minlength=80)
    print("dispersed:", dict(tr.cnt), "margin", tr.margin, "per read", per_read.min(), per_read.max())
    assert per_read.min() > 16 and per_read.sum() == 3721
    assert tr.cnt["secondary"] == 3641 and tr.cnt["sub_n"] == 3641
    prim = info["secondary"] < 0
    assert prim.sum() == 80 and np.all(info["mapq"][prim] == 0)
    assert tr.cnt["drop_p"] + tr.cnt["drop_q"] + tr.cnt["patch_tried"] == 0
    assert tr.margin >= 1e-6


def test_seeding_set():
    p = pipe_set("seeding")
    regs, rd, info, first, tr = p.want_plain
    print("seeding:", dict(tr.cnt), "margin", tr.margin, "mapq values", len(np.unique(info["mapq"])))
    assert (int((p.plain["ext"] != 0).sum()), len(p.plain["ext"])) == (2249, 6640)
    assert tr.cnt["secondary"] == 346 and tr.cnt["sub_n"] == 163 and len(np.unique(info["mapq"])) == 33
    assert tr.cnt["drop_p"] + tr.cnt["drop_q"] + tr.cnt["patch_tried"] == 0
    assert tr.margin >= 1e-6


def _all_branches():
    tot = sp.Counter()
    margin = 1.0
    runs = [pipe_set("dispersed").want[4], pipe_set("seeding").want[4], hand_want()[4][4], hand_want(patch=0)[4][4],
            hand_want(mask_level_redun=1.0)[4][4], hand_want(mapQ_coef_len=0)[4][4]]
    for tr in runs:
        tot.update(tr.cnt)
        margin = min(margin, tr.margin)
    return tot, margin


def test_combined_batches_reach_every_branch_with_margin():
    tot, margin = _all_branches()
    print("branches:", dict(tot), "margin", margin)
    assert all(tot[k] > 0 for k in sp.BRANCHES), {k: tot[k] for k in sp.BRANCHES}
    for which in ("dispersed", "seeding"):
        tr = pipe_set(which).want[4]
        assert tr.cnt["drop_p"] > 0 and tr.cnt["drop_q"] > 0 and tr.cnt["patch_ok"] > 0 and tr.cnt["patch_ratio"] > 0
        assert tr.cnt["mapq_frac_rep"] > 0 and tr.rounds == 2
    assert margin >= 1e-6


# ---------------------------------------------------------------- CPU: the header
def test_library_exports_the_sel_header():
    assert declared("bsw_sel.h") == set(bsw.SEL_SYMBOLS)
    assert declared("bsw_sel.h") <= exported(), declared("bsw_sel.h") - exported()
    assert not set(bsw.SEL_SYMBOLS) & set(bsw.ABI_SYMBOLS) and not set(bsw.SEL_SYMBOLS) & set(bsw.ALN_SYMBOLS)
    import hashlib
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8
    assert hashlib.sha256(" ".join(bsw.ABI_SYMBOLS).encode()).hexdigest()[:16] == "5e89056d442d8f6f"


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_sel_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_sel.h"\n'
                   f"{sa}(sizeof(bsw_sel_opt_t) == 56 && offsetof(bsw_sel_opt_t, l_pac) == 8, \"opt\");\n"
                   f"{sa}(offsetof(bsw_sel_opt_t, mask_level) == 20 && offsetof(bsw_sel_opt_t, id0) == 48, \"opt\");\n"
                   f"{sa}(sizeof(bsw_selinfo_t) == 36 && offsetof(bsw_selinfo_t, frac_rep) == 32, \"info\");\n"
                   f"{sa}(sizeof(bsw_sel_stats_t) == 48 && offsetof(bsw_sel_stats_t, dp_ms) == 40, \"stats\");\n"
                   f"{sa}(BSW_SEL_API == 1 && BSW_ABI_VERSION == 8, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.SelOpt) == 56 and bsw.SelOpt.l_pac.offset == 8 and bsw.SelOpt.id0.offset == 48
    assert bsw.SelOpt.mask_level.offset == 20 and ctypes.sizeof(bsw.SelStats) == 48 and bsw.SelStats.dp_ms.offset == 40
    assert bsw.SELINFO_DTYPE == sp.SELINFO_DTYPE and bsw.SELINFO_DTYPE.itemsize == 36


def test_defaults_and_invalid_arguments_need_no_device():
    o = bsw.sel_opt()
    got = {f: getattr(o, f) for f, _ in o._fields_ if f != "reserved"}
    want = dict(sp.DEFAULT_OPT)
    assert {k: (round(v, 6) if isinstance(v, float) else v) for k, v in got.items()} == want
    L = bsw.hip_lib()
    n = ctypes.c_int32(0)
    args = [None] * 3 + [0] + [None] * 5 + [0] + [None] * 6 + [0]
    assert L.bsw_regs_select(None, None, *args, ctypes.byref(n)) == -22
    assert L.bsw_regs_select_resident(None, ctypes.byref(o), *args, ctypes.byref(n), None) == -22
    assert L.bsw_sel_last_stats(None, None) == -22


# ---------------------------------------------------------------- GPU
def _gpu_select(eng, arr, opt, scoring=DEFAULT, **kw):
    o = bsw.sel_opt(**{k: v for k, v in opt.items()})
    return bsw.regs_select(eng, arr["reads"], arr["off"], arr["lens"], arr["seeds"], arr["sr"], arr["sc"], arr["regs"],
                           arr["ext"], o, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", SCORINGS)
def test_gpu_hand_built_reads(scoring):
    a, b, od, ed, oi, ei = scoring
    eng = bsw.Engine(bsw.default_params(a=a, b=b, o_del=od, e_del=ed, o_ins=oi, e_ins=ei))
    for patch in (1, 0):
        T, bt, arr, opt, want = hand_want(patch=patch, scoring=scoring)
        bsw.set_reference(eng, T)
        got = _gpu_select(eng, arr, opt)
        st = bsw.sel_last_stats(eng)
        same_sel(want, got, f"hand-built {scoring} patch={patch}", st)
        assert st.n_reads == len(arr["lens"]) and (st.dp_ms > 0) == (st.rounds > 0) and st.helper_ms > 0
    if scoring == DEFAULT:
        for kw in (dict(mask_level_redun=1.0), dict(mapQ_coef_len=0), dict(id0=1 << 40), dict(max_chain_gap=100)):
            T, bt, arr, opt, want = hand_want(**kw)
            same_sel(want, _gpu_select(eng, arr, opt), f"hand-built {kw}", bsw.sel_last_stats(eng))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dispersed", "seeding"])
def test_gpu_pipeline_set_host_arrays(which):
    p = pipe_set(which)
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    got = _gpu_select(eng, p.full, p.opt, csub=p.csub, frac_rep=p.full_frac)
    same_sel(p.want, got, which, bsw.sel_last_stats(eng))
    got = _gpu_select(eng, p.plain, p.opt)
    same_sel(p.want_plain, got, which + " plain", bsw.sel_last_stats(eng))
    assert bsw.sel_last_stats(eng).rounds == 0 and bsw.sel_last_stats(eng).dp_ms == 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dispersed", "seeding"])
def test_gpu_pipeline_set_device_to_device(which):
    """bsw_chain2aln_resident's buffers -> bsw_regs_select_resident -> bsw_reg2aln_resident"""
    p = pipe_set(which)
    a = p.plain
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"])
    b.put(seeds=a["seeds"], sr=a["sr"], sc=a["sc"])
    b.chain2aln(p.eopt)
    k = b.select(bsw.sel_opt(l_pac=p.l_pac))
    wr = p.want_plain[0]
    assert k == len(wr)
    same_sel(p.want_plain, fetch(b, *b.lists[0]), which + " device to device", bsw.sel_last_stats(eng))
    b.reg2aln(p.eopt)
    aln = got_aln(b)
    mat, gaps = mat_gaps(DEFAULT)
    sel = np.zeros(k, dtype=bsw.ALNREG_DTYPE)
    for f in REG_FIELDS:
        sel[f] = wr[f]
    same_aln(rp.reg2aln(p.T, p.l_pac, a["reads"], a["off"], a["lens"], sel, p.want_plain[1], mat, gaps, p.eopt.w), aln,
             which + ": alignments of the survivors")
    eng.close()


def _first_reads(arr, nr):
    m = arr["sr"] < nr
    out = {k: arr[k][m] for k in ("seeds", "sr", "sc", "regs", "ext")}
    out.update(reads=arr["reads"][:int(arr["lens"][:nr].sum())], off=arr["off"][:nr], lens=arr["lens"][:nr])
    return out, m


@pytest.mark.gpu
def test_gpu_batch_sizes():
    p = pipe_set("seeding")
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    wr, wrd, wi, wf, tr = p.want
    for nr in (0, 1, 63, 64, 65, 257):
        sub, m = _first_reads(p.full, nr)
        got = _gpu_select(eng, sub, p.opt, csub=p.csub[m], frac_rep=p.full_frac[:nr])
        k = wf[nr]
        same_sel((wr[:k], wrd[:k], wi[:k], wf[:nr + 1], tr), got, f"n_reads={nr}")
        assert bsw.sel_last_stats(eng).n_reads == nr and bsw.sel_last_stats(eng).n_sel == k
    eng.close()


def _fuzz_read(b, T, s, k, rng, name):
    regs = []
    for _ in range(k):
        qb = int(rng.integers(0, 100))
        ln = int(rng.integers(30, 152 - qb))
        rb = s + qb + int(rng.integers(-20, 21))
        re_ = rb + ln + int(rng.integers(-3, 4))
        regs.append((qb, qb + ln, rb, re_, int(rng.integers(20, ln + 1)), int(rng.choice([0, 5, 100]))))
    for i in range(2, k, 5):                                   # tied re
        g = regs[i]
        regs[i] = (*g[:3], regs[i - 1][3] if regs[i - 1][3] > g[2] else g[3], *g[4:])
    b.add(name, T[s:s + 151], regs)


@pytest.mark.gpu
def test_gpu_regions_per_read():
    T = small_text()
    rng = np.random.default_rng(11)
    mixed, ones, twos = Batch(), Batch(), Batch()
    for rep in range(6):
        for k in (0, 1, 2, 16, 17, 46):
            _fuzz_read(mixed, T, 400 + 150 * rep, k, rng, f"fuzz{k}")
    for i in range(130):
        _fuzz_read(ones, T, 300 + 13 * i, 1, rng, "one")
    three = [c for c in hand_cases(T) if c[0] == "three_pieces"][0]
    for i in range(70):
        twos.add(*three)
    eng = bsw.Engine()
    bsw.set_reference(eng, T)
    opt = sp.sel_opt(l_pac=len(T) // 2)
    for tag, b in (("mixed", mixed), ("one region each", ones), ("two rounds each", twos)):
        arr = b.arrays()
        want = _select(T, arr, opt=opt)
        got = _gpu_select(eng, arr, opt)
        st = bsw.sel_last_stats(eng)
        same_sel(want, got, tag, st)
        if tag == "mixed":
            c = want[4].cnt
            assert c["drop_p"] > 10 and c["drop_q"] > 10 and c["patch_dp"] > 10 and c["patch_ok"] > 0 and c["secondary"] > 10, c
            assert want[4].margin >= 1e-6
        if tag == "one region each":
            assert (st.rounds, st.n_patch_tried, st.n_regs_in, st.n_sel) == (0, 0, 130, 130)
        if tag == "two rounds each":
            assert (st.rounds, st.n_dp, st.n_patch_ok, st.n_sel) == (2, 140, 140, 70)
    eng.close()


@pytest.mark.gpu
def test_gpu_errors_and_recovery():
    T, bt, arr, opt, want = hand_want()
    eng = bsw.Engine()
    with pytest.raises(bsw.BswError, match="-22"):            # no resident reference
        _gpu_select(eng, arr, opt)
    bsw.set_reference(eng, T)
    with pytest.raises(bsw.BswError, match="-22"):            # l_pac does not fit the resident text
        _gpu_select(eng, arr, dict(opt, l_pac=opt["l_pac"] - 1))
    need = len(want[0])
    with pytest.raises(bsw.BswError, match="-34") as ei:
        _gpu_select(eng, arr, opt, sel_cap=need - 1)
    assert ei.value.needed == need
    same_sel(want, _gpu_select(eng, arr, opt, sel_cap=need), "sel_cap exact")
    for field, v in (("qe", 152), ("qb", -1), ("re", len(T) + 1), ("rb", -1)):
        bad = dict(arr, regs=arr["regs"].copy())
        bad["regs"][0][field] = v
        with pytest.raises(bsw.BswError, match="-34"):
            _gpu_select(eng, bad, opt)
    for sr in (np.where(np.arange(len(arr["sr"])) == 3, len(arr["lens"]), arr["sr"]), arr["sr"][::-1]):
        with pytest.raises(bsw.BswError, match="-34"):
            _gpu_select(eng, dict(arr, sr=np.ascontiguousarray(sr, dtype=np.int32)), opt)
    T2, arr2, opt2 = long_span_batch()
    bsw.set_reference(eng, T2)
    with pytest.raises(bsw.BswError, match="-34"):            # a patch span above BSW_MAX_LEN
        _gpu_select(eng, arr2, opt2)
    assert len(_gpu_select(eng, arr2, dict(opt2, w=100))[0]) == 2
    eng.close()
    eng = bsw.Engine()                                        # fresh slots: the first growth is this call's
    bsw.set_reference(eng, T)
    try:
        eng.set_option("test_fail_alloc", 1)
        with pytest.raises(bsw.BswError, match="-12"):
            _gpu_select(eng, arr, opt)
    finally:
        eng.set_option("test_fail_alloc", 0)
    same_sel(want, _gpu_select(eng, arr, opt), "after a failed growth", bsw.sel_last_stats(eng))
    eng.close()
