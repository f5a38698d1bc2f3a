"""Final alignments (include/bsw_aln.h): regions -> position, CIGAR, NM, MD, upstream's
mem_reg2aln -> bwa_gen_cigar2 per reported alignment.

CPU: hand-built regions with known answers through the Python restatement (tests/reg2aln_py.py;
its DP is the oracle's ksw_global2, cross-checked here against the band-matrix formulation of
tests/ksw_global_py.py), the header's symbols and struct layouts.
GPU: bsw_reg2aln / bsw_reg2aln_resident == the Python restatement field for field, and for
regions without overflow CIGAR word for word and MD byte for byte.  Parity is unpinned by the
reference tree (it holds no source of these functions; bsw_aln.h restates them).
"""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bsw
import oracle
import ksw_global_py as kg
import reg2aln_py as rp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import DEFAULT, SCORINGS, declared, exported, got_aln, mat_gaps, revcomp, same_aln

LET = "ACGTN"


def _reg(qb, qe, rb, re, truesc, w=100):
    r = np.zeros(1, dtype=bsw.ALNREG_DTYPE)[0]
    r["qb"], r["qe"], r["rb"], r["re"], r["truesc"], r["w"], r["score"] = qb, qe, rb, re, truesc, w, truesc
    return r


def _mirror(read, reg, l_pac):
    """the same alignment seen from the other strand"""
    l = len(read)
    return revcomp(read), _reg(l - reg["qe"], l - reg["qb"], 2 * l_pac - reg["re"], 2 * l_pac - reg["rb"],
                               reg["truesc"], reg["w"])


class Hand:
    """The hand-built recipes on a random 2.5 kb reference and its two-strand text."""

    def __init__(self, seed=4):
        rng = np.random.default_rng(seed)
        self.ref = ref = rng.integers(0, 4, 2500).astype(np.uint8)
        ref[2039] = (ref[2029] + 1) % 4                        # (del10_ins10's deletion cannot shift left)
        self.l_pac = L = len(ref)
        self.T = np.concatenate([ref, revcomp(ref)])
        c = {}
        exact = ref[500:560].copy()
        c["exact"] = (exact, _reg(0, 60, 500, 560, 60))
        c["lead2"] = (exact, _reg(0, 60, 498, 560, 52))
        c["trail2"] = (exact, _reg(0, 60, 500, 562, 52))
        rc = np.concatenate([[(ref[559] + 1) % 4, 1, 2], revcomp(exact), [0, (ref[500] + 2) % 4]]).astype(np.uint8)
        c["rev_clipped"] = (rc, _reg(3, 63, 2 * L - 560, 2 * L - 500, 60))
        d3 = np.concatenate([ref[1000:1030], ref[1033:1070]])
        d3[50] = (d3[50] + 1) % 4
        c["del3"] = (d3, _reg(0, 67, 1000, 1070, 53))
        c["del3_mirror"] = _mirror(*c["del3"], L)
        gf = ref[1500:1560].copy()
        gf[10] = 4
        gf[40] = (gf[40] + 1) % 4
        c["rev_gapfree_n"] = _mirror(gf, _reg(0, 60, 1500, 1560, 53), L)
        c["del3_overstated"] = (d3, _reg(0, 67, 1000, 1070, 61))
        R = ref[2000:2110]
        ins = (R[69:79] + 1 + np.arange(10) % 2) % 4          # unlike the bases either side of it
        di = np.concatenate([R[:30], R[40:79], ins, R[79:]]).astype(np.uint8)
        assert len(di) == 110
        c["del10_ins10"] = (di, _reg(0, 110, 2000, 2110, 98))
        d8 = np.concatenate([ref[1200:1230], ref[1238:1268]])
        c["del8"] = (d8, _reg(0, 60, 1200, 1268, 46))
        c["del3_wreg7"] = (d3, _reg(0, 67, 1000, 1070, 53, w=7))
        c["straddle"] = (exact, _reg(0, 60, L - 30, L + 30, 60))
        c["empty_span"] = (exact, _reg(0, 60, 500, 500, 60))
        c["empty_query"] = (exact, _reg(20, 20, 500, 560, 60))
        c["unmapped"] = (exact, _reg(0, 60, -1, -1, 0))
        c["zeroed"] = (exact, np.zeros(1, dtype=bsw.ALNREG_DTYPE)[0])
        c["clip_fwd"] = (np.concatenate([[3, 3], exact, [0]]).astype(np.uint8), _reg(2, 62, 500, 560, 60))
        self.cases = c

    def batch(self, names=None, mirrors=False):
        """(reads, read_off, read_len, regs, reg_read, names) over the named recipes, optionally
        followed by every recipe's other-strand mirror"""
        items = [(n, *self.cases[n]) for n in (names or self.cases)]
        if mirrors:
            items += [(n + "~", *_mirror(rd, rg, self.l_pac)) for n, rd, rg in items
                      if rg["rb"] >= 0 and not (rg["rb"] < self.l_pac < rg["re"])]
        reads = np.concatenate([rd for _, rd, _ in items])
        lens = np.array([len(rd) for _, rd, _ in items], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        regs = np.array([rg for _, _, rg in items], dtype=bsw.ALNREG_DTYPE)
        return reads, off, lens, regs, np.arange(len(items), dtype=np.int32), [n for n, _, _ in items]


@pytest.fixture(scope="module")
def hand():
    return Hand()


def _one(hand, name, W=100, scoring=DEFAULT, dp=None, cigar_stride=16, md_stride=64):
    mat, gaps = mat_gaps(scoring)
    read, reg = hand.cases[name]
    kw = {"dp": dp} if dp else {}
    f, cg, md, br = rp.reg2aln_one(hand.T, hand.l_pac, read, reg, mat, gaps, W, cigar_stride, md_stride, **kw)
    return f, rp.cigar_str(cg), md.decode(), br


# ---------------------------------------------------------------- CPU: known answers
def test_exact_read_is_one_pass_without_dp(hand):
    f, cg, md, br = _one(hand, "exact")
    assert (f["n_pass"], f["flags"], cg, f["NM"], md, f["pos"], f["score"], f["w"]) == (1, rp.NODP, "60M", 0, "60", 500, 60, 0)
    assert "gapfree" in br and "dp" not in br


def test_leading_and_trailing_deletions_are_squeezed(hand):
    f, cg, md, br = _one(hand, "lead2")
    assert (f["score"], cg, f["pos"], f["NM"], md) == (52, "60M", 500, 0, "60") and "squeeze_lead" in br
    f, cg, md, br = _one(hand, "trail2")
    assert (f["score"], cg, f["pos"], f["NM"], md) == (52, "60M", 500, 0, "60") and "squeeze_trail" in br


def test_reverse_strand_region_with_clips(hand):
    f, cg, md, br = _one(hand, "rev_clipped")
    assert (cg, f["is_rev"], f["pos"], f["NM"], md) == ("2S60M3S", 1, 500, 0, "60")
    assert {"rev", "clip5", "clip3", "gapfree"} <= br


def test_deletion_and_substitution_and_the_mirrored_region(hand):
    f, cg, md, br = _one(hand, "del3")
    assert re.fullmatch(r"\d+M3D\d+M", cg) and f["NM"] == 4 and f["n_pass"] == 1 and f["score"] == 53
    assert re.fullmatch(r"\d+\^[ACGT]{3}\d+[ACGT]\d+", md), md
    m = re.fullmatch(r"(\d+)M3D(\d+)M", cg)
    y = 1000 + int(m.group(1))
    assert md.split("^")[1][:3] == "".join(LET[b] for b in hand.ref[y:y + 3])
    # the left-alignment property the reversal exists for: the other strand's view of the same
    # alignment gives the same forward-strand CIGAR, MD and position
    f2, cg2, md2, br2 = _one(hand, "del3_mirror")
    assert (cg2, md2, f2["pos"], f2["NM"], f2["score"]) == (cg, md, f["pos"], 4, 53) and f2["is_rev"] == 1


def test_gapfree_reverse_region_reports_forward_bases(hand):
    f, cg, md, br = _one(hand, "rev_gapfree_n")
    want = f"10{LET[hand.ref[1510]]}29{LET[hand.ref[1540]]}19"
    assert (f["NM"], md, cg, f["flags"], f["is_rev"], f["pos"]) == (2, want, "60M", rp.NODP, 1, 1500)


def test_band_loop_passes(hand):
    f, cg, md, br = _one(hand, "del3_overstated")
    assert f["n_pass"] == 2 and f["score"] == 53 and (f["w"], "pass2" in br) == (6, True)
    f, cg, md, br = _one(hand, "del10_ins10")
    assert (f["n_pass"], cg, f["w"], f["score"]) == (3, "30M10D39M10I31M", 32, 68) and "pass3" in br
    f, cg, md, br = _one(hand, "del8", W=2)
    assert f["n_pass"] == 1 and f["w"] == 8 and "cap_break" in br and "8D" in cg
    f, cg, md, br = _one(hand, "del3_wreg7", W=5)
    assert f["w"] == 7 and "min_w_reg" in br and f["score"] == 53


def test_rejected_regions(hand):
    for name in ("straddle", "empty_span", "empty_query", "unmapped", "zeroed"):
        f, cg, md, br = _one(hand, name)
        assert f == dict(pos=-1, is_rev=0, n_cigar=0, NM=-1, score=0, w=0, n_pass=1, md_len=0, flags=rp.REJECTED), name
        assert br == {"rejected"}
    with pytest.raises(ValueError):
        rp.reg2aln_one(hand.T, hand.l_pac, hand.cases["exact"][0], _reg(0, 61, 500, 561, 60), *mat_gaps(DEFAULT),
                       100, 16, 64)


def test_overflow_flags(hand):
    f, cg, md, br = _one(hand, "del3", cigar_stride=2)
    assert (f["n_cigar"], f["flags"], f["score"], f["n_pass"]) == (-1, rp.OVERFLOW, 53, 1)
    f, cg, md, br = _one(hand, "rev_clipped", cigar_stride=2)     # 60M fits, 2S60M3S does not
    assert f["n_cigar"] == -1 and f["flags"] == rp.OVERFLOW | rp.NODP
    f, cg, md, br = _one(hand, "del3", md_stride=4)
    assert (f["md_len"], f["flags"], f["n_cigar"], f["NM"]) == (-1, rp.OVERFLOW, 3, 4)
    f, cg, md, br = _one(hand, "del3", md_stride=0)
    assert (f["md_len"], f["flags"], md) == (0, 0, "")


def test_recipes_agree_under_the_band_matrix_dp(hand):
    """the same answers with the independent Python DP (tests/ksw_global_py.py) in place of the oracle"""
    for name, W in (("lead2", 100), ("del3", 100), ("del3_mirror", 100), ("del10_ins10", 100), ("del8", 2)):
        assert _one(hand, name, W) == _one(hand, name, W, dp=kg.ksw_global2), name


def _hand_reference(hand, scoring, W, cigar_stride=16, md_stride=64):
    mat, gaps = mat_gaps(scoring)
    b = hand.batch(mirrors=True)
    b[3]["truesc"] *= scoring[0]                 # (the recipes' truesc are in units of a = 1)
    return b, rp.reg2aln(hand.T, hand.l_pac, *b[:5], mat, gaps, W, cigar_stride, md_stride)


def test_hand_batch_reaches_every_branch(hand):
    tot = {k: 0 for k in rp.BRANCHES}
    for W in (100, 5, 2):
        _, want = _hand_reference(hand, DEFAULT, W)
        for k, v in rp.branch_counts(want[3]).items():
            tot[k] += v
    assert all(v > 0 for v in tot.values()), tot


# ---------------------------------------------------------------- CPU: the header
def test_library_exports_the_aln_header():
    assert declared("bsw_aln.h") == set(bsw.ALN_SYMBOLS)
    assert declared("bsw_aln.h") <= exported(), declared("bsw_aln.h") - exported()
    assert not set(bsw.ALN_SYMBOLS) & set(bsw.ABI_SYMBOLS)
    assert bsw.hip_lib().bsw_abi_version() == 8


def test_aln_header_layouts_compile(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "bsw_aln.h"\n'
                   "_Static_assert(sizeof(bsw_aln_t) == 40, \"aln\");\n"
                   "_Static_assert(offsetof(bsw_aln_t, n_cigar) == 12 && offsetof(bsw_aln_t, flags) == 36, \"aln\");\n"
                   "_Static_assert(sizeof(bsw_aln_stats_t) == 32, \"stats\");\n"
                   "_Static_assert(BSW_ALN_API == 1 && BSW_ABI_VERSION == 8, \"api\");\n")
    r = subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert bsw.ALN_DTYPE == rp.ALN_DTYPE and ctypes.sizeof(bsw.AlnStats) == 32
    assert (bsw.ALN_REJECTED, bsw.ALN_NODP, bsw.ALN_OVERFLOW) == (rp.REJECTED, rp.NODP, rp.OVERFLOW)


def test_invalid_arguments_need_no_device():
    L = bsw.hip_lib()
    assert L.bsw_reg2aln(None, None, None, None, None, 0, None, None, 0, None, None, 1, None, 0) == -22
    assert L.bsw_reg2aln_resident(None, None, None, None, None, 0, None, None, 0, None, None, 1, None, 0, None) == -22
    assert L.bsw_aln_last_stats(None, None) == -22


# ---------------------------------------------------------------- pipeline-shaped regions
class Pipeline:
    """~3,000 reads of 101 and 151 bp sampled from both strands of a 200 kb reference with
    substitutions, short indels and N bases (some reads random), one or two hand-placed exact
    seeds each, taken to regions by the oracle's mem_chain2aln.  The band loop's further passes
    answer a truesc the first pass's band cannot reach; these reads never produce one (infer_bw
    sizes the band from the very score deficit the extension found), so `extra` repeats a share
    of the regions with truesc raised by 5..12, upstream's case of an overestimated score."""

    def __init__(self, n_reads=3000, ref_len=200_000, seed=9):
        rng = np.random.default_rng(seed)
        ref = bsw.synth_reference(ref_len, seed=21)
        self.l_pac = ref_len
        self.T = T = np.concatenate([ref, revcomp(ref)])
        reads, lens, seeds, sr = [], [], [], []
        for i in range(n_reads):
            L = 101 if i % 2 else 151
            strand = int(rng.integers(0, 2))
            start = int(rng.integers(0, ref_len - L - 100)) + strand * ref_len
            rd, tpos, t = [], [], start
            noisy = rng.random() < 0.5
            while len(rd) < L:
                u = rng.random()
                if noisy and u < 0.012:
                    rd.append((int(T[t]) + int(rng.integers(1, 4))) % 4 if T[t] < 4 else 0); tpos.append(-1); t += 1
                elif noisy and u < 0.015:
                    t += int(rng.integers(1, 4)) if rng.random() < 0.8 else int(rng.integers(4, 13))
                    tpos = tpos[:-1] + [-1] if tpos else tpos          # (no seed across the deletion)
                elif noisy and u < 0.018:
                    k = int(rng.integers(1, 4))
                    rd += [int(x) for x in rng.integers(0, 4, k)]; tpos += [-1] * k
                elif u < 0.020:
                    rd.append(4); tpos.append(-1); t += 1
                else:
                    rd.append(int(T[t])); tpos.append(t); t += 1
            rd, tpos = np.array(rd[:L], dtype=np.uint8), np.array(tpos[:L])
            if rng.random() < 0.05:                      # a random read around a 22-base copy
                keep = int(rng.integers(0, L - 22))
                ok = tpos[keep:keep + 22].copy()
                rd2 = rng.integers(0, 4, L).astype(np.uint8)
                rd2[keep:keep + 22] = rd[keep:keep + 22]
                rd, tpos2 = rd2, np.full(L, -1)
                tpos2[keep:keep + 22] = ok
                tpos = tpos2
            # maximal runs of bases copied from consecutive text positions
            runs, a = [], 0
            for k in range(1, L + 1):
                if k == L or tpos[k] < 0 or tpos[k - 1] < 0 or tpos[k] != tpos[k - 1] + 1:
                    if tpos[a] >= 0 and k - a >= 19:
                        runs.append((a, k))
                    a = k
            runs.sort(key=lambda r: r[0] - r[1])
            for (a, k) in sorted(runs[:2]):
                ln = min(k - a, int(rng.integers(19, 45)))
                seeds.append((int(tpos[a]), a, ln)); sr.append(i)
            reads.append(rd); lens.append(L)
        self.reads = np.concatenate(reads)
        self.lens = np.array(lens, dtype=np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int64)
        self.seeds = np.array(seeds, dtype=[("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")]).view(bsw.SEED_DTYPE)
        self.sr = np.array(sr, dtype=np.int32)
        self.sc = np.zeros(len(sr), dtype=np.int32)
        self.opt = bsw.ext_opt(l_pac=ref_len)
        self.mat, self.gaps = mat_gaps(DEFAULT)
        self.regs, self.ext = oracle.chain2aln(oracle.make_params(), self.opt, T, self.reads, self.off, self.lens,
                                               self.seeds, self.sr, self.sc)
        pick = np.flatnonzero(self.ext)[::25]
        extra = self.regs[pick].copy()
        extra["truesc"] += rng.integers(5, 13, len(pick)).astype(np.int32)
        self.all_regs = np.concatenate([self.regs, extra])
        self.all_read = np.concatenate([self.sr, self.sr[pick]])
        self.n_chain = len(self.regs)
        self.want = rp.reg2aln(T, self.l_pac, self.reads, self.off, self.lens, self.all_regs, self.all_read, self.mat,
                               self.gaps, self.opt.w)

    def subset(self, idx):
        aln, cig, md, br = self.want
        return aln[idx], cig[idx], md[idx], [br[i] for i in idx]


_pipeline = None


@pytest.fixture()
def pipe():
    global _pipeline
    if _pipeline is None:
        _pipeline = Pipeline()
    return _pipeline


def _pipe_conditions(p):
    cnt = rp.branch_counts(p.want[3])
    n = len(p.all_regs)
    assert cnt["fwd"] > 0.2 * n and cnt["rev"] > 0.2 * n, cnt
    assert cnt["gapfree"] > 0.2 * n and cnt["dp"] > 0.1 * n and cnt["pass2"] > 20 and cnt["rejected"] > 20, cnt
    assert (p.ext == 0).sum() > 20 and cnt["clip5"] > 0 and cnt["clip3"] > 0, cnt
    assert set(np.unique(p.lens)) == {101, 151}


def test_pipeline_set_holds_every_kind_of_region(pipe):
    _pipe_conditions(pipe)
    aln = pipe.want[0]
    ok = aln["n_cigar"] > 0
    assert ok.sum() > 0.5 * len(aln) and np.all(aln["pos"][ok] >= 0) and np.all(aln["pos"][ok] < pipe.l_pac)
    # reads without edits come back at their origin with their own length in M
    gf = np.flatnonzero(ok & (aln["NM"] == 0) & (aln["n_cigar"] == 1))
    assert len(gf) > 100 and all((int(pipe.want[1][k, 0]) >> 4) == pipe.lens[pipe.all_read[k]] for k in gf[:50])


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("scoring", SCORINGS)
def test_gpu_hand_built_regions(hand, scoring):
    a, b, od, ed, oi, ei = scoring
    refs = {W: _hand_reference(hand, scoring, W) for W in (100, 5, 2)}
    tot = {k: 0 for k in rp.BRANCHES}
    for _, want in refs.values():
        for k, v in rp.branch_counts(want[3]).items():
            tot[k] += v
    # under the default scoring the recipes reach every branch; the other scorings move the
    # thresholds the recipes' truesc were built around (infer_bw, the loop's truesc - a), so the
    # pass counts and the cap break are not required of them
    need = rp.BRANCHES if scoring == DEFAULT else ("rejected", "gapfree", "dp", "squeeze_lead", "squeeze_trail",
                                                   "clip5", "clip3", "fwd", "rev")
    if (od + ed - a) * 2 <= 0:       # infer_bw's zero needs l*a - truesc below this: out of reach of a
        need = [k for k in need if k != "gapfree"]   # truesc <= l*a, so such a scoring never skips the DP
    assert all(tot[k] > 0 for k in need), tot
    eng = bsw.Engine(bsw.default_params(a=a, b=b, o_del=od, e_del=ed, o_ins=oi, e_ins=ei))
    bsw.set_reference(eng, hand.T)
    for W, (bt, want) in refs.items():
        got = bsw.reg2aln(eng, *bt[:5], bsw.ext_opt(w=W, l_pac=hand.l_pac))
        same_aln(want, got, f"hand-built {scoring} W={W}")
        st = bsw.aln_last_stats(eng)
        cnt = rp.branch_counts(want[3])
        assert (st.n_regs, st.n_rejected, st.n_gapfree) == (len(bt[3]), cnt["rejected"], cnt["gapfree"])
        n_pass = want[0]["n_pass"][[("dp" in s) for s in want[3]]]
        assert list(st.n_dp) == [int((n_pass >= k).sum()) for k in (1, 2, 3)]
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_regions_host_arrays(pipe):
    _pipe_conditions(pipe)
    eng = bsw.Engine()
    bsw.set_reference(eng, pipe.T)
    got = bsw.reg2aln(eng, pipe.reads, pipe.off, pipe.lens, pipe.all_regs, pipe.all_read, pipe.opt)
    same_aln(pipe.want, got, "pipeline regions")
    st = bsw.aln_last_stats(eng)
    cnt = rp.branch_counts(pipe.want[3])
    assert (st.n_rejected, st.n_gapfree, st.n_dp[0]) == (cnt["rejected"], cnt["gapfree"], cnt["dp"])
    assert st.n_dp[1] > 0 and st.dp_ms > 0 and st.helper_ms > 0
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_device_to_device(pipe):
    """bsw_chain2aln_resident's output buffers go straight into bsw_reg2aln_resident"""
    p = pipe
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, p.reads, p.off, p.lens)
    b.put(seeds=p.seeds, sr=p.sr, sc=p.sc)
    n = len(p.seeds)
    b.chain2aln(p.opt)
    b.reg2aln(p.opt)
    got = got_aln(b)
    regs = b.get("regs")
    assert all(np.array_equal(regs[f], p.regs[f]) for f in bsw.ALNREG_DTYPE.names)
    same_aln(p.subset(np.arange(n)), got, "device to device")
    eng.close()


@pytest.mark.gpu
def test_gpu_batch_sizes_and_uniform_batches(pipe):
    p = pipe
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    br = p.want[3]
    kinds = {"gap-free": np.flatnonzero([("gapfree" in s) for s in br])[:300],
             "dp": np.flatnonzero([("dp" in s) for s in br])[:300],
             "rejected": np.flatnonzero([("rejected" in s) for s in br])[:70]}
    for nr in (1, 63, 64, 65, 257):
        kinds[f"n={nr}"] = np.arange(100, 100 + nr)
    kinds["empty"] = np.arange(0)
    for tag, idx in kinds.items():
        assert len(idx) > 0 or tag == "empty"
        got = bsw.reg2aln(eng, p.reads, p.off, p.lens, p.all_regs[idx], p.all_read[idx], p.opt)
        same_aln(p.subset(idx), got, tag)
        st = bsw.aln_last_stats(eng)
        assert st.n_regs == len(idx)
        if tag == "gap-free":
            assert st.n_gapfree == len(idx) and list(st.n_dp) == [0, 0, 0] and st.dp_ms == 0
        if tag == "dp":
            assert st.n_dp[0] == len(idx) and st.n_gapfree == 0
        if tag == "rejected":
            assert st.n_rejected == len(idx) and st.n_dp[0] == 0
    eng.close()


@pytest.mark.gpu
def test_gpu_long_read_takes_the_wide_global_kernel():
    rng = np.random.default_rng(12)
    ref = rng.integers(0, 4, 3000).astype(np.uint8)
    T, l_pac = np.concatenate([ref, revcomp(ref)]), len(ref)
    read = np.concatenate([ref[400:520], rng.integers(0, 4, 4).astype(np.uint8), ref[520:646]])
    assert len(read) == 250
    sub = np.array([10, 30, 50, 70, 90, 110, 140, 160, 180, 200, 220, 240])
    read[sub] = (read[sub] + 1) % 4
    # 234 matches, 12 substitutions, 4I: truesc 176 -> infer_bw 66 -> band 62: neither a band class
    # (2w + 2 <= 96) nor a column class (qlen <= 160) of the global kernels
    items = [(read, _reg(0, 250, 400, 646, 176))]
    items.append(_mirror(*items[0], l_pac))
    reads = np.concatenate([r for r, _ in items])
    off, lens = np.array([0, 250], np.int64), np.array([250, 250], np.int32)
    regs = np.array([g for _, g in items], dtype=bsw.ALNREG_DTYPE)
    mat, gaps = mat_gaps(DEFAULT)
    want = rp.reg2aln(T, l_pac, reads, off, lens, regs, [0, 1], mat, gaps, 100)
    assert rp.cigar_str(want[1][0, :want[0]["n_cigar"][0]]) == rp.cigar_str(want[1][1, :want[0]["n_cigar"][1]])
    assert "4I" in rp.cigar_str(want[1][0, :3]) and list(want[0]["w"]) == [66, 66] and list(want[0]["NM"]) == [16, 16]
    eng = bsw.Engine()
    bsw.set_reference(eng, T)
    got = bsw.reg2aln(eng, reads, off, lens, regs, [0, 1], bsw.ext_opt(l_pac=l_pac))
    same_aln(want, got, "250 bp")
    assert bsw.global_last_stats(eng).n_wide == 2
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cigar_stride,md_stride", [(2, 0), (2, 4), (3, 0), (3, 4)])
def test_gpu_overflow_flags(hand, cigar_stride, md_stride):
    bt, want = _hand_reference(hand, DEFAULT, 100, cigar_stride, md_stride)
    fl = want[0]["flags"]
    assert (fl & rp.OVERFLOW).any() and not (fl & rp.OVERFLOW).all()
    assert (want[0]["n_cigar"] == -1).any() and ((want[0]["md_len"] == -1).any() or md_stride == 0)
    eng = bsw.Engine()
    bsw.set_reference(eng, hand.T)
    got = bsw.reg2aln(eng, *bt[:5], bsw.ext_opt(l_pac=hand.l_pac), cigar_stride=cigar_stride, md_stride=md_stride)
    same_aln(want, got, f"strides {cigar_stride}, {md_stride}")
    eng.close()


@pytest.mark.gpu
def test_gpu_errors(hand):
    bt = hand.batch(["exact", "del3"])
    opt = bsw.ext_opt(l_pac=hand.l_pac)
    eng = bsw.Engine()
    with pytest.raises(bsw.BswError, match="-22"):            # no resident reference
        bsw.reg2aln(eng, *bt[:5], opt)
    bsw.set_reference(eng, hand.T)
    with pytest.raises(bsw.BswError, match="-22"):            # l_pac does not fit the resident text
        bsw.reg2aln(eng, *bt[:5], bsw.ext_opt(l_pac=hand.l_pac - 1))
    for field, v in (("qe", 61), ("qb", -1), ("re", 2 * hand.l_pac + 1)):
        regs = bt[3].copy()
        regs[0][field] = v
        if field == "re":
            regs[0]["rb"] = 2 * hand.l_pac - 59
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.reg2aln(eng, bt[0], bt[1], bt[2], regs, bt[4], opt)
    with pytest.raises(bsw.BswError, match="-34"):            # a read index outside the reads
        bsw.reg2aln(eng, bt[0], bt[1], bt[2], bt[3], np.array([0, 2], np.int32), opt)
    mat, gaps = mat_gaps(DEFAULT)
    want = rp.reg2aln(hand.T, hand.l_pac, *bt[:5], mat, gaps, 100)
    eng.close()
    eng = bsw.Engine()                                        # fresh slots: the first growth is this call's
    bsw.set_reference(eng, hand.T)
    try:
        eng.set_option("test_fail_alloc", 1)
        with pytest.raises(bsw.BswError, match="-12"):
            bsw.reg2aln(eng, *bt[:5], opt)
    finally:
        eng.set_option("test_fail_alloc", 0)
    same_aln(want, bsw.reg2aln(eng, *bt[:5], opt), "after a failed growth")
    eng.close()
