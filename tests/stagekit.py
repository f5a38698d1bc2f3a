"""What the stage tests (reg2aln, regsel, pe, matesw, rec, contigs, resident) share: the scorings, the engine
of a scoring, the header / export checks, and the comparators of each stage's outputs against its restatement.
A plain module, not a test."""

import os
import re
import subprocess

import numpy as np

import bsw
import matesw_py as mp
import pe_py as pp
import rec_py as rq
import reg2aln_py as rp
import regsel_py as sp
from conftest import ROOT
from ksw_ext_ref import bwa_fill_scmat

DEFAULT = (1, 4, 6, 1, 6, 1)
SCORINGS = [DEFAULT, (1, 3, 5, 2, 3, 1), (2, 5, 0, 1, 1, 2)]
REG_FIELDS = sp.ALNREG_FIELDS


def revcomp(codes):
    c = np.asarray(codes, dtype=np.uint8)
    return np.where(c < 4, 3 - c, c)[::-1].astype(np.uint8)


def mat_gaps(scoring):
    a, b, od, ed, oi, ei = scoring
    return [int(v) for v in bwa_fill_scmat(a, b)], (od, ed, oi, ei)


def engine_of(scoring=DEFAULT):
    a, b, od, ed, oi, ei = scoring
    return bsw.Engine(bsw.default_params(a=a, b=b, o_del=od, e_del=ed, o_ins=oi, e_ins=ei))


# ---------------------------------------------------------------- the headers
def declared(header):
    """the functions include/<header> declares"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(bsw_[a-z_0-9]+)\s*\(", src))


def exported():
    """the functions the library exports"""
    out = subprocess.run(["nm", "-D", "--defined-only", bsw.HIP_LIB], capture_output=True, text=True).stdout
    return set(re.findall(r" T (bsw_\w+)", out))


# ---------------------------------------------------------------- comparators
def same_aln(want, got, tag):
    wa, wc, wm = want[:3]
    ga, gc, gm = got
    assert len(wa) == len(ga)
    ovf = wa["n_cigar"] < 0
    for f in bsw.ALN_DTYPE.names:
        m = np.ones(len(wa), bool) if f in ("score", "w", "n_pass", "flags") else ~ovf
        bad = np.flatnonzero((wa[f] != ga[f]) & m)
        assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} regions, first {bad[:5]}: want {wa[f][bad[:5]]} got {ga[f][bad[:5]]}"
    keep = np.arange(wc.shape[1])[None, :] < np.where(ovf, 0, wa["n_cigar"])[:, None]
    bad = np.flatnonzero(((wc != gc) & keep).any(axis=1))
    assert len(bad) == 0, f"{tag}: CIGAR differs at {len(bad)} regions, first {bad[:5]}: want {wc[bad[:1]]} got {gc[bad[:1]]}"
    if wm is not None:
        keep = np.arange(wm.shape[1])[None, :] < np.where(ovf, 0, np.maximum(wa["md_len"], 0))[:, None]
        bad = np.flatnonzero(((wm != gm) & keep).any(axis=1))
        assert len(bad) == 0, f"{tag}: MD differs at {len(bad)} regions, first {bad[:5]}: want {bytes(wm[bad[0]])} got {bytes(gm[bad[0]])}"
    else:
        assert gm is None


def same_sel(want, got, tag, st=None):
    wr, wrd, wi, wf, tr = want
    gr, grd, gi, gf = got
    assert np.array_equal(wf, gf), f"{tag}: read offsets differ, first at read {np.flatnonzero(wf != gf)[:5]}"
    assert len(wr) == len(gr), f"{tag}: n_sel {len(gr)}, want {len(wr)}"
    assert np.array_equal(wrd, grd), f"{tag}: sel_read differs"
    for f in REG_FIELDS:
        bad = np.flatnonzero(wr[f] != gr[f])
        assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} regions, first {bad[:5]}: want {wr[f][bad[:5]]} got {gr[f][bad[:5]]}"
    for f in bsw.SELINFO_DTYPE.names:
        bad = np.flatnonzero(wi[f] != gi[f])
        assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} regions, first {bad[:5]}: want {wi[f][bad[:5]]} got {gi[f][bad[:5]]}"
    if st is not None:
        for k, v in sp.stats_of(tr).items():
            assert getattr(st, k) == v, f"{tag}: stats {k} = {getattr(st, k)}, want {v}"
        assert st.n_sel == len(wr)


def same_pes(want, got, tag):
    for f in ("low", "high", "failed", "n"):
        assert np.array_equal(want[f], got[f]), f"{tag}: {f} {got[f]}, want {want[f]}"
    for f in ("avg", "std"):
        for d in range(4):
            assert abs(got[d][f] - want[d][f]) <= 1e-10 * abs(want[d][f]), f"{tag}: {f}[{d}] {got[d][f]!r}, want {want[d][f]!r}"


def same_pair(want, got, tag, st=None):
    wr, wi, wp, tr = want
    gr, gi, gp = got
    assert len(wr) == len(gr) and len(wp) == len(gp), tag
    for f in bsw.PAIR_DTYPE.names:
        diff = wp[f] != gp[f]
        bad = np.flatnonzero(diff.any(axis=1) if diff.ndim > 1 else diff)
        assert len(bad) == 0, f"{tag}: pair.{f} differs at {len(bad)} pairs, first {bad[:5]}: want {wp[f][bad[:5]]} got {gp[f][bad[:5]]}"
    for f in sp.ALNREG_FIELDS:
        bad = np.flatnonzero(wr[f] != gr[f])
        assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} regions, first {bad[:5]}: want {wr[f][bad[:5]]} got {gr[f][bad[:5]]}"
    for f in bsw.SELINFO_DTYPE.names:
        bad = np.flatnonzero(wi[f] != gi[f])
        assert len(bad) == 0, f"{tag}: info.{f} differs at {len(bad)} regions, first {bad[:5]}: want {wi[f][bad[:5]]} got {gi[f][bad[:5]]}"
    if st is not None:
        for k, v in pp.stats_of(tr, len(wp)).items():
            assert getattr(st, k) == v, f"{tag}: stats {k} = {getattr(st, k)}, want {v}"
        assert st.kernel_ms > 0 or len(wp) == 0


def same_msw(want, got, tag, st=None):
    wr, wd, wi, wf, tr = want
    gr, gd, gi, gf = got
    assert np.array_equal(wf, gf), f"{tag}: first differs at {np.flatnonzero(wf != gf)[:5]}: want {wf[:12]} got {gf[:12]}"
    assert len(wr) == len(gr), tag
    assert np.array_equal(wd, gd), f"{tag}: reg_read"
    for f in sp.ALNREG_FIELDS:
        bad = np.flatnonzero(wr[f] != gr[f])
        assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} regions, first {bad[:5]}: want {wr[f][bad[:5]]} got {gr[f][bad[:5]]}"
    for f in bsw.SELINFO_DTYPE.names:
        bad = np.flatnonzero(wi[f] != gi[f])
        assert len(bad) == 0, f"{tag}: info.{f} differs at {len(bad)} regions, first {bad[:5]}: want {wi[f][bad[:5]]} got {gi[f][bad[:5]]}"
    if st is not None:
        for k, v in mp.stats_of(tr, (len(wf) - 1) // 2, len(wr)).items():
            assert getattr(st, k) == v, f"{tag}: stats {k} = {getattr(st, k)}, want {v}"
        assert (st.sw_ms > 0) == (tr.cnt["jobs"] > 0), tag


def same_records(w, got, tag, st=None):
    recs, first, aln, aln_reg, cig, md = got
    assert np.array_equal(w.rec_first, first), f"{tag}: rec_first"
    assert len(recs) == len(w.recs) and len(aln) == len(w.aln), f"{tag}: counts {len(recs)} {len(aln)}, want {len(w.recs)} {len(w.aln)}"
    for f in rq.REC_DTYPE.names:
        bad = np.flatnonzero(w.recs[f] != recs[f])
        assert len(bad) == 0, f"{tag}: rec.{f} differs at {len(bad)} records, first {bad[:5]}: want {w.recs[f][bad[:5]]} got {recs[f][bad[:5]]}"
    assert np.array_equal(w.aln_reg, aln_reg), f"{tag}: aln_reg"
    for f in rp.ALN_DTYPE.names:
        bad = np.flatnonzero(w.aln[f] != aln[f])
        assert len(bad) == 0, f"{tag}: aln.{f} differs at {len(bad)} alignments, first {bad[:5]}: want {w.aln[f][bad[:5]]} got {aln[f][bad[:5]]}"
    assert np.array_equal(w.cigar, cig), f"{tag}: cigar at {np.flatnonzero((w.cigar != cig).any(axis=1))[:5]}"
    assert np.array_equal(w.md, md), f"{tag}: md at {np.flatnonzero((w.md != md).any(axis=1))[:5]}"
    if st is not None:
        for k, v in rq.stats_of(w).items():
            assert getattr(st, k) == v, f"{tag}: stats {k} = {getattr(st, k)}, want {v}"


def same_text(text, toff, got, tag):
    gt, go = got
    assert np.array_equal(toff, go), f"{tag}: text_off differs at {np.flatnonzero(toff != go)[:5]}"
    if gt != text:
        k = next(i for i in range(min(len(gt), len(text))) if gt[i] != text[i])
        r = int(np.searchsorted(toff, k, side="right")) - 1
        raise AssertionError(f"{tag}: text differs at byte {k} (record {r}): want {text[toff[r]:toff[r + 1]]!r} got {gt[toff[r]:toff[r + 1]]!r}")
    assert len(gt) == len(text), tag


# ---------------------------------------------------------------- what a ResidentBatch holds, in the comparators' order
RECORDS = ("recs", "rec_first", "aln", "aln_reg", "cigar", "md")


def fetch(b, *names):
    """downloads, e.g. fetch(b, *b.lists[0]): the current (regs, read, info, first); fetch(b, *RECORDS)"""
    return tuple(b.get(x) for x in names)


def got_aln(b, into="aln"):
    pre = into[:-len("aln")]
    return fetch(b, into, pre + "cigar", pre + "md")


def got_pair(b):
    regs, _, info, _ = b.lists[0]
    return fetch(b, regs, info, "pairs")


def got_text(b):
    return b.get("text").tobytes(), b.get("text_off")
