"""bsw_ksw_global2, one kernel class at a time (bsw_global.hip: five band kernels, five column
kernels, the wide kernel, and the narrow traceback corridor of the column kernels).

CPU tests pin tests/glob_plan_py.py -- a restatement of the planner (glob_class, glob_cap_dw) and of
the corridor rule -- and the INPUTS of the GPU tests: every class gets a full wave and a tail, every
class edge of qlen and w has a job on each side, the corridor batch retries between 20 % and 80 %
of its jobs.  GPU tests require the engine to equal oracle.ksw_global2_batch job for job (score, op
count, every CIGAR word), the class counts in the statistics to equal the planner's, and
n_tb_retry to equal the number of jobs whose oracle path leaves the corridor."""

import functools
import random

import numpy as np
import pytest

import bsw
import oracle
import glob_plan_py as gp
import ksw_global_py as kg
from test_global import _check, _engine
from test_mate_rescue import _random_batch as _mate_batch, _same as _mate_same

DEFAULT = (1, 4, 6, 1, 6, 1)
OTHER = (1, 3, 5, 2, 3, 1)
STRIDE = 512                               # no CIGAR of these tests has more ops (asserted per call)

Q_GRID = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 200)
W_GRID = (0, 3, 14, 15, 16, 22, 23, 24, 30, 31, 32, 38, 39, 40, 46, 47, 48, 60)
Q_EDGES = ((32, 33), (64, 65), (96, 97), (128, 129), (160, 161))
W_EDGES = ((15, 16), (23, 24), (31, 32), (39, 40), (47, 48))
# Two jobs per grid cell (qlen, w, d, kind): the sparsest class of a grid call is the wide one,
# qlen in {161, 200} x w in {48, 60} x 5 d x 3 kinds = 60 jobs, under the 65 of a wave and a tail
GRID_REPS = 2


@pytest.fixture(params=["column", "band"])
def routing(request):
    return request.param


def _params(scoring):
    a, b, od, ed, oi, ei = scoring
    return bsw.default_params(a=a, b=b, o_del=od, e_del=ed, o_ins=oi, e_ins=ei)


def _oracle(pairs, ref, qer, scoring, stride=STRIDE):
    od, ed, oi, ei = scoring[2:]
    return oracle.ksw_global2_batch(pairs, ref, qer, list(_params(scoring).mat), od, ed, oi, ei, stride=stride,
                                    nthreads=16)


# ---------------------------------------------------------------- job builders
def _pack(jobs):
    """[(query, target, w), ...] (uint8 arrays) -> (pairs, ref, qer)."""
    n = len(jobs)
    pairs = np.zeros(n, dtype=bsw.SEQPAIR_DTYPE)
    ql = np.array([len(j[0]) for j in jobs], dtype=np.int64)
    tl = np.array([len(j[1]) for j in jobs], dtype=np.int64)
    pairs["len2"], pairs["len1"] = ql, tl
    pairs["idq"] = np.concatenate(([0], np.cumsum(ql)[:-1]))
    pairs["idr"] = np.concatenate(([0], np.cumsum(tl)[:-1]))
    pairs["h0"] = [j[2] for j in jobs]
    pairs["id"] = np.arange(n)
    z = np.zeros(1, np.uint8)
    qer = np.concatenate([np.asarray(j[0], np.uint8) for j in jobs] + [z])
    ref = np.concatenate([np.asarray(j[1], np.uint8) for j in jobs] + [z])
    return pairs, ref, qer


def _seq(rng, n, codes=4):
    return rng.integers(0, codes, size=max(n, 0), dtype=np.uint8)


def _fit(rng, s, n):
    """s cut or padded with random bases to length n."""
    return s[:n] if len(s) >= n else np.concatenate([s, _seq(rng, n - len(s))])


def _target_of(rng, q, tlen, kind):
    """kind 0: unrelated (N bases allowed); 1: q with substitutions, a balanced indel pair and the
    net indel tlen - qlen at one place; 2: as 1 with a tenth of both sequences turned into N."""
    if kind == 0 or len(q) < 4:
        return q, _seq(rng, tlen, 5)
    t = q.copy()
    sub = rng.random(len(t)) < 0.04
    t[sub] = _seq(rng, int(sub.sum()))
    e = int(rng.integers(0, 4))
    a, b = len(t) // 4, 3 * len(t) // 4
    if rng.random() < 0.5:
        t = np.concatenate([t[:a], _seq(rng, e), t[a:b], t[b + e:]])
    else:
        t = np.concatenate([t[:a], t[a + e:b], _seq(rng, e), t[b:]])
    d = tlen - len(t)
    m = int(rng.integers(1, len(t)))
    t = np.concatenate([t[:m], _seq(rng, d), t[m:]]) if d >= 0 else np.concatenate([t[:m], t[m - d:]])
    t = _fit(rng, t, tlen)
    if kind == 2:
        q = q.copy()
        q[rng.random(len(q)) < 0.1] = 4
        t[rng.random(len(t)) < 0.1] = 4
    return q, t


@functools.lru_cache(maxsize=None)
def _grid():
    """The class grid: every qlen x w x d x kind, GRID_REPS jobs each, qlen >= tlen - w throughout."""
    rng = np.random.default_rng(20240)
    jobs = []
    for qlen in Q_GRID:
        for w in W_GRID:
            for d in (-9, -2, 0, min(w, 3), min(w, 11)):
                for kind in (0, 1, 2):
                    for _ in range(GRID_REPS):
                        q, t = _target_of(rng, _seq(rng, qlen), max(qlen + d, 0), kind)
                        jobs.append((q, t, w))
    return _pack(jobs)


def _class_job(rng, cls, rt):
    """(qlen, tlen, w) of a job that glob_class sends to `cls` under routing rt (default scoring)."""
    if cls < gp.LANE0:
        w = int(rng.integers((0, 16, 24, 32, 40)[cls], (16, 24, 32, 40, 48)[cls]))
        qlen = int(rng.integers(161, 221)) if rt == "column" else int(rng.integers(8, 221))
    else:
        w = int(rng.integers(48, 71)) if (rt == "band" or cls == gp.WIDE) else int(rng.integers(0, 71))
        lo, hi = ((1, 32), (33, 64), (65, 96), (97, 128), (129, 160), (161, 220))[cls - gp.LANE0]
        qlen = int(rng.integers(lo, hi + 1))
    return qlen, qlen + int(rng.integers(-min(8, qlen - 1), min(w, 8) + 1)), w


@functools.lru_cache(maxsize=None)
def _class_alone(cls, rt):
    rng = np.random.default_rng(300 + cls)
    jobs = []
    for j in range(65):
        qlen, tlen, w = _class_job(rng, cls, rt)
        q, t = _target_of(rng, _seq(rng, qlen), tlen, j % 3)
        jobs.append((q, t, w))
    return jobs


@functools.lru_cache(maxsize=None)
def _loose():
    """Random geometry with no fix-up of w: qlen < tlen - w (undefined, -2) and qlen > tlen + w (last
    column unreachable) both occur, in band, column and wide classes under either routing."""
    rng = np.random.default_rng(77)
    jobs = []
    for j in range(3000):
        qlen = int(rng.choice((rng.integers(1, 161), rng.integers(161, 221))))
        tlen = max(1, min(260, qlen + int(rng.integers(-60, 61))))
        w = int(rng.choice((0, 3, 10, 20, 35, 50, 70)))
        q, t = _target_of(rng, _seq(rng, qlen), tlen, j % 3)
        jobs.append((q, t, w))
    return _pack(jobs)


CORR_Q = (32, 64, 96, 128, 160)
CORR_DLT = (-18, -17, -16, -8, 0, 8, 16, 17, 18)
CORR_GAPS = (1, 4, 2, 1, 2, 1)


@functools.lru_cache(maxsize=None)
def _excursions():
    """Planted excursions: per column width, dlt = qlen - tlen and e = 0..13 a query made from its
    target by an e-base insertion at one third, the net indel dlt in the middle and an e-base
    deletion at two thirds -- and the mirror image of that job.  w = 40."""
    rng = np.random.default_rng(555)
    jobs = []
    for qlen in CORR_Q:
        for dlt in CORR_DLT:
            for e in range(14):
                t = _seq(rng, qlen - dlt)
                p1, pm, p2 = len(t) // 3, len(t) // 2, 2 * len(t) // 3
                mid = _seq(rng, dlt) if dlt > 0 else t[:0]
                q = np.concatenate([t[:p1], _seq(rng, e), t[p1:pm], mid, t[pm + max(-dlt, 0):p2],
                                    t[max(p2, pm + max(-dlt, 0)) + e:]])
                q = _fit(rng, q, qlen)
                jobs.append((q, t, 40))
                jobs.append((q[::-1].copy(), t[::-1].copy(), 40))
    return _pack(jobs)


I16 = (92, 92, 6, 1, 6, 1)
I16_BIG = (120, 120, 6, 1, 6, 1)


@functools.lru_cache(maxsize=None)
def _i16_edge():
    """qlen 159 against tlen 183 (bound 14999: int16 row) and 184 (15000: not), w 30 and 50; and the
    most negative score the int16 row meets, -14628 on the diagonal alone."""
    rng = np.random.default_rng(92)
    jobs = []
    for tlen in (183, 184):
        for w in (30, 50):
            for _ in range(20):
                q = _seq(rng, 159)
                jobs.append((q, np.concatenate([q, _seq(rng, tlen - 159)]), w))       # near +14628
                c = int(rng.integers(0, 4))                                         # no base matches
                jobs.append((np.full(159, c, np.uint8), ((c + 1 + _seq(rng, tlen, 3)) % 4).astype(np.uint8), w))
                qn, tn = _target_of(rng, q, tlen, 2)
                qn[rng.random(159) < 0.4] = 4                                       # N-rich
                jobs.append((qn, tn, w))
                m = int(rng.integers(10, 150))
                jobs.append((q, np.concatenate([q[:m], _seq(rng, tlen - 159), q[m:]]), w))   # one deletion
    # With gaps at 6 / 1 a path through the band zigzags round every mismatch, so the pairs without
    # a matching base above score about -900.  On the diagonal alone (w = 0, tlen = qlen = 159, bound
    # 14975: the int16 row under default routing) they score -14628.
    for _ in range(20):
        c = int(rng.integers(0, 4))
        jobs.append((np.full(159, c, np.uint8), ((c + 1 + _seq(rng, 159, 3)) % 4).astype(np.uint8), 0))
    return _pack(jobs)


@functools.lru_cache(maxsize=None)
def _i16_big():
    """Identical pairs of qlen 160 at a = 120: score 19200, beyond the planner's +-15000.  The int16
    row could still hold that value; what it cannot hold is a finite value below its -inf of -16384,
    so the batch also has pairs without a matching base at w = 0 (diagonal only): -19200."""
    rng = np.random.default_rng(120)
    jobs = []
    for w in (10, 20, 47, 50, 60):
        for _ in range(26):
            q = _seq(rng, 160)
            jobs.append((q, q.copy(), w))
    for _ in range(26):
        q = _seq(rng, 160)
        jobs.append((q, ((q + 1 + _seq(rng, 160, 3)) % 4).astype(np.uint8), 0))
    return _pack(jobs)


# ---------------------------------------------------------------- CPU: the restatement
# qlen of the grid -> column class (None: wider than every column kernel), written out by hand
COL_OF = {1: 5, 31: 5, 32: 5, 33: 6, 63: 6, 64: 6, 65: 7, 95: 7, 96: 7, 97: 8, 127: 8, 128: 8, 129: 9, 159: 9,
          160: 9, 161: None, 200: None}
# w of the grid -> band class (None: 2w + 2 slots exceed every band kernel)
BAND_OF = {0: 0, 3: 0, 14: 0, 15: 0, 16: 1, 22: 1, 23: 1, 24: 2, 30: 2, 31: 2, 32: 3, 38: 3, 39: 3, 40: 4, 46: 4,
           47: 4, 48: None, 60: None}


def test_class_table_at_the_edges():
    """Default scoring (every bound far below 15000): column routing takes the column kernel when
    qlen <= 160, else the band kernel when w <= 47, else the wide one; band routing takes the band
    kernel first."""
    p = _params(DEFAULT)
    for q in Q_GRID:
        for w in W_GRID:
            col, band = COL_OF[q], BAND_OF[w]
            for t in (q, q + min(w, 5), max(q - 7, 0)):
                want_c = col if col is not None else band if band is not None else 10
                want_b = band if band is not None else col if col is not None else 10
                assert gp.glob_class(q, t, w, p, 0) == want_c, (q, t, w)
                assert gp.glob_class(q, t, w, p, 1) == want_b, (q, t, w)
    assert gp.glob_class(-1, 5, 3, p, 0) == -1 and gp.glob_class(5, 1024, 3, p, 0) == -1
    assert gp.glob_class(1023, 1023, 3, p, 0) == 0 and gp.glob_class(5, 5, -1, p, 1) == -1


def test_cap_dw_and_narrow_window():
    assert [gp.cap_dw(c, 200, 60) for c in range(5)] == [4, 6, 8, 10, 12]
    # column classes: min(band window, QMAX / 8); the band window is ((2 wmax) >> 3) + 2 dwords
    assert [gp.cap_dw(c, 160, 40) for c in range(5, 10)] == [4, 8, 12, 12, 12]
    assert [gp.cap_dw(c, 160, 3) for c in range(5, 10)] == [2, 2, 2, 2, 2]
    assert gp.cap_dw(10, 200, 60) == 17 and gp.cap_dw(10, 161, 200) == 22
    # the 3-dword window is taken when the full one is wider: band window > 3 <=> wmax >= 8
    assert [gp.narrow_tb(5, w, 32) for w in (0, 7, 8, 40)] == [False, False, True, True]
    assert not gp.narrow_tb(4, 40, 200) and not gp.narrow_tb(10, 60, 200)
    # corridor slack: xs = (8 * 3 - 8 - |dlt|) / 2 truncated toward zero; room up to |dlt| = 17
    assert [gp.corridor(100, 100 - d)[0] for d in (0, 1, 16, 17, 18, 19, -17, -18)] == [8, 7, 0, 0, -1, -1, 0, -1]
    assert gp.corridor(100, 90) == (3, -3) and gp.corridor(90, 100) == (3, -13)


def test_int16_bound_values():
    p = _params(I16)
    assert gp.glob_bound(159, 183, p) == 14999 and gp.glob_bound(159, 184, p) == 15000
    assert gp.glob_class(159, 183, 50, p, 0) == 9 and gp.glob_class(159, 184, 50, p, 0) == 10
    assert gp.glob_class(159, 183, 30, p, 0) == 9 and gp.glob_class(159, 184, 30, p, 0) == 2
    assert gp.glob_class(159, 183, 30, p, 1) == 2 and gp.glob_class(159, 183, 50, p, 1) == 9
    pairs, _, _ = _i16_edge()
    assert set(pairs["len2"]) == {159} and set(pairs["len1"]) == {159, 183, 184}
    assert gp.glob_bound(159, 159, p) == 14975 and gp.glob_class(159, 159, 0, p, 0) == 9
    big = _params(I16_BIG)
    bp, _, _ = _i16_big()
    for rt in (0, 1):
        cls = gp.plan(bp, big, rt)[0]
        assert gp.WIDE in cls and 0 in cls and all(c < gp.LANE0 or c == gp.WIDE for c in cls)


@pytest.mark.parametrize("seed", range(2))
def test_path_walk_over_oracle_cigars(seed):
    """The walk rebuilt from the oracle's CIGAR stays inside the band, ends when a coordinate runs
    out, accounts for every base of the CIGAR, and its moves re-score to the oracle's score."""
    rnd = random.Random(40 + seed)
    rng = np.random.default_rng(40 + seed)
    n = 0
    for _ in range(100):
        qlen, w = rnd.randint(1, 70), rnd.choice((0, 1, 4, 9, 20, 40))
        tlen = max(1, qlen + rnd.randint(-min(w, 12) - 4, min(w, 12)))
        q, t = _target_of(rng, _seq(rng, qlen), tlen, rnd.randrange(3))
        a, b, od, ed, oi, ei = rnd.choice((DEFAULT, OTHER, CORR_GAPS))
        mat = list(_params((a, b, od, ed, oi, ei)).mat)
        sc, cig = oracle.ksw_global2(q, t, mat, od, ed, oi, ei, w)
        if gp.undefined_geometry(qlen, tlen, w):
            continue
        cells, (i, k) = gp.path_walk(cig, qlen, tlen, w)
        assert i < 0 or k < 0
        assert cells[0] == (tlen - 1, min(tlen + w, qlen) - 1)
        for ci, ck in cells:
            lo, hi = kg.band(ci, w, qlen)
            assert lo <= ck < hi, (ci, ck, w, qlen)
        assert sum(ln for _, ln in cig) == len(cells) + max(i + 1, 0) + max(k + 1, 0)
        if qlen <= tlen + w:                                   # (else the last column is unreachable)
            rs, ti, qj = kg.rescore(q, t, mat, od, ed, oi, ei, cig)
            assert (rs, ti, qj) == (sc, tlen, qlen)
            n += 1
    assert n > 60


def test_leaves_corridor_by_hand():
    # 100M on the main diagonal: xs = 8, the window of row i starts at dword (i - 8) >> 3
    assert not gp.leaves_corridor([(0, 100)], 100, 100, 40)
    # 8 columns right of the diagonal and back: cell (i, i + 8) is in dword (i + 8) >> 3, at most 2 past
    assert not gp.leaves_corridor([(0, 30), (1, 8), (0, 30), (2, 8), (0, 32)], 100, 100, 40)
    # 16 columns right: row 30 keeps dwords 2..4 and the walk reads column 46 (dword 5)
    assert gp.leaves_corridor([(0, 30), (1, 16), (0, 30), (2, 16), (0, 24)], 100, 100, 40)
    # 9 columns left: row 39 keeps dwords 3..5 (from column 31) and the walk reads column 30
    assert gp.leaves_corridor([(0, 30), (2, 9), (0, 30), (1, 9), (0, 31)], 100, 100, 40)
    assert gp.leaves_corridor([(0, 60), (1, 18)], 78, 60, 40)          # |dlt| = 18: no room, xs < 0
    assert not gp.leaves_corridor([], 10, 60, 5)                       # undefined geometry: never


def _coverage(pairs, params):
    out = {}
    for rt in (0, 1):
        cls, st = gp.plan(pairs, params, rt)
        out[rt] = (cls, st)
    return out


@pytest.mark.parametrize("scoring", [DEFAULT, OTHER])
def test_grid_covers_every_class_and_edge(scoring):
    pairs, _, _ = _grid()
    assert np.all(pairs["len2"] >= pairs["len1"] - pairs["h0"])
    p = _params(scoring)
    for rt, (cls, st) in _coverage(pairs, p).items():
        assert sorted(st) == list(range(gp.N_CLASSES)), (rt, sorted(st))
        assert min(v[0] for v in st.values()) >= 65, (rt, st)
        cls = np.array(cls)
        for lo, hi in Q_EDGES:                     # both sides of a column edge, each in its own class
            a, b = set(cls[pairs["len2"] == lo]), set(cls[pairs["len2"] == hi])
            ca, cb = gp.QMAX.index(lo) + gp.LANE0, gp.QMAX.index(lo) + gp.LANE0 + 1
            assert ca in a and ca not in b, (rt, lo)
            assert (cb in b and cb not in a) or hi == 161, (rt, hi)
            if hi == 161:
                assert not any(gp.LANE0 <= c < gp.WIDE for c in b) and gp.WIDE in b
        for lo, hi in W_EDGES:
            a, b = set(cls[pairs["h0"] == lo]), set(cls[pairs["h0"] == hi])
            ca = gp.BAND_W.index(2 * lo + 2)
            assert ca in a and ca not in b, (rt, lo)
            if hi == 48:
                assert not any(c < gp.LANE0 for c in b)
            else:
                assert ca + 1 in b and ca + 1 not in a, (rt, hi)


def test_class_alone_jobs_have_their_class():
    p = _params(DEFAULT)
    for rt in ("column", "band"):
        for cls in range(gp.N_CLASSES):
            for q, t, w in _class_alone(cls, rt):
                assert gp.glob_class(len(q), len(t), w, p, rt == "band") == cls, (cls, rt, len(q), len(t), w)


def test_loose_batch_covers_the_undefined_geometry():
    pairs, _, _ = _loose()
    undef = (pairs["len2"] < pairs["len1"] - pairs["h0"])
    unreach = (pairs["len2"] > pairs["len1"] + pairs["h0"])
    for rt in (0, 1):
        cls = np.array(gp.plan(pairs, _params(DEFAULT), rt)[0])
        for fam in (cls < gp.LANE0, (cls >= gp.LANE0) & (cls < gp.WIDE), cls == gp.WIDE):
            assert (fam & undef).sum() >= 10 and (fam & unreach).sum() >= 10, rt


@functools.lru_cache(maxsize=None)
def _excursion_truth(scoring):
    pairs, ref, qer = _excursions()
    want = _oracle(pairs, ref, qer, scoring)
    n, flags = gp.predict_retries(pairs, want[1], want[2], _params(scoring), False)
    return want, n, np.array(flags)


@pytest.mark.parametrize("scoring", [CORR_GAPS, DEFAULT])
def test_excursion_batch_has_both_outcomes(scoring):
    """A condition on the inputs of the corridor tests: between 20 % and 80 % of the jobs retry, every
    class is on the narrow window, |dlt| = 18 always retries, and the rows dlt = 0 and dlt = +-17
    hold jobs of both outcomes."""
    pairs, _, _ = _excursions()
    assert len(pairs) == 5 * 9 * 14 * 2 and np.all(pairs["len2"] >= pairs["len1"] - 40)
    cls, st = gp.plan(pairs, _params(scoring), False)
    assert sorted(st) == [5, 6, 7, 8, 9] and all(gp.narrow_tb(c, v[1], v[2]) for c, v in st.items())
    want, n, flags = _excursion_truth(scoring)
    assert np.all(want[2] > 0)
    assert 0.2 * len(pairs) <= n <= 0.8 * len(pairs), n
    dlt = pairs["len2"] - pairs["len1"]
    assert flags[np.abs(dlt) == 18].all()
    for d in (0, 17, -17, 16, -16, 8, -8):
        assert flags[dlt == d].any(), d
    for d in (0, 17, 16, -16, 8, -8):
        assert not flags[dlt == d].all(), d


# ---------------------------------------------------------------- GPU
_TRUTH = {}


def _truth(key, pairs, ref, qer, scoring, rt):
    """Oracle outputs and predicted statistics of a batch under a routing, computed once."""
    if (key, scoring) not in _TRUTH:
        _TRUTH[key, scoring] = _oracle(pairs, ref, qer, scoring)
    want = _TRUTH[key, scoring]
    if (key, scoring, rt) not in _TRUTH:
        assert np.all(want[2] != -1)
        cls, st = gp.plan(pairs, _params(scoring), rt == "band")
        _TRUTH[key, scoring, rt] = (st, gp.predict_retries(pairs, want[1], want[2], _params(scoring), rt == "band")[0])
    return (want,) + _TRUTH[key, scoring, rt]


def _run(eng, key, batch, scoring, rt, tag):
    """One CIGAR call: outputs equal the oracle, the statistics equal the planner's prediction."""
    pairs, ref, qer = batch
    want, st, n_retry = _truth(key, pairs, ref, qer, scoring, rt)
    got = bsw.ksw_global2(eng, pairs.copy(), ref, qer, stride=STRIDE)
    _check(want, got, tag)
    assert not np.any(got[2] == -3), tag
    gs = bsw.global_last_stats(eng)
    n_wide = st.get(gp.WIDE, (0, 0, 0))[0]
    assert (gs.n_jobs, gs.n_wide, gs.n_lane) == (len(pairs), n_wide, len(pairs) - n_wide), tag
    assert gs.n_launches >= len(st), tag
    assert gs.n_tb_retry == n_retry, (tag, gs.n_tb_retry, n_retry)
    return got, gs


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", [DEFAULT, OTHER])
def test_gpu_class_grid(scoring, routing):
    eng = _engine(_params(scoring), routing)
    _run(eng, "grid", _grid(), scoring, routing, f"grid {scoring} {routing}")
    eng.close()


@pytest.mark.gpu
def test_gpu_one_class_alone(routing):
    """Calls of 1 and of 65 jobs of one class: a wave with one live lane takes wmax, tmax and the
    widest query from that lane alone."""
    eng = _engine(_params(DEFAULT), routing)
    for cls in range(gp.N_CLASSES):
        jobs = _class_alone(cls, routing)
        for n in (1, 65):
            got, gs = _run(eng, ("alone", cls, n, routing), _pack(jobs[:n]), DEFAULT, routing,
                           f"class {cls} alone, {n} jobs, {routing}")
            assert gs.n_launches >= 1
    eng.close()


@pytest.mark.gpu
def test_gpu_undefined_geometry_and_unreachable_column(routing):
    pairs, ref, qer = _loose()
    eng = _engine(_params(DEFAULT), routing)
    got, _ = _run(eng, "loose", (pairs, ref, qer), DEFAULT, routing, f"loose {routing}")
    undef = pairs["len2"] < pairs["len1"] - pairs["h0"]
    assert np.array_equal(got[2] == -2, undef) and undef.sum() > 100
    eng.close()


def _device_call(eng, pairs, ref, qer, stride, stream=0, pad=(64, 16), sentinel=0xA5A5A5A5):
    """bsw_ksw_global2_device over uploaded copies -> (score, cigar, n_cigar, words behind both arrays)."""
    import hiprt
    n = len(pairs)
    d_pairs, d_ref, d_qer = (hiprt.DeviceBuffer.from_array(x) for x in (pairs, ref, qer))
    cig = np.full(n * stride + pad[0], sentinel, dtype=np.uint32)
    ncig = np.full(n + pad[1], sentinel, dtype=np.uint32)
    d_cig, d_nc = hiprt.DeviceBuffer.from_array(cig), hiprt.DeviceBuffer.from_array(ncig)
    bsw.ksw_global2_device(eng, d_pairs.ptr, d_ref.ptr, d_qer.ptr, n, d_cig.ptr if stride else 0, stride,
                           d_nc.ptr if stride else 0, stream)
    out = pairs.copy()
    d_pairs.download(out)
    d_cig.download(cig)
    d_nc.download(ncig)
    for b in (d_pairs, d_ref, d_qer, d_cig, d_nc):
        b.free()
    return (out["score"].copy(), cig[:n * stride].reshape(n, stride) if stride else None,
            ncig[:n].view(np.int32).copy(), (cig[n * stride:], ncig[n:]))


@functools.lru_cache(maxsize=None)
def _by_op_count():
    """Grid jobs (default scoring) by the number of ops of their oracle CIGAR."""
    pairs, ref, qer = _grid()
    nc = _oracle(pairs, ref, qer, DEFAULT)[2]
    return {k: np.flatnonzero(nc == k)[:200] for k in (1, 2, 3, 5, 8, 12)}


def _subset(batch, idx):
    pairs, ref, qer = batch
    return np.ascontiguousarray(pairs[idx]), ref, qer


@pytest.mark.gpu
def test_gpu_stride_edges(routing):
    """A CIGAR of exactly k ops: complete at stride k, -1 at stride k - 1 (score still right);
    nothing is written behind the n * stride words or the n counts."""
    eng = _engine(_params(DEFAULT), routing)
    for k, idx in _by_op_count().items():
        assert len(idx) >= 20, k
        pairs, ref, qer = _subset(_grid(), idx)
        for stride in (k, k - 1):
            want = _oracle(pairs, ref, qer, DEFAULT, stride=stride)
            sc, cig, nc, tails = _device_call(eng, pairs, ref, qer, stride)
            assert np.all(tails[0] == 0xA5A5A5A5) and np.all(tails[1] == 0xA5A5A5A5), (k, stride)
            if stride == 0:                                  # scores only: neither array is touched
                assert np.array_equal(sc, want[0]) and np.all(nc.view(np.uint32) == 0xA5A5A5A5)
                continue
            _check(want, (sc, cig, nc), f"{k} ops at stride {stride}")
            assert np.all(nc == (k if stride == k else -1)), (k, stride)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", [CORR_GAPS, DEFAULT])
def test_gpu_corridor_retries_are_the_paths_that_leave_it(scoring):
    """n_tb_retry equals the number of jobs whose oracle path leaves the 3-dword corridor; a second,
    identical call gives identical outputs and the same count."""
    eng = _engine(_params(scoring), "column")
    a, sa = _run(eng, "excursions", _excursions(), scoring, "column", f"excursions {scoring}")
    b, sb = _run(eng, "excursions", _excursions(), scoring, "column", f"excursions {scoring}, second call")
    assert sa.n_tb_retry == sb.n_tb_retry == _excursion_truth(scoring)[1]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    for i in range(len(a[2])):
        assert np.array_equal(a[1][i, :a[2][i]], b[1][i, :b[2][i]]), i
    eng.close()


@functools.lru_cache(maxsize=None)
def _tall():
    """qlen 160 against about 170 unrelated bases, w = 60: most jobs rerun with the full window."""
    rng = np.random.default_rng(160)
    return _pack([(_seq(rng, 160), _seq(rng, int(rng.integers(165, 176))), 60) for _ in range(256)])


@pytest.mark.gpu
def test_gpu_matrix_reuse_across_calls():
    """The traceback matrix is reused without clearing: a call after a larger one equals the oracle
    and the same call on a fresh engine."""
    eng = _engine(_params(CORR_GAPS), "column")
    _, sa = _run(eng, "tall", _tall(), CORR_GAPS, "column", "A")
    assert sa.n_tb_retry > 128
    b, sb = _run(eng, "excursions", _excursions(), CORR_GAPS, "column", "B after A")
    _run(eng, "tall", _tall(), CORR_GAPS, "column", "A after B")
    eng.close()
    fresh = _engine(_params(CORR_GAPS), "column")
    f, sf = _run(fresh, "excursions", _excursions(), CORR_GAPS, "column", "B on a fresh engine")
    fresh.close()
    assert sb.n_tb_retry == sf.n_tb_retry and sb.z_bytes == sf.z_bytes
    _check(f, b, "B after A against B fresh")


@pytest.mark.gpu
def test_gpu_int16_row_at_its_limit(routing):
    eng = _engine(_params(I16), routing)
    pairs, ref, qer = _i16_edge()
    got, gs = _run(eng, "i16", (pairs, ref, qer), I16, routing, f"a = b = 92, {routing}")
    assert got[0].max() == 92 * 159 - (6 + 24) and got[0].min() == -92 * 159
    if routing == "column":                     # w = 50: tlen 183 on the register row, tlen 184 not
        assert gs.n_wide == int(((pairs["len1"] == 184) & (pairs["h0"] == 50)).sum()) > 0
    eng.close()


@pytest.mark.gpu
def test_gpu_scores_beyond_the_int16_row(routing):
    """Identical 160-base pairs at a = 120 score 19200: the planner keeps them off the int16 row."""
    eng = _engine(_params(I16_BIG), routing)
    got, gs = _run(eng, "i16big", _i16_big(), I16_BIG, routing, f"a = 120, {routing}")
    same = _i16_big()[0]["h0"] > 0
    assert np.all(got[0][same] == 19200) and np.all(got[0][~same] == -19200) and np.all(got[2] == 1)
    assert gs.n_wide == 52
    eng.close()


@pytest.mark.gpu
def test_gpu_global2_device_form(routing):
    """bsw_ksw_global2_device on the engine's stream and on a caller's stream: equal to the host form
    and the oracle; without CIGAR arrays only the scores are written and no matrix is used."""
    import torch
    pairs, ref, qer = _subset(_grid(), np.arange(7, len(_grid()[0]), 4)[:2000])
    want = _oracle(pairs, ref, qer, DEFAULT)
    eng = _engine(_params(DEFAULT), routing)
    host = bsw.ksw_global2(eng, pairs.copy(), ref, qer, stride=STRIDE)
    _check(want, host, "host form")
    hs = bsw.global_last_stats(eng)
    ts = torch.cuda.Stream()
    for name, stream in (("engine stream", 0), ("caller stream", ts.cuda_stream)):
        sc, cig, nc, tails = _device_call(eng, pairs, ref, qer, STRIDE, stream)
        _check(want, (sc, cig, nc), f"device form, {name}")
        _check(host, (sc, cig, nc), f"device form against host form, {name}")
        gs = bsw.global_last_stats(eng)
        assert (gs.n_jobs, gs.n_lane, gs.n_wide, gs.n_tb_retry, gs.z_bytes) == \
            (hs.n_jobs, hs.n_lane, hs.n_wide, hs.n_tb_retry, hs.z_bytes) and gs.z_bytes > 0
        sc0, _, nc0, tails = _device_call(eng, pairs, ref, qer, 0, stream)
        assert np.array_equal(sc0, want[0]) and np.all(nc0.view(np.uint32) == 0xA5A5A5A5)
        assert np.all(tails[0] == 0xA5A5A5A5) and bsw.global_last_stats(eng).z_bytes == 0
        # n = 0: success, nothing read or written (null pointers)
        bsw.ksw_global2_device(eng, 0, 0, 0, 0, 0, STRIDE, 0, stream)
    eng.close()


@pytest.mark.gpu
def test_gpu_align2_device_form():
    """bsw_ksw_align2_device equals bsw_ksw_align2 and the oracle on both kinds of stream."""
    import hiprt
    import torch
    a, b, od, ed, oi, ei = DEFAULT
    pairs, ref, qer = _mate_batch(3000, seed=a * 100 + od)
    p = _params(DEFAULT)
    want = oracle.ksw_align2_batch(pairs, ref, qer, list(p.mat), od, ed, oi, ei, nthreads=16)
    eng = bsw.Engine(p)
    host = bsw.ksw_align2(eng, pairs, ref, qer)
    _mate_same(want, host, "host form")
    d_pairs, d_ref, d_qer = (hiprt.DeviceBuffer.from_array(x) for x in (pairs, ref, qer))
    ts = torch.cuda.Stream()
    for name, stream in (("engine stream", 0), ("caller stream", ts.cuda_stream)):
        out = np.full(len(pairs) + 4, -7, dtype=bsw.KSWR_DTYPE)
        d_aln = hiprt.DeviceBuffer.from_array(out)
        bsw.ksw_align2_device(eng, d_pairs.ptr, d_ref.ptr, d_qer.ptr, len(pairs), d_aln.ptr, stream)
        d_aln.download(out)
        _mate_same(want, out[:len(pairs)], f"device form, {name}")
        _mate_same(host, out[:len(pairs)], f"device form against host form, {name}")
        assert all(np.all(out[len(pairs):][f] == -7) for f in bsw.KSWR_DTYPE.names)
        assert bsw.mate_last_stats(eng).n_fwd == len(pairs)
        bsw.ksw_align2_device(eng, 0, 0, 0, 0, 0, stream)       # n = 0
        d_aln.free()
    for b_ in (d_pairs, d_ref, d_qer):
        b_.free()
    eng.close()
