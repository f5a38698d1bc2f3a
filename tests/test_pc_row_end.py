"""The packed-column kernel's row end (bsw_pc.hip) on the GPU, after its rewrite on lane masks:
the z-drop distance, the best / best_i / best_j / max_off update and the one certificate block of a marked
wave (§3 items 12 and 13), with the P field put without a max.  Small batches that reach each rewritten block,
all six output fields against the CPU oracle, through the engine's C ABI.  The CPU model of the kernel's loop
(tests/pc_wave_model.py, in the engine's wave layout) is checked against the oracle first and vouches that
each batch shows the event it is here for, so no case passes vacuously; where the loaded library is the stats
build (BSW_HIP_LIB = libbsw_hip_stats.so: `make stats`), the kernel's redo lanes must also be the model's."""

import ctypes

import numpy as np
import pytest

import bsw
import bswgen
import hiprt
import oracle
import pc_batches as pcb
import pc_wave_model as pwm
from test_right_prune_model import vouch

pytestmark = pytest.mark.gpu

Z100 = dict(zdrop=100)
Z0 = dict(zdrop=0)
DEFAULT = dict(zdrop=100, end_bonus=5)


def tied_wave(seed=91, n=64):
    """One wave of pairs whose every late row has two equal maxima, four columns apart.  Target = P U^r, query
    = P X U^r: U a permutation of ACGT (period exactly 4), X = U with two bases changed.  The diagonal pays two
    mismatches (2 x 5 under a perfect copy), the path that inserts X one gap of four (6 + 4): from the first U on
    cell (i, i) and cell (i, i + 4) hold the same value, both grow by one per row, and the window ends with
    them -- the last row sets the final best on a tie, which goes to the later column (ksw_extend2 keeps
    mj = j on h == m): qle = tle + 4 and max_off = 4."""
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = int(rng.integers(17, 22))
        a = 96 - (4 * r + 4) + int(rng.integers(0, 11))      # qlen 96 .. 106: all in the QMAX 128 class
        p = rng.integers(0, 4, a).astype(np.uint8)
        u = rng.permutation(4).astype(np.uint8)
        x = u.copy()
        for k in rng.choice(4, 2, replace=False):
            x[k] = (x[k] + int(rng.integers(1, 4))) & 3
        t = np.concatenate([p, np.tile(u, r)])
        q = np.concatenate([p, x, np.tile(u, r)])
        items.append((t, q, int(rng.integers(20, 61))))
    return bswgen.assemble(items)


def vouch_tie(pairs, ref, qer, want):
    """The oracle's own outputs show the tie: the later column wins, and the same query without its last four
    columns -- where only the diagonal's cell is left on the last row -- reaches the same score."""
    assert len(set(pcb.qmax_class(pairs))) == 1, "the tied pairs must share a class: one wave"
    assert (want["qle"] == want["tle"] + 4).all() and (want["tle"] == pairs["len1"]).all()
    assert (want["max_off"] == 4).all()
    cut = pairs.copy()
    cut["len2"] -= 4
    oracle.get_scores(oracle.make_params(**DEFAULT), cut, ref, qer, 100, nthreads=8)
    assert (cut["score"] == want["score"]).all() and (cut["qle"] == cut["tle"]).all()


# name: (builder, w, scoring, the event the model must show: test_right_prune_model.vouch's names, or "tie")
CASES = {
    # the z-drop distance with both signs of di - dj, in marked waves: exactly the two odd lanes of each wave redone
    "odd_lane_z10": (lambda: pcb.odd_lane(16, 88), 100, dict(zdrop=10), "odd"),
    # crossing and final certificates, P carried to lane exit
    "late_collapse_z100": (lambda: pcb.late_collapse(1024, 74, at=120), 100, Z100, "final"),
    "late_collapse_z0": (lambda: pcb.late_collapse(1024, 74, at=120), 100, Z0, "final"),
    "clipped_tails_z100": (lambda: pcb.clipped_tails(1536, 81), 100, Z100, "final"),
    "clipped_tails_z0": (lambda: pcb.clipped_tails(1536, 81), 100, Z0, "final"),
    # retreat, then clip again: P is written more than once
    "late_insertion": (lambda: pcb.late_insertion(1024, 84), 100, DEFAULT, "retreat"),
    # marked, never clipped: P is never set by a row and no lane is redone for crossing
    "low_h0": (lambda: pcb.low_h0(2048, 85), 100, DEFAULT, "low_h0"),
    "c2_w20": (lambda: pcb.c2_shaped(2048, 86), 20, DEFAULT, "band"),
    # both classes with the rules, and one class without
    "class_edges": (lambda: pcb.class_edges(512, 76), 100, DEFAULT, "classes"),
    # best_j / max_off tie order through the select form
    "tied_wave": (tied_wave, 100, DEFAULT, "tie"),
}
_cache = {}


def _case(name, tmp_path_factory):
    """(pairs, ref, qer, w, scoring, event, oracle outputs, the model's redo marks and per-wave figures), once."""
    if name not in _cache:
        make, w, sc, what = CASES[name]
        pairs, ref, qer = make()
        assert len(pairs) <= 2048
        par = oracle.make_params(**sc)
        want = pairs.copy()
        oracle.get_scores(par, want, ref, qer, w, nthreads=8)
        lib = pwm.build(tmp_path_factory.mktemp("pc_model"))
        got, _, redo, wst = pwm.run_planned(lib, par, pairs, ref, qer, w)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: the model disagrees with the oracle in {f}"
        _cache[name] = (pairs, ref, qer, w, sc, what, want, redo, wst)
    return _cache[name]


_engines = {}


@pytest.fixture(scope="module")
def engine():
    def get(kernel8, sc):
        key = (kernel8, tuple(sorted(sc.items())))
        if key not in _engines:
            _engines[key] = bsw.Engine(bsw.default_params(**sc), kernel8=kernel8, small_batch=0, mid_batch=0)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def _kernel_redo():
    """The redo lanes the kernel has counted since the last call (the stats build only, else None)."""
    L = bsw.hip_lib()
    if not hasattr(L, "bsw_pc_stats"):
        return None
    L.bsw_pc_stats.argtypes = [ctypes.c_void_p, ctypes.c_int]
    st = (ctypes.c_ulonglong * 19)()
    assert L.bsw_pc_stats(st, 1) == 0
    return int(st[12])


def _run(eng, pairs, ref, qer, w, want, tag):
    dp, dr, dq = (hiprt.DeviceBuffer.from_array(a) for a in (pairs, ref, qer))
    eng.get_scores_device(dp.ptr, dr.ptr, dq.ptr, len(pairs), w)
    got = dp.download(np.empty_like(pairs))
    assert eng.last_stats().n_packed == len(pairs), f"{tag}: not every pair ran in the packed-column kernel"
    bad = np.zeros(len(want), bool)
    for f in bsw.OUT_FIELDS:
        bad |= want[f] != got[f]
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {len(want)} pairs differ; first idx {i} "
                             f"len1={want[i]['len1']} len2={want[i]['len2']} h0={want[i]['h0']} "
                             f"want={[int(want[i][f]) for f in bsw.OUT_FIELDS]} "
                             f"got={[int(got[i][f]) for f in bsw.OUT_FIELDS]}")


@pytest.mark.parametrize("name", list(CASES))
def test_row_end_case(engine, tmp_path_factory, name):
    """The int16 planes: the classes that carry items 12 and 13 (QMAX 128, 160) and those that do not."""
    pairs, ref, qer, w, sc, what, want, redo, wst = _case(name, tmp_path_factory)
    if what == "tie":
        vouch_tie(pairs, ref, qer, want)
    else:
        vouch(name, what, pairs, ref, qer, redo, wst)
    _kernel_redo()                              # (the stats build: the count starts at 0)
    _run(engine(1, sc), pairs, ref, qer, w, want, name)
    nredo = _kernel_redo()
    if nredo is not None:
        assert nredo == int(redo.sum()), f"{name}: the kernel redid {nredo} lanes, the model {int(redo.sum())}"


@pytest.mark.parametrize("name", ["tied_wave", "odd_lane_z10"])
def test_row_end_byte_planes(engine, tmp_path_factory, name):
    """The byte planes carry no certificate but the same row end: the tie order and the z-drop distance."""
    pairs, ref, qer, w, sc, what, want, redo, wst = _case(name, tmp_path_factory)
    _run(engine(2, sc), pairs, ref, qer, w, want, f"{name} kernel8=2")
