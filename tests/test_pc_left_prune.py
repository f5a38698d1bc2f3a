"""The packed-column kernel's left prune and its redo pass (bsw_pc.hip) on the
GPU: all six output fields bit-exact against the CPU oracle on small batches of the shapes where a
prune that dropped a cell the outputs need, a certificate that missed a lane, or a redo list that
lost or repeated one would show.  The int16 planes (kernel8 = 1) carry the rule in the QMAX 128 and
160 classes; the byte planes (kernel8 = 2) and the 96 class are compiled without it and run the same
batches.  The CPU model of the kernel's loop (tests/pc_wave_model.py with the right prune off, in the
engine's wave layout) vouches that each batch prunes, and that the collapse batches redo."""

import numpy as np
import pytest

import bsw
import hiprt
import oracle
import pc_batches as pcb
import pc_wave_model as pwm

pytestmark = pytest.mark.gpu

DEFAULT = dict(zdrop=100, end_bonus=5)
Z10 = dict(zdrop=10)


def _collapse_b():
    """b. 1,024 pairs with every lane collapsing at base 130 and 1,024 with one lane in eight."""
    return pcb.concat(pcb.late_collapse(1024, 72), pcb.late_collapse(1024, 73, every=8))


def _mixed_e():
    """e. Zeros inside rows, a lane that pins gz, uneven lifetimes, the live boundary -- and a
    partial last wave: 37 + 64 k pairs."""
    parts = [pcb.interior_zeros(512, 66), pcb.pinned_waves(3, 67, True), pcb.uneven_lifetimes(6, 68),
             pcb.boundary_alive(512, 65)]
    p, r, q = pcb.concat(*parts)
    n = (len(p) - 37) // 64 * 64 + 37
    return p[:n], r, q


BATCHES = {
    "a_c2_shaped": (lambda: pcb.c2_shaped(4096, 71), 100, DEFAULT),
    "b_late_collapse": (_collapse_b, 100, Z10),
    "c_collapse_120_z100": (lambda: pcb.late_collapse(1024, 74, at=120), 100, dict(zdrop=100)),
    "c_collapse_135_z0": (lambda: pcb.late_collapse(1024, 75, at=135), 100, dict(zdrop=0)),
    "d_classes_w100": (lambda: pcb.class_edges(512, 76), 100, DEFAULT),
    "d_classes_w20": (lambda: pcb.class_edges(512, 77), 20, DEFAULT),
    "e_mixed": (_mixed_e, 100, Z10),
}
_cache = {}


def _batch(name, tmp_path_factory):
    """(pairs, ref, qer, w, scoring, oracle outputs, model's redo marks and per-wave figures), once."""
    if name not in _cache:
        make, w, sc = BATCHES[name]
        pairs, ref, qer = make()
        par = oracle.make_params(**sc)
        want = pairs.copy()
        oracle.get_scores(par, want, ref, qer, w, nthreads=8)
        lib = pwm.build(tmp_path_factory.mktemp("pc_model"))
        got, _, redo, wst = pwm.run_planned(lib, par, pairs, ref, qer, w, rprune=False)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: the model disagrees with the oracle in {f}"
        _cache[name] = (pairs, ref, qer, w, sc, want, redo, wst)
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


def _compare(want, got, tag):
    bad = np.zeros(len(want), bool)
    for f in bsw.OUT_FIELDS:
        bad |= want[f] != got[f]
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {len(want)} pairs differ; first idx {i} "
                             f"len1={want[i]['len1']} len2={want[i]['len2']} h0={want[i]['h0']} "
                             f"want={[int(want[i][f]) for f in bsw.OUT_FIELDS]} "
                             f"got={[int(got[i][f]) for f in bsw.OUT_FIELDS]}")


def _run(eng, pairs, ref, qer, w, want, tag):
    dp, dr, dq = (hiprt.DeviceBuffer.from_array(a) for a in (pairs, ref, qer))
    eng.get_scores_device(dp.ptr, dr.ptr, dq.ptr, len(pairs), w)
    got = dp.download(np.empty_like(pairs))
    assert eng.last_stats().n_packed == len(pairs), f"{tag}: not every pair ran in the packed-column kernel"
    _compare(want, got, tag)


def _vouch(name, pairs, ref, qer, redo, wst):
    """What the model must show for the batch to test what it is built for."""
    ev, nredo = int(wst[:, 3].sum()), int(redo.sum())
    print(f"{name}: {len(pairs)} pairs in {len(wst)} waves, model: prune events {ev}, redo lanes {nredo}, "
          f"groups per row {wst[:, 1].sum() / wst[:, 0].sum():.2f}")
    assert ev > 0, f"{name}: the model never prunes on this batch"
    if name.startswith("b_"):
        cls = pcb.qmax_class(pairs)
        assert (cls == 4).all() and nredo > 64, f"{name}: {nredo} redo lanes in one class"
        assert (wst[:, 4] > 0).sum() > 2               # spread over several waves of the main launch
    if name.startswith(("a_", "c_")):
        assert nredo == 0, f"{name}: {nredo} redo lanes"
    if name.startswith("d_"):
        order = pcb.default_order(pairs, ref, qer)
        wcls = pcb.qmax_class(pairs)[order][::64]
        for c in (3, 4):                       # the classes that carry the rule
            assert wst[wcls == c, 3].sum() > 0, f"{name}: class {c} never pruned"
    if name.startswith("e_"):
        assert len(pairs) % 64 == 37 and nredo > 0


@pytest.mark.parametrize("kernel8", [1, 2])
@pytest.mark.parametrize("name", list(BATCHES))
def test_left_prune_batch(engine, tmp_path_factory, name, kernel8):
    pairs, ref, qer, w, sc, want, redo, wst = _batch(name, tmp_path_factory)
    _vouch(name, pairs, ref, qer, redo, wst)
    eng = engine(kernel8, sc)
    _run(eng, pairs, ref, qer, w, want, f"{name} kernel8={kernel8}")
    if name.startswith("b_"):                  # once more on the same engine: the redo counter starts at 0 again
        _run(eng, pairs, ref, qer, w, want, f"{name} kernel8={kernel8} second run")


def test_left_prune_host_buffers(engine, tmp_path_factory):
    """f. Batch b through the host-buffer entry point, above the small-batch route (small_batch = 0):
    the same planned path and redo pass."""
    pairs, ref, qer, w, sc, want, redo, wst = _batch("b_late_collapse", tmp_path_factory)
    assert int(redo.sum()) > 64
    eng = engine(1, sc)
    got = pairs.copy()
    eng.get_scores(got, ref, qer, w)
    assert eng.last_stats().n_packed == len(pairs)
    _compare(want, got, "b_late_collapse host buffers")
