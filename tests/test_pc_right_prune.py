"""The packed-column kernel's right prune (bsw_pc.hip) on the GPU: all six output
fields bit-exact against the CPU oracle on small batches of the shapes where a cap that dropped a cell
the outputs need, a certificate that missed a lane, or a redo list that lost or repeated one would
show.  The int16 planes (kernel8 = 1) carry the rule in the QMAX 128 and 160 classes; the byte planes
(kernel8 = 2) are compiled without it and run the same batches.  The CPU model of the kernel's loop
(tests/pc_wave_model.py, in the engine's wave layout) is checked against the oracle first and
vouches that each batch prunes, retreats or redoes as stated."""

import numpy as np
import pytest

import bsw
import hiprt
import oracle
import pc_batches as pcb
import pc_wave_model as pwm
from test_right_prune_model import BUILT, vouch

pytestmark = pytest.mark.gpu


def _mixed():
    """Zeros inside rows, a lane that pins gz, uneven lifetimes, the live boundary -- and a partial
    last wave: 37 + 64 k pairs (the left prune's mixed batch)."""
    parts = [pcb.interior_zeros(512, 66), pcb.pinned_waves(3, 67, True), pcb.uneven_lifetimes(6, 68),
             pcb.boundary_alive(512, 65)]
    p, r, q = pcb.concat(*parts)
    n = (len(p) - 37) // 64 * 64 + 37
    return p[:n], r, q


BATCHES = dict(BUILT)
BATCHES["mixed"] = (_mixed, 100, dict(zdrop=10), "exact")
_cache = {}


def _batch(name, tmp_path_factory):
    """(pairs, ref, qer, w, scoring, oracle outputs, model's redo marks and per-wave figures), once."""
    if name not in _cache:
        make, w, sc, what = BATCHES[name]
        pairs, ref, qer = make()
        assert len(pairs) <= 4096
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


@pytest.mark.parametrize("kernel8", [1, 2])
@pytest.mark.parametrize("name", list(BATCHES))
def test_right_prune_batch(engine, tmp_path_factory, name, kernel8):
    pairs, ref, qer, w, sc, what, want, redo, wst = _batch(name, tmp_path_factory)
    if what != "exact":
        vouch(name, what, pairs, ref, qer, redo, wst)
    eng = engine(kernel8, sc)
    _run(eng, pairs, ref, qer, w, want, f"{name} kernel8={kernel8}")
    if what == "final":                        # once more on the same engine: the redo counter starts at 0 again
        _run(eng, pairs, ref, qer, w, want, f"{name} kernel8={kernel8} second run")


def test_right_prune_launches(engine, tmp_path_factory):
    """The rule adds no launch and no statistic: the clipped-tail batch, whose every lane is redone, runs
    the launches and reports the per-kernel counts of the flagship-shaped batch, which redoes none."""
    seen = []
    for name in ("c2_shaped", "a_clipped_tails_z100"):
        pairs, ref, qer, w, sc, what, want, redo, wst = _batch(name, tmp_path_factory)
        eng = engine(1, sc)
        _run(eng, pairs, ref, qer, w, want, name)
        st = eng.last_stats()
        seen.append((st.n_launches, st.n_packed == len(pairs)))
    assert seen[0] == seen[1], seen
