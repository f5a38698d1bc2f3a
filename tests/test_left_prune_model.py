"""The packed-column kernel's left prune as a CPU model of the KERNEL's loop
(tests/pc_wave_model.py with the right prune off): the left skip's model with gz also passing over non-zero groups that
cannot reach gscore in any live lane, the wave-level `pruned` flag, the row-end certificate and the
redo lanes recomputed without the rule.  It must give the oracle's six outputs on every pair, run
no more rows per lane than the literal loop, remove a real share of the flagship's entered groups
and send next to no flagship lane to the redo pass."""

import itertools

import numpy as np
import pytest

import bsw
import early_stop_model as esm
import oracle
import pc_batches as pcb
import pc_wave_model as pwm


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("pc_model")
    return pwm.build(d), esm.build(d)


def _check(models, params, pairs, ref, qer, w, order, tag, want=None, rows0=None):
    """The model with the prune on the lanes in `order`: 0 differing fields against the oracle,
    rows per lane no more than the literal loop's.  Returns (want, rows0, per-wave sums)."""
    lib, elib = models
    if want is None:
        want = pairs.copy()
        oracle.get_scores(params, want, ref, qer, w, nthreads=8)
        _, rows0, _ = esm.run(elib, params, pairs, ref, qer, w, 0)
    got, rows, _, wst = pwm.run(lib, params, pairs, ref, qer, w, order=order, rprune=False)
    for f in bsw.OUT_FIELDS:
        bad = np.flatnonzero(want[f] != got[f])
        assert len(bad) == 0, (f"{tag}: field {f} differs in {len(bad)} pairs; first {bad[0]} "
                               f"tlen={pairs['len1'][bad[0]]} qlen={pairs['len2'][bad[0]]} h0={pairs['h0'][bad[0]]} "
                               f"want {want[f][bad[0]]} got {got[f][bad[0]]}")
    assert (rows <= rows0).all(), f"{tag}: a lane ran more rows than the literal loop"
    return want, rows0, wst[:, :5].sum(0)


def test_model_random_shapes(models):
    """>= 300,000 shapes over the combinations of test_left_skip_model.py: w 0, 1 and every tenth
    value up to 200, zdrop 0 / 10 / 100, end_bonus 0 / 5; waves by the default sort key and shuffled."""
    combos = list(itertools.product((0, 1) + tuple(range(10, 201, 10)), (0, 10, 100), (0, 5)))
    per = 300_000 // len(combos) + 1
    n = 0
    tot = {"sorted": np.zeros(5, np.int64), "shuffled": np.zeros(5, np.int64)}
    for k, (w, zdrop, eb) in enumerate(combos):
        if k % 12 == 0:
            pairs, ref, qer = esm.diagonal_pairs(per // 4, seed=3000 + k, twice=bool(k & 1), h0=(1, 60))
        else:
            pairs, ref, qer = esm.random_shapes(per, seed=2000 + k)
        params = oracle.make_params(zdrop=zdrop, end_bonus=eb)
        tag = f"w={w} zdrop={zdrop} end_bonus={eb}"
        want, rows0, st = _check(models, params, pairs, ref, qer, w, pcb.default_order(pairs, ref, qer), tag + " sorted")
        tot["sorted"] += st
        shuffled = np.random.default_rng(k).permutation(len(pairs)).astype(np.int32)
        _, _, st = _check(models, params, pairs, ref, qer, w, shuffled, tag + " shuffled", want, rows0)
        tot["shuffled"] += st
        n += len(pairs)
    extra = 0                     # the diagonal batches are a quarter the size: make up the count
    while n + extra < 300_000:
        pairs, ref, qer = esm.random_shapes(per, seed=5000 + extra)
        want, rows0, st = _check(models, oracle.make_params(), pairs, ref, qer, 100,
                                 pcb.default_order(pairs, ref, qer), "extra sorted")
        tot["sorted"] += st
        extra += len(pairs)
    n += extra
    assert n >= 300_000
    for name, (rows, ent, skp, ev, redo) in tot.items():
        print(f"random shapes, {name} waves: {n} pairs, groups per row {ent / rows:.2f}, prune events {ev}, "
              f"redo lanes {redo} ({redo / n:.4f})")
        assert ev > 0, f"the prune never fired on the {name} waves"


def test_model_c2(models):
    """100,000 pairs of the flagship batch (150 bp query, 300 bp window, w = 100) in the waves of
    the default sort key: exact, at least 5 % of the groups the skip alone enters removed, at most
    0.1 % of the lanes sent to the redo pass."""
    lib, _ = models
    pairs, ref, qer = bsw.synth_batch(100_000)
    params = oracle.make_params()
    order = pcb.default_order(pairs, ref, qer)
    _, _, (rows, ent, skp, ev, redo) = _check(models, params, pairs, ref, qer, 100, order, "C2")
    _, _, _, wst0 = pwm.run(lib, params, pairs, ref, qer, 100, order=order, prune=False, rprune=False)
    r0, e0, _ = wst0[:, :3].sum(0)
    share = 1.0 - ent / e0
    print(f"C2: rows per wave {rows / len(wst0):.1f} ({r0 / len(wst0):.1f} with the skip alone), groups entered per "
          f"row {ent / rows:.2f} ({e0 / r0:.2f}); share of entered groups removed {share:.4f}; prune events {ev}; "
          f"redo lanes {redo} of {len(pairs)}")
    assert share >= 0.05, f"the prune removes only {share:.4f} of the groups the skip enters"
    assert redo <= 0.001 * len(pairs), f"{redo} redo lanes"


BUILT = {
    "a_c2_shaped": (lambda: pcb.c2_shaped(4096, 71), 100, dict(zdrop=100, end_bonus=5)),
    "b_collapse_all": (lambda: pcb.late_collapse(1024, 72), 100, dict(zdrop=10)),
    "b_collapse_one_in_8": (lambda: pcb.late_collapse(1024, 73, every=8), 100, dict(zdrop=10)),
    "c_collapse_120_z100": (lambda: pcb.late_collapse(1024, 74, at=120), 100, dict(zdrop=100)),
    "c_collapse_135_z0": (lambda: pcb.late_collapse(1024, 75, at=135), 100, dict(zdrop=0)),
    "d_classes_w100": (lambda: pcb.class_edges(512, 76), 100, dict(zdrop=100, end_bonus=5)),
    "d_classes_w20": (lambda: pcb.class_edges(512, 77), 20, dict(zdrop=100, end_bonus=5)),
    "e_interior_zeros": (lambda: pcb.interior_zeros(2048, 66), 100, dict(zdrop=100, end_bonus=5)),
    "e_pinned": (lambda: pcb.pinned_waves(5, 67, True), 100, pcb.PIN_SCORING),
    "e_uneven_lifetimes": (lambda: pcb.uneven_lifetimes(30, 68), 100, dict(zdrop=100, end_bonus=5)),
    "e_boundary_alive": (lambda: pcb.boundary_alive(2048, 65), 100, dict(zdrop=100, end_bonus=5)),
}


def test_model_built_cases(models):
    """The batches the GPU test runs, in the engine's wave layout: exact, each prunes, the
    z-drop collapse batches redo -- more than one wave's worth in one class."""
    lib, elib = models
    for name, (make, w, sc) in BUILT.items():
        pairs, ref, qer = make()
        params = oracle.make_params(**sc)
        want = pairs.copy()
        oracle.get_scores(params, want, ref, qer, w, nthreads=8)
        _, rows0, _ = esm.run(elib, params, pairs, ref, qer, w, 0)
        got, rows, redo, wst = pwm.run_planned(lib, params, pairs, ref, qer, w, rprune=False)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: field {f} differs"
        assert (rows <= rows0).all()
        ev, nredo = int(wst[:, 3].sum()), int(redo.sum())
        print(f"{name}: {len(pairs)} pairs, prune events {ev}, redo lanes {nredo}")
        assert ev > 0, f"{name}: the prune never fired"
        if name.startswith("b_"):
            assert nredo > 64, f"{name}: {nredo} redo lanes"
        if name.startswith(("a_", "c_")):
            assert nredo == 0, f"{name}: {nredo} redo lanes"
        if name.startswith("d_"):            # every class that carries the rule prunes
            cls = pcb.qmax_class(pairs)[pcb.default_order(pairs, ref, qer)][::64]
            assert len(cls) == len(wst)
            for c in (3, 4):                 # QMAX 128 and 160; the 96 class is compiled without the rule
                assert wst[cls == c, 3].sum() > 0, f"{name}: class {c} never pruned"
