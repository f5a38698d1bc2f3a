"""The packed-column kernel's right prune as a CPU model of the KERNEL's loop
(tests/pc_wave_model.py): the left prune's model with the wave-uniform right cap, the zeroing
walk, the per-row crossing certificate, the soft retreat, the final certificate and the redo lanes
recomputed without either rule.  It must give the oracle's six outputs on every pair, run no more
rows per lane than the literal loop, remove a real share of the groups the left prune alone enters on
the flagship batch and send next to none of its lanes to the redo pass."""

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
    """The model with both prunes on the lanes in `order`: 0 differing fields against the oracle,
    rows per lane no more than the literal loop's.  Returns (want, rows0, per-wave sums by name)."""
    lib, elib = models
    if want is None:
        want = pairs.copy()
        oracle.get_scores(params, want, ref, qer, w, nthreads=8)
        _, rows0, _ = esm.run(elib, params, pairs, ref, qer, w, 0)
    got, rows, _, wst = pwm.run(lib, params, pairs, ref, qer, w, order=order)
    for f in bsw.OUT_FIELDS:
        bad = np.flatnonzero(want[f] != got[f])
        assert len(bad) == 0, (f"{tag}: field {f} differs in {len(bad)} pairs; first {bad[0]} "
                               f"tlen={pairs['len1'][bad[0]]} qlen={pairs['len2'][bad[0]]} h0={pairs['h0'][bad[0]]} "
                               f"want {want[f][bad[0]]} got {got[f][bad[0]]}")
    assert (rows <= rows0).all(), f"{tag}: a lane ran more rows than the literal loop"
    return want, rows0, pwm.totals(wst)


def _add(tot, st):
    for k, v in st.items():
        tot[k] = tot.get(k, 0) + v


def test_model_random_shapes(models):
    """>= 300,000 shapes over the combinations of test_left_prune_model.py: w 0, 1 and every tenth
    value up to 200, zdrop 0 / 10 / 100, end_bonus 0 / 5; waves by the default sort key and shuffled."""
    combos = list(itertools.product((0, 1) + tuple(range(10, 201, 10)), (0, 10, 100), (0, 5)))
    per = 300_000 // len(combos) + 1
    n = 0
    tot = {"sorted": {}, "shuffled": {}}
    for k, (w, zdrop, eb) in enumerate(combos):
        if k % 12 == 0:
            pairs, ref, qer = esm.diagonal_pairs(per // 4, seed=3000 + k, twice=bool(k & 1), h0=(1, 60))
        else:
            pairs, ref, qer = esm.random_shapes(per, seed=2000 + k)
        params = oracle.make_params(zdrop=zdrop, end_bonus=eb)
        tag = f"w={w} zdrop={zdrop} end_bonus={eb}"
        want, rows0, st = _check(models, params, pairs, ref, qer, w, pcb.default_order(pairs, ref, qer), tag + " sorted")
        _add(tot["sorted"], st)
        shuffled = np.random.default_rng(k).permutation(len(pairs)).astype(np.int32)
        _, _, st = _check(models, params, pairs, ref, qer, w, shuffled, tag + " shuffled", want, rows0)
        _add(tot["shuffled"], st)
        n += len(pairs)
    extra = 0                     # the diagonal batches are a quarter the size: make up the count
    while n + extra < 300_000:
        pairs, ref, qer = esm.random_shapes(per, seed=5000 + extra)
        want, rows0, st = _check(models, oracle.make_params(), pairs, ref, qer, 100,
                                 pcb.default_order(pairs, ref, qer), "extra sorted")
        _add(tot["sorted"], st)
        shuffled = np.random.default_rng(7000 + extra).permutation(len(pairs)).astype(np.int32)
        _, _, st = _check(models, oracle.make_params(), pairs, ref, qer, 100, shuffled, "extra shuffled", want, rows0)
        _add(tot["shuffled"], st)
        extra += len(pairs)
    n += extra
    assert n >= 300_000
    for name, t in tot.items():
        print(f"random shapes, {name} waves: {n} pairs, groups per row {t['entered'] / t['rows']:.2f}, right-prune "
              f"events {t['right_events']}, retreats {t['retreats']}, redo lanes {t['redo']} ({t['redo'] / n:.4f}: "
              f"crossing {t['redo_crossing']}, item 12's {t['redo_item12']}, final {t['redo_final']})")
        assert t["right_events"] > 0, f"the right prune never fired on the {name} waves"


def test_model_c2(models):
    """100,000 pairs of the flagship batch (150 bp query, 300 bp window, w = 100) in the waves of the
    default sort key: exact, at least 7 % of the groups the left prune alone enters removed, at most
    0.1 % of the lanes sent to the redo pass (a cap, not a target)."""
    lib, _ = models
    pairs, ref, qer = bsw.synth_batch(100_000)
    params = oracle.make_params()
    order = pcb.default_order(pairs, ref, qer)
    _, _, t = _check(models, params, pairs, ref, qer, 100, order, "C2")
    _, _, _, wst0 = pwm.run(lib, params, pairs, ref, qer, 100, order=order, rprune=False)
    r0, e0 = int(wst0[:, 0].sum()), int(wst0[:, 1].sum())
    share = 1.0 - t["entered"] / e0
    print(f"C2: rows per wave {t['rows'] / len(wst0):.1f} ({r0 / len(wst0):.1f} with the left prune alone), groups "
          f"entered per row {t['entered'] / t['rows']:.2f} ({e0 / r0:.2f}); share of entered groups removed {share:.4f}; "
          f"right-prune events {t['right_events']}, group tests {t['group_tests']}, retreats {t['retreats']}; redo lanes "
          f"{t['redo']} of {len(pairs)} (crossing {t['redo_crossing']}, item 12's {t['redo_item12']}, final {t['redo_final']})")
    assert share >= 0.07, f"the right prune removes only {share:.4f} of the groups the left prune enters"
    assert t["redo"] <= 0.001 * len(pairs), f"{t['redo']} redo lanes"


Z100 = dict(zdrop=100)
DEFAULT = dict(zdrop=100, end_bonus=5)
# name: (builder, w, scoring, the event the batch is built for)
BUILT = {
    "c2_shaped": (lambda: pcb.c2_shaped(4096, 71), 100, DEFAULT, "prunes"),
    "collapse_120_z100": (lambda: pcb.late_collapse(1024, 74, at=120), 100, Z100, "final"),
    "classes_w100": (lambda: pcb.class_edges(512, 76), 100, DEFAULT, "classes"),
    "a_clipped_tails_z100": (lambda: pcb.clipped_tails(1536, 81), 100, Z100, "final"),
    "a_clipped_tails_z0": (lambda: pcb.clipped_tails(1536, 82), 100, dict(zdrop=0), "final"),
    "b_second_diagonal": (lambda: pcb.second_diagonal(1024, 83), 100, DEFAULT, "refuse_or_redo"),
    "c_late_insertion": (lambda: pcb.late_insertion(1024, 84), 100, DEFAULT, "retreat"),
    "d_low_h0": (lambda: pcb.low_h0(2048, 85), 100, DEFAULT, "low_h0"),
    "e_w20": (lambda: pcb.c2_shaped(2048, 86), 20, DEFAULT, "band"),
    "f_class_tops": (lambda: pcb.class_tops(3, 87), 100, DEFAULT, "classes"),
    "g_odd_lane": (lambda: pcb.odd_lane(16, 88), 100, dict(zdrop=10), "odd"),
}


def vouch(name, what, pairs, ref, qer, redo, wst):
    """What the model must show for a built batch to test what it is built for (the GPU test calls it
    too).  `redo` is the per-pair redo mark, `wst` the per-wave figures."""
    t = pwm.totals(wst)
    n = len(pairs)
    print(f"{name}: {n} pairs in {len(wst)} waves, model: right-prune events {t['right_events']}, group tests refused "
          f"{t['refused']}, clipped lanes {t['clipped']}, retreats {t['retreats']}, redo lanes {t['redo']} (crossing "
          f"{t['redo_crossing']}, item 12's {t['redo_item12']}, final {t['redo_final']}), groups per row "
          f"{t['entered'] / t['rows']:.2f}")
    assert int(redo.sum()) == t["redo"]
    assert t["right_events"] > 0, f"{name}: the right prune never fired"
    if what == "prunes":              # the cap is set, clips lanes and costs next to no redo
        assert t["clipped"] > 0 and t["redo"] <= n // 100
    if what == "final":               # (a) tails that do not align: the final certificate redoes the capped lanes
        assert t["clipped"] > 64 and t["redo_final"] > 64, f"{name}: {t['redo_final']} lanes redone by the final certificate"
    if what == "refuse_or_redo":      # (b) high cells right of the cap: the zeroing test refuses, or the lane is redone
        assert t["refused"] > 0
        assert t["clipped"] == 0 or t["redo"] >= t["clipped"], f"{name}: a capped lane was certified"
    if what == "retreat":             # (c) soft retreat and certificate
        assert t["clipped"] > 0 and t["retreats"] > 0
        assert t["redo_crossing"] + t["redo_final"] > 0, f"{name}: no certificate fired"
    if what == "low_h0":              # (d) the tail dies left of any cap: no lane is redone for crossing it
        assert t["redo_crossing"] == 0 and t["redo"] <= n // 100
    if what == "band":                # (e) the band's edge stays left of the cap, throughout
        assert t["clipped"] == 0 and t["redo"] == 0, f"{name}: {t['clipped']} lanes clipped, {t['redo']} redone"
    if what == "classes":             # (f) both classes that carry the rule prune
        wcls = pcb.qmax_class(pairs)[pcb.default_order(pairs, ref, qer)][::64]
        assert len(wcls) == len(wst)
        for c in (3, 4):
            assert wst[wcls == c, pwm.WST.index("right_events")].sum() > 0, f"{name}: class {c} never pruned"
        assert t["clipped"] > 0
    if what == "odd":                 # (g) P is raised in staying lanes only: exactly the odd lanes are redone, the
        odd = np.arange(n) % 64       # lanes that stay owe nothing for them
        odd = (odd == 7) | (odd == 29)
        assert t["clipped"] > 0 and not redo[~odd].any(), f"{name}: {int(redo[~odd].sum())} related lanes redone"
        assert t["redo_final"] == 0 and t["redo_crossing"] == 0


def test_model_built_cases(models):
    """The batches the GPU test runs, in the engine's wave layout: exact, each shows its event."""
    lib, elib = models
    for name, (make, w, sc, what) in BUILT.items():
        pairs, ref, qer = make()
        params = oracle.make_params(**sc)
        want = pairs.copy()
        oracle.get_scores(params, want, ref, qer, w, nthreads=8)
        _, rows0, _ = esm.run(elib, params, pairs, ref, qer, w, 0)
        got, rows, redo, wst = pwm.run_planned(lib, params, pairs, ref, qer, w)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: field {f} differs"
        assert (rows <= rows0).all()
        vouch(name, what, pairs, ref, qer, redo, wst)
