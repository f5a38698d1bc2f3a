"""The packed-column kernel's left skip as a CPU model of the KERNEL's loop
(tests/pc_wave_model.py with both prunes off): 64 lanes per wave with the static left edge, the wave-uniform prefix
bound gz refreshed on the kernel's phase from the live lanes' stored rows, groups below gz not
computed, and the early stop scanning only entered groups.  It must give the oracle's six outputs
on every pair, run no more rows per lane than the literal loop -- and must actually skip groups,
or the check would be vacuous."""

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
    """The model with the skip on the lanes in `order`: 0 differing fields against the oracle, rows
    per lane no more than the literal loop's.  Returns (want, rows0, [rows, entered, skipped])."""
    lib, elib = models
    if want is None:
        want = pairs.copy()
        oracle.get_scores(params, want, ref, qer, w, nthreads=8)
        _, rows0, _ = esm.run(elib, params, pairs, ref, qer, w, 0)
    got, rows, _, wst = pwm.run(lib, params, pairs, ref, qer, w, order=order, prune=False, rprune=False)
    for f in bsw.OUT_FIELDS:
        bad = np.flatnonzero(want[f] != got[f])
        assert len(bad) == 0, (f"{tag}: field {f} differs in {len(bad)} pairs; first {bad[0]} "
                               f"tlen={pairs['len1'][bad[0]]} qlen={pairs['len2'][bad[0]]} h0={pairs['h0'][bad[0]]} "
                               f"want {want[f][bad[0]]} got {got[f][bad[0]]}")
    assert (rows <= rows0).all(), f"{tag}: a lane ran more rows than the literal loop"
    return want, rows0, wst[:, :3].sum(0)


def test_model_random_shapes(models):
    """>= 300,000 shapes of early_stop_model.random_shapes and diagonal_pairs: w 0, 1 and every
    tenth value up to 200, zdrop 0 / 10 / 100, end_bonus 0 / 5; the lanes grouped into waves by the
    default sort key and shuffled (lanes of every length and h0 side by side: one lane with no zero
    prefix pins gz for its wave)."""
    combos = list(itertools.product((0, 1) + tuple(range(10, 201, 10)), (0, 10, 100), (0, 5)))
    per = 300_000 // len(combos) + 1
    n = 0
    tot = {"sorted": np.zeros(3, np.int64), "shuffled": np.zeros(3, np.int64)}
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
    # the diagonal batches are a quarter the size of the others: make up the count
    extra = 0
    while n + extra < 300_000:
        pairs, ref, qer = esm.random_shapes(per, seed=5000 + extra)
        want, rows0, st = _check(models, oracle.make_params(), pairs, ref, qer, 100,
                                 pcb.default_order(pairs, ref, qer), "extra sorted")
        tot["sorted"] += st
        extra += len(pairs)
    n += extra
    assert n >= 300_000
    for name, (rows, ent, skp) in tot.items():
        print(f"random shapes, {name} waves: {n} pairs, groups per row {ent / rows:.2f} with the skip, "
              f"{(ent + skp) / rows:.2f} without; skipped share {skp / (ent + skp):.4f}")
    # (the pinning lane itself is asserted on waves built for it: test_model_built_cases)
    for name in tot:
        assert tot[name][2] > 0, f"the skip never fired on the {name} waves"


def test_model_c2(models):
    """100,000 pairs of the flagship batch (150 bp query, 300 bp window, w = 100) in the waves of
    the default sort key: the figures the stats build (tools/pc_stats.py) is compared with."""
    lib, _ = models
    pairs, ref, qer = bsw.synth_batch(100_000)
    params = oracle.make_params()
    order = pcb.default_order(pairs, ref, qer)
    _, _, (rows, ent, skp) = _check(models, params, pairs, ref, qer, 100, order, "C2")
    _, rows_off, _, wst_off = pwm.run(lib, params, pairs, ref, qer, 100, order=order, skip=False, prune=False, rprune=False)
    r0, e0, s0 = wst_off[:, :3].sum(0)
    assert s0 == 0 and e0 == ent + skp and r0 >= rows
    share = skp / (ent + skp)
    cfg = pwm.defaults(lib)
    print(f"C2 (refresh on rows with (i & {cfg.skip_mask}) == {cfg.skip_row}): rows per wave {rows / len(wst_off):.1f} "
          f"({r0 / len(wst_off):.1f} without the skip), groups entered per row {ent / rows:.2f} with the skip, "
          f"{e0 / r0:.2f} without; skipped share of entered groups {share:.4f}")
    assert share >= 0.05, f"the skip removes only {share:.4f} of the entered groups"


def test_model_built_cases(models):
    """The batches the GPU test runs, in the engine's wave layout: exact, and each skips."""
    lib, elib = models
    skipped = {}
    for name, (pairs, ref, qer) in {
        "boundary_alive": pcb.boundary_alive(512, 11),
        "pin_dies": pcb.pinned_waves(4, 12, True),
        "pin_lives": pcb.pinned_waves(4, 12, False),
        "uneven": pcb.uneven_lifetimes(5, 13),
        "interior": pcb.interior_zeros(512, 14),
    }.items():
        params = oracle.make_params(**(pcb.PIN_SCORING if name.startswith("pin") else {}))
        want = pairs.copy()
        oracle.get_scores(params, want, ref, qer, 100, nthreads=8)
        _, rows0, _ = esm.run(elib, params, pairs, ref, qer, 100, 0)
        got, rows, _, wst = pwm.run_planned(lib, params, pairs, ref, qer, 100, prune=False, rprune=False)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: field {f} differs"
        assert (rows <= rows0).all()
        skipped[name] = int(wst[:, 2].sum())
        print(f"{name}: {len(pairs)} pairs, skipped groups {skipped[name]} of {int(wst[:, 1:3].sum())}")
        assert skipped[name] > 0, f"{name}: the skip never fired"
    # every wave of the pinned batches holds its one pinning lane, first in the wave
    for dies in (True, False):
        pairs, ref, qer = pcb.pinned_waves(4, 12, dies)
        order = pcb.default_order(pairs, ref, qer).reshape(-1, 64)
        assert (pairs["h0"][order[:, 0]] == 100).all() and (pairs["h0"][order[:, 1:]] <= 10).all()
    # a pinning lane that lives on holds gz back for about its h0 rows
    assert skipped["pin_lives"] < skipped["pin_dies"]
