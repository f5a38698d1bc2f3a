"""The early stop of the packed-column kernel as a CPU model: the literal
ksw_extend2 loop with the rule added (tests/early_stop_model.py) must give the oracle's six
outputs on every pair, for the scalar bound, the per-cell bound and the kernel's schedule of the
two -- and must actually retire pairs, or the check would be vacuous."""

import itertools

import numpy as np
import pytest

import bsw
import early_stop_model as esm
import oracle

MODES = {1: "scalar bound", 2: "per-cell bound", 3: "kernel schedule"}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return esm.build(tmp_path_factory.mktemp("es_model"))


def _check(model, params, pairs, ref, qer, w, tag):
    """Outputs of every mode against the oracle; returns {mode: (retired pairs, rows)} and the
    literal loop's rows."""
    want = pairs.copy()
    oracle.get_scores(params, want, ref, qer, w, nthreads=8)
    got0, rows0, fired0 = esm.run(model, params, pairs, ref, qer, w, 0)
    assert (fired0 == -1).all()
    res = {}
    for mode in (0, 1, 2, 3):
        got, rows, fired = (got0, rows0, fired0) if mode == 0 else esm.run(model, params, pairs, ref, qer, w, mode)
        for f in bsw.OUT_FIELDS:
            bad = np.flatnonzero(want[f] != got[f])
            assert len(bad) == 0, (f"{tag} mode {mode}: field {f} differs in {len(bad)} pairs; first {bad[0]} "
                                   f"tlen={pairs['len1'][bad[0]]} qlen={pairs['len2'][bad[0]]} "
                                   f"h0={pairs['h0'][bad[0]]} want {want[f][bad[0]]} got {got[f][bad[0]]} "
                                   f"fired at row {fired[bad[0]]}")
        assert (rows <= rows0).all()
        res[mode] = (int((rows < rows0).sum()), int(rows.sum()))
    return res


def test_model_random_shapes(model):
    """>= 300,000 random shapes: tlen 1-320, qlen 1-159, h0 0-96, w 0, 1 and every tenth value up
    to 200, zdrop 0 / small / 100, end_bonus 0 / 5; random, exact, mutated, heavily mutated and
    period-2 queries, an eighth at diagonal offsets up to 40."""
    combos = list(itertools.product((0, 1) + tuple(range(10, 201, 10)), (0, 10, 100), (0, 5)))
    per = 300_000 // len(combos) + 1
    n = 0
    retired = {1: 0, 2: 0, 3: 0}
    for k, (w, zdrop, eb) in enumerate(combos):
        pairs, ref, qer = esm.random_shapes(per, seed=1000 + k)
        res = _check(model, oracle.make_params(zdrop=zdrop, end_bonus=eb), pairs, ref, qer, w,
                     f"random w={w} zdrop={zdrop} end_bonus={eb}")
        n += len(pairs)
        for mode in retired:
            retired[mode] += res[mode][0]
    assert n >= 300_000
    share = {MODES[m]: round(retired[m] / n, 3) for m in retired}
    print(f"random shapes: {n} pairs, retired early {share}")
    for mode in (1, 2):
        assert retired[mode] >= 0.40 * n, f"{MODES[mode]} retired only {retired[mode]} of {n}"


def test_model_c2(model):
    """100,000 pairs of the flagship batch (150 bp query, 300 bp window, w = 100)."""
    pairs, ref, qer = bsw.synth_batch(100_000)
    res = _check(model, oracle.make_params(), pairs, ref, qer, 100, "C2")
    n = len(pairs)
    print("C2: rows per pair " + ", ".join(f"{'literal' if m == 0 else MODES[m]} {res[m][1] / n:.1f}" for m in res)
          + "; retired early " + ", ".join(f"{MODES[m]} {res[m][0] / n:.3f}" for m in (1, 2, 3)))
    for mode in (1, 2, 3):
        assert res[mode][0] >= 0.85 * n, f"{MODES[mode]} retired only {res[mode][0]} of {n}"
