"""The packed-column kernel's early stop (bsw_pc.hip) on the GPU: all six output
fields against the CPU oracle, for the int16 planes (kernel8 = 1) and the byte planes (kernel8 = 2),
on small batches of the shapes where a premature or a disturbing stop would show.  The CPU model of
the rule (tests/early_stop_model.py, the kernel's schedule) vouches that each batch exercises it:
at least half of its pairs are retired early."""

import numpy as np
import pytest

import bsw
import bswgen
import early_stop_model as esm
import hiprt
import oracle

pytestmark = pytest.mark.gpu

N = 1536                      # pairs per batch: 24 waves


def _related(shapes, seed):
    return bswgen.pairs_from_shapes(shapes, seed, p_unrelated=0.0)


def _narrow(w):
    """tlen >> qlen under a narrow band: beg > 0 and end == qlen early and for many rows."""
    rng = np.random.default_rng(100 + w)
    q = rng.integers(30, 159, N)
    return _related([(int(x) + int(rng.integers(80, 160)), int(x), int(rng.integers(0, 90))) for x in q], 200 + w)


def _short_windows():
    """tlen in {qlen - 5, qlen, qlen + 3} under a narrow band: the window ends within a few rows of
    the query's last column, so the scalar bound's tlen - 1 - i cap decides.  Only windows longer
    than the query leave rows to drop: they are three fifths of the batch."""
    rng = np.random.default_rng(31)
    q = rng.integers(40, 159, N)
    d = rng.choice([-5, 0, 3, 3, 3], N)
    return _related([(int(x + y), int(x), int(rng.integers(10, 90))) for x, y in zip(q, d)], 32)


def _c2_small(seed, h0=None):
    """The flagship shape at test size: qlen 120-150, window 2 qlen; h0 = None draws 19-100, else
    h0 + min(qlen, tlen) == h0 (the 8-bit regime's top value)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(120, 151, N)
    return _related([(2 * int(x), int(x), int(rng.integers(19, 101)) if h0 is None else h0 - int(x)) for x in q],
                    seed + 1)


def _mixed():
    """Lanes that retire at row ~ qlen beside lanes that run to the window's end: the same
    (tlen, qlen) and h0 range for both, so no sort key separates them.  The run-on pairs place the
    query 92-96 rows down the window, so that it runs off the window's last row (best improves on
    every row to the end); three fifths retire."""
    rng = np.random.default_rng(77)
    items = []
    Q, T = 140, 232
    for k in range(260):
        r = rng.integers(0, 4, T).astype(np.uint8)
        d = 0 if k % 5 < 3 else int(rng.integers(92, 97))
        q = bswgen.mutate(rng, r[d:], Q, 0.02, 0.002)
        items.append((r, q, int(rng.integers(105, 111))))
    return bswgen.assemble(items)


def _qclass(qlen):
    h0s = np.random.default_rng(qlen).integers(5, min(96, 255 - qlen), N)
    return _related([(2 * qlen + 20, qlen, int(h)) for h in h0s], 900 + qlen)


DEFAULT = dict(zdrop=100, end_bonus=5)
BATCHES = {
    "narrow_w1": (lambda: _narrow(1), 1, DEFAULT),
    "narrow_w5": (lambda: _narrow(5), 5, DEFAULT),
    "narrow_w20": (lambda: _narrow(20), 20, DEFAULT),
    "late_diagonal": (lambda: esm.diagonal_pairs(N, 41), 100, DEFAULT),
    "late_twice": (lambda: esm.diagonal_pairs(N, 42, twice=True), 100, DEFAULT),
    "gscore_ties": (lambda: bswgen.repeat_pairs(N, 43, L=(20, 158), h0=(1, 95)), 100, DEFAULT),
    "short_windows_w5": (_short_windows, 5, DEFAULT),
    "short_windows_w20": (_short_windows, 20, DEFAULT),
    "zdrop0": (lambda: _c2_small(51), 100, dict(zdrop=0, end_bonus=5)),
    "end_bonus0": (lambda: _c2_small(52), 100, dict(zdrop=100, end_bonus=0)),
    "h255": (lambda: _c2_small(53, h0=255), 100, DEFAULT),
    "mixed": (_mixed, 100, DEFAULT),
    **{f"qlen{q}": ((lambda q=q: _qclass(q)), 100, DEFAULT) for q in (20, 60, 90, 120, 150, 158)},
}
MIXED_SIZES = (1, 63, 64, 65, 257)
_cache = {}


def _batch(name, tmp_path_factory):
    """(pairs, ref, qer, w, scoring, oracle outputs, model's retired flags, model's rows), built once."""
    if name not in _cache:
        make, w, sc = BATCHES[name]
        pairs, ref, qer = make()
        par = oracle.make_params(**sc)
        want = pairs.copy()
        oracle.get_scores(par, want, ref, qer, w, nthreads=8)
        lib = esm.build(tmp_path_factory.mktemp("es_model"))
        _, rows0, _ = esm.run(lib, par, pairs, ref, qer, w, 0)
        got, rows3, _ = esm.run(lib, par, pairs, ref, qer, w, 3)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: the model disagrees with the oracle in {f}"
        _cache[name] = (pairs, ref, qer, w, sc, want, rows3 < rows0, rows3)
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


def _run(eng, pairs, ref, qer, w, want, tag):
    dp, dr, dq = (hiprt.DeviceBuffer.from_array(a) for a in (pairs, ref, qer))
    eng.get_scores_device(dp.ptr, dr.ptr, dq.ptr, len(pairs), w)
    got = dp.download(np.empty_like(pairs))
    assert eng.last_stats().n_packed == len(pairs), f"{tag}: not every pair ran in the packed-column kernel"
    bad = np.zeros(len(pairs), bool)
    for f in bsw.OUT_FIELDS:
        bad |= want[f] != got[f]
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {len(pairs)} pairs differ; first idx {i} "
                             f"len1={want[i]['len1']} len2={want[i]['len2']} h0={want[i]['h0']} "
                             f"want={[int(want[i][f]) for f in bsw.OUT_FIELDS]} "
                             f"got={[int(got[i][f]) for f in bsw.OUT_FIELDS]}")


@pytest.mark.parametrize("kernel8", [1, 2])
@pytest.mark.parametrize("name", [n for n in BATCHES if n != "mixed"])
def test_early_stop_batch(engine, tmp_path_factory, name, kernel8):
    pairs, ref, qer, w, sc, want, retired, _ = _batch(name, tmp_path_factory)
    print(f"{name}: {len(pairs)} pairs, model retires {retired.mean():.3f} early")
    assert retired.mean() >= 0.5, f"{name}: only {retired.mean():.3f} of the pairs exercise the rule"
    if name == "h255":
        assert (pairs["h0"] + np.minimum(pairs["len1"], pairs["len2"]) == 255).all()
    _run(engine(kernel8, sc), pairs, ref, qer, w, want, f"{name} kernel8={kernel8}")


@pytest.mark.parametrize("kernel8", [1, 2])
@pytest.mark.parametrize("n", MIXED_SIZES)
def test_early_stop_mixed_waves(engine, tmp_path_factory, n, kernel8):
    """Retired lanes beside lanes that run on, at batch sizes around the wave size: the retired
    ones must not disturb the band union or their neighbours' outputs."""
    pairs, ref, qer, w, sc, want, retired, rows = _batch("mixed", tmp_path_factory)
    runon = rows[:n] == pairs["len1"][:n]               # the model ran the window's every row
    print(f"mixed n={n}: model retires {retired[:n].mean():.3f} early (rows {rows[:n][retired[:n]].mean():.0f}), "
          f"{runon.mean():.3f} run to the last row")
    assert retired[:n].mean() >= 0.5 and (n == 1 or runon.mean() >= 0.3)
    assert np.median(rows[:n][retired[:n]]) <= 160      # the retiring lanes stop soon after row qlen = 140
    _run(engine(kernel8, sc), pairs[:n].copy(), ref, qer, w, want[:n], f"mixed n={n} kernel8={kernel8}")
