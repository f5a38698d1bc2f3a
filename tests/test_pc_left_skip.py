"""The packed-column kernel's left skip (bsw_pc.hip) on the GPU: all six
output fields bit-exact against the CPU oracle, for the int16 planes (kernel8 = 1) and the byte
planes (kernel8 = 2), on small batches of the shapes where a skip that dropped live cells -- or a
dead lane that held gz back or corrupted it -- would show.  The CPU model of the kernel's loop
(tests/pc_wave_model.py with both prunes off, run in the engine's wave layout) vouches that each batch exercises the
skip: it reports the groups it removed from the entered set."""

import numpy as np
import pytest

import bsw
import bswgen
import hiprt
import oracle
import pc_batches as pcb
import pc_wave_model as pwm

pytestmark = pytest.mark.gpu

DEFAULT = dict(zdrop=100, end_bonus=5)


def _prefix_at_beg0():
    """a. The common case: qlen 150, tlen 300, w 100 -- the prefix forms while beg == 0."""
    shapes = [(300, 150, h0) for h0 in (1, 7, 19, 30) for _ in range(512)]
    return bswgen.pairs_from_shapes(shapes, 61, p_unrelated=0.05)


def _quick_prefix(seed):
    """b. Every QMAX class (qlen 31, 63, 95, 127, 159), exact and 5 %-mutated queries, h0 0-30.
    Under a narrow band a lane's static beg soon leaves column 0 behind, and a stale boundary
    value in slot 0 (h0 > o_del + e_del (w + 1)) then pins gz for good: the default key sorts
    the exact pairs of one length by h0, so only the waves of the smallest h0 get to skip -- hence
    six waves of exact pairs per length."""
    rng = np.random.default_rng(seed)
    items = []
    for qlen in (31, 63, 95, 127, 159):
        for k in range(512):
            r = rng.integers(0, 4, qlen + 90).astype(np.uint8)
            q = r[:qlen].copy() if k & 3 else bswgen.mutate(rng, r, qlen, 0.05, 0.0)
            items.append((r, q, int(rng.integers(0, 31))))
    return bswgen.assemble(items)


BATCHES = {
    "a_prefix_at_beg0": (_prefix_at_beg0, 100, DEFAULT),
    "b_quick_w5": (lambda: _quick_prefix(62), 5, DEFAULT),
    "b_quick_w10": (lambda: _quick_prefix(63), 10, DEFAULT),
    "b_quick_w20": (lambda: _quick_prefix(64), 20, DEFAULT),
    "c_boundary_alive": (lambda: pcb.boundary_alive(2048, 65), 100, DEFAULT),
    "d_interior_zeros": (lambda: pcb.interior_zeros(2048, 66), 100, DEFAULT),
    "e_pin_dies": (lambda: pcb.pinned_waves(5, 67, True), 100, pcb.PIN_SCORING),
    "e_pin_lives": (lambda: pcb.pinned_waves(5, 67, False), 100, pcb.PIN_SCORING),
    "f_uneven_lifetimes": (lambda: pcb.uneven_lifetimes(30, 68), 100, DEFAULT),
}
_cache = {}


def _batch(name, tmp_path_factory):
    """(pairs, ref, qer, w, scoring, oracle outputs, model's per-wave figures), built once."""
    if name not in _cache:
        make, w, sc = BATCHES[name]
        pairs, ref, qer = make()
        par = oracle.make_params(**sc)
        want = pairs.copy()
        oracle.get_scores(par, want, ref, qer, w, nthreads=8)
        lib = pwm.build(tmp_path_factory.mktemp("pc_model"))
        got, _, _, wst = pwm.run_planned(lib, par, pairs, ref, qer, w, prune=False, rprune=False)
        for f in bsw.OUT_FIELDS:
            assert np.array_equal(want[f], got[f]), f"{name}: the model disagrees with the oracle in {f}"
        _cache[name] = (pairs, ref, qer, w, sc, want, wst)
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
@pytest.mark.parametrize("name", list(BATCHES))
def test_left_skip_batch(engine, tmp_path_factory, name, kernel8):
    pairs, ref, qer, w, sc, want, wst = _batch(name, tmp_path_factory)
    rows, ent, skp = (int(x) for x in wst[:, :3].sum(0))
    print(f"{name}: {len(pairs)} pairs in {len(wst)} waves, model skips {skp} of {ent + skp} entered groups "
          f"({(ent + skp) / rows:.2f} -> {ent / rows:.2f} per row)")
    assert skp > 0, f"{name}: the model never skips a group on this batch"
    if name.startswith("e_"):
        # the waves are the ones built: the pinning lane first, its 63 neighbours after it
        order = pcb.default_order(pairs, ref, qer).reshape(-1, 64)
        assert (pairs["h0"][order[:, 0]] == 100).all() and (pairs["h0"][order[:, 1:]] <= 10).all()
        other = _batch("e_pin_lives" if name == "e_pin_dies" else "e_pin_dies", tmp_path_factory)[6]
        lives, dies = (wst, other) if name == "e_pin_lives" else (other, wst)
        assert lives[:, 2].sum() < dies[:, 2].sum()          # a pinning lane that lives on holds gz back
    if name.startswith("f_"):
        assert len(pairs) % 64 != 0 and (pairs["len1"] <= 40).any() and (pairs["len1"] == 300).any()
    if name.startswith("c_"):
        assert (pairs["h0"] == 100).all()
    _run(engine(kernel8, sc), pairs, ref, qer, w, want, f"{name} kernel8={kernel8}")
