"""The packed-column kernel's right-edge (masked-R) group body on the packed F chain (bsw_pc.hip,
DESIGN.md §4.2) on the GPU.  All six output fields bit-exact against the CPU oracle, for the int16
planes (kernel8 = 1) and the byte planes (kernel8 = 2), on small batches built so that the band's
right edge takes every shape the body tells apart: where a lane's end falls in its group, lanes
of one wave at the same end, one column apart or many, ends that shrink and grow again, and lanes
that die beside live ones.  (Batch a was laid out for the qlen-tail body as well, one qlen per
wave; that body was measured slower and is not in the tree, DESIGN.md §9 -- the batch stays as the
case where every live lane of a wave shares its end.)"""

import numpy as np
import pytest

import bsw
import bswgen
import hiprt
import oracle
import pc_batches as pcb

pytestmark = pytest.mark.gpu

DEFAULT = dict(zdrop=100, end_bonus=5)
CLASS_TOPS = (32, 64, 96, 128, 160)


def _seq(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _exact(rng, qlen, tlen, h0):
    r = _seq(rng, max(tlen, qlen))
    return (r[:tlen], r[:qlen].copy(), h0)


def _one_qlen_per_wave():
    """a. qlen at every residue mod 4 below each class edge (28-31 .. 156-159; the multiples of 4 put
    slot end alone in the last group), exact copies (end == qlen from row 0), 128 pairs = two whole
    waves per qlen: every wave has one qlen, so all its live lanes share one end on every row."""
    rng = np.random.default_rng(71)
    items = []
    for top in CLASS_TOPS:
        for qlen in range(top - 4, top):
            items += [_exact(rng, qlen, qlen + 40, int(rng.integers(1, 31))) for _ in range(128)]
    return bswgen.assemble(items)


def _mixed_qlens():
    """b. The same pairs with three qlens (top - 4, top - 3, top - 1), 44 pairs each, and two
    (top - 2, top - 1), 40 each, per class: the default key ties them into shared waves, whose
    lanes end one to three columns apart on every row."""
    rng = np.random.default_rng(72)
    items = []
    for top in CLASS_TOPS:
        for qlen, n in ((top - 4, 44), (top - 3, 44), (top - 1, 44)):
            items += [_exact(rng, qlen, qlen + 40, int(rng.integers(1, 31))) for _ in range(n)]
    a = bswgen.assemble(items)
    items = []
    for top in CLASS_TOPS:
        for qlen, n in ((top - 2, 40), (top - 1, 40)):
            items += [_exact(rng, qlen, qlen + 40, int(rng.integers(1, 31))) for _ in range(n)]
    return a, bswgen.assemble(items)


def _close_ends():
    """c. Lanes of one wave whose band ends differ by a few columns on the same rows: one qlen and
    one tlen / 32 bucket per wave, every query an exact copy of the window's first 40 bases (the
    default key then ties in all but h0, as in pc_batches.pinned_waves) and 2-10 % substitutions
    after them; h0 1-100 sets how far right of the diagonal a row stays positive."""
    rng = np.random.default_rng(73)
    items = []
    for qlen, tlen in ((150, 300), (101, 230), (150, 170)):
        for _ in range(448):
            r = _seq(rng, tlen)
            q = r[:qlen].copy()
            sub = np.flatnonzero(rng.random(qlen) < rng.uniform(0.02, 0.10))
            sub = sub[sub >= 40]
            q[sub] = (q[sub] + rng.integers(1, 4, len(sub))) & 3
            items.append((r, q, int(rng.integers(1, 101))))
    return bswgen.assemble(items)


def _degenerate():
    """e. qlen 1-4, tlen 1, h0 = 1, h0 + min(qlen, tlen) = 255 (the key's top byte), N runs in
    queries and windows, and lanes that die in the first rows beside live ones (bases 10-40 copy the
    window, so the key ties; bases 0-10 do not, and h0 = 1 ends the lane at once)."""
    rng = np.random.default_rng(75)
    items = []
    for qlen in (1, 2, 3, 4):
        for tlen in (1, 2, 5, 50):
            for h0 in (1, 2, 20, 250):
                items += [_exact(rng, qlen, tlen, h0) for _ in range(4)]
                items.append((_seq(rng, tlen), _seq(rng, qlen), h0))
    for qlen in (5, 10, 31, 32, 63, 100, 150, 159):
        items += [_exact(rng, qlen, max(qlen, 1), 1) for _ in range(8)]          # h0 = 1
        items += [(_seq(rng, 1), _seq(rng, qlen), h0) for h0 in (1, 7, 60)]        # tlen 1
        r = _seq(rng, 1)
        items += [(r, np.full(qlen, r[0], np.uint8), 30)]
    for qlen, tlen in ((150, 300), (100, 60), (31, 40), (159, 159), (4, 9)):
        items += [_exact(rng, qlen, tlen, 255 - min(qlen, tlen)) for _ in range(16)]
    for _ in range(192):                                                          # N runs
        r = _seq(rng, 300)
        q = r[:150].copy()
        for arr in (r, q):
            for _ in range(int(rng.integers(0, 3))):
                s = int(rng.integers(0, len(arr) - 12))
                arr[s:s + int(rng.integers(1, 12))] = 4
        items.append((r, q, int(rng.integers(1, 60))))
    for k in range(384):                                                          # early deaths
        r = _seq(rng, 300)
        q = r[:150].copy()
        if k % 4 == 1:
            q[:10] = (q[:10] + 1 + (k >> 2) % 3) & 3
            items.append((r, q, 1))
        else:
            items.append((r, q, int(rng.integers(1, 40))))
    return bswgen.assemble(items)


BATCHES = {
    "a_tail": (_one_qlen_per_wave, 100),
    "b_mixed3": (lambda: _mixed_qlens()[0], 100),
    "b_mixed2": (lambda: _mixed_qlens()[1], 100),
    "c_close_ends": (_close_ends, 100),
    "c_close_ends_w20": (_close_ends, 20),
    "d_stale_slots": (lambda: pcb.interior_zeros(2048, 74), 100),
    "e_degenerate": (_degenerate, 100),
}
_cache = {}


def _batch(name):
    """(pairs, ref, qer, w, oracle outputs), built once and left unchanged."""
    if name not in _cache:
        make, w = BATCHES[name]
        pairs, ref, qer = make()
        want = pairs.copy()
        oracle.get_scores(oracle.make_params(**DEFAULT), want, ref, qer, w, nthreads=8)
        _cache[name] = (pairs, ref, qer, w, want)
    return _cache[name]


_engines = {}


@pytest.fixture(scope="module")
def engine():
    def get(kernel8):
        if kernel8 not in _engines:
            _engines[kernel8] = bsw.Engine(bsw.default_params(**DEFAULT), kernel8=kernel8, small_batch=0, mid_batch=0)
        return _engines[kernel8]
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
def test_right_edge_batch(engine, name, kernel8):
    pairs, ref, qer, w, want = _batch(name)
    if name == "a_tail":                 # one qlen per wave, in the engine's own lane order
        order = pcb.default_order(pairs, ref, qer)
        cls = pcb.qmax_class(pairs)[order]
        for c in range(5):
            q = pairs["len2"][order][cls == c].reshape(-1, 64)
            assert (q == q[:, :1]).all()
    if name.startswith("b_"):            # every class has a wave of two qlens
        order = pcb.default_order(pairs, ref, qer)
        cls = pcb.qmax_class(pairs)[order]
        for c in range(5):
            q = pairs["len2"][order][cls == c]
            assert any(len(set(q[k:k + 64])) > 1 for k in range(0, len(q), 64))
    _run(engine(kernel8), pairs, ref, qer, w, want, f"{name} kernel8={kernel8}")
