"""Band edges and class bounds of the wave-per-alignment kernel (bsw_wv.hip),
and band-edge inputs on every extension kernel.  Every comparison is against the literal
ksw_extend2 oracle, all six output fields, tolerance zero.

What the cases pin down, by the place in the code:
  a  wv_kernel<16> (8-register planes, in-lane F prefix over 8 registers), with and without the
     window slide (qlen 600 < 1024 < 1100);
  b  the band caps wl = 125 | 126, 251 | 252, 503 | 504 between C = 4, 8, 16 and the wide kernel:
     at the tight ones the band, slot `end` and the C-alignment of the window start fill the
     64 * C window to its last column (`end` at wb + WIN - 1);
  c  the best path ON the band edge (|j - i| = w) of the wave kernel at those three caps: an
     off-by-one in beg / end, in the `j <= end` / `j < end` write masks or in the slide changes
     score or max_off here and nowhere in mutate()'s 1-3 bp indels;
  d  the same edge on the packed-column, lane and row-group kernels (left skip, left prune and
     right-edge pruning included) and once more on the wave kernel;
  e  columns that enter the sliding window with a non-zero first row (`jn` in the slide loop),
     and e': inputs whose outputs are made of those entering values;
  f  the int16 class bounds of wv_class() at their last admitted value;
  g  non-default scoring on long queries (kem at large j, the per-pair band cap);
  h  one block running a longer, then a shorter or empty pair (s_q refill, grid = 8192).

Input conditions (that the inputs are what the case needs) are asserted from the oracle and the
routing model alone, before any GPU call, and stand as CPU tests of their own below.
"""

from functools import lru_cache

import numpy as np
import pytest

import bsw
import bswgen
import first_row_model
import oracle
import route_py
from ksw_ext_ref import bwa_fill_scmat

gpu = pytest.mark.gpu

DEFAULT = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, zdrop=100, end_bonus=5)
ZDROP0 = dict(DEFAULT, zdrop=0)
E_INS3 = dict(DEFAULT, e_ins=3)
# case g: three max(mat) == 1 scorings
SCORINGS = (dict(a=1, b=4, o_del=5, e_del=2, o_ins=7, e_ins=3, zdrop=50, end_bonus=3),
            dict(a=1, b=3, o_del=6, e_del=1, o_ins=6, e_ins=1, zdrop=0, end_bonus=0),
            dict(a=1, b=4, o_del=8, e_del=3, o_ins=4, e_ins=2, zdrop=100, end_bonus=10))
PLANNED = dict(small_batch=0, mid_batch=0)      # every batch on the planned path, BSW_OPT_LONG 1


def _oparams(sc):
    return oracle.make_params(o_del=sc["o_del"], e_del=sc["e_del"], o_ins=sc["o_ins"], e_ins=sc["e_ins"],
                              zdrop=sc["zdrop"], end_bonus=sc["end_bonus"], mat=bwa_fill_scmat(sc["a"], sc["b"]))


def _gparams(sc):
    return bsw.default_params(**sc)


def _want(sc, pairs, ref, qer, w):
    want = pairs.copy()
    oracle.get_scores(_oparams(sc), want, ref, qer, w, nthreads=8)
    return want


def _assert_same(want, got, tag):
    bad = np.zeros(len(want), bool)
    for f in bsw.OUT_FIELDS:
        bad |= want[f] != got[f]
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {len(want)} pairs differ; first idx {i} "
                             f"len1={want[i]['len1']} len2={want[i]['len2']} h0={want[i]['h0']} "
                             f"want={[int(want[i][f]) for f in bsw.OUT_FIELDS]} "
                             f"got={[int(got[i][f]) for f in bsw.OUT_FIELDS]}")


def _parity(eng, pairs, ref, qer, w, want, tag, cell_bits=16):
    """One call; the six fields equal the oracle's; returns the call's Stats."""
    got = pairs.copy()
    for f in bsw.OUT_FIELDS:
        got[f] = -9
    eng.get_scores(got, ref, qer, w, cell_bits)
    _assert_same(want, got, tag)
    return eng.last_stats()


def _classes(pairs, sc, w, long):
    return route_py.class_counts(pairs, _gparams(sc), w, long)


def _counts(d):
    return {**{4: 0, 8: 0, 16: 0, "lane": 0, "wide": 0}, **d}


def _assert_routed(st, pairs, sc, w, long, tag):
    n_wave, n_wide = route_py.expected_counts(pairs, _gparams(sc), w, long)
    assert (st.n_wave, st.n_wide) == (n_wave, n_wide), f"{tag}: n_wave, n_wide = {st.n_wave}, {st.n_wide}"


def _edge_shares(want, meta, w):
    """Per (g, kind): the share of pairs whose oracle max_off is g.  Asserts the band-edge
    condition: at least 3/4 for g <= w, and no pair past the band (max_off <= w) for g = w + 1."""
    shares = {}
    for cell in sorted(set(meta)):
        sel = np.array([m == cell for m in meta])
        g = cell[0]
        shares[cell] = float((want["max_off"][sel] == g).mean())
        if g <= w:
            assert shares[cell] >= 0.75, f"w={w} {cell}: only {shares[cell]:.2f} of the pairs have max_off == g"
        else:
            assert int(want["max_off"][sel].max()) <= w, f"w={w} {cell}: max_off past the band"
    return shares


# ---- the routing model itself ---------------------------------------------------------------------

def test_route_model_bounds():
    """route_py.wv_class at every bound of the contract in bsw_kernels.h (default scoring: the
    band cap is min(w, qlen))."""
    p = bsw.default_params()
    got = [route_py.wv_class(p, w, 700, 800, 100) for w in (0, 125, 126, 251, 252, 503, 504)]
    assert got == [4, 4, 8, 8, 16, 16, None]
    assert [route_py.wv_class(p, 503, q, q + 100, 100) for q in (125, 126, 251, 252)] == [4, 8, 8, 16]
    assert route_py.wv_class(p, 100, 2699, 2799, 100) == 4 and route_py.wv_class(p, 100, 2700, 2800, 100) is None
    p3 = bsw.default_params(**E_INS3)
    assert route_py.wv_class(p3, 100, 899, 999, 100) == 4 and route_py.wv_class(p3, 100, 900, 1000, 100) is None
    assert route_py.wv_class(p, 100, 300, 400, 29398) == 4 and route_py.wv_class(p, 100, 300, 400, 29399) is None
    assert route_py.wv_class(p, 100, 300, 400, -1) is None
    assert route_py.wv_class(bsw.default_params(a=2), 100, 300, 400, 50) is None
    # the cap in C integer arithmetic: (ni + e) / e truncates toward zero, then max(., 1)
    assert route_py.band_cap(p3, 100, 0) == 1 and route_py.band_cap(p, 100, 0) == 1
    assert route_py.band_cap(p3, 500, 899) == 300 and route_py.band_cap(bsw.default_params(**SCORINGS[0]), 260, 161) == 53
    # routes: short int16-safe queries stay on the register kernels unless forced
    assert route_py.route(p, 100, 150, 300, 50, 1) == "lane" and route_py.route(p, 100, 150, 300, 50, 2) == 4
    assert route_py.route(p, 100, 161, 300, 50, 1) == 4 and route_py.route(p, 100, 161, 300, 50, 0) == "wide"
    assert route_py.route(p, 100, 150, 300, 32700, 1) == "wide"


# ---- a. C = 16 reads --------------------------------------------------------------------------------

A_BANDS = (252, 300, 503)


@lru_cache(maxsize=None)
def _case_a(L):
    pairs, ref, qer = bswgen.random_pairs(96, seed=1600 + L, tlen=(L + 50, L + 150), qlen=(L, L), h0=(1, 200),
                                          p_sub=(0.0, 0.05), p_indel=(0.0, 0.01))
    for w in A_BANDS:
        assert _classes(pairs, DEFAULT, w, 1) == _counts({16: 96}), f"L={L} w={w}"
    return pairs, ref, qer, {w: _want(DEFAULT, pairs, ref, qer, w) for w in A_BANDS}


@pytest.mark.parametrize("L", [600, 1100])
def test_inputs_c16_reads(L):
    """C1, case a: the model puts all 96 reads in C = 16 at w = 252, 300 and 503; L = 1100 is past
    the 1024-column window, so it slides."""
    pairs, _, _, wants = _case_a(L)
    assert (pairs["len2"] == L).all() and (L > 64 * 16) == (L == 1100)
    assert all((wants[w]["score"] > 0).all() for w in A_BANDS)


@gpu
@pytest.mark.parametrize("L", [600, 1100])
def test_wave_c16_reads(L):
    pairs, ref, qer, wants = _case_a(L)
    e = bsw.Engine(**PLANNED)
    for w in A_BANDS:
        st = _parity(e, pairs, ref, qer, w, wants[w], f"C=16 reads L={L} w={w}")
        assert st.n_wave == len(pairs) and st.n_wide == 0
        _assert_routed(st, pairs, DEFAULT, w, 1, f"L={L} w={w}")
    e.close()


# ---- b. class bounds of wl ------------------------------------------------------------------------

B_BANDS = {125: 4, 126: 8, 251: 8, 252: 16, 503: 16, 504: "wide"}
B_SPREAD_N = 1024


@lru_cache(maxsize=None)
def _case_b():
    pairs, ref, qer = bswgen.random_pairs(48, seed=125, tlen=(800, 800), qlen=(700, 700), h0=(1, 200),
                                          p_sub=(0.0, 0.05), p_indel=(0.0, 0.01), p_unrelated=0.0)
    for w, c in B_BANDS.items():
        assert _classes(pairs, DEFAULT, w, 1) == _counts({c: 48}), f"w={w}"
    return pairs, ref, qer, {w: _want(DEFAULT, pairs, ref, qer, w) for w in B_BANDS}


@lru_cache(maxsize=None)
def _case_b_spread():
    """qlen uniform in 100..700 at w = 503, forced to the wave kernel: the per-pair cap
    wl = min(503, qlen) spreads one batch over C = 4 (qlen <= 125), 8 (<= 251) and 16.
    Only 26 of the 601 lengths fall in C = 4, so 256 pairs would give ~11 there; the batch holds
    1024 pairs of the same distribution (~44 expected) to have at least 32 in every class."""
    rng = np.random.default_rng(503)
    shapes = [(q + 100, q, int(rng.integers(1, 201))) for q in rng.integers(100, 701, B_SPREAD_N).tolist()]
    pairs, ref, qer = bswgen.pairs_from_shapes(shapes, seed=504, p_unrelated=0.0)
    cls = _classes(pairs, DEFAULT, 503, 2)
    assert min(cls[4], cls[8], cls[16]) >= 32 and cls[4] + cls[8] + cls[16] == B_SPREAD_N, cls
    q = pairs["len2"]
    assert cls == _counts({4: int((q <= 125).sum()), 8: int(((q > 125) & (q <= 251)).sum()), 16: int((q > 251).sum())})
    return pairs, ref, qer, _want(DEFAULT, pairs, ref, qer, 503), cls


def test_inputs_class_bounds():
    """C1, case b: 48 reads of qlen 700 sit in C = 4, 8, 8, 16, 16 and on the wide kernel at
    w = 125, 126, 251, 252, 503, 504; the mixed-length batch has >= 32 pairs in each C."""
    _case_b()
    cls = _case_b_spread()[4]
    print("case b spread, pairs per class:", cls)


@gpu
@pytest.mark.parametrize("w", list(B_BANDS))
def test_wave_class_bounds(w):
    pairs, ref, qer, wants = _case_b()
    e = bsw.Engine(**PLANNED)
    st = _parity(e, pairs, ref, qer, w, wants[w], f"class bound w={w}")
    if w == 504:
        assert st.n_wide == len(pairs) and st.n_wave == 0
    _assert_routed(st, pairs, DEFAULT, w, 1, f"w={w}")
    e.close()


@gpu
def test_wave_class_spread():
    pairs, ref, qer, want, _ = _case_b_spread()
    e = bsw.Engine(long=2)
    st = _parity(e, pairs, ref, qer, 503, want, "mixed classes at w=503")
    assert st.n_wave == len(pairs)
    _assert_routed(st, pairs, DEFAULT, 503, 2, "mixed classes")
    e.close()


# ---- c. band-edge gaps, wave kernel --------------------------------------------------------------

C_BANDS = {125: 4, 251: 8, 503: 16}


@lru_cache(maxsize=None)
def _case_c(w):
    pairs, ref, qer, meta = bswgen.gap_pairs(w, 8, seed=w, flank=w + 300, after=300, h0=50)
    assert _classes(pairs, DEFAULT, w, 2) == _counts({C_BANDS[w]: len(pairs)})
    want0 = _want(ZDROP0, pairs, ref, qer, w)
    shares = _edge_shares(want0, meta, w)          # the 3/4 cap holds at zdrop = 0 only:
    # at zdrop = 100 chance matches beside the gap z-drop about half of the w = 503 deletions
    return pairs, ref, qer, {0: want0, 100: _want(DEFAULT, pairs, ref, qer, w)}, shares


@pytest.mark.parametrize("w", list(C_BANDS))
def test_inputs_gap_wave(w):
    """C1, case c: at zdrop = 0 the oracle's max_off is g for at least 3/4 of each (g <= w, kind)
    cell and never past w for g = w + 1; the model puts the batch in C = 4, 8, 16."""
    pairs, _, _, _, shares = _case_c(w)
    assert len(pairs) == 48
    print(f"case c w={w}, share with max_off == g:", shares)


@gpu
@pytest.mark.parametrize("zdrop", [0, 100])
@pytest.mark.parametrize("w", list(C_BANDS))
def test_wave_gap_on_band_edge(w, zdrop):
    pairs, ref, qer, wants, _ = _case_c(w)
    sc = dict(DEFAULT, zdrop=zdrop)
    e = bsw.Engine(_gparams(sc), long=2)
    st = _parity(e, pairs, ref, qer, w, wants[zdrop], f"gap on the band edge w={w} zdrop={zdrop}")
    assert st.n_wave == len(pairs)
    _assert_routed(st, pairs, sc, w, 2, f"w={w}")
    e.close()


# ---- d. band-edge gaps, register kernels -----------------------------------------------------------

@lru_cache(maxsize=None)
def _case_d(w):
    pairs, ref, qer, meta = bswgen.gap_pairs(w, 64, seed=100 + w, flank=30, after=45, h0=50)
    assert int(pairs["len2"].max()) <= 157
    assert int((pairs["h0"] + np.minimum(pairs["len2"], pairs["len1"])).max()) <= 255
    assert _classes(pairs, DEFAULT, w, 1) == _counts({"lane": len(pairs)})
    assert _classes(pairs, DEFAULT, w, 2) == _counts({4: len(pairs)})
    want = _want(DEFAULT, pairs, ref, qer, w)
    return pairs, ref, qer, want, _edge_shares(want, meta, w)


@pytest.mark.parametrize("w", [8, 20, 40])
def test_inputs_gap_register(w):
    """C1, case d: qlen <= 157, the 8-bit regime, and the 3/4 cap at the default zdrop = 100."""
    pairs, _, _, _, shares = _case_d(w)
    assert len(pairs) == 384
    print(f"case d w={w}, share with max_off == g:", shares)


D_ENGINES = {
    "packed": (dict(PLANNED), "n_packed"),
    "lane": (dict(PLANNED, kernel8=0), "n_i16"),
    "group32": ({}, "n_group"),
    "group16": (dict(gq32_max=0), "n_group"),
    "quad": (dict(small_batch=0), "n_group"),
    "wave": (dict(long=2), "n_wave"),
}


@gpu
@pytest.mark.parametrize("kernel", list(D_ENGINES))
@pytest.mark.parametrize("w", [8, 20, 40])
def test_gap_on_band_edge_register_kernels(w, kernel):
    pairs, ref, qer, want, _ = _case_d(w)
    n = len(pairs)
    opts, field = D_ENGINES[kernel]
    e = bsw.Engine(**opts)
    for cell_bits in ((16, 8) if kernel == "packed" else (16,)):
        st = _parity(e, pairs, ref, qer, w, want, f"gap on the band edge, {kernel} w={w} cell_bits={cell_bits}", cell_bits)
        assert getattr(st, field) == n and st.n_wide == 0
        assert st.n_packed == (n if kernel == "packed" else 0)
        assert st.n_group == (n if field == "n_group" else 0)
        assert st.n_wave == (n if kernel == "wave" else 0)
    e.close()


# ---- e. entering columns with a positive first row -----------------------------------------------

E_SHAPES = {(100, 600, 700): 4, (200, 1100, 1200): 8, (400, 2200, 2300): 16}
E_H0 = 3000


@lru_cache(maxsize=None)
def _case_e(shape):
    w, qlen, tlen = shape
    c = E_SHAPES[shape]
    pairs, ref, qer = bswgen.random_pairs(32, seed=qlen, tlen=(tlen, tlen), qlen=(qlen, qlen), h0=(E_H0, E_H0),
                                          p_sub=(0.0, 0.05), p_indel=(0.0, 0.01), p_unrelated=0.0)
    assert qlen > 64 * c                                           # the window slides
    assert E_H0 - DEFAULT["o_ins"] - qlen * DEFAULT["e_ins"] > 0     # the whole first row is positive
    assert _classes(pairs, DEFAULT, w, 2) == _counts({c: 32})
    return pairs, ref, qer, _want(DEFAULT, pairs, ref, qer, w)


@pytest.mark.parametrize("shape", list(E_SHAPES))
def test_inputs_positive_first_row(shape):
    """C1, case e: one shape per C with qlen > 64 * C and h0 - o_ins - qlen * e_ins > 0, so every
    column that enters the window on lane 63 brings a non-zero first-row value."""
    _case_e(shape)


@gpu
@pytest.mark.parametrize("shape", list(E_SHAPES))
def test_wave_positive_first_row(shape):
    pairs, ref, qer, want = _case_e(shape)
    e = bsw.Engine(long=2)
    st = _parity(e, pairs, ref, qer, shape[0], want, f"positive first row {shape}")
    assert st.n_wave == len(pairs)
    _assert_routed(st, pairs, DEFAULT, shape[0], 2, f"{shape}")
    e.close()


# ---- e'. entering columns whose first-row value is read ----------------------------------------------
#
# In case e the band edge stays alive (h0 is large), so every slot is written by the row before the
# one that reads it and `hin` is carried along unread: a wv_kernel whose slide loop computes `hin`
# for column jn + 2 passes case e.  Here the band end falls back and then grows, two columns a row,
# over columns >= 64 * C that no row has written (bswgen.late_front_pairs, first_row_model.py),
# and gscore is made of those values.

L_SHAPES = {(100, 4): 8, (125, 4): 8, (200, 8): 4, (400, 16): 3}       # (w, C): pairs


@lru_cache(maxsize=None)
def _case_late(shape):
    w, c = shape
    n = L_SHAPES[shape]
    pairs, ref, qer = bswgen.late_front_pairs(w, 64 * c, n, seed=64 * c + w)
    assert _classes(pairs, ZDROP0, w, 2) == _counts({c: n})
    want = _want(ZDROP0, pairs, ref, qer, w)
    sc = ZDROP0
    args = (bwa_fill_scmat(sc["a"], sc["b"]), sc["o_del"], sc["e_del"], sc["o_ins"], sc["e_ins"], w,
            sc["end_bonus"], sc["zdrop"])
    depend = 0
    for k, p in enumerate(pairs):
        q = qer[p["idq"]:p["idq"] + p["len2"]].tolist()
        t = ref[p["idr"]:p["idr"] + p["len1"]].tolist()
        out, late = first_row_model.extend(q, t, *args, int(p["h0"]), 64 * c)
        assert out == tuple(int(want[k][f]) for f in bsw.OUT_FIELDS), f"pair {k}: the model is not the oracle"
        assert late >= 10, f"pair {k}: {late} reads of first-row values in columns >= {64 * c}"
        depend += first_row_model.extend(q, t, *args, int(p["h0"]), 64 * c, shift=2)[0] != out
    # the end walks over every second column, so column qlen - 1 is on its way in about half the pairs
    assert 2 * depend >= n, f"the outputs of only {depend} of {n} pairs depend on the entering columns"
    return pairs, ref, qer, want, depend


@pytest.mark.parametrize("shape", list(L_SHAPES))
def test_inputs_late_first_row(shape):
    """C1, case e': every pair reads at least 10 never-written slots >= 64 * C whose first-row value
    is positive; for at least half of the pairs the outputs change when those slots hold the values
    of column j + 2."""
    print(f"case e' {shape}: outputs of {_case_late(shape)[4]} of {L_SHAPES[shape]} pairs depend on the entering columns")


@gpu
@pytest.mark.parametrize("shape", list(L_SHAPES))
def test_wave_late_first_row(shape):
    pairs, ref, qer, want, _ = _case_late(shape)
    e = bsw.Engine(_gparams(ZDROP0), long=2)
    st = _parity(e, pairs, ref, qer, shape[0], want, f"first-row values read late {shape}")
    assert st.n_wave == len(pairs)
    _assert_routed(st, pairs, ZDROP0, shape[0], 2, f"{shape}")
    e.close()


# ---- f. int16 class bounds ---------------------------------------------------------------------------

def _prefix_items(rng, n, qlen, tlen, h0, p_sub):
    items = []
    for _ in range(n):
        r = rng.integers(0, 4, tlen).astype(np.uint8)
        q = r[:qlen].copy()
        if p_sub:
            hit = rng.random(qlen) < p_sub
            q[hit] = (q[hit] + rng.integers(1, 4, int(hit.sum())).astype(np.uint8)) & 3
        items.append((r, q, h0))
    return items


@lru_cache(maxsize=None)
def _case_f_h0():
    """h0 + min(qlen, tlen) + e_ins * (qlen + 1) = 29398 + 300 + 301 = 29999: the last value the
    wave kernel admits; h0 = 29399 goes to the wide kernel.  Pairs 0..15 and 32..47 identical."""
    rng = np.random.default_rng(29999)
    items = []
    for h0 in (29398, 29399):
        items += _prefix_items(rng, 16, 300, 400, h0, 0.0) + _prefix_items(rng, 16, 300, 400, h0, 0.03)
    pairs, ref, qer = bswgen.assemble(items)
    assert _classes(pairs, DEFAULT, 100, 1) == _counts({4: 32, "wide": 32})
    want = _want(DEFAULT, pairs, ref, qer, 100)
    ident = np.r_[0:16, 32:48]
    assert (want["score"][ident] == pairs["h0"][ident] + 300).all()
    assert (want["score"][:16] == 29698).all()
    return pairs, ref, qer, want


@lru_cache(maxsize=None)
def _case_f_qlen(e_ins):
    """e_ins * qlen < 2700: qlen 2699 | 2700 at e_ins = 1, 899 | 900 at e_ins = 3."""
    sc = DEFAULT if e_ins == 1 else E_INS3
    q = 2699 if e_ins == 1 else 899
    a = bswgen.random_pairs(8, seed=q, tlen=(q + 100, q + 100), qlen=(q, q), h0=(100, 100),
                            p_sub=(0.0, 0.05), p_indel=(0.0, 0.01), p_unrelated=0.0)
    b = bswgen.random_pairs(8, seed=q + 1, tlen=(q + 101, q + 101), qlen=(q + 1, q + 1), h0=(100, 100),
                            p_sub=(0.0, 0.05), p_indel=(0.0, 0.01), p_unrelated=0.0)
    items = [(r[p["idr"]:p["idr"] + p["len1"]], qq[p["idq"]:p["idq"] + p["len2"]], int(p["h0"]))
             for ps, r, qq in (a, b) for p in ps]
    pairs, ref, qer = bswgen.assemble(items)
    assert _classes(pairs, sc, 100, 1) == _counts({4: 8, "wide": 8})
    return pairs, ref, qer, _want(sc, pairs, ref, qer, 100), sc


def test_inputs_int16_bounds():
    """C1, case f: the identical pairs score h0 + 300 (29698 at the last admitted h0) and the model
    splits each batch in half between the wave kernel and the wide kernel."""
    _case_f_h0()
    _case_f_qlen(1)
    _case_f_qlen(3)


@gpu
def test_wave_int16_bound_h0():
    pairs, ref, qer, want = _case_f_h0()
    e = bsw.Engine(**PLANNED)
    st = _parity(e, pairs, ref, qer, 100, want, "h0 at the int16 bound")
    assert (st.n_wave, st.n_wide) == (32, 32)
    _assert_routed(st, pairs, DEFAULT, 100, 1, "h0 bound")
    e.close()


@gpu
@pytest.mark.parametrize("e_ins", [1, 3])
def test_wave_int16_bound_qlen(e_ins):
    pairs, ref, qer, want, sc = _case_f_qlen(e_ins)
    e = bsw.Engine(_gparams(sc), **PLANNED)
    st = _parity(e, pairs, ref, qer, 100, want, f"e_ins * qlen at 2700, e_ins={e_ins}")
    assert (st.n_wave, st.n_wide) == (8, 8)
    _assert_routed(st, pairs, sc, 100, 1, f"e_ins={e_ins}")
    e.close()


# ---- g. non-default scoring on long queries ----------------------------------------------------------

G_BANDS = (60, 260)


@lru_cache(maxsize=None)
def _case_g(k):
    sc = SCORINGS[k]
    pairs, ref, qer = bswgen.random_pairs(300, seed=4110 + k, tlen=(100, 900), qlen=(161, 800), h0=(1, 300))
    cls = {w: _classes(pairs, sc, w, 1) for w in G_BANDS}
    assert cls[60] == _counts({4: 300})
    by_w = _classes(pairs, DEFAULT, 260, 1)
    assert cls[260]["lane"] == 0 and cls[260]["wide"] == 0 and by_w[16] > 0
    if sc["e_ins"] > 1 or sc["e_del"] > 1:
        # the cap (qlen + end_bonus - o + e) / e moves pairs to lower classes: with qlen uniform in
        # 161..800 about 1/3 (k = 0) or more of the 300 pairs leave C = 16 for C = 4 and C = 8
        assert cls[260][4] >= 50 and cls[260][8] >= 50 and cls[260][16] < by_w[16]
    return pairs, ref, qer, {w: _want(sc, pairs, ref, qer, w) for w in G_BANDS}, cls


@pytest.mark.parametrize("k", range(len(SCORINGS)))
def test_inputs_scoring_long(k):
    """C1, case g: every pair is the wave kernel's; at w = 260 the per-pair cap spreads them over
    the classes, further down for e > 1."""
    cls = _case_g(k)[4]
    print(f"case g scoring {k}, pairs per class:", cls)


@gpu
@pytest.mark.parametrize("w", G_BANDS)
@pytest.mark.parametrize("k", range(len(SCORINGS)))
def test_wave_scoring_long(k, w):
    pairs, ref, qer, wants, _ = _case_g(k)
    sc = SCORINGS[k]
    e = bsw.Engine(_gparams(sc), **PLANNED)
    st = _parity(e, pairs, ref, qer, w, wants[w], f"scoring {k} w={w}")
    _assert_routed(st, pairs, sc, w, 1, f"scoring {k} w={w}")
    assert st.n_wave == len(pairs)
    e.close()


# ---- h. two pairs per block with mixed shapes --------------------------------------------------------

H_GRID = 8192                                    # launch_wv_kernel: grid = min(n, 8192)


@lru_cache(maxsize=None)
def _case_h():
    n = H_GRID + 640
    pairs, ref, qer = bswgen.random_pairs(n, seed=8192, qlen=(0, 96), tlen=(0, 120), h0=(0, 150))
    assert int(((pairs["len2"] == 0) | (pairs["len1"] == 0)).sum()) >= 100
    assert _classes(pairs, DEFAULT, 30, 2) == _counts({4: n})
    return pairs, ref, qer, _want(DEFAULT, pairs, ref, qer, 30)


def test_inputs_two_pairs_per_block():
    """C1, case h: 8832 pairs in one class, so 640 blocks run a second pair -- by the sort
    (qlen descending) a shorter or empty one after one of the longest."""
    _case_h()


@gpu
def test_wave_two_pairs_per_block():
    pairs, ref, qer, want = _case_h()
    e = bsw.Engine(long=2)
    st = _parity(e, pairs, ref, qer, 30, want, "two pairs per block")
    assert st.n_wave == len(pairs)
    _assert_routed(st, pairs, DEFAULT, 30, 2, "two pairs per block")
    e.close()
