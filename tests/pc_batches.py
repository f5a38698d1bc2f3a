"""Batches and lane orders for the packed-column kernel's wave-level rules: the
engine's lane order and QMAX classes, and the batches built to exercise the left skip, the left prune, the right
prune and the redo pass -- shared by the CPU model tests (tests/pc_wave_model.py) and the GPU tests."""

from __future__ import annotations

import numpy as np


def qmax_class(pairs):
    """Index of the packed-column QMAX class (32, 64, 96, 128, 160) of each pair: qlen + 1 <= QMAX."""
    return np.searchsorted(np.array([32, 64, 96, 128, 160]), pairs["len2"].astype(np.int64) + 1)


def seed_matches(pairs, ref, qer):
    """plan_kernel's lifetime predictor: identities of query[10, 40) with target[4 + s, 34 + s),
    best over s in 0..12 (31 for pairs too short to tell)."""
    n = len(pairs)
    Q, T = pairs["len2"].astype(np.int64), pairs["len1"].astype(np.int64)
    ok = (Q >= 40) & (T >= 46)
    mt = np.full(n, 31, np.int64)
    k = np.flatnonzero(ok)
    if len(k):
        q = np.asarray(qer)[pairs["idq"][k].astype(np.int64)[:, None] + 10 + np.arange(30)]
        best = np.zeros(len(k), np.int64)
        for s in range(13):
            r = np.asarray(ref)[pairs["idr"][k].astype(np.int64)[:, None] + 4 + s + np.arange(30)]
            best = np.maximum(best, (q == r).sum(1))
        mt[k] = best
    return mt


def default_order(pairs, ref, qer):
    """The lane order of one packed-column class under plan_kernel's default key: (qlen desc,
    related first, tlen / 32 desc, seed identities desc, h0 desc), ties by index (a stable sort)."""
    Q, T = pairs["len2"].astype(np.int64), pairs["len1"].astype(np.int64)
    mt = seed_matches(pairs, ref, qer)
    rel = (mt > 18).astype(np.int64)
    cls = qmax_class(pairs)
    key = ((cls << 28) | ((255 - np.minimum(Q, 255)) << 20) | ((1 - rel) << 19)
           | ((63 - np.minimum(T >> 5, 63)) << 13) | ((31 - np.minimum(mt, 31)) << 8)
           | (255 - np.minimum(np.maximum(pairs["h0"].astype(np.int64), 0), 255)))
    return np.argsort(key, kind="stable").astype(np.int32)


# ---- batches built to exercise the skip ----

def _rng_seq(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def boundary_alive(n, seed, qlen=150, tlen=300, h0=100, head=24, offs=(0, 40)):
    """The column -1 boundary outlives the first columns: h0 = 100 keeps slot 0 positive for about
    94 rows, while the query's first `head` bases are unrelated to the window and the rest is an
    exact copy of it at a diagonal offset -- the first columns die long before slot 0 does, and a
    skip that started from slot 1 would drop the boundary's deletions."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = _rng_seq(rng, tlen)
        d = int(rng.integers(offs[0], offs[1] + 1))
        q = _rng_seq(rng, qlen)
        q[head:] = r[d + head:d + qlen]
        items.append((r, q, h0))
    return bswgen.assemble(items)


PIN_SCORING = dict(zdrop=10)   # pinned_waves: z-drop ends the unrelated pinning lane soon after base 40


def pinned_waves(nwaves, seed, pin_dies, qlen=150, pin_h0=100):
    """One wave per tlen / 32 bucket (tlen = 300 - 32 v, at least 172), 64 pairs each: every pair's
    query starts with an exact copy of the window's first 40 bases, so the default key ties in
    everything but tlen / 32 and h0 -- and the one lane of each wave with h0 = pin_h0 comes first,
    the 63 lanes with h0 1-10 after it.  Those 63 are exact copies (their zero prefix forms within
    a dozen rows); the pinning lane has no zero prefix for about pin_h0 rows.  With `pin_dies`
    its query is unrelated past base 40 (under PIN_SCORING the lane is z-dropped some ten rows later
    and releases gz), else it is an exact copy too and lives as long as its neighbours."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    assert 1 <= nwaves <= 5
    for v in range(nwaves):
        tlen = 300 - 32 * v
        for k in range(64):
            r = _rng_seq(rng, tlen)
            q = r[:qlen].copy()
            if k == 0 and pin_dies:
                q[40:] = _rng_seq(rng, qlen - 40)
            items.append((r, q, pin_h0 if k == 0 else int(rng.integers(1, 11))))
    return bswgen.assemble(items)


def uneven_lifetimes(nwaves, seed, tail=37):
    """One wave per query length (150 - v): 40 exact pairs with a 300-base window beside 24 whose
    window is 1-40 bases (they run out of rows while the others' zero prefix forms); the last wave
    holds only `tail` pairs, so the batch is no multiple of 64."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for v in range(nwaves):
        qlen = 150 - v
        for k in range(64 if v < nwaves - 1 else tail):
            short = k % 8 >= 5
            tlen = int(rng.integers(1, 41)) if short else 300
            r = _rng_seq(rng, max(tlen, qlen) if short else tlen)
            q = bswgen.mutate(rng, r, qlen, 0.02, 0.0)
            items.append((r[:tlen], q, int(rng.integers(1, 31))))
    return bswgen.assemble(items)


def interior_zeros(n, seed):
    """Period-2 windows and queries (light mutation) and heavily mutated queries (25 %): H falls to
    0 inside a row and rises again to its right -- only the PREFIX of zeros may be skipped."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for k in range(n):
        Q = int(rng.integers(100, 160))
        T = Q + int(rng.integers(40, 140))
        if k & 1:
            motif = _rng_seq(rng, 2)
            if motif[0] == motif[1]:
                motif[1] = (motif[1] + 1) & 3
            r = np.tile(motif, T // 2 + 1)[:T].copy()
            q = bswgen.mutate(rng, np.tile(motif, Q // 2 + 2)[int(rng.integers(0, 2)):], Q, 0.04, 0.01)
        else:
            r = _rng_seq(rng, T)
            q = bswgen.mutate(rng, r, Q, 0.25, 0.02)
        items.append((r, q, int(rng.integers(1, 31))))
    return bswgen.assemble(items)


# ---- batches built to exercise the left prune and the redo pass ----

def c2_shaped(n, seed, tlen=300, qlen=150):
    """Flagship-shaped pairs: h0 19-100, 2 % substitutions, 0.2 % indels, 5 % unrelated."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = _rng_seq(rng, tlen)
        if rng.random() < 0.05:
            q = _rng_seq(rng, qlen)
        else:
            q = bswgen.mutate(rng, r, qlen, 0.02, 0.002)
        items.append((r, q, int(rng.integers(19, 101))))
    return bswgen.assemble(items)


def late_collapse(n, seed, at=130, every=1, qlen=150, tlen=300, h0=(19, 60)):
    """The query is an exact copy of the window up to base `at` and random after it, in one lane
    of `every` (the others are exact copies throughout): the diagonal grows gscore's bound and the
    left cells are pruned long before the alignment collapses -- by z-drop, by m == 0 or not at
    all, as the scoring decides."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for k in range(n):
        r = _rng_seq(rng, tlen)
        q = r[:qlen].copy()
        if k % every == 0:
            q[at:] = (q[at:] + rng.integers(1, 4, qlen - at).astype(np.uint8)) & 3   # every base differs
        items.append((r, q, int(rng.integers(h0[0], h0[1] + 1))))
    return bswgen.assemble(items)


def class_edges(n, seed, qlens=(95, 127, 159), extra=150):
    """qlen at the top of every class that carries the rule, tlen = qlen + `extra`."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for qlen in qlens:
        for k in range(n):
            r = _rng_seq(rng, qlen + extra)
            q = r[:qlen].copy() if k & 3 else bswgen.mutate(rng, r, qlen, 0.03, 0.002)
            items.append((r, q, int(rng.integers(5, 61))))
    return bswgen.assemble(items)


def concat(*batches):
    """Several (pairs, ref, qer) batches as one."""
    pairs, refs, qers, ro, qo = [], [], [], 0, 0
    for p, r, q in batches:
        p = p.copy()
        p["idr"] += ro
        p["idq"] += qo
        pairs.append(p), refs.append(np.asarray(r, np.uint8)), qers.append(np.asarray(q, np.uint8))
        ro += len(r)
        qo += len(q)
    return np.concatenate(pairs), np.concatenate(refs), np.concatenate(qers)


# ---- batches built to exercise the right cap, the certificates and the redo pass ----

def clipped_tails(n, seed):
    """a. late_collapse at base 60, 100 and 130: the query's tail does not align, gscore stays far below
    best and the final certificate sends the capped lanes to redo."""
    per = n // 3
    return concat(*(late_collapse(per, seed + k, at=at) for k, at in enumerate((60, 100, 130))))


def second_diagonal(n, seed, xlen=75, tlen=300):
    """b. query = X X' (X' a light mutation of X) against a window that holds X once, at its start: the
    cells (i, xlen + i) of the second copy score high to the right of the main diagonal."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = _rng_seq(rng, tlen)
        x = r[:xlen]
        q = np.concatenate([x, bswgen.mutate(rng, x, xlen, 0.02, 0.0)])
        items.append((r, q, int(rng.integers(19, 101))))
    return bswgen.assemble(items)


def late_insertion(n, seed, qlen=150, tlen=300, near=100):
    """c. 20-40 query bases inserted near base `near` of an otherwise exact copy: the optimal path jumps
    right along one row, through columns a careless cap would have removed."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = _rng_seq(rng, tlen)
        ins = int(rng.integers(20, 41))
        at = near + int(rng.integers(-8, 9))
        q = np.concatenate([r[:at], _rng_seq(rng, ins), r[at:]])[:qlen]
        items.append((r, q.astype(np.uint8), int(rng.integers(19, 101))))
    return bswgen.assemble(items)


def low_h0(n, seed):
    """d. flagship-shaped pairs with h0 1-15: the first row's tail dies within a few columns."""
    p, r, q = c2_shaped(n, seed)
    p["h0"] = np.random.default_rng(seed + 1).integers(1, 16, len(p))
    return p, r, q


def class_tops(nwaves, seed, qlens=(127, 159), tail=37):
    """f. qlen at the top of both classes that carry the rule; 37 + 64 k pairs per class."""
    return class_edges(64 * nwaves + tail, seed, qlens=qlens)


def odd_lane(nwaves, seed, qlen=150, tlen=300):
    """g. related pairs with two early-dying lanes in every 64: their queries copy the window up to base
    40 or 70 and are unrelated after it, so the default key (seed identities over query[10, 40)) sorts
    them among the related lanes, h0 deciding the wave."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for v in range(nwaves):
        for k in range(64):
            r = _rng_seq(rng, tlen)
            q = r[:qlen].copy()
            if k == 7:
                q[70:] = _rng_seq(rng, qlen - 70)
            if k == 29:
                q[40:] = _rng_seq(rng, qlen - 40)
            items.append((r, q, int(rng.integers(30, 101))))
    return bswgen.assemble(items)
