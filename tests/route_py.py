"""Routing model of the planned path (bsw_dispatch.hip plan_kernel), restated from the kernels'
contracts in bsw_kernels.h: which pairs the wave-per-alignment kernel takes, in which of its
three column counts, and which stay on the int32 wide kernel.  Plain Python, no GPU.

The parity tests assert Stats.n_wave / n_wide against it, so a bound that drifts in wv_class()
or in the kernel's own guard is noticed even where the outputs stay equal.
"""

from __future__ import annotations

WV_QMAX = 4096                 # kWvQmax
WV_COLS = (4, 8, 16)           # wv_kernel<C>: a window of 64 * C columns
LANE_QMAX = 160                # kLaneQmaxMax: the register kernels' columns


def _cdiv(a, b):
    """C integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _maxsc(params):
    return max(int(v) for v in params.mat)


def band_cap(params, w, qlen):
    """A.2: the pair's band, min(w, max_ins, max_del) in the integer form the kernels use."""
    maxsc = _maxsc(params)
    ni = qlen * maxsc + params.end_bonus - params.o_ins
    nd = qlen * maxsc + params.end_bonus - params.o_del
    wl = min(w, max(_cdiv(ni + params.e_ins, params.e_ins), 1))
    return min(wl, max(_cdiv(nd + params.e_del, params.e_del), 1))


def wv_class(params, w, qlen, tlen, h0):
    """Columns per lane (4, 8 or 16) of the wave kernel that takes the pair, None if none does."""
    if _maxsc(params) != 1 or qlen > WV_QMAX or h0 < 0:
        return None
    if params.e_ins * qlen >= 2700:
        return None
    if 128 + params.o_del + 2 * params.e_del >= 30000 or 128 + params.o_ins + 2 * params.e_ins >= 30000:
        return None
    if h0 + min(qlen, tlen) + params.e_ins * (qlen + 1) >= 30000:
        return None
    wl = band_cap(params, w, qlen)
    for c in WV_COLS:
        if 2 * wl + c + 2 <= 64 * c:
            return c
    return None


def route(params, w, qlen, tlen, h0, long):
    """'lane' (a register kernel: lane or packed-column), 'wide', or the wave kernel's 4 / 8 / 16,
    for an engine whose batches all take the planned path (small_batch = mid_batch = 0, or
    long != 1) with BSW_OPT_LONG = long."""
    qlen, tlen = max(qlen, 0), max(tlen, 0)
    wvc = wv_class(params, w, qlen, tlen, h0) if long else None
    if long == 2 and wvc is not None:
        return wvc
    hi = max(h0, 0) + max(_maxsc(params), 0) * min(qlen, tlen)
    if hi < 32768 and h0 >= 0 and qlen <= LANE_QMAX:
        return "lane"
    return wvc if wvc is not None else "wide"


def class_counts(pairs, params, w, long):
    """{4: n, 8: n, 16: n, 'lane': n, 'wide': n} over a SeqPair array."""
    out = {4: 0, 8: 0, 16: 0, "lane": 0, "wide": 0}
    for q, t, h in zip(pairs["len2"].tolist(), pairs["len1"].tolist(), pairs["h0"].tolist()):
        out[route(params, w, q, t, h, long)] += 1
    return out


def expected_counts(pairs, params, w, long):
    """(n_wave, n_wide) of Stats after one call."""
    c = class_counts(pairs, params, w, long)
    return c[4] + c[8] + c[16], c["wide"]
