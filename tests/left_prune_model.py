"""CPU model of the packed-column kernel's left prune.

tests/left_skip_model.py's loop -- one wavefront of up to 64 lanes in lockstep, the static left
edge, the lazy right edge, the early stop and the prefix bound gz on the kernel's schedule -- with
the prune added in the exact form the kernel (bsw_pc.hip) uses:

  - at the refresh, when group gz fails the zero test, gz also passes over it when i > wl_max
    (every lane's static beg > 0) and every lane that stays alive has end == qlen, gsc > 0 and
        H plane: every slot s of the group with s > beg and h[s] > 0 has h[s] + (qlen - s) < gsc
        E plane: every slot s of the group with s >= beg and e[s] > 0 has e[s] + (qlen - 1 - s) < gsc
    (the explicit E test, not the one-slot lookahead through H), in the classes from QMAX 128 up;
    the group's slots are then set to 0 in every lane and the wave's `pruned` flag is set;
  - on every later row of a pruned wave, after the row-end update of best / alive and before the
    early stop, a lane is sent to REDO when it is act, not better, m > 0 and z-dropped by the
    mj-free bound best - m > zdrop, or still alive with h1 == 0.  A redo lane retires and stores
    nothing.  A lane whose row maximum is 0 retires as in the plain loop and keeps its outputs:
    every cell of its true row is then a changed cell, below the early stop's bound (§3 item 12).

Redo lanes are recomputed by left_skip_model (the kernel without the rule) in waves of their own,
in list order.  Per pair the model returns the six outputs, the rows the lane ran (a redo lane's
are those of its second run) and the redo mark; per wave [rows, groups entered, groups the skip
and the prune removed from the entered set, prune events (non-zero groups passed over), redo lanes].
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import left_skip_model as lsm

MODEL_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int32_t idr, idq, id, len1, len2, h0, seqid, regid, score, tle, gtle, qle, gscore, max_off; } pair_t;
typedef struct { int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus; int8_t mat[25]; } par_t;

#define QCAP 164
typedef struct {
    int h[QCAP], e[QCAP];            /* slot s: h = H(i-1, s-1), e = E(i, s) */
    int qlen, tlen, h0, wl, endc, beg, end, h1, m, mj;
    int best, best_i, best_j, max_ie, gsc, moff, alive, act, want, rows, redo;
    const uint8_t *tg, *qy;
} lane_t;

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

/* one wave: lanes idx[0 .. nl), nl <= 64.  wst = {rows, entered, skipped, prune events, redo lanes} */
static void wave(const par_t *p, pair_t *pairs, const int32_t *idx, int nl, const uint8_t *ref, const uint8_t *qer,
                 int w, int prune, int smask, int srow, int sphase, int sqmin, int32_t *lrows, uint8_t *lredo,
                 int64_t *wst)
{
    lane_t *L = (lane_t *)calloc((size_t)nl, sizeof(lane_t));
    const int oe_ins = p->o_ins + p->e_ins, oe_del = p->o_del + p->e_del;
    int maxsc = 0, k, i, j, maxq = 0, wl_max = -1, gz = 0, pruned = 0, skip = 1;
    for (k = 0; k < 25; ++k) maxsc = imax(maxsc, p->mat[k]);
    for (k = 0; k < nl; ++k) {
        lane_t *l = &L[k];
        const pair_t *sp = &pairs[idx[k]];
        l->qlen = sp->len2, l->tlen = sp->len1, l->h0 = sp->h0;
        l->tg = ref + sp->idr, l->qy = qer + sp->idq;
        l->h[0] = l->h0;
        for (j = 1; j <= l->qlen; ++j) l->h[j] = imax(l->h0 - oe_ins - (j - 1) * p->e_ins, 0);
        {
            const int ni = l->qlen * maxsc + p->end_bonus - p->o_ins, nd = l->qlen * maxsc + p->end_bonus - p->o_del;
            l->wl = imin(w, imax((ni + p->e_ins) / p->e_ins, 1));
            l->wl = imin(l->wl, imax((nd + p->e_del) / p->e_del, 1));
        }
        l->best = l->h0, l->best_i = l->best_j = l->max_ie = l->gsc = -1, l->endc = l->qlen;
        l->alive = l->tlen > 0;
        if (l->alive) wl_max = imax(wl_max, l->wl);
        maxq = imax(maxq, l->qlen);
    }
    const int QMAX = maxq < 32 ? 32 : maxq < 64 ? 64 : maxq < 96 ? 96 : maxq < 128 ? 128 : 160;
    const int NG = QMAX / 4;
    if (QMAX < sqmin) skip = 0;
    if (QMAX < prune) prune = 0;          /* prune: 0 (off) or the smallest QMAX class that carries the rule */
    for (i = 0;; ++i) {
        int any = 0, emax = -1;
        for (k = 0; k < nl; ++k) {
            lane_t *l = &L[k];
            l->act = l->alive && i < l->tlen;
            l->alive = l->act;
            if (!l->act) continue;
            any = 1;
            l->beg = imax(0, i - l->wl);
            l->end = imin(imin(l->endc, i + l->wl + 1), l->qlen);
            l->endc = l->end;
            emax = imax(emax, l->end);
        }
        if (!any) break;
        const int glo = imax(0, i - wl_max) >> 2, ghi = imin(emax, QMAX - 1) >> 2;
        const int gfirst = skip ? imax(glo, gz) : glo;
        const int jstart = 4 * gfirst;
        wst[0] += 1;
        wst[1] += imax(ghi - gfirst + 1, 0);
        wst[2] += imax(ghi - glo + 1, 0) - imax(ghi - gfirst + 1, 0);
        for (k = 0; k < nl; ++k) {
            lane_t *l = &L[k];
            if (!l->act) continue;
            const int8_t *srw = &p->mat[5 * (l->tg[i] > 4 ? 4 : l->tg[i])];
            int f = 0, m = 0, mj = -1;
            int h1 = l->beg == 0 ? imax(l->h0 - (p->o_del + p->e_del * (i + 1)), 0) : 0;
            l->rows += 1;
            for (j = jstart; j <= l->end; ++j) {
                int M = l->h[j], e = l->e[j], h, t;
                if (j == l->beg && j > 0) f = 0, h1 = 0;
                if (j == l->end) break;
                l->h[j] = h1;
                M = M ? M + srw[l->qy[j] > 4 ? 4 : l->qy[j]] : 0;
                h = imax(imax(M, e), f);
                h1 = h;
                if (j >= l->beg) {
                    if (!(m > h)) mj = j;
                    m = imax(m, h);
                }
                t = imax(M - oe_del, 0);
                l->e[j] = imax(e - p->e_del, t);
                t = imax(M - oe_ins, 0);
                f = imax(f - p->e_ins, t);
            }
            if (l->end >= jstart) l->h[l->end] = h1, l->e[l->end] = 0;
            l->h1 = h1, l->m = m, l->mj = mj;
            if (l->end == l->qlen) {
                if (!(l->gsc > h1)) l->max_ie = i;
                l->gsc = imax(l->gsc, h1);
            }
            {
                const int di = i - l->best_i, dj = mj - l->best_j;
                const int dz = di > dj ? l->best - m - (di - dj) * p->e_del : l->best - m - (dj - di) * p->e_ins;
                const int better = m > l->best;
                l->alive = m > 0 && (better || !(p->zdrop > 0 && dz > p->zdrop));
                /* the certificate of a pruned wave (best is still the old one when not better) */
                if (pruned && ((!better && m > 0 && p->zdrop > 0 && l->best - m > p->zdrop) ||
                               (l->alive && h1 == 0)))
                    l->redo = 1, l->alive = 0;
                if (better) {
                    l->moff = imax(l->moff, abs(mj - i));
                    l->best_i = i, l->best_j = mj, l->best = m;
                }
            }
        }
        /* early stop: scalar bound on every row, per-cell bound on the scan's rows */
        {
            int anywant = 0;
            for (k = 0; k < nl; ++k) {
                lane_t *l = &L[k];
                if (!l->act) continue;
                const int edge = l->end == l->qlen && l->beg > 0;
                const int ubs = l->m - 1 + imin(l->qlen - l->beg, l->tlen - i);
                if (edge && ubs <= l->best && ubs < l->gsc) l->alive = 0;
                const int ubm = l->m - 1 + l->qlen - l->mj;
                l->want = QMAX > 64 && l->alive && edge && ubm <= l->best && ubm < l->gsc;
                anywant |= l->want;
            }
            if (QMAX > 64 && (i & sphase) == sphase && anywant)
                for (k = 0; k < nl; ++k) {
                    lane_t *l = &L[k];
                    if (!l->act || !l->want) continue;
                    int ub = 0, s;
                    for (s = imax(l->beg + 1, jstart); s <= imin(l->end, 4 * ghi + 3); ++s)
                        ub = imax(ub, l->h[s] + (l->qlen - s));
                    if (ub <= l->best && ub < l->gsc) l->alive = 0;
                }
        }
        /* the prefix bound: while group gz is zero in both planes of every lane still alive -- or,
           with the prune, cannot reach gscore in any of them */
        if (skip && (i & smask) == srow)
            while (gz < NG) {
                int z = 1;
                for (k = 0; k < nl && z; ++k) {
                    const lane_t *l = &L[k];
                    if (!l->act || !l->alive) continue;
                    for (j = 4 * gz; j < 4 * gz + 4; ++j) z &= l->h[j] == 0 && l->e[j] == 0;
                }
                if (!z) {
                    int ok = prune && i > wl_max;
                    for (k = 0; k < nl && ok; ++k) {
                        const lane_t *l = &L[k];
                        if (!l->act || !l->alive) continue;
                        ok &= l->end == l->qlen && l->gsc > 0;
                    }
                    for (k = 0; k < nl && ok; ++k) {
                        const lane_t *l = &L[k];
                        if (!l->act || !l->alive) continue;
                        int ub = 0;
                        for (j = 4 * gz; j < 4 * gz + 4; ++j) {
                            if (j > l->beg && l->h[j] > 0) ub = imax(ub, l->h[j] + (l->qlen - j));
                            if (j >= l->beg && l->e[j] > 0) ub = imax(ub, l->e[j] + (l->qlen - 1 - j));
                        }
                        ok &= ub < l->gsc;
                    }
                    if (!ok) break;
                    for (k = 0; k < nl; ++k)
                        for (j = 4 * gz; j < 4 * gz + 4; ++j) L[k].h[j] = L[k].e[j] = 0;
                    pruned = 1;
                    wst[3] += 1;
                }
                ++gz;
            }
        /* next row's band end from the last positive slot (slot s > 0 holds column s - 1) */
        for (k = 0; k < nl; ++k) {
            lane_t *l = &L[k];
            if (!l->act) continue;
            if (l->alive) {
                int lp1 = l->end;
                if (l->h1 == 0) {
                    for (lp1 = l->end; lp1 > 0 && l->h[lp1] <= 0; --lp1)
                        ;
                }
                l->endc = imin(lp1 + 2, l->qlen);
            }
        }
    }
    for (k = 0; k < nl; ++k) {
        lane_t *l = &L[k];
        pair_t *sp = &pairs[idx[k]];
        lrows[idx[k]] = l->rows;
        lredo[idx[k]] = (uint8_t)l->redo;
        wst[4] += l->redo;
        if (l->redo) continue;                 /* a redo lane stores no outputs */
        sp->score = l->best, sp->tle = l->best_i + 1, sp->gtle = l->max_ie + 1, sp->qle = l->best_j + 1;
        sp->gscore = l->gsc, sp->max_off = l->moff;
    }
    free(L);
}

/* waves wa .. wb - 1 of the lane order idx[0 .. n): wave v holds idx[64 v .. 64 v + 63] */
void lp_model(const par_t *p, pair_t *pairs, const int32_t *idx, int32_t n, const uint8_t *ref, const uint8_t *qer,
              int32_t w, int32_t prune, int32_t smask, int32_t srow, int32_t sphase, int32_t sqmin, int32_t wa,
              int32_t wb, int32_t *lrows, uint8_t *lredo, int64_t *wst)
{
    for (int32_t v = wa; v < wb; ++v)
        wave(p, pairs, idx + 64 * v, imin(64, n - 64 * v), ref, qer, w, prune, smask, srow, sphase, sqmin, lrows,
             lredo, wst + 5 * v);
}
"""

PRUNE_QMIN = 128               # BSW_PC_PRUNE_QMIN: the classes below it are compiled without the rule
_lib = None


def build(dirpath):
    """Compile this model and left_skip_model into `dirpath`; once per process.  Returns the pair
    (prune model, skip model) that run() takes."""
    global _lib
    if _lib is None:
        src = os.path.join(str(dirpath), "lp_model.c")
        so = os.path.join(str(dirpath), "liblp_model.so")
        with open(src, "w") as f:
            f.write(MODEL_C)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src], check=True)
        _lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int32
        _lib.lp_model.argtypes = [P, P, P, I, P, P, I, I, I, I, I, I, I, I, P, P, P]
        _lib.lp_model.restype = None
    return _lib, lsm.build(dirpath)


def run(libs, params, pairs, ref, qer, w, order=None, prune=True, threads=8):
    """(outputs, rows per pair, redo mark per pair, per-wave [rows, entered, skipped, prune events,
    redo lanes]): `pairs` is not modified.  `order` as in left_skip_model.run().  The redo lanes
    are recomputed without the rule, in list order, and their outputs and rows merged in."""
    lib, slib = libs
    out = pairs.copy()
    idx = np.ascontiguousarray(np.arange(len(out)) if order is None else order, np.int32)
    n = len(idx)
    nw = (n + 63) // 64
    rows = np.zeros(len(out), np.int32)
    redo = np.zeros(len(out), np.uint8)
    wst = np.zeros((nw, 5), np.int64)
    ref = np.ascontiguousarray(ref, np.uint8)
    qer = np.ascontiguousarray(qer, np.uint8)
    step = max(1, (nw + threads - 1) // threads)

    def part(a):
        lib.lp_model(ctypes.byref(params), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(idx.ctypes.data), n,
                     ctypes.c_void_p(ref.ctypes.data), ctypes.c_void_p(qer.ctypes.data), w, PRUNE_QMIN if prune else 0, lsm.SKIP_MASK,
                     lsm.SKIP_ROW, lsm.SCAN_PHASE, lsm.SKIP_QMIN, a, min(nw, a + step),
                     ctypes.c_void_p(rows.ctypes.data), ctypes.c_void_p(redo.ctypes.data),
                     ctypes.c_void_p(wst.ctypes.data))

    if nw:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(part, range(0, nw, step)))
    again = idx[redo[idx] != 0]
    if len(again):
        o2, r2, _ = lsm.run(slib, params, pairs, ref, qer, w, order=again, threads=threads)
        out[again], rows[again] = o2[again], r2[again]
    return out, rows, redo, wst


def run_planned(libs, params, pairs, ref, qer, w, **kw):
    """As run(), in the engine's layout: one launch per QMAX class over its slice of the default
    order, each class with a redo list of its own."""
    order = lsm.default_order(pairs, ref, qer)
    cls = lsm.qmax_class(pairs)[order]
    out, rows, redo, wsts = pairs.copy(), np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.uint8), []
    for c in np.unique(cls):
        sub = order[cls == c]
        o, r, d, wst = run(libs, params, pairs, ref, qer, w, order=sub, **kw)
        out[sub], rows[sub], redo[sub] = o[sub], r[sub], d[sub]
        wsts.append(wst)
    return out, rows, redo, np.concatenate(wsts) if wsts else np.zeros((0, 5), np.int64)


# ---- batches built to exercise the prune and the redo pass (CPU model test and GPU test) ----

def c2_shaped(n, seed, tlen=300, qlen=150):
    """Flagship-shaped pairs: h0 19-100, 2 % substitutions, 0.2 % indels, 5 % unrelated."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = lsm._rng_seq(rng, tlen)
        if rng.random() < 0.05:
            q = lsm._rng_seq(rng, qlen)
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
        r = lsm._rng_seq(rng, tlen)
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
            r = lsm._rng_seq(rng, qlen + extra)
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
