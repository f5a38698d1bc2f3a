"""CPU model of the packed-column kernel's right prune.

tests/left_prune_model.py's loop -- one wavefront of up to 64 lanes in lockstep, the static left edge,
the lazy right edge, the early stop, the prefix bound gz and the left prune on the kernel's schedule --
with the right prune added in the exact form the kernel (bsw_pc.hip) uses:

  - a wave-uniform right cap gr (a group index, QMAX / 4 = no cap): every lane's band end is clamped to
    slot 4 gr at the row head, so the groups above gr leave the entered set and group gr runs as the
    row's right-edge group;
  - at the refresh, after the walk of gz: when i >= ROW0 and every lane that stays alive had a new best
    within the last K rows, the cap walks down from group
    gr - 1 while, in every staying lane, every slot s of the group has
        h[s] > 0:  h[s] + (qlen - s)     + SLACK < T        T = best - MARGIN (best after the row)
        e[s] > 0:  e[s] + (qlen - 1 - s) + SLACK < T
        floor:     1 + (qlen - 4 G)      + SLACK < T
    and the group lies at or above gz + 2; a passed group is set to 0 in every lane, the wave is marked
    and every staying lane's P (the largest threshold ever applied to it) takes T.  When the precheck
    fails under a cap the cap retreats one group;
  - on every row of a marked wave, after the row-end update of best / alive: a lane that is active, has
    no new best, m > 0 and best - m > zdrop goes to REDO (item 12's certificate b); a lane whose band
    end sits at the cap (end == 4 gr < qlen) is marked CLIPPED for good; a clipped lane with end < qlen
    and h1 > 0 goes to REDO when h1 + (qlen - end) >= T, else its P takes T;
  - at the refresh of a marked wave, after the precheck and the walk, the cap retreats one group when some
    staying lane with end < qlen at the cap or within RWIN slots under it has h1 + (qlen - end) + SLACK2
    >= T -- a cap the walk has just put above a moving band edge is taken back before the edge reaches
    it, so a band narrower than the query never clips; once marked, a wave walks only on every fourth
    refresh;
  - when a lane with P set ends, by any route, it goes to REDO unless gsc >= P (thresholds below 0 are
    applied as 0, as the kernel's bit field stores them).  TOUCHED = 1 is the one-bit form the kernel does
    not carry: gsc >= best - MARGIN for every lane that was alive at a prune.

Redo lanes are recomputed by left_skip_model (the kernel without either rule) in waves of their own.
Per pair the model returns the six outputs, the rows the lane ran and the redo mark; per wave the
NST figures named in WST.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import left_prune_model as lpm
import left_skip_model as lsm

MODEL_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>

typedef struct { int32_t idr, idq, id, len1, len2, h0, seqid, regid, score, tle, gtle, qle, gscore, max_off; } pair_t;
typedef struct { int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus; int8_t mat[25]; } par_t;
/* the schedule and the right prune's constants (the kernel's macros) */
typedef struct { int32_t prune, smask, srow, sphase, sqmin, rprune, margin, slack, slack2, k, row0, wmask, rwin, touched; } cfg_t;

#define QCAP 164
#define NST 13
typedef struct {
    int h[QCAP], e[QCAP];            /* slot s: h = H(i-1, s-1), e = E(i, s) */
    int qlen, tlen, h0, wl, endc, beg, end, h1, m, mj;
    int best, best_i, best_j, max_ie, gsc, moff, alive, act, want, rows, redo, P, clip;
    const uint8_t *tg, *qy;
} lane_t;

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

/* one wave: lanes idx[0 .. nl), nl <= 64.  wst: see WST in the Python part */
static void wave(const par_t *p, const cfg_t *c, pair_t *pairs, const int32_t *idx, int nl, const uint8_t *ref,
                 const uint8_t *qer, int w, int32_t *lrows, uint8_t *lredo, int64_t *wst)
{
    lane_t *L = (lane_t *)calloc((size_t)nl, sizeof(lane_t));
    const int oe_ins = p->o_ins + p->e_ins, oe_del = p->o_del + p->e_del;
    int maxsc = 0, k, i, j, maxq = 0, wl_max = -1, wl_min = 1 << 30, gz = 0, pruned = 0, skip = 1, rmark = 0;
    int prune = c->prune, rprune = c->rprune;
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
        l->P = INT_MIN;
        l->alive = l->tlen > 0;
        if (l->alive) wl_max = imax(wl_max, l->wl), wl_min = imin(wl_min, l->wl);
        maxq = imax(maxq, l->qlen);
    }
    const int QMAX = maxq < 32 ? 32 : maxq < 64 ? 64 : maxq < 96 ? 96 : maxq < 128 ? 128 : 160;
    const int NG = QMAX / 4;
    int gr = NG;                          /* the right cap: NG = none */
    if (QMAX < c->sqmin) skip = 0;
    if (QMAX < prune) prune = 0;          /* 0 (off) or the smallest QMAX class that carries the rule */
    if (QMAX < rprune || !skip) rprune = 0;
    for (i = 0;; ++i) {
        int any = 0, emax = -1, emaxu = -1;
        for (k = 0; k < nl; ++k) {
            lane_t *l = &L[k];
            l->act = l->alive && i < l->tlen;
            l->alive = l->act;
            if (!l->act) continue;
            any = 1;
            l->beg = imax(0, i - l->wl);
            l->end = imin(imin(l->endc, i + l->wl + 1), l->qlen);
            emaxu = imax(emaxu, imin(i + l->wl + 1, l->qlen));
            l->end = imin(l->end, 4 * gr);                /* the cap */
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
        if (rmark && gr < NG) wst[6] += imax((imin(emaxu, QMAX - 1) >> 2) - ghi, 0);   /* up to the static band end */
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
                /* item 12's certificate, in a wave marked by either prune (best is still the old one) */
                if ((pruned || rmark) && !better && m > 0 && p->zdrop > 0 && l->best - m > p->zdrop) {
                    if (!l->redo) wst[9] += 1;
                    l->redo = 1, l->alive = 0;
                }
                if (pruned && l->alive && h1 == 0) {
                    if (!l->redo) wst[9] += 1;
                    l->redo = 1, l->alive = 0;
                }
                if (better) {
                    l->moff = imax(l->moff, abs(mj - i));
                    l->best_i = i, l->best_j = mj, l->best = m;
                }
                /* the right prune's certificate: what leaves the computed columns goes through h1 */
                if (rmark && l->end == 4 * gr && l->end < l->qlen) wst[12] += !l->clip, l->clip = 1;
                if (rmark && !l->redo && l->clip && l->end < l->qlen) {
                    const int T = l->best - c->margin;
                    if (h1 > 0 && h1 + (l->qlen - l->end) >= T) {
                        wst[8] += 1;
                        l->redo = 1, l->alive = 0;
                    } else
                        l->P = imax(l->P, imax(T, 0));
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
            if (QMAX > 64 && (i & c->sphase) == c->sphase && anywant)
                for (k = 0; k < nl; ++k) {
                    lane_t *l = &L[k];
                    if (!l->act || !l->want) continue;
                    int ub = 0, s;
                    for (s = imax(l->beg + 1, jstart); s <= imin(l->end, 4 * ghi + 3); ++s)
                        ub = imax(ub, l->h[s] + (l->qlen - s));
                    if (ub <= l->best && ub < l->gsc) l->alive = 0;
                }
        }
        if (skip && (i & c->smask) == c->srow) {
            /* the prefix bound: while group gz is zero in both planes of every lane still alive -- or,
               with the left prune, cannot reach gscore in any of them */
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
            /* the right cap: the precheck, then, on every refresh until the wave is marked and on every fourth
               one after that, the walk down from the group under the cap; then the soft retreat -- one group
               up when a staying lane's crossing value at the cap or within RWIN slots under it comes near its
               threshold */
            if (rprune) {
                int pre = 1, stay = 0;
                for (k = 0; k < nl; ++k) {
                    const lane_t *l = &L[k];
                    if (!l->act || !l->alive) continue;
                    stay = 1;
                    pre &= i >= c->row0 && i - l->best_i <= c->k;
                }
                if (!pre) {
                    if (rmark && gr < NG) gr += 1, wst[7] += 1;
                } else if (stay && (!rmark || (i & c->wmask) == (c->srow & c->wmask)))
                    while (gr - 1 >= gz + 2) {
                        const int G = gr - 1;
                        int ok = 1;
                        wst[11] += 1;
                        for (k = 0; k < nl && ok; ++k) {
                            const lane_t *l = &L[k];
                            if (!l->act || !l->alive) continue;
                            const int T = l->best - c->margin;
                            int ub = 1 + (l->qlen - 4 * G);
                            for (j = 4 * G; j < 4 * G + 4; ++j) {
                                if (l->h[j] > 0) ub = imax(ub, l->h[j] + (l->qlen - j));
                                if (l->e[j] > 0) ub = imax(ub, l->e[j] + (l->qlen - 1 - j));
                            }
                            ok &= ub + c->slack < T;
                        }
                        if (!ok) break;
                        for (k = 0; k < nl; ++k) {
                            lane_t *l = &L[k];
                            for (j = 4 * G; j < 4 * G + 4; ++j) l->h[j] = l->e[j] = 0;
                            if (l->act && l->alive) l->P = imax(l->P, imax(l->best - c->margin, 0));
                        }
                        gr = G, rmark = 1;
                        wst[5] += 1;
                    }
            }
            if (rprune && rmark && gr < NG) {
                int up = 0;
                for (k = 0; k < nl; ++k) {
                    const lane_t *l = &L[k];
                    if (!l->act || !l->alive || l->end >= l->qlen || l->end + c->rwin < 4 * gr) continue;
                    up |= l->h1 + (l->qlen - l->end) + c->slack2 >= l->best - c->margin;
                }
                if (up) gr += 1, wst[7] += 1;
            }
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
        /* the final certificate: P tracked, or (touched form) best - MARGIN for every lane with P set */
        if (!l->redo && l->P != INT_MIN && l->gsc < (c->touched ? imax(l->best - c->margin, 0) : l->P))
            l->redo = 1, wst[10] += 1;
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
void rp_model(const par_t *p, const cfg_t *c, pair_t *pairs, const int32_t *idx, int32_t n, const uint8_t *ref,
              const uint8_t *qer, int32_t w, int32_t wa, int32_t wb, int32_t *lrows, uint8_t *lredo, int64_t *wst)
{
    for (int32_t v = wa; v < wb; ++v)
        wave(p, c, pairs, idx + 64 * v, imin(64, n - 64 * v), ref, qer, w, lrows, lredo, wst + NST * v);
}
"""

# the kernel's macros (bsw_pc.hip)
MARGIN = 20                    # BSW_PC_RP_MARGIN: T = best - MARGIN
SLACK = 12                     # BSW_PC_RP_SLACK: the zeroing test's distance from T
SLACK2 = 11                    # BSW_PC_RP_SLACK2: the soft retreat's
K = 16                         # BSW_PC_RP_K: rows since the last new best the precheck allows
WMASK = 15                     # BSW_PC_RP_WALK_MASK: a marked wave walks on refresh rows with (i & WMASK) == (SKIP_ROW & WMASK)
RWIN = 4                       # BSW_PC_RP_RWIN: the retreat looks at lanes whose band end is within RWIN slots of the cap
ROW0 = 25                      # BSW_PC_RP_ROW0: the first row on which the cap may be set
TOUCHED = 0                    # 0 (as built): P tracked per lane (thresholds below 0 count as 0); 1: the one-bit form,
                               # final certificate gsc >= best - MARGIN for every lane that was alive at a prune
RPRUNE_QMIN = lpm.PRUNE_QMIN   # the classes BSW_PC_PRUNE_QMIN selects

# per-wave figures.  cap_span: groups between the wave's clamped band end and its static band end, summed over the
# rows under a cap -- an upper bound of what the cap removes (the lazy edge may have dropped some of them anyway);
# what it removes is the difference in `entered` against left_prune_model.  clipped: lanes whose band end ever sat
# at the cap.  redo_item12: item 12's certificate (z-drop, or h1 == 0 in a left-pruned wave)
WST = ("rows", "entered", "skipped", "left_events", "redo", "right_events", "cap_span", "retreats",
       "redo_crossing", "redo_item12", "redo_final", "group_tests", "clipped")
NST = len(WST)


class Cfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("prune", "smask", "srow", "sphase", "sqmin", "rprune", "margin",
                                               "slack", "slack2", "k", "row0", "wmask", "rwin", "touched")]


_lib = None


def build(dirpath):
    """Compile this model and the two it leans on into `dirpath`; once per process.  Returns the
    triple (right-prune model, left-prune model, skip model) that run() takes."""
    global _lib
    if _lib is None:
        src = os.path.join(str(dirpath), "rp_model.c")
        so = os.path.join(str(dirpath), "librp_model.so")
        with open(src, "w") as f:
            f.write(MODEL_C)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src], check=True)
        _lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int32
        _lib.rp_model.argtypes = [P, P, P, P, I, P, P, I, I, I, P, P, P]
        _lib.rp_model.restype = None
    llib, slib = lpm.build(dirpath)
    return _lib, llib, slib


def run(libs, params, pairs, ref, qer, w, order=None, rprune=True, threads=8, margin=None, slack=None, slack2=None,
        k=None, row0=None, wmask=None, rwin=None, touched=None):
    """(outputs, rows per pair, redo mark per pair, per-wave figures [nw, NST]): `pairs` is not modified.
    `order` as in left_skip_model.run().  The redo lanes are recomputed without either prune, in list
    order, and their outputs and rows merged in.  The constants default to the module's values."""
    lib, _, slib = libs
    pick = lambda v, d: d if v is None else v            # noqa: E731
    cfg = Cfg(lpm.PRUNE_QMIN, lsm.SKIP_MASK, lsm.SKIP_ROW, lsm.SCAN_PHASE, lsm.SKIP_QMIN,
              RPRUNE_QMIN if rprune else 1 << 20, pick(margin, MARGIN), pick(slack, SLACK), pick(slack2, SLACK2),
              pick(k, K), pick(row0, ROW0), pick(wmask, WMASK), pick(rwin, RWIN), pick(touched, TOUCHED))
    out = pairs.copy()
    idx = np.ascontiguousarray(np.arange(len(out)) if order is None else order, np.int32)
    n = len(idx)
    nw = (n + 63) // 64
    rows = np.zeros(len(out), np.int32)
    redo = np.zeros(len(out), np.uint8)
    wst = np.zeros((nw, NST), np.int64)
    ref = np.ascontiguousarray(ref, np.uint8)
    qer = np.ascontiguousarray(qer, np.uint8)
    step = max(1, (nw + threads - 1) // threads)

    def part(a):
        lib.rp_model(ctypes.byref(params), ctypes.byref(cfg), ctypes.c_void_p(out.ctypes.data),
                     ctypes.c_void_p(idx.ctypes.data), n, ctypes.c_void_p(ref.ctypes.data),
                     ctypes.c_void_p(qer.ctypes.data), w, a, min(nw, a + step), ctypes.c_void_p(rows.ctypes.data),
                     ctypes.c_void_p(redo.ctypes.data), ctypes.c_void_p(wst.ctypes.data))

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
    return out, rows, redo, np.concatenate(wsts) if wsts else np.zeros((0, NST), np.int64)


def totals(wst):
    """The per-wave figures summed, by name."""
    t = dict(zip(WST, (int(v) for v in wst.sum(0))))
    t["refused"] = t["group_tests"] - t["right_events"]      # group tests the walk stopped at
    return t


# ---- batches built to exercise the cap, the certificates and the redo pass (CPU model test and GPU test) ----

def clipped_tails(n, seed):
    """a. late_collapse at base 60, 100 and 130: the query's tail does not align, gscore stays far below
    best and the final certificate sends the capped lanes to redo."""
    per = n // 3
    return lpm.concat(*(lpm.late_collapse(per, seed + k, at=at) for k, at in enumerate((60, 100, 130))))


def second_diagonal(n, seed, xlen=75, tlen=300):
    """b. query = X X' (X' a light mutation of X) against a window that holds X once, at its start: the
    cells (i, xlen + i) of the second copy score high to the right of the main diagonal."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        r = lsm._rng_seq(rng, tlen)
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
        r = lsm._rng_seq(rng, tlen)
        ins = int(rng.integers(20, 41))
        at = near + int(rng.integers(-8, 9))
        q = np.concatenate([r[:at], lsm._rng_seq(rng, ins), r[at:]])[:qlen]
        items.append((r, q.astype(np.uint8), int(rng.integers(19, 101))))
    return bswgen.assemble(items)


def low_h0(n, seed):
    """d. flagship-shaped pairs with h0 1-15: the first row's tail dies within a few columns."""
    p, r, q = lpm.c2_shaped(n, seed)
    p["h0"] = np.random.default_rng(seed + 1).integers(1, 16, len(p))
    return p, r, q


def class_tops(nwaves, seed, qlens=(127, 159), tail=37):
    """f. qlen at the top of both classes that carry the rule; 37 + 64 k pairs per class."""
    return lpm.class_edges(64 * nwaves + tail, seed, qlens=qlens)


def odd_lane(nwaves, seed, qlen=150, tlen=300):
    """g. related pairs with two early-dying lanes in every 64: their queries copy the window up to base
    40 or 70 and are unrelated after it, so the default key (seed identities over query[10, 40)) sorts
    them among the related lanes, h0 deciding the wave."""
    import bswgen
    rng = np.random.default_rng(seed)
    items = []
    for v in range(nwaves):
        for k in range(64):
            r = lsm._rng_seq(rng, tlen)
            q = r[:qlen].copy()
            if k == 7:
                q[70:] = lsm._rng_seq(rng, qlen - 70)
            if k == 29:
                q[40:] = lsm._rng_seq(rng, qlen - 40)
            items.append((r, q, int(rng.integers(30, 101))))
    return bswgen.assemble(items)
