"""CPU model of the packed-column kernel's left skip.

Unlike tests/early_stop_model.py, which is the literal ksw_extend2 loop with a rule added, this
models the KERNEL's loop (bsw_pc.hip), one wavefront of up to 64 lanes in lockstep:

  - the static left edge beg = max(0, i - w) (§3 item 1) and the lazy right edge (§3 items 3, 9);
  - per row the wave's entered groups [min beg >> 2, max end >> 2] of four slots each; every lane
    computes every column of an entered group up to its own end, the columns left of its own beg
    included (their values are never read: F and H are reset entering column beg);
  - gz, the wave-uniform number of leading groups that hold H == 0 and E == 0 in every slot of every
    lane still alive, refreshed after rows with (i & SKIP_MASK) == SKIP_ROW from the stored rows;
    groups below gz are not computed and keep their stored values;
  - the early stop (§3 item 10) on the kernel's schedule, its per-cell scan reading only the slots
    of entered groups;
  - the QMAX class of a wave is that of its longest query (qlen < QMAX); classes below
    SKIP_QMIN carry no skip and classes up to 64 no per-cell scan, as compiled.

Per pair it returns the six outputs and the rows the lane ran; per wave the rows, the groups
entered and the groups the skip removed from the entered set.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

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
    int best, best_i, best_j, max_ie, gsc, moff, alive, act, want, rows;
    const uint8_t *tg, *qy;
} lane_t;

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

/* one wave: lanes idx[0 .. nl), nl <= 64.  wst = {rows, groups entered, groups skipped} */
static void wave(const par_t *p, pair_t *pairs, const int32_t *idx, int nl, const uint8_t *ref, const uint8_t *qer,
                 int w, int skip, int smask, int srow, int sphase, int sqmin, int32_t *lrows, int64_t *wst)
{
    lane_t *L = (lane_t *)calloc((size_t)nl, sizeof(lane_t));
    const int oe_ins = p->o_ins + p->e_ins, oe_del = p->o_del + p->e_del;
    int maxsc = 0, k, i, j, maxq = 0, wl_max = -1, wl_min = 1 << 30, gz = 0;
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
        if (l->alive) wl_max = imax(wl_max, l->wl), wl_min = imin(wl_min, l->wl);
        maxq = imax(maxq, l->qlen);
    }
    const int QMAX = maxq < 32 ? 32 : maxq < 64 ? 64 : maxq < 96 ? 96 : maxq < 128 ? 128 : 160;
    const int NG = QMAX / 4;
    if (QMAX < sqmin) skip = 0;
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
                if (j == l->beg && j > 0) f = 0, h1 = 0;      /* the reset entering column beg (beg == end too) */
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
        /* the prefix bound: while group gz is zero in both planes of every lane still alive */
        if (skip && (i & smask) == srow)
            while (gz < NG) {
                int z = 1;
                for (k = 0; k < nl && z; ++k) {
                    const lane_t *l = &L[k];
                    if (!l->act || !l->alive) continue;
                    for (j = 4 * gz; j < 4 * gz + 4; ++j) z &= l->h[j] == 0 && l->e[j] == 0;
                }
                if (!z) break;
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
        sp->score = l->best, sp->tle = l->best_i + 1, sp->gtle = l->max_ie + 1, sp->qle = l->best_j + 1;
        sp->gscore = l->gsc, sp->max_off = l->moff;
        lrows[idx[k]] = l->rows;
    }
    free(L);
}

/* waves wa .. wb - 1 of the lane order idx[0 .. n): wave v holds idx[64 v .. 64 v + 63] */
void ls_model(const par_t *p, pair_t *pairs, const int32_t *idx, int32_t n, const uint8_t *ref, const uint8_t *qer,
              int32_t w, int32_t skip, int32_t smask, int32_t srow, int32_t sphase, int32_t sqmin, int32_t wa,
              int32_t wb, int32_t *lrows, int64_t *wst)
{
    for (int32_t v = wa; v < wb; ++v)
        wave(p, pairs, idx + 64 * v, imin(64, n - 64 * v), ref, qer, w, skip, smask, srow, sphase, sqmin, lrows,
             wst + 3 * v);
}
"""

# the kernel's compiled-in schedule (bsw_pc.hip)
SKIP_MASK = 3                  # BSW_PC_SKIP_MASK
SKIP_ROW = 1                   # BSW_PC_SKIP_ROW
SKIP_QMIN = 96                 # BSW_PC_SKIP_QMIN
SCAN_PHASE = 3                 # BSW_PC_SCAN_PHASE
_lib = None


def build(dirpath) -> ctypes.CDLL:
    """Compile the model into `dirpath` (a test's tmp_path) and load it; once per process."""
    global _lib
    if _lib is None:
        src = os.path.join(str(dirpath), "ls_model.c")
        so = os.path.join(str(dirpath), "libls_model.so")
        with open(src, "w") as f:
            f.write(MODEL_C)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src], check=True)
        _lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int32
        _lib.ls_model.argtypes = [P, P, P, I, P, P, I, I, I, I, I, I, I, I, P, P]
        _lib.ls_model.restype = None
    return _lib


def run(lib, params, pairs, ref, qer, w, order=None, skip=True, threads=8, skip_mask=SKIP_MASK, skip_row=SKIP_ROW,
        scan_phase=SCAN_PHASE, skip_qmin=SKIP_QMIN):
    """(outputs, rows per pair, per-wave [rows, groups entered, groups skipped]): `pairs` is not
    modified.  `order` lists the lanes (wave v = order[64 v : 64 v + 64]; default: every pair, as
    given); pairs it leaves out keep their input fields and 0 rows."""
    out = pairs.copy()
    idx = np.ascontiguousarray(np.arange(len(out)) if order is None else order, np.int32)
    n = len(idx)
    nw = (n + 63) // 64
    rows = np.zeros(len(out), np.int32)
    wst = np.zeros((nw, 3), np.int64)
    ref = np.ascontiguousarray(ref, np.uint8)
    qer = np.ascontiguousarray(qer, np.uint8)
    step = max(1, (nw + threads - 1) // threads)

    def part(a):
        lib.ls_model(ctypes.byref(params), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(idx.ctypes.data), n,
                     ctypes.c_void_p(ref.ctypes.data), ctypes.c_void_p(qer.ctypes.data), w, int(skip), skip_mask,
                     skip_row, scan_phase, skip_qmin, a, min(nw, a + step), ctypes.c_void_p(rows.ctypes.data),
                     ctypes.c_void_p(wst.ctypes.data))

    if nw:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(part, range(0, nw, step)))
    return out, rows, wst


def run_planned(lib, params, pairs, ref, qer, w, **kw):
    """As run(), with the lanes laid out as the engine lays them out: one launch per QMAX class
    over its slice of default_order() -- no wave holds pairs of two classes."""
    order = default_order(pairs, ref, qer)
    cls = qmax_class(pairs)[order]
    out, rows, wsts = pairs.copy(), np.zeros(len(pairs), np.int32), []
    for c in np.unique(cls):
        sub = order[cls == c]
        o, r, wst = run(lib, params, pairs, ref, qer, w, order=sub, **kw)
        out[sub], rows[sub] = o[sub], r[sub]
        wsts.append(wst)
    return out, rows, np.concatenate(wsts) if wsts else np.zeros((0, 3), np.int64)


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


# ---- batches built to exercise the skip (CPU model test and GPU test) ----

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
