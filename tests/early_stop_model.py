"""CPU model of the packed-column kernel's early stop and the batch builders of
its tests.

The model is the literal ksw_extend2 loop (written out again here) with the
stopping rule added after each completed row.  It is compiled by the tests with the system C
compiler and loaded through ctypes.  Modes:

  0  literal loop, no rule
  1  scalar bound on every row
  2  per-cell bound on every row
  3  the kernel's schedule: scalar bound on every row; per-cell bound on rows with
     (i & SCAN_PHASE) == SCAN_PHASE where the arg-max pre-test passes, and only for qlen >= 64
     (the QMAX 32 / 64 classes carry no scan)

Per pair it returns the six outputs, the number of rows it ran, their band cells and the row at
which the rule fired (-1: never).  A pair counts as retired early when the rule made it run fewer rows than the
literal loop.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import bswgen

MODEL_C = r"""
#include <stdint.h>
#include <stdlib.h>

typedef struct { int32_t idr, idq, id, len1, len2, h0, seqid, regid, score, tle, gtle, qle, gscore, max_off; } pair_t;
typedef struct { int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus; int8_t mat[25]; } par_t;
typedef struct { int32_t h, e; } cell_t;

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

static void one(const par_t *p, pair_t *sp, const uint8_t *tg, const uint8_t *qy, int w, int mode, int phase,
                int32_t *rows_out, int32_t *fired_out, int32_t *cells_out)
{
    const int qlen = sp->len2, tlen = sp->len1, h0 = sp->h0;
    const int oe_del = p->o_del + p->e_del, oe_ins = p->o_ins + p->e_ins;
    cell_t *eh = (cell_t *)calloc((size_t)qlen + 2, sizeof(cell_t));
    int maxsc = 0, i, j, rows = 0, fired = -1, cells = 0;
    for (i = 0; i < 25; ++i) maxsc = imax(maxsc, p->mat[i]);
    eh[0].h = h0;
    eh[1].h = h0 > oe_ins ? h0 - oe_ins : 0;
    for (j = 2; j <= qlen && eh[j - 1].h > p->e_ins; ++j) eh[j].h = eh[j - 1].h - p->e_ins;
    {
        int cap = (int)((double)(qlen * maxsc + p->end_bonus - p->o_ins) / p->e_ins + 1.);
        w = imin(w, imax(cap, 1));
        cap = (int)((double)(qlen * maxsc + p->end_bonus - p->o_del) / p->e_del + 1.);
        w = imin(w, imax(cap, 1));
    }
    int best = h0, best_i = -1, best_j = -1, max_ie = -1, gsc = -1, max_off = 0, beg = 0, end = qlen;
    for (i = 0; i < tlen; ++i) {
        int f = 0, h1, m = 0, mj = -1;
        const int8_t *srow = &p->mat[5 * (tg[i] > 4 ? 4 : tg[i])];
        ++rows;
        beg = imax(beg, i - w);
        end = imin(imin(end, i + w + 1), qlen);
        h1 = beg == 0 ? imax(h0 - (p->o_del + p->e_del * (i + 1)), 0) : 0;
        cells += imax(end - beg, 0);
        for (j = beg; j < end; ++j) {
            cell_t *c = &eh[j];
            int M = c->h, e = c->e, h, t;
            c->h = h1;
            M = M ? M + srow[qy[j] > 4 ? 4 : qy[j]] : 0;
            h = imax(imax(M, e), f);
            h1 = h;
            if (!(m > h)) mj = j;
            m = imax(m, h);
            t = imax(M - oe_del, 0);
            c->e = imax(e - p->e_del, t);
            t = imax(M - oe_ins, 0);
            f = imax(f - p->e_ins, t);
        }
        eh[end].h = h1;
        eh[end].e = 0;
        if (j == qlen) {
            if (!(gsc > h1)) max_ie = i;
            gsc = imax(gsc, h1);
        }
        if (m == 0) break;
        if (m > best) {
            best = m, best_i = i, best_j = mj;
            max_off = imax(max_off, abs(mj - i));
        } else if (p->zdrop > 0) {
            const int di = i - best_i, dj = mj - best_j;
            if (di > dj) {
                if (best - m - (di - dj) * p->e_del > p->zdrop) break;
            } else {
                if (best - m - (dj - di) * p->e_ins > p->zdrop) break;
            }
        }
        if (mode) {
            /* the rule, on the completed row i: slot s = eh[s].h = H(i, s - 1) for s in (beg, end];
             * kbeg is the kernel's left edge max(0, i - w): the slots in (kbeg, beg] are zero cells
             * the kernel computes and scans all the same */
            const int kbeg = imax(0, i - w);
            if (end == qlen && kbeg > 0) {
                int stop = 0;
                if (mode == 1 || mode == 3) {
                    const int ub = m + maxsc * imin(qlen - 1 - kbeg, tlen - 1 - i);
                    stop = ub <= best && ub < gsc;
                }
                if (!stop && mode >= 2) {
                    int scan = 1;
                    if (mode == 3) {
                        const int pre = m + maxsc * (qlen - 1 - mj);
                        scan = qlen >= 64 && (i & phase) == phase && pre <= best && pre < gsc;
                    }
                    if (scan) {
                        int ub = 0, s;
                        for (s = kbeg + 1; s <= end; ++s) ub = imax(ub, eh[s].h + maxsc * (qlen - s));
                        stop = ub <= best && ub < gsc;
                    }
                }
                if (stop) { fired = i; break; }
            }
        }
        for (j = beg; j < end && eh[j].h == 0 && eh[j].e == 0; ++j)
            ;
        beg = j;
        for (j = end; j >= beg && eh[j].h == 0 && eh[j].e == 0; --j)
            ;
        end = imin(j + 2, qlen);
    }
    free(eh);
    sp->score = best, sp->tle = best_i + 1, sp->gtle = max_ie + 1, sp->qle = best_j + 1;
    sp->gscore = gsc, sp->max_off = max_off;
    *rows_out = rows, *fired_out = fired, *cells_out = cells;
}

void es_model(const par_t *p, pair_t *pairs, const uint8_t *ref, const uint8_t *qer, int32_t n, int32_t w,
              int32_t mode, int32_t phase, int32_t *rows, int32_t *fired, int32_t *cells)
{
    for (int32_t k = 0; k < n; ++k)
        one(p, &pairs[k], ref + pairs[k].idr, qer + pairs[k].idq, w, mode, phase, &rows[k], &fired[k], &cells[k]);
}
"""

SCAN_PHASE = 3                 # the kernel's BSW_PC_SCAN_PHASE (bsw_pc.hip)
_lib = None


def build(dirpath) -> ctypes.CDLL:
    """Compile the model into `dirpath` (a test's tmp_path) and load it; once per process."""
    global _lib
    if _lib is None:
        src = os.path.join(str(dirpath), "es_model.c")
        so = os.path.join(str(dirpath), "libes_model.so")
        with open(src, "w") as f:
            f.write(MODEL_C)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src], check=True)
        _lib = ctypes.CDLL(so)
        P = ctypes.c_void_p
        _lib.es_model.argtypes = [P, P, P, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P, P]
        _lib.es_model.restype = None
    return _lib


def run(lib, params, pairs, ref, qer, w, mode, threads=8, phase=SCAN_PHASE, cells=None):
    """(outputs, rows, fired): `pairs` is not modified.  `cells` (an int32 array, one per pair)
    receives the band cells of the rows that ran (the literal loop's narrowed [beg, end))."""
    out = pairs.copy()
    n = len(out)
    rows = np.zeros(n, np.int32)
    fired = np.full(n, -1, np.int32)
    if cells is None:
        cells = np.zeros(n, np.int32)
    ref = np.ascontiguousarray(ref, np.uint8)
    qer = np.ascontiguousarray(qer, np.uint8)
    step = max(1, (n + threads - 1) // threads)

    def part(a):
        b = min(n, a + step)
        lib.es_model(ctypes.byref(params), ctypes.c_void_p(out[a:b].ctypes.data), ctypes.c_void_p(ref.ctypes.data),
                     ctypes.c_void_p(qer.ctypes.data), b - a, w, mode, phase, ctypes.c_void_p(rows[a:b].ctypes.data),
                     ctypes.c_void_p(fired[a:b].ctypes.data), ctypes.c_void_p(cells[a:b].ctypes.data))

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(0, n, step)))
    return out, rows, fired


def retired_fraction(lib, params, pairs, ref, qer, w, mode=3):
    """Share of the pairs on which the rule (mode) runs fewer rows than the literal loop."""
    _, rows0, _ = run(lib, params, pairs, ref, qer, w, 0)
    _, rows1, _ = run(lib, params, pairs, ref, qer, w, mode)
    return float((rows1 < rows0).mean())


def random_shapes(n, seed, tlen=(1, 320), qlen=(1, 159), h0=(0, 96)):
    """Vectorised mixed batch: a fifth each of random, exact, mutated (5 % substitutions and one
    indel of 1-3 bp), heavily mutated (25 %) and period-2 repeat queries; an eighth of the pairs
    start the query at a diagonal offset of up to 40 rows into the window."""
    rng = np.random.default_rng(seed)
    T = rng.integers(tlen[0], tlen[1] + 1, n)
    Q = rng.integers(qlen[0], qlen[1] + 1, n)
    kind = rng.integers(0, 5, n)
    off = np.where(rng.random(n) < 0.125, rng.integers(0, 41, n), 0)
    pairs = np.zeros(n, dtype=bswgen.SEQPAIR_DTYPE)
    idr = np.concatenate([[0], np.cumsum(T)[:-1]])
    idq = np.concatenate([[0], np.cumsum(Q)[:-1]])
    pairs["idr"], pairs["idq"], pairs["id"] = idr, idq, np.arange(n)
    pairs["len1"], pairs["len2"] = T, Q
    pairs["h0"] = rng.integers(h0[0], h0[1] + 1, n)
    pairs["seqid"] = np.arange(n)
    ref = rng.integers(0, 4, int(T.sum())).astype(np.uint8)
    ref[rng.random(len(ref)) < 0.005] = 4
    # period-2 repeats: the window is one motif tiled, at a random phase
    rp = np.repeat(np.arange(n), T)                      # pair of each reference base
    rk = np.arange(len(ref)) - np.repeat(idr, T)         # its row
    motif = rng.integers(0, 4, (n, 2)).astype(np.uint8)
    phase = rng.integers(0, 2, n)
    rep = kind[rp] == 4
    ref[rep] = motif[rp[rep], (rk[rep] + phase[rp[rep]]) & 1]
    # queries
    qp = np.repeat(np.arange(n), Q)
    qk = np.arange(int(Q.sum())) - np.repeat(idq, Q)
    qer = rng.integers(0, 4, len(qp)).astype(np.uint8)
    ipos = rng.integers(0, np.maximum(Q, 1))             # one indel per mutated pair
    ilen = np.where(np.isin(kind, (2, 3)), rng.integers(-3, 4, n), 0)
    src = qk + off[qp] + np.where(qk >= ipos[qp], ilen[qp], 0)
    copy = (kind[qp] != 0) & (src >= 0) & (src < T[qp])
    qer[copy] = ref[idr[qp[copy]] + src[copy]]
    psub = np.array([0.0, 0.0, 0.05, 0.25, 0.02])[kind]
    sub = copy & (rng.random(len(qp)) < psub[qp]) & (qer < 4)
    qer[sub] = (qer[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
    return pairs, ref, qer


def diagonal_pairs(n, seed, qlen=(60, 150), offs=(10, 40), twice=False, h0=(5, 90)):
    """Late improvements: the query's best placement lies `offs` rows down the window; with
    `twice` the window also holds a degraded copy of the query at its top, so the first
    alignment is overtaken by a later one."""
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        Q = int(rng.integers(qlen[0], qlen[1] + 1))
        d = int(rng.integers(offs[0], offs[1] + 1))
        q = rng.integers(0, 4, Q).astype(np.uint8)
        T = Q + d + int(rng.integers(20, 120))
        r = rng.integers(0, 4, T).astype(np.uint8)
        r[d:d + Q] = q
        if twice:
            k = min(d, Q)
            head = q[:k].copy()
            bad = rng.random(k) < 0.15
            head[bad] = (head[bad] + 1) & 3
            r[:k] = head
        if rng.random() < 0.5:
            q = bswgen.mutate(rng, q, Q, 0.03, 0.01)
        items.append((r, q, int(rng.integers(h0[0], h0[1] + 1))))
    return bswgen.assemble(items)
