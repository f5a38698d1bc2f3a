/* CPU model of the packed-column kernel's row loop (bsw_pc.hip), one wavefront of up to 64 lanes in lockstep,
 * with the kernel's three wave-level rules, each behind a flag of cfg_t.  The
 * constants are the kernel's own: bsw_pc_rules.h, through pc_model_defaults().  tests/pc_wave_model.py is the
 * Python side.
 *
 * The loop: the static left edge beg = max(0, i - w) (§3 item 1) and the lazy right edge (§3 items 3, 9); per
 * row the wave's entered groups [min beg >> 2, max end >> 2] of four slots each, every lane computing every
 * column of an entered group up to its own end, the columns left of its own beg included (their values are
 * never read: F and H are reset entering column beg); the early stop (§3 item 10) on the kernel's schedule, its
 * per-cell scan reading only the slots of entered groups.  The QMAX class of a wave is that of its longest
 * query (qlen < QMAX); classes below skip_qmin carry no skip, classes below prune_qmin neither prune, and
 * classes up to 64 no per-cell scan, as compiled.
 *
 * skip (item 11): gz, the wave-uniform number of leading groups that hold H == 0 and E == 0 in every slot of
 * every lane still alive, refreshed after rows with (i & skip_mask) == skip_row from the stored rows; groups
 * below gz are not computed and keep their stored values.
 *
 * prune (item 12): at the refresh, when group gz fails the zero test, gz also passes over it when i > wl_max
 * (every lane's static beg > 0) and every lane that stays alive has end == qlen, gsc > 0 and
 *     H plane: every slot s of the group with s > beg and h[s] > 0 has h[s] + (qlen - s) < gsc
 *     E plane: every slot s of the group with s >= beg and e[s] > 0 has e[s] + (qlen - 1 - s) < gsc
 * (the explicit E test, not the one-slot lookahead through H); the group's slots are then set to 0 in every
 * lane and the wave's `pruned` flag is set.  On every later row of a pruned wave, after the row-end update of
 * best / alive and before the early stop, a lane is sent to REDO when it is act, not better, m > 0 and
 * z-dropped by the mj-free bound best - m > zdrop, or still alive with h1 == 0.  A redo lane retires and stores
 * nothing.  A lane whose row maximum is 0 retires as in the plain loop and keeps its outputs: every cell of its
 * true row is then a changed cell, below the early stop's bound.
 *
 * rprune (item 13):
 *   - a wave-uniform right cap gr (a group index, QMAX / 4 = no cap): every lane's band end is clamped to
 *     slot 4 gr at the row head, so the groups above gr leave the entered set and group gr runs as the
 *     row's right-edge group;
 *   - at the refresh, after the walk of gz: when i >= row0 and every lane that stays alive had a new best
 *     within the last k rows, the cap walks down from group gr - 1 while, in every staying lane, every slot s
 *     of the group has
 *         h[s] > 0:  h[s] + (qlen - s)     + slack < T        T = best - margin (best after the row)
 *         e[s] > 0:  e[s] + (qlen - 1 - s) + slack < T
 *         floor:     1 + (qlen - 4 G)      + slack < T
 *     and the group lies at or above gz + 2; a passed group is set to 0 in every lane, the wave is marked
 *     and every staying lane's P (the largest threshold ever applied to it) takes T.  When the precheck
 *     fails under a cap the cap retreats one group;
 *   - on every row of a marked wave, after the row-end update of best / alive: a lane that is active, has
 *     no new best, m > 0 and best - m > zdrop goes to REDO (item 12's certificate b); a lane whose band
 *     end sits at the cap (end == 4 gr < qlen) is marked CLIPPED for good; a clipped lane with end < qlen
 *     and h1 > 0 goes to REDO when h1 + (qlen - end) >= T, else its P takes T;
 *   - at the refresh of a marked wave, after the precheck and the walk, the cap retreats one group when some
 *     staying lane with end < qlen at the cap or within rwin slots under it has h1 + (qlen - end) + slack2
 *     >= T -- a cap the walk has just put above a moving band edge is taken back before the edge reaches
 *     it, so a band narrower than the query never clips; once marked, a wave walks only on the refresh rows
 *     that walk_mask selects;
 *   - when a lane with P set ends, by any route, it goes to REDO unless gsc >= P (thresholds below 0 are
 *     applied as 0, as the kernel's bit field stores them).  touched = 1 is the one-bit form the kernel does
 *     not carry: gsc >= best - margin for every lane that was alive at a prune.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include "bsw_pc_rules.h"

typedef struct { int32_t idr, idq, id, len1, len2, h0, seqid, regid, score, tle, gtle, qle, gscore, max_off; } pair_t;
typedef struct { int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus; int8_t mat[25]; } par_t;
/* the rules' flags, then the schedule and the constants (the kernel's macros, named in pc_model_defaults) */
typedef struct {
    int32_t skip, prune, rprune;
    int32_t skip_mask, skip_row, scan_phase, skip_qmin, prune_qmin;
    int32_t margin, slack, slack2, k, row0, walk_mask, rwin, touched;
} cfg_t;

void pc_model_defaults(cfg_t *c)
{
    c->skip = BSW_PC_LEFT_SKIP, c->prune = BSW_PC_LEFT_PRUNE, c->rprune = BSW_PC_RIGHT_PRUNE;
    c->skip_mask = BSW_PC_SKIP_MASK, c->skip_row = BSW_PC_SKIP_ROW, c->scan_phase = BSW_PC_SCAN_PHASE;
    c->skip_qmin = BSW_PC_SKIP_QMIN, c->prune_qmin = BSW_PC_PRUNE_QMIN;
    c->margin = BSW_PC_RP_MARGIN, c->slack = BSW_PC_RP_SLACK, c->slack2 = BSW_PC_RP_SLACK2, c->k = BSW_PC_RP_K;
    c->row0 = BSW_PC_RP_ROW0, c->walk_mask = BSW_PC_RP_WALK_MASK, c->rwin = BSW_PC_RP_RWIN;
    c->touched = 0;       /* (no kernel macro: the form the kernel does not carry) */
}

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

/* one wave: lanes idx[0 .. nl), nl <= 64.  wst: NST figures, named by WST in the Python part */
static void wave(const par_t *p, const cfg_t *c, pair_t *pairs, const int32_t *idx, int nl, const uint8_t *ref,
                 const uint8_t *qer, int w, int32_t *lrows, uint8_t *lredo, int64_t *wst)
{
    lane_t *L = (lane_t *)calloc((size_t)nl, sizeof(lane_t));
    const int oe_ins = p->o_ins + p->e_ins, oe_del = p->o_del + p->e_del;
    int maxsc = 0, k, i, j, maxq = 0, wl_max = -1, gz = 0, pruned = 0, rmark = 0;
    int skip = c->skip, prune = c->prune, rprune = c->rprune;
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
        if (l->alive) wl_max = imax(wl_max, l->wl);
        maxq = imax(maxq, l->qlen);
    }
    const int QMAX = maxq < 32 ? 32 : maxq < 64 ? 64 : maxq < 96 ? 96 : maxq < 128 ? 128 : 160;
    const int NG = QMAX / 4;
    int gr = NG;                          /* the right cap: NG = none */
    if (QMAX < c->skip_qmin) skip = 0;
    if (QMAX < c->prune_qmin) prune = rprune = 0;
    if (!skip) rprune = 0;              /* (and no prune: it is a step of the skip's refresh) */
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
            if (QMAX > 64 && (i & c->scan_phase) == c->scan_phase && anywant)
                for (k = 0; k < nl; ++k) {
                    lane_t *l = &L[k];
                    if (!l->act || !l->want) continue;
                    int ub = 0, s;
                    for (s = imax(l->beg + 1, jstart); s <= imin(l->end, 4 * ghi + 3); ++s)
                        ub = imax(ub, l->h[s] + (l->qlen - s));
                    if (ub <= l->best && ub < l->gsc) l->alive = 0;
                }
        }
        if (skip && (i & c->skip_mask) == c->skip_row) {
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
                } else if (stay && (!rmark || (i & c->walk_mask) == (c->skip_row & c->walk_mask)))
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
void pc_model(const par_t *p, const cfg_t *c, pair_t *pairs, const int32_t *idx, int32_t n, const uint8_t *ref,
              const uint8_t *qer, int32_t w, int32_t wa, int32_t wb, int32_t *lrows, uint8_t *lredo, int64_t *wst)
{
    for (int32_t v = wa; v < wb; ++v)
        wave(p, c, pairs, idx + 64 * v, imin(64, n - 64 * v), ref, qer, w, lrows, lredo, wst + NST * v);
}
