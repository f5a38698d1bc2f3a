"""Pure-Python restatement of mem_pestat, mem_pair and the decision block of mem_sam_pe as
include/bsw_pe.h states them -- TEST INFRASTRUCTURE (tests/test_pe.py).  Primary marking, MAPQ and
hash_64 are tests/regsel_py.py's, the marking's sort klib's ks_introsort (tests/memchain_py.py);
mem_pair's u is built and sorted whole here (the library never stores it).  Every call reports the
branches taken and the distance of every (int)(x + .499) from its integer boundary."""

import math

import numpy as np

import regsel_py as sp
from memchain_py import introsort  # noqa: F401  (regsel_py.mark_primary sorts with it)

PESTAT_DTYPE = np.dtype([("low", np.int32), ("high", np.int32), ("failed", np.int32), ("n", np.int32),
                         ("avg", np.float64), ("std", np.float64)])
PAIR_DTYPE = np.dtype([("paired", np.int32), ("z", np.int32, (2,)), ("mapq", np.int32, (2,)), ("proper", np.int32),
                       ("score", np.int32), ("sub", np.int32), ("n_sub", np.int32), ("q_pe", np.int32)])

DEFAULT_OPT = dict(l_pac=0, id0=0, max_ins=10000, min_seed_len=19, b=4, T=30, pen_unpaired=17, mapQ_coef_len=50,
                   mapQ_coef_fac=3, mask_level=0.5)
PE_MAX_INS = 1 << 16
MAX_PER_READ = 1 << 20

BRANCHES = ("stat_empty", "stat_sub_skip", "stat_is_zero", "stat_far", "stat_kept", "dir_few", "dir_low_clamp",
            "dir_widen_low", "dir_widen_high", "dir_minor_failed",
            "fast_path", "general_path", "pair_tried", "dir_failed_skip", "no_last", "dist_break", "dist_skip",
            "q_clamp0", "u_push", "u_empty", "u_many", "n_sub", "z_nonzero", "multi", "paired", "unpaired_preferred",
            "proper", "chosen_secondary", "lift40", "csub_cap", "frac_rep_pe", "nopair_none", "nopair_proper",
            "empty_end", "remark_reorder")

M64 = (1 << 64) - 1
M_SQRT1_2 = 0.70710678118654752440


def pe_opt(**kw):
    o = dict(DEFAULT_OPT)
    o.update(kw)
    return o


def check_opt(o, n_reads):
    if n_reads < 0 or n_reads & 1 or o["l_pac"] <= 0 or o["id0"] & 1 or not 1 <= o["max_ins"] <= PE_MAX_INS:
        raise ValueError("BSW_E_INVAL")


def infer_dir(l_pac, b1, b2):
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def cal_sub(o, a, scoring_a):
    ml = np.float32(o["mask_level"])
    for j in range(1, len(a)):
        b_max, e_min = max(a[j]["qb"], a[0]["qb"]), min(a[j]["qe"], a[0]["qe"])
        if e_min > b_max:
            min_l = min(a[j]["qe"] - a[j]["qb"], a[0]["qe"] - a[0]["qb"])
            if np.float32(e_min - b_max) >= np.float32(min_l) * ml:
                return a[j]["score"]
    return o["min_seed_len"] * scoring_a


def lists_of(o, sel_regs, sel_info, read_first):
    """per read its list of region dicts; raises where the library returns BSW_E_RANGE"""
    first = [int(v) for v in read_first]
    if first[0] < 0 or any(b < a for a, b in zip(first, first[1:])) or first[-1] > len(sel_regs):
        raise ValueError("BSW_E_RANGE: read_first")
    out = []
    for r in range(len(first) - 1):
        if first[r + 1] - first[r] > MAX_PER_READ:
            raise ValueError("BSW_E_RANGE: list length")
        a = []
        for k in range(first[r], first[r + 1]):
            x = {f: int(sel_regs[k][f]) for f in sp.ALNREG_FIELDS}
            x.update({f: int(sel_info[k][f]) for f in sp.SELINFO_DTYPE.names if f != "frac_rep"})
            x["frac_rep"] = np.float32(sel_info[k]["frac_rep"])
            if not 0 <= x["rb"] < 2 * o["l_pac"]:
                raise ValueError("BSW_E_RANGE: rb")
            a.append(x)
        out.append(a)
    return out


# ---------------------------------------------------------------- statistics
def pestat_of(q, tr):
    """one direction: q = its kept insert sizes -> dict(low, high, failed, n, avg, std)"""
    q = sorted(q)
    n = len(q)
    r = dict(low=0, high=0, failed=0, n=n, avg=0.0, std=0.0)
    if n < 10:
        tr.cnt["dir_few"] += 1
        r["failed"] = 1
        return r
    p25, p75 = q[tr.trunc(.25 * n + .499)], q[tr.trunc(.75 * n + .499)]
    q[tr.trunc(.50 * n + .499)]                              # p50: taken upstream, used only in its log line
    low = tr.trunc(p25 - 2.0 * (p75 - p25) + .499)
    low = max(low, 1)
    high = tr.trunc(p75 + 2.0 * (p75 - p25) + .499)
    avg, x = 0.0, 0
    for v in q:
        if low <= v <= high:
            avg += v
            x += 1
    avg /= x
    std = 0.0
    for v in q:
        if low <= v <= high:
            std += (v - avg) * (v - avg)
    std = math.sqrt(std / x)
    low = tr.trunc(p25 - 3.0 * (p75 - p25) + .499)
    high = tr.trunc(p75 + 3.0 * (p75 - p25) + .499)
    if low > avg - 4.0 * std:
        tr.cnt["dir_widen_low"] += 1
        low = tr.trunc(avg - 4.0 * std + .499)
    if high < avg + 4.0 * std:
        tr.cnt["dir_widen_high"] += 1
        high = tr.trunc(avg + 4.0 * std + .499)
    if low < 1:
        tr.cnt["dir_low_clamp"] += 1
        low = 1
    r.update(low=low, high=high, avg=avg, std=std)
    return r


def pestat_of_dirs(isize, tr):
    """isize[d] = the kept values of direction d -> pes PESTAT_DTYPE [4]"""
    rs = [pestat_of(isize[d], tr) for d in range(4)]
    mx = max(r["n"] for r in rs)
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    for d, r in enumerate(rs):
        if r["failed"] == 0 and r["n"] < mx * 0.05:
            tr.cnt["dir_minor_failed"] += 1
            r["failed"] = 1
        for f in PESTAT_DTYPE.names:
            pes[d][f] = r[f]
    return pes


def pe_stat(sel_regs, sel_info, read_first, opt, scoring_a, tr=None):
    """the library's bsw_pe_stat: -> (pes, Trace, isize[4])"""
    o = opt
    tr = tr if tr is not None else sp.Trace()
    check_opt(o, len(read_first) - 1)
    L = lists_of(o, sel_regs, sel_info, read_first)
    isize = [[], [], [], []]
    for p in range(len(L) // 2):
        a0, a1 = L[2 * p], L[2 * p + 1]
        if not a0 or not a1:
            tr.cnt["stat_empty"] += 1
            continue
        if any(cal_sub(o, a, scoring_a) > 0.8 * a[0]["score"] for a in (a0, a1)):
            tr.cnt["stat_sub_skip"] += 1
            continue
        d, dist = infer_dir(o["l_pac"], a0[0]["rb"], a1[0]["rb"])
        if dist == 0:
            tr.cnt["stat_is_zero"] += 1
        elif dist > o["max_ins"]:
            tr.cnt["stat_far"] += 1
        else:
            tr.cnt["stat_kept"] += 1
            isize[d].append(dist)
    return pestat_of_dirs(isize, tr), tr, isize


# ---------------------------------------------------------------- pairing
def _raw(tr, d, a):
    return tr.trunc(6.02 * d / a + .499)


def mem_pair(o, pes, a0, a1, p, scoring_a, gaps, tr):
    """-> (u.n, o, sub, n_sub, z) -- z None and the scores 0 when u is empty"""
    l_pac = o["l_pac"]
    v = []
    for r, a in enumerate((a0, a1)):
        for i, x in enumerate(a):
            st = 1 if x["rb"] >= l_pac else 0
            v.append((x["rb"] if not st else 2 * l_pac - 1 - x["rb"], (x["score"] & 0xffffffff) << 32 | i << 2 | st << 1 | r))
    v.sort()
    id32 = ((o["id0"] >> 1) + p) & 0xffffffff
    t = (id32 << 8) & 0xffffffff
    t = t - (1 << 32) if t & 0x80000000 else t                # (int32), then sign-extended to 64 bits
    u = []
    last = [-1] * 4
    for i, (xi, yi) in enumerate(v):
        for r in (0, 1):
            d = pes[r << 1 | (yi >> 1 & 1)]
            if d["failed"]:
                tr.cnt["dir_failed_skip"] += 1
                continue
            which = r << 1 | ((yi & 1) ^ 1)
            if last[which] < 0:
                tr.cnt["no_last"] += 1
                continue
            for k in range(last[which], -1, -1):
                xk, yk = v[k]
                if (yk & 3) != which:
                    continue
                dist = xi - xk
                if dist > d["high"]:
                    tr.cnt["dist_break"] += 1
                    break
                if dist < d["low"]:
                    tr.cnt["dist_skip"] += 1
                    continue
                ns = (dist - float(d["avg"])) / float(d["std"])
                e = 2. * math.erfc(abs(ns) * M_SQRT1_2)
                lg = math.log(e) if e > 0 else -math.inf
                q = tr.trunc(float((yi >> 32) + (yk >> 32)) + .721 * lg * scoring_a + .499)
                if q < 0:
                    tr.cnt["q_clamp0"] += 1
                    q = 0
                uy = k << 32 | i
                u.append((q << 32 | (sp.hash_64(uy ^ (t & M64)) & 0xffffffff), uy))
                tr.cnt["u_push"] += 1
        last[yi & 3] = i
    if not u:
        tr.cnt["u_empty"] += 1
        return 0, 0, 0, 0, None
    u.sort()
    if len(u) > 2:
        tr.cnt["u_many"] += 1
    k, i = u[-1][1] >> 32, u[-1][1] & 0xffffffff
    z = [0, 0]
    z[v[k][1] & 1] = (v[k][1] & 0xffffffff) >> 2
    z[v[i][1] & 1] = (v[i][1] & 0xffffffff) >> 2
    best = u[-1][0] >> 32
    sub = u[-2][0] >> 32 if len(u) > 1 else 0
    o_del, e_del, o_ins, e_ins = gaps
    tmp = max(scoring_a + o["b"], o_del + e_del, o_ins + e_ins)
    n_sub = sum(1 for x, _ in u[:-1] if sub - (x >> 32) <= tmp)
    if n_sub:
        tr.cnt["n_sub"] += 1
    return len(u), best, sub, n_sub, z


def _remark(o, a, r, scoring_a, gaps, tr):
    """step 1 on one read's list"""
    if not a:
        return a
    before = [x["src"] for x in a]
    a = sp.mark_primary(o, a, r, scoring_a, gaps, tr)
    if [x["src"] for x in a] != before:
        tr.cnt["remark_reorder"] += 1
    for x in a:
        x["mapq"] = sp.approx_mapq(o, x, scoring_a, float(x["frac_rep"]), tr)
    return a


def pe_pair(pes, sel_regs, sel_info, read_first, opt, mat, gaps, tr=None):
    """the library's bsw_pe_pair: -> (sel_regs, sel_info, pairs PAIR_DTYPE, Trace); the inputs are
    left alone"""
    o = opt
    tr = tr if tr is not None else sp.Trace()
    check_opt(o, len(read_first) - 1)
    pes = [{f: pes[d][f] for f in ("low", "high", "failed", "avg", "std")} for d in range(4)]
    for d in pes:
        d.update(low=int(d["low"]), high=int(d["high"]), failed=int(d["failed"]))
        if not d["failed"] and not (math.isfinite(d["std"]) and d["std"] > 0 and math.isfinite(d["avg"])):
            raise ValueError("BSW_E_INVAL: std")
    a_sc = int(mat[0])
    L = lists_of(o, sel_regs, sel_info, read_first)
    pairs = np.zeros(len(L) // 2, dtype=PAIR_DTYPE)
    for p in range(len(L) // 2):
        tr.cnt["fast_path" if len(L[2 * p]) <= 1 and len(L[2 * p + 1]) <= 1 else "general_path"] += 1
        for e in (0, 1):
            L[2 * p + e] = _remark(o, L[2 * p + e], 2 * p + e, a_sc, gaps, tr)
        a = (L[2 * p], L[2 * p + 1])
        out = pairs[p]
        nu, best, sub, n_sub, z = 0, 0, 0, 0, None
        if a[0] and a[1]:
            tr.cnt["pair_tried"] += 1
            nu, best, sub, n_sub, z = mem_pair(o, pes, a[0], a[1], p, a_sc, gaps, tr)
            tr.cnt["n_u"] += nu
            out["score"], out["sub"], out["n_sub"] = best, sub, n_sub
        else:
            tr.cnt["empty_end"] += 1
        no_pairing = True
        if a[0] and a[1] and best > 0:
            if any(x["secondary"] < 0 and x["score"] >= o["T"] for e in (0, 1) for x in a[e][1:]):
                tr.cnt["multi"] += 1
            else:
                no_pairing = False
                score_un = a[0][0]["score"] + a[1][0]["score"] - o["pen_unpaired"]
                subo = max(sub, score_un)
                q_pe = _raw(tr, best - subo, a_sc)
                if n_sub > 0:
                    q_pe -= tr.trunc(4.343 * math.log(n_sub + 1) + .499)
                q_pe = max(min(q_pe, 60), 0)
                fr = np.float32(a[0][0]["frac_rep"]) + np.float32(a[1][0]["frac_rep"])
                if fr != 0:
                    tr.cnt["frac_rep_pe"] += 1
                q_pe = tr.trunc(q_pe * (1. - .5 * float(fr)) + .499)
                out["q_pe"] = q_pe
                tr.cnt["paired"] += 1
                out["paired"] = 1
                if best > score_un:
                    if z[0] or z[1]:
                        tr.cnt["z_nonzero"] += 1
                    for e in (0, 1):
                        c = a[e][z[e]]
                        if c["secondary"] >= 0:
                            tr.cnt["chosen_secondary"] += 1
                            c["sub"] = a[e][c["secondary"]]["score"]
                            c["secondary"] = -2
                        q_se = sp.approx_mapq(o, c, a_sc, float(c["frac_rep"]), tr)
                        if q_se <= q_pe:
                            if q_se + 40 < q_pe:
                                tr.cnt["lift40"] += 1
                            q_se = min(q_pe, q_se + 40)
                        cap = _raw(tr, c["score"] - c["csub"], a_sc)
                        if cap < q_se:
                            tr.cnt["csub_cap"] += 1
                            q_se = cap
                        out["z"][e], out["mapq"][e] = z[e], q_se
                    out["proper"] = 1
                else:
                    tr.cnt["unpaired_preferred"] += 1
                    for e in (0, 1):
                        out["z"][e] = 0
                        out["mapq"][e] = sp.approx_mapq(o, a[e][0], a_sc, float(a[e][0]["frac_rep"]), tr)
                    out["proper"] = 0
        if no_pairing:
            which = [0 if a[e] and a[e][0]["score"] >= o["T"] else -1 for e in (0, 1)]
            for e in (0, 1):
                out["z"][e] = which[e]
                out["mapq"][e] = a[e][0]["mapq"] if which[e] == 0 else 0
                if which[e] < 0:
                    tr.cnt["nopair_none"] += 1
            if which[0] == 0 and which[1] == 0:
                d, dist = infer_dir(o["l_pac"], a[0][0]["rb"], a[1][0]["rb"])
                if not pes[d]["failed"] and pes[d]["low"] <= dist <= pes[d]["high"]:
                    tr.cnt["nopair_proper"] += 1
                    out["proper"] = 1
        if out["proper"]:
            tr.cnt["proper"] += 1
    flat = [x for a in L for x in a]
    regs = np.zeros(len(flat), dtype=[(f, np.int64 if f in ("rb", "re") else np.int32) for f in sp.ALNREG_FIELDS])
    info = np.zeros(len(flat), dtype=sp.SELINFO_DTYPE)
    for i, x in enumerate(flat):
        for f in sp.ALNREG_FIELDS:
            regs[i][f] = x[f]
        for f in sp.SELINFO_DTYPE.names:
            info[i][f] = x[f]
    return regs, info, pairs, tr


def stats_of(tr, n_pairs):
    """the counters bsw_pe_last_stats reports after a pair call, from a Trace"""
    c = tr.cnt
    return dict(n_pairs=n_pairs, n_pairing_tried=c["pair_tried"], n_paired=c["paired"], n_multi=c["multi"],
                n_unpaired_preferred=c["unpaired_preferred"], n_proper=c["proper"], n_u=c["n_u"])
