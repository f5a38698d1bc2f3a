"""Pure-Python restatement of mem_sort_dedup_patch, mem_mark_primary_se and mem_approx_mapq_se as
include/bsw_sel.h states them -- TEST INFRASTRUCTURE (tests/test_regsel.py).  The sorts are klib's
ks_introsort (tests/memchain_py.py), the patch score is gen_cigar2 of tests/reg2aln_py.py (the CPU
oracle's ksw_global2 underneath); the loops, the float comparisons (numpy.float32, as C's float
options), the hash and MAPQ are written out here.  Every call reports the branches taken and the
distance of every (int)(x + .499) from its integer boundary."""

import math
from collections import Counter

import numpy as np

import reg2aln_py as rp
from memchain_py import introsort

SELINFO_DTYPE = np.dtype([("seedcov", np.int32), ("sub", np.int32), ("csub", np.int32), ("sub_n", np.int32),
                          ("n_comp", np.int32), ("secondary", np.int32), ("mapq", np.int32), ("src", np.int32),
                          ("frac_rep", np.float32)])
ALNREG_FIELDS = ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedlen0")

BRANCHES = ("fast_path", "drop_p", "drop_q", "patch_off", "patch_strand", "patch_order", "patch_w", "patch_r",
            "patch_dp", "patch_gapfree", "patch_ok", "patch_ratio", "identical", "secondary", "sub_n",
            "mapq_secondary", "mapq_sub_ge", "mapq_coef", "mapq_seedcov", "mapq_lowid", "mapq_subn", "mapq_frac_rep")

DEFAULT_OPT = dict(w=100, l_pac=0, max_chain_gap=10000, mask_level_redun=0.95, mask_level=0.5, min_seed_len=19, b=4,
                   mapQ_coef_len=50, mapQ_coef_fac=3, patch=1, id0=0)

M64 = (1 << 64) - 1


def sel_opt(**kw):
    o = dict(DEFAULT_OPT)
    o.update(kw)
    return o


def hash_64(key):
    key &= M64
    key = (key + (~(key << 32) & M64)) & M64
    key ^= key >> 22
    key = (key + (~(key << 13) & M64)) & M64
    key ^= key >> 8
    key = (key + (key << 3)) & M64
    key ^= key >> 15
    key = (key + (~(key << 27) & M64)) & M64
    key ^= key >> 31
    return key


class Trace:
    """branch counters and truncation margins of one call"""

    def __init__(self):
        self.cnt = Counter()
        self.margin = 1.0
        self.rounds = 0

    def trunc(self, x):
        """(int)(x) of C for x = ... + .499, remembering how close x came to an integer"""
        if not math.isfinite(x) or abs(x) >= 2 ** 31:
            return -(1 << 31)                        # (a conversion out of int's range saturates low)
        f = x - math.floor(x)
        self.margin = min(self.margin, f, 1.0 - f)
        return int(x)


def _f32(x):
    return np.float32(x)


def patch_reg(o, T, read, a, b, mat, gaps, tr, dp):
    """-> (score, w); 0 when refused.  a.rb <= b.rb"""
    W, l_pac = o["w"], o["l_pac"]
    if not o["patch"]:
        tr.cnt["patch_off"] += 1
        return 0, 0
    if a["rb"] < l_pac and b["rb"] >= l_pac:
        tr.cnt["patch_strand"] += 1
        return 0, 0
    if a["qb"] >= b["qb"] or a["qe"] >= b["qe"] or a["re"] >= b["re"]:
        tr.cnt["patch_order"] += 1
        return 0, 0
    w = abs((a["re"] - b["rb"]) - (a["qe"] - b["qb"]))
    r = abs(float(a["re"] - b["rb"]) / (b["re"] - a["rb"]) - float(a["qe"] - b["qb"]) / (b["qe"] - a["qb"]))
    near = a["re"] < b["rb"] or a["qe"] < b["qb"]
    if w > (W << 1 if near else W << 2):
        tr.cnt["patch_w"] += 1
        return 0, 0
    if r >= (0.05 if near else 0.10):
        tr.cnt["patch_r"] += 1
        return 0, 0
    w = min(w + a["w"] + b["w"], W << 2)
    qb, qe, rb, re = a["qb"], b["qe"], a["rb"], b["re"]
    tr.cnt["patch_tried"] += 1
    if qe - qb > 32767 or re - rb > 32767:
        raise ValueError("patch span above BSW_MAX_LEN")
    if qe - qb <= 0 or rb >= re or (l_pac > 0 and rb < l_pac and re > l_pac):
        score = 0
    else:
        score, _, _, _, nodp = rp.gen_cigar2(T, l_pac, read[qb:qe], rb, re, w, mat, gaps, dp)
        tr.cnt["patch_gapfree" if nodp else "patch_dp"] += 1
        tr.dp_here = not nodp
    s = b["score"] + a["score"]
    q_s = tr.trunc(float(b["qe"] - a["qb"]) / ((b["qe"] - b["qb"]) + (a["qe"] - a["qb"])) * s + .499)
    r_s = tr.trunc(float(b["re"] - a["rb"]) / ((b["re"] - b["rb"]) + (a["re"] - a["rb"])) * s + .499)
    m = max(q_s, r_s)
    ratio = float(score) / m if m != 0 else (math.nan if score == 0 else math.copysign(math.inf, score))
    if ratio < 0.90:
        tr.cnt["patch_ratio"] += 1
        return 0, 0
    return score, w


def sort_dedup_patch(o, T, read, a, mat, gaps, tr, dp):
    """list of region dicts -> the kept ones; also the number of DP rounds the read needed"""
    n = len(a)
    if n <= 1:
        return a, 0
    gap, mlr = o["max_chain_gap"], _f32(o["mask_level_redun"])
    introsort(a, lambda x, y: x["re"] < y["re"])
    n_dp = 0
    for i in range(1, n):
        p = a[i]
        if p["rb"] >= a[i - 1]["re"] + gap:
            continue
        j = i - 1
        while j >= 0 and p["rb"] < a[j]["re"] + gap:
            q = a[j]
            j -= 1
            if q["qe"] == q["qb"]:
                continue
            orr = q["re"] - p["rb"]
            oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
            mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
            mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
            if _f32(orr) > mlr * _f32(mr) and _f32(oq) > mlr * _f32(mq):
                if p["score"] < q["score"]:
                    tr.cnt["drop_p"] += 1
                    p["qe"] = p["qb"]
                    break
                tr.cnt["drop_q"] += 1
                q["qe"] = q["qb"]
            elif q["rb"] < p["rb"]:
                tr.dp_here = False
                score, w = patch_reg(o, T, read, q, p, mat, gaps, tr, dp)
                n_dp += tr.dp_here
                if score > 0:
                    tr.cnt["patch_ok"] += 1
                    p["n_comp"] += q["n_comp"] + 1
                    for f in ("seedcov", "sub", "csub"):
                        p[f] = max(p[f], q[f])
                    p["qb"], p["rb"] = q["qb"], q["rb"]
                    p["truesc"] = p["score"] = score
                    p["w"] = w
                    q["qb"] = q["qe"]
    a = [x for x in a if x["qe"] > x["qb"]]
    introsort(a, lambda x, y: (x["score"], -x["rb"], -x["qb"]) > (y["score"], -y["rb"], -y["qb"]))
    for i in range(1, len(a)):
        if all(a[i][f] == a[i - 1][f] for f in ("score", "rb", "qb")):
            a[i]["qe"] = a[i]["qb"]
            tr.cnt["identical"] += 1
    a = a[:1] + [x for x in a[1:] if x["qe"] > x["qb"]]
    return a, n_dp


def mark_primary(o, a, r, scoring_a, gaps, tr):
    for i, x in enumerate(a):
        x["sub"], x["secondary"], x["hash"] = 0, -1, hash_64(o["id0"] + r + i)
    introsort(a, lambda x, y: (x["score"], -x["hash"]) > (y["score"], -y["hash"]))
    o_del, e_del, o_ins, e_ins = gaps
    tmp = max(scoring_a + o["b"], o_del + e_del, o_ins + e_ins)
    ml = _f32(o["mask_level"])
    z = [0]
    for i in range(1, len(a)):
        for j in z:
            b_max, e_min = max(a[j]["qb"], a[i]["qb"]), min(a[j]["qe"], a[i]["qe"])
            if e_min > b_max:
                min_l = min(a[i]["qe"] - a[i]["qb"], a[j]["qe"] - a[j]["qb"])
                if _f32(e_min - b_max) >= _f32(min_l) * ml:
                    if a[j]["sub"] == 0:
                        a[j]["sub"] = a[i]["score"]
                    if a[j]["score"] - a[i]["score"] <= tmp:
                        a[j]["sub_n"] += 1
                        tr.cnt["sub_n"] += 1
                    a[i]["secondary"] = j
                    tr.cnt["secondary"] += 1
                    break
        else:
            z.append(i)
    return a


def approx_mapq(o, x, scoring_a, frac_rep, tr):
    if x["secondary"] >= 0:
        tr.cnt["mapq_secondary"] += 1
        return 0
    score, a, b = x["score"], scoring_a, o["b"]
    sub = x["sub"] if x["sub"] else o["min_seed_len"] * a
    sub = max(sub, x["csub"])
    if sub >= score:
        tr.cnt["mapq_sub_ge"] += 1
        return 0
    l = max(x["qe"] - x["qb"], x["re"] - x["rb"])
    identity = 1. - float(l * a - score) / (a + b) / l
    if score == 0:
        mapq = 0
    elif o["mapQ_coef_len"] > 0:
        tr.cnt["mapq_coef"] += 1
        t = 1. if l < o["mapQ_coef_len"] else o["mapQ_coef_fac"] / math.log(l)
        t *= identity * identity
        mapq = tr.trunc(6.02 * (score - sub) / a * t * t + .499)
    else:
        tr.cnt["mapq_seedcov"] += 1
        lg = math.log(x["seedcov"]) if x["seedcov"] > 0 else -math.inf
        mapq = tr.trunc(30.0 * (1. - float(sub) / score) * lg + .499)
        if identity < 0.95:
            tr.cnt["mapq_lowid"] += 1
            mapq = tr.trunc(mapq * identity * identity + .499)
    if x["sub_n"] > 0:
        tr.cnt["mapq_subn"] += 1
        mapq -= tr.trunc(4.343 * math.log(x["sub_n"] + 1) + .499)
    mapq = max(min(mapq, 60), 0)
    if frac_rep != 0:
        tr.cnt["mapq_frac_rep"] += 1
    return tr.trunc(mapq * (1. - float(np.float32(frac_rep))) + .499)


def gather(read_len, seeds, seed_chain, regs, extended, b, e, scoring_a, T_len, csub):
    """av of the read whose seed slots are [b, e), in upstream's order"""
    av = []
    c0 = b
    while c0 < e:
        c1 = c0
        while c1 < e and seed_chain[c1] == seed_chain[c0]:
            c1 += 1
        mine = [k for k in range(c0, c1) if extended[k] and regs[k]["qe"] != regs[k]["qb"]]
        mine.sort(key=lambda k: (-int(seeds[k]["len"]) * scoring_a, -k))
        for k in mine:
            x = {f: int(regs[k][f]) for f in ALNREG_FIELDS}
            if x["qb"] < 0 or x["qe"] > read_len or x["qe"] < x["qb"] or x["rb"] < 0 or x["rb"] > x["re"] or \
                    x["re"] > T_len:
                raise ValueError("region outside its read or the text")
            cov = 0
            for t in range(c0, c1):
                qbeg, rbeg, ln = int(seeds[t]["qbeg"]), int(seeds[t]["rbeg"]), int(seeds[t]["len"])
                if qbeg >= x["qb"] and qbeg + ln <= x["qe"] and rbeg >= x["rb"] and rbeg + ln <= x["re"]:
                    cov += ln
            x.update(seedcov=cov, sub=0, sub_n=0, n_comp=1, secondary=-1, src=k, csub=int(csub[k]) if csub is not None else 0)
            av.append(x)
        c0 = c1
    return av


def regs_select(T, reads, read_off, read_len, seeds, seed_read, seed_chain, regs, extended, mat, gaps, opt=None,
                csub=None, frac_rep=None, dp=rp._oracle_dp):
    """The library's call: -> (sel_regs [(field, ...)] as a structured array with ALNREG_FIELDS,
    sel_read, sel_info SELINFO_DTYPE, read_first, Trace).  Raises ValueError where the library
    returns BSW_E_RANGE."""
    o = opt if opt is not None else sel_opt()
    mat = [int(v) for v in mat]
    a_sc = mat[0]
    tr = Trace()
    n_reads, n = len(read_len), len(seeds)
    sr = np.asarray(seed_read)
    if n and (sr.min() < 0 or sr.max() >= n_reads or np.any(np.diff(sr) < 0)):
        raise ValueError("seed_read unsorted or outside the reads")
    out, first = [], [0]
    k = 0
    for r in range(n_reads):
        b = k
        while k < n and sr[k] == r:
            k += 1
        read = reads[int(read_off[r]):int(read_off[r]) + int(read_len[r])]
        av = gather(int(read_len[r]), seeds, seed_chain, regs, extended, b, k, a_sc, len(T), csub)
        tr.cnt["regs_in"] += len(av)
        if len(av) <= 1:
            tr.cnt["fast_path"] += 1
        av, n_dp = sort_dedup_patch(o, T, read, av, mat, gaps, tr, dp)
        tr.rounds = max(tr.rounds, n_dp)
        av = mark_primary(o, av, r, a_sc, gaps, tr) if av else av
        fr = float(frac_rep[r]) if frac_rep is not None else 0.0
        for x in av:
            x["mapq"] = approx_mapq(o, x, a_sc, fr, tr)
            x["frac_rep"] = fr
            x["read"] = r
        out += av
        first.append(len(out))
    sel_regs = np.zeros(len(out), dtype=[(f, np.int64 if f in ("rb", "re") else np.int32) for f in ALNREG_FIELDS])
    info = np.zeros(len(out), dtype=SELINFO_DTYPE)
    for i, x in enumerate(out):
        for f in ALNREG_FIELDS:
            sel_regs[i][f] = x[f]
        for f in SELINFO_DTYPE.names:
            info[i][f] = x[f]
    return sel_regs, np.array([x["read"] for x in out], dtype=np.int32), info, np.array(first, dtype=np.int32), tr


def stats_of(tr):
    """the counters bsw_sel_last_stats reports, from a Trace"""
    c = tr.cnt
    return dict(n_regs_in=c["regs_in"], n_redundant=c["drop_p"] + c["drop_q"], n_identical=c["identical"],
                n_patch_tried=c["patch_tried"], n_patch_ok=c["patch_ok"], n_patch_ratio=c["patch_ratio"],
                n_dp=c["patch_dp"], rounds=tr.rounds)
