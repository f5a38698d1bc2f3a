"""Pure-Python restatement of mem_matesw and the rescue block of mem_sam_pe as include/bsw_matesw.h
states them -- TEST INFRASTRUCTURE (tests/test_matesw.py).  Built from parts that exist: the dedup is
regsel_py.sort_dedup_patch with patch = 0, infer_dir is pe_py's, ksw_align2 is injected (the
query-order formulation of tests/ksw_align_py.py for hand cases, the C oracle's literal striped one
for bulk).  Every call reports the branches taken; `replan` counts calls whose skip set differs from
what the pair's ORIGINAL lists would give, `anchor_gone` calls whose anchor copy is no longer in its
own list -- the two reasons the jobs cannot be planned up front."""

import numpy as np

import pe_py as pp
import regsel_py as sp

KSW_XBYTE, KSW_XSUBO, KSW_XSTART = 0x10000, 0x40000, 0x80000
MATE_MAX_QLEN, MAX_LEN = 256, 32767

DEFAULT_OPT = dict(l_pac=0, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
                   mask_level_redun=0.95, reserved=0)

BRANCHES = ("cand_below", "cand_cut", "calls", "all_skipped", "dir_failed", "dir_consistent", "jobs", "jobs_u8",
            "jobs_i16", "job_fwd", "job_rev", "short_window", "empty_window", "clamp0", "clamp_end", "cut_left",
            "cut_right", "aln_low", "aln_noqb", "pushed", "push_tie", "push_end", "dedup_run", "dedup_small",
            "drop_p", "drop_q", "identical", "lists_changed", "replan", "anchor_gone", "call_no_job")


def matesw_opt(**kw):
    o = dict(DEFAULT_OPT)
    o.update(kw)
    return o


def check_opt(o, pes, n_reads):
    if n_reads < 0 or n_reads & 1 or o["l_pac"] <= 0 or o["max_matesw"] < 0 or o["min_seed_len"] <= 0:
        raise ValueError("BSW_E_INVAL")
    if any(not d["failed"] and d["low"] > d["high"] for d in pes):
        raise ValueError("BSW_E_INVAL: low > high")


def revcomp(codes):
    return [3 - c if c < 4 else 4 for c in reversed(codes)]


def window(o, d, r, arb, l_ms, tr=None):
    """direction r's window around an anchor at arb -> (rb, re, a job runs)"""
    l_pac = o["l_pac"]
    is_rev, is_larger = (r >> 1) != (r & 1), not r >> 1
    if not is_rev:
        rb = arb + d["low"] if is_larger else arb - d["high"]
        re = (arb + d["high"] if is_larger else arb - d["low"]) + l_ms
    else:
        rb = (arb + d["low"] if is_larger else arb - d["high"]) - l_ms
        re = arb + d["high"] if is_larger else arb - d["low"]
    if tr is not None:
        tr.cnt["clamp0"] += rb < 0
        tr.cnt["clamp_end"] += re > 2 * l_pac
    rb, re = max(rb, 0), min(re, 2 * l_pac)
    if rb < re:
        mid = (rb + re) >> 1
        if mid < l_pac:
            if tr is not None:
                tr.cnt["cut_left"] += re > l_pac
            re = min(re, l_pac)
        else:
            if tr is not None:
                tr.cnt["cut_right"] += rb < l_pac
            rb = max(rb, l_pac)
    return rb, re, rb < re and re - rb >= o["min_seed_len"]


def skip_set(o, pes, arb, ma, tr=None):
    skip = [1 if d["failed"] else 0 for d in pes]
    if tr is not None:
        tr.cnt["dir_failed"] += sum(skip)
    for m in ma:
        r, dist = pp.infer_dir(o["l_pac"], arb, m["rb"])
        if pes[r]["low"] <= dist <= pes[r]["high"]:
            if tr is not None and not skip[r]:
                tr.cnt["dir_consistent"] += 1
            skip[r] = 1
    return skip


def _dedup(o, ma, tr):
    if len(ma) <= 1:
        tr.cnt["dedup_small"] += 1
        return ma
    tr.cnt["dedup_run"] += 1
    so = sp.sel_opt(l_pac=o["l_pac"], max_chain_gap=o["max_chain_gap"], mask_level_redun=o["mask_level_redun"], patch=0)
    return sp.sort_dedup_patch(so, None, None, ma, None, None, tr, None)[0]


def matesw(o, pes, T, anchor, ms, ma, scoring_a, ksw, tr, ma_orig, jobs=None):
    """one call -> (ma, number of jobs)"""
    l_pac, l_ms, msl = o["l_pac"], len(ms), o["min_seed_len"]
    tr.cnt["calls"] += 1
    skip = skip_set(o, pes, anchor["rb"], ma, tr)
    if skip != skip_set(o, pes, anchor["rb"], ma_orig):
        tr.cnt["replan"] += 1
    if all(skip):
        tr.cnt["all_skipped"] += 1
        return ma, 0
    n = 0
    for r in range(4):
        if skip[r]:
            continue
        is_rev = (r >> 1) != (r & 1)
        rb, re, job = window(o, pes[r], r, anchor["rb"], l_ms, tr)
        if job:
            if l_ms > MATE_MAX_QLEN or re - rb > MAX_LEN:
                raise ValueError("BSW_E_RANGE: job size")
            seq = revcomp(ms) if is_rev else list(ms)
            byte = l_ms * scoring_a < 250
            xtra = KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if byte else 0) | (msl * scoring_a)
            if jobs is not None:
                jobs.append((seq, [int(c) for c in T[rb:re]], xtra))
            score, te, qe, score2, te2, tb, qb = ksw(seq, T[rb:re], xtra)
            n += 1
            tr.cnt["jobs"] += 1
            tr.cnt["jobs_u8" if byte else "jobs_i16"] += 1
            tr.cnt["job_rev" if is_rev else "job_fwd"] += 1
            if score < msl:
                tr.cnt["aln_low"] += 1
            elif qb < 0:
                tr.cnt["aln_noqb"] += 1
            else:
                x = {f: 0 for f in sp.ALNREG_FIELDS}
                x.update({f: 0 for f in sp.SELINFO_DTYPE.names})
                x["qb"] = l_ms - (qe + 1) if is_rev else qb
                x["qe"] = l_ms - qb if is_rev else qe + 1
                x["rb"] = 2 * l_pac - (rb + te + 1) if is_rev else rb + tb
                x["re"] = 2 * l_pac - (rb + tb) if is_rev else rb + te + 1
                x.update(score=score, csub=score2, secondary=-1, src=-1, frac_rep=np.float32(0))
                x["seedcov"] = min(x["re"] - x["rb"], x["qe"] - x["qb"]) >> 1
                i = 0
                while i < len(ma) and ma[i]["score"] >= score:
                    i += 1
                tr.cnt["pushed"] += 1
                tr.cnt["push_end"] += i == len(ma)
                tr.cnt["push_tie"] += i > 0 and ma[i - 1]["score"] == score
                ma = ma[:i] + [x] + ma[i:]
        else:
            tr.cnt["short_window" if rb < re else "empty_window"] += 1
        if n > 0:
            ma = _dedup(o, ma, tr)
    if n == 0:
        tr.cnt["call_no_job"] += 1
    return ma, n


def _key(x):
    return tuple(x[f] for f in ("rb", "re", "qb", "qe", "score"))


def mate_rescue(pes, T, reads, read_off, read_len, sel_regs, sel_info, read_first, opt, mat, gaps, ksw_align2,
                tr=None, jobs=None):
    """the library's bsw_matesw: -> (regs, reg_read, info, first, Trace).  ksw_align2(query, target, mat,
    o_del, e_del, o_ins, e_ins, xtra) -> the 7 kswr_t fields.  jobs: a list that receives every job as
    (query, target, xtra).  Raises ValueError where the library returns an error."""
    o = opt
    tr = tr if tr is not None else sp.Trace()
    n_reads = len(read_first) - 1
    pes = [dict(low=int(pes[d]["low"]), high=int(pes[d]["high"]), failed=int(pes[d]["failed"])) for d in range(4)]
    check_opt(o, pes, n_reads)
    if gaps[2] == 0 or max(mat) < 1:
        raise ValueError("BSW_E_INVAL: scoring")
    if len(T) != 2 * o["l_pac"]:
        raise ValueError("BSW_E_INVAL: text")
    a_sc = int(mat[0])
    mat = [int(v) for v in mat]
    ksw = lambda q, t, xtra: ksw_align2(q, t, mat, gaps[0], gaps[1], gaps[2], gaps[3], xtra)   # noqa: E731
    L = pp.lists_of(o, sel_regs, sel_info, read_first)
    changed = set()
    tr.per_pair = []                                         # (jobs, regions pushed) of each pair
    for p in range(n_reads // 2):
        before = (tr.cnt["jobs"], tr.cnt["pushed"])
        orig = [[dict(x) for x in L[2 * p + e]] for e in (0, 1)]
        b = []
        for e in (0, 1):
            a = orig[e]
            c = [x for x in a if x["score"] >= a[0]["score"] - o["pen_unpaired"]]
            tr.cnt["cand_below"] += len(a) - len(c)
            tr.cnt["cand_cut"] += max(len(c) - o["max_matesw"], 0)
            b.append(c[:o["max_matesw"]])
        rounds = 0
        for e in (0, 1):
            mr = 2 * p + 1 - e
            ms = [int(c) for c in reads[int(read_off[mr]):int(read_off[mr]) + int(read_len[mr])]]
            for anchor in b[e]:
                if _key(anchor) not in {_key(x) for x in L[2 * p + e]}:
                    tr.cnt["anchor_gone"] += 1
                L[mr], n = matesw(o, pes, T, anchor, ms, L[mr], a_sc, ksw, tr, orig[1 - e], jobs)
                if n:
                    rounds += 1
                    changed.add(mr)
        tr.rounds = max(tr.rounds, rounds)
        tr.per_pair.append((tr.cnt["jobs"] - before[0], tr.cnt["pushed"] - before[1]))
    tr.cnt["lists_changed"] = len(changed)
    flat = [(r, x) for r, a in enumerate(L) for x in a]
    regs = np.zeros(len(flat), dtype=[(f, np.int64 if f in ("rb", "re") else np.int32) for f in sp.ALNREG_FIELDS])
    info = np.zeros(len(flat), dtype=sp.SELINFO_DTYPE)
    for i, (_, x) in enumerate(flat):
        for f in sp.ALNREG_FIELDS:
            regs[i][f] = x[f]
        for f in sp.SELINFO_DTYPE.names:
            info[i][f] = x[f]
    first = np.cumsum([0] + [len(a) for a in L]).astype(np.int32)
    return regs, np.array([r for r, _ in flat], dtype=np.int32), info, first, tr


def stats_of(tr, n_pairs, n_out):
    """the counters bsw_matesw_last_stats reports, from a Trace"""
    c = tr.cnt
    return dict(n_pairs=n_pairs, n_calls=c["calls"], n_calls_all_skipped=c["all_skipped"], n_jobs=c["jobs"],
                n_jobs_u8=c["jobs_u8"], n_short_window=c["short_window"] + c["empty_window"], n_pushed=c["pushed"],
                n_redundant=c["drop_p"] + c["drop_q"], n_identical=c["identical"], n_lists_changed=c["lists_changed"],
                rounds=tr.rounds, n_out=n_out)
