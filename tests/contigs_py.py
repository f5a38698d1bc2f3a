"""Pure-Python restatement of the contig table (include/bsw_contigs.h) and of the functions whose upstream
text reads a rid, for the stages that read the table -- TEST INFRASTRUCTURE (tests/test_contigs.py).
Everything that reads no rid is imported from the existing restatements (pe_py, matesw_py, reg2aln_py, rec_py): the
contig-aware versions below call them and restate only the rid rule on top.

  Table            the prefix sums, seg / rid / crosses as csrc/bsw_contig_seg.h states them
  pe_stat / pe_pair
                   mem_pestat, mem_pair and no_pairing's proper flag: hits on different contigs are no pair
  window / mate_rescue
                   mem_matesw's window: clipped to its midpoint's segment, no job under another rid
  reg2aln_one / reg2aln
                   bwa_gen_cigar2's reject: a region with seg(rb) != seg(re - 1) is REJECTED
  records          mem_aln2sam's TLEN: 0 unless the record's and the mate's rid are equal; a needed
                   region that bridges a join fails the call
  sam_text         RNAME / POS / RNEXT / PNEXT and the SA:Z / XA:Z entries by contig

Every rid branch has a counter in the trace dict the restatements carry (res.tr.cnt); BRANCHES lists them."""

import bisect
import math

import numpy as np

import memchain_py as mc
import pe_py as pp
import rec_py as rq
import reg2aln_py as rp
import regsel_py as sp

MAX_NAME = 63

# rid branches: the hand set of test_contigs.py reaches all of them
BRANCHES = ("rej_join", "rej_strand", "same_seg", "tlen_same_rid", "tlen_cross_rid", "rnext_eq", "rnext_name",
            "sa_same_rname", "sa_other_rname", "xa_same_rname", "xa_other_rname", "pos_one", "pos_last",
            "stat_same_rid", "stat_cross_rid", "pair_same_rid", "pair_rid_break", "nopair_cross_rid", "nopair_same_rid",
            "msw_clip", "msw_whole", "msw_other_rid", "msw_same_rid",
            "seed_join", "seed_strand", "seed_kept", "merge_other_rid", "merge_same_rid",
            "dedup_other_rid", "dedup_same_rid")


class Table:
    """n contigs: lens[i] > 0 bases, names[i] 1..63 bytes.  two_strand: the text is forward + reverse
    complement of l_pac = sum(lens) bases; otherwise one strand of that many"""

    def __init__(self, lens, names, two_strand=True):
        lens = [int(v) for v in lens]
        names = [s.encode() if isinstance(s, str) else bytes(s) for s in names]
        if len(lens) != len(names) or any(v <= 0 for v in lens) or any(not 1 <= len(s) <= MAX_NAME for s in names):
            raise ValueError("BSW_E_INVAL: contig table")
        self.lens, self.names, self.n = lens, names, len(lens)
        self.off = [0]
        for v in lens:
            self.off.append(self.off[-1] + v)
        self.sum = self.off[-1]
        self.l_pac = self.sum if two_strand else 0

    def contig_of(self, y):
        """the largest k with off[k] <= y, clamped to [0, n)"""
        return min(max(bisect.bisect_right(self.off, y) - 1, 0), self.n - 1)

    def seg(self, x):
        if self.l_pac > 0 and x >= self.l_pac:
            return 2 * self.n - 1 - self.contig_of(2 * self.l_pac - 1 - x)
        return self.contig_of(x)

    def rid(self, x):
        s = self.seg(x)
        return s if s < self.n else 2 * self.n - 1 - s

    def crosses(self, b, e):
        return self.seg(b) != self.seg(e - 1)

    def bounds(self):
        """the sorted boundaries of the text: seg(x) is the interval of these that holds x"""
        if self.l_pac == 0:
            return list(self.off)
        return self.off + [2 * self.l_pac - o for o in self.off[-2::-1]]

    def check(self, l_pac, ref_len):
        """a stage call's l_pac against the table (BSW_E_INVAL)"""
        if self.sum != (l_pac if l_pac > 0 else ref_len):
            raise ValueError("BSW_E_INVAL: l_pac is not the sum of the contig lengths")


# ---------------------------------------------------------------- bwa_gen_cigar2's reject
def _valid(reg):
    return not (reg["rb"] < 0 or reg["re"] < 0 or reg["qe"] - reg["qb"] <= 0 or reg["rb"] >= reg["re"])


def reg2aln_one(tab, T, read, reg, mat, gaps, W, cigar_stride, md_stride, tr=None, **kw):
    """reg2aln_py.reg2aln_one with the table's reject in place of the l_pac one"""
    if _valid(reg) and tab.crosses(int(reg["rb"]), int(reg["re"])):
        if tr is not None:
            strand = tab.l_pac > 0 and reg["rb"] < tab.l_pac < reg["re"]
            tr.cnt["rej_strand" if strand else "rej_join"] += 1
        return (dict(pos=-1, is_rev=0, n_cigar=0, NM=-1, score=0, w=0, n_pass=1, md_len=0, flags=rp.REJECTED),
                [], b"", {"rejected"})
    if tr is not None and _valid(reg):
        tr.cnt["same_seg"] += 1
    return rp.reg2aln_one(T, tab.l_pac, read, reg, mat, gaps, W, cigar_stride, md_stride, **kw)


def reg2aln(tab, T, reads, read_off, read_len, regs, reg_read, mat, gaps, W, cigar_stride=16, md_stride=64, tr=None):
    """the batch form: regions that bridge a join are handed to reg2aln_py as invalid ones (rb = -1), whose
    row is the rejected row"""
    regs = np.array(regs, dtype=regs.dtype)
    for k in range(len(regs)):
        if _valid(regs[k]) and tab.crosses(int(regs[k]["rb"]), int(regs[k]["re"])):
            if tr is not None:
                strand = tab.l_pac > 0 and regs[k]["rb"] < tab.l_pac < regs[k]["re"]
                tr.cnt["rej_strand" if strand else "rej_join"] += 1
            regs[k]["rb"] = -1
        elif tr is not None and _valid(regs[k]):
            tr.cnt["same_seg"] += 1
    return rp.reg2aln(T, tab.l_pac, reads, read_off, read_len, regs, reg_read, mat, gaps, W, cigar_stride, md_stride)


# ---------------------------------------------------------------- mem_chain
def _test_and_merge(tab, opt, l_pac, c, p, tr):
    """memchain_py._test_and_merge with upstream's first test: a seed of another contig than the chain's (that of
    its first seed) asks for a new chain"""
    if tab.rid(p[0]) != tab.rid(c["seeds"][0][0]):
        tr.cnt["merge_other_rid"] += 1
        return False
    tr.cnt["merge_same_rid"] += 1
    last = c["seeds"][-1]
    first = c["seeds"][0]
    qend, rend = last[1] + last[2], last[0] + last[2]
    if p[1] >= first[1] and p[1] + p[2] <= qend and p[0] >= first[0] and p[0] + p[2] <= rend:
        return True
    if (last[0] < l_pac or first[0] < l_pac) and p[0] >= l_pac:
        return False
    x, y = p[1] - last[1], p[0] - last[0]
    if y >= 0 and x - y <= opt["w"] and y - x <= opt["w"] and x - last[2] < opt["max_chain_gap"] and \
            y - last[2] < opt["max_chain_gap"]:
        c["seeds"].append(p)
        return True
    return False


def mem_chain_read(tab, opt, sa, l_pac, read_len, mems, tr):
    """memchain_py.mem_chain_read under the table: a seed that bridges a join is dropped (bns_intv2rid < 0), and
    _test_and_merge is the one above; mem_chain_flt behind it reads no rid"""
    chains = []
    if read_len < opt["min_seed_len"]:
        return []
    for (k0, _l, s, info) in mems:
        slen = (info & 0xffffffff) - (info >> 32)
        step = s // opt["max_occ"] if s > opt["max_occ"] else 1
        k = count = 0
        while k < s and count < opt["max_occ"]:
            p = (int(sa[k0 + k]), info >> 32, slen)
            k += step
            count += 1
            if tab.crosses(p[0], p[0] + p[2]):
                tr.cnt["seed_strand" if p[0] < l_pac < p[0] + p[2] else "seed_join"] += 1
                continue
            tr.cnt["seed_kept"] += 1
            starts = [c["pos"] for c in chains]
            lo = next((i for i, x in enumerate(starts) if x >= p[0]), len(chains))
            eq = lo < len(chains) and starts[lo] == p[0]
            lower = lo if eq else lo - 1
            if lower >= 0 and _test_and_merge(tab, opt, l_pac, chains[lower], p, tr):
                continue
            chains.insert(lo + 1 if eq else lo, {"pos": p[0], "seeds": [p]})
    # mem_chain_flt
    a = []
    for c in chains:
        c["w"], c["kept"], c["first"] = mc._weight(c), 0, -1
        if c["w"] >= opt["min_chain_weight"]:
            a.append(c)
    if not a:
        return []
    mc.introsort(a, lambda x, y: x["w"] > y["w"])
    beg = lambda c: c["seeds"][0][1]                           # noqa: E731
    end = lambda c: c["seeds"][-1][1] + c["seeds"][-1][2]      # noqa: E731
    ml, dr = mc._f32(opt["mask_level"]), mc._f32(opt["drop_ratio"])   # C: int * float is a float product
    a[0]["kept"] = 3
    kept = [0]
    for i in range(1, len(a)):
        large = False
        broke = False
        for j in kept:
            b_max, e_min = max(beg(a[j]), beg(a[i])), min(end(a[j]), end(a[i]))
            if e_min > b_max:
                min_l = min(end(a[i]) - beg(a[i]), end(a[j]) - beg(a[j]))
                if mc._f32(e_min - b_max) >= mc._f32(min_l) * ml and min_l < opt["max_chain_gap"]:
                    large = True
                    if a[j]["first"] < 0:
                        a[j]["first"] = i
                    if mc._f32(a[i]["w"]) < mc._f32(a[j]["w"]) * dr and a[j]["w"] - a[i]["w"] >= opt["min_seed_len"] << 1:
                        broke = True
                        break
        if not broke:
            kept.append(i)
            a[i]["kept"] = 2 if large else 3
    for j in kept:
        if a[j]["first"] >= 0:
            a[a[j]["first"]]["kept"] = 1
    k = 0
    i = 0
    while i < len(a):
        if a[i]["kept"] not in (0, 3):
            k += 1
            if k >= opt["max_chain_extend"]:
                break
        i += 1
    for i2 in range(i, len(a)):
        if a[i2]["kept"] < 3:
            a[i2]["kept"] = 0
    return [c["seeds"] for c in a if c["kept"] != 0]


# ---------------------------------------------------------------- mem_chain2aln's window, by decomposition
def chain2aln(tab, oracle, params, opt, T, reads, off, lens, seeds, sr, sc, tr=None):
    """The chain-to-alignment oracle is C (oracle/ext_ref.c) and knows one sequence.  Under the table it is used by
    decomposition: for every segment of the text, oracle.chain2aln on the slice T[b0:b1] as a ONE-STRAND
    reference, with the chains whose first seed lies in that segment, their rbeg shifted by -b0; the regions are
    shifted back.  This is exact: (1) the slice's clip to [0, ref_len) is the clip to the segment (bns_fetch_seq
    with mid = the first seed); (2) a chain's seeds all lie in its first seed's segment (test_and_merge: one rid,
    one strand), so every region of the chain is confined to that segment; (3) chains interact only through the
    containment test of a seed against EARLIER regions of the read, which can fire only for a seed inside such a
    region's [rb, re) -- never across segments -- and within a segment the chains keep their order, their seeds
    their relative indices (the tie rule of the seed order).  -> (regs, extended) in the seeds' slots"""
    n = len(seeds)
    regs, ext = None, np.zeros(n, np.int32)
    b = tab.bounds()
    first = {}
    for k in range(n):                                       # a chain's segment = its first live seed's
        key = (int(sr[k]), int(sc[k]))
        if key not in first and seeds[k]["len"] > 0:
            first[key] = tab.seg(int(seeds[k]["rbeg"]))
    seg_of = np.array([first.get((int(sr[k]), int(sc[k])), -1) for k in range(n)])
    o1 = type(opt)()
    for f, _ in opt._fields_:
        setattr(o1, f, getattr(opt, f))
    o1.l_pac = 0
    for s in range(len(b) - 1):
        idx = np.flatnonzero(seg_of == s)
        if len(idx) == 0:
            continue
        sub = seeds[idx].copy()
        sub["rbeg"] -= b[s]
        r, e = oracle.chain2aln(params, o1, np.ascontiguousarray(T[b[s]:b[s + 1]]), reads, off, lens, sub, sr[idx], sc[idx])
        live = e != 0
        r = r.copy()
        r["rb"][live] += b[s]
        r["re"][live] += b[s]
        if regs is None:
            regs = np.zeros(n, dtype=r.dtype)
        regs[idx] = r
        ext[idx] = e
        if tr is not None:
            tr.cnt["win_segments"] += 1
    if regs is None:
        regs, _ = oracle.chain2aln(params, o1, np.zeros(1, np.uint8), reads, off, lens, seeds[:0], sr[:0], sc[:0])
        regs = np.zeros(n, dtype=regs.dtype)
    return regs, ext


def mem_chain(tab, opt, sa, read_len, mems, cnt, seed_dtype, tr):
    """every read through mem_chain_read -> (seeds, seed_read, seed_chain) in the layout of bsw_mem_chain_device"""
    rows, sr, sc = [], [], []
    for r in range(len(read_len)):
        ms = [(int(m["k"]), int(m["l"]), int(m["s"]), int(m["info"])) for m in mems[r, :cnt[r]]]
        for c, chain in enumerate(mem_chain_read(tab, opt, sa, tab.l_pac, int(read_len[r]), ms, tr)):
            for (rb, qb, ln) in chain:
                rows.append((rb, qb, ln))
                sr.append(r)
                sc.append(c)
    seeds = np.zeros(len(rows), dtype=seed_dtype)
    for k, (rb, qb, ln) in enumerate(rows):
        seeds[k] = (rb, qb, ln)
    return seeds, np.array(sr, np.int32), np.array(sc, np.int32)


def regs_select(tab, *args, **kw):
    """regsel_py.regs_select with the sort_dedup_patch below in place of its own"""
    plain = sp.sort_dedup_patch
    sp.sort_dedup_patch = lambda o, T, read, a, mat, gaps, tr, dp: sort_dedup_patch(tab, o, T, read, a, mat, gaps, tr, dp)
    try:
        return sp.regs_select(*args, **kw)
    finally:
        sp.sort_dedup_patch = plain


# ---------------------------------------------------------------- mem_sort_dedup_patch
def sort_dedup_patch(tab, o, T, read, a, mat, gaps, tr, dp):
    """regsel_py.sort_dedup_patch with upstream's rid tests: the outer skip also moves on when p and a[i - 1] lie on
    different contigs, the inner loop runs only while p and a[j] lie on one -- so the patch never sees two"""
    n = len(a)
    if n <= 1:
        return a, 0
    gap, mlr = o["max_chain_gap"], sp._f32(o["mask_level_redun"])
    sp.introsort(a, lambda x, y: x["re"] < y["re"])
    n_dp = 0
    for i in range(1, n):
        p = a[i]
        if tab.rid(p["rb"]) != tab.rid(a[i - 1]["rb"]):
            tr.cnt["dedup_other_rid"] += 1
            continue
        if p["rb"] >= a[i - 1]["re"] + gap:
            continue
        j = i - 1
        while j >= 0 and p["rb"] < a[j]["re"] + gap:
            if tab.rid(p["rb"]) != tab.rid(a[j]["rb"]):
                tr.cnt["dedup_other_rid"] += 1
                break
            tr.cnt["dedup_same_rid"] += 1
            q = a[j]
            j -= 1
            if q["qe"] == q["qb"]:
                continue
            orr = q["re"] - p["rb"]
            oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
            mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
            mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
            if sp._f32(orr) > mlr * sp._f32(mr) and sp._f32(oq) > mlr * sp._f32(mq):
                if p["score"] < q["score"]:
                    tr.cnt["drop_p"] += 1
                    p["qe"] = p["qb"]
                    break
                tr.cnt["drop_q"] += 1
                q["qe"] = q["qb"]
            elif q["rb"] < p["rb"]:
                tr.dp_here = False
                score, w = sp.patch_reg(o, T, read, q, p, mat, gaps, tr, dp)
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
    sp.introsort(a, lambda x, y: (x["score"], -x["rb"], -x["qb"]) > (y["score"], -y["rb"], -y["qb"]))
    for i in range(1, len(a)):
        if all(a[i][f] == a[i - 1][f] for f in ("score", "rb", "qb")):
            a[i]["qe"] = a[i]["qb"]
            tr.cnt["identical"] += 1
    a = a[:1] + [x for x in a[1:] if x["qe"] > x["qb"]]
    return a, n_dp


# ---------------------------------------------------------------- mem_pestat, mem_pair, the proper flag
# Written as upstream writes them, on (rid, position - offset): mem_pestat tests the rids of the two top regions
# behind the cal_sub tests; mem_pair sorts v by rid << 32 | (forward position - offset) and its scan over
# earlier entries ends at a rid change; no_pairing's proper flag needs equal rids.  (The kernels do it another
# way -- they move contigs 2^40 apart on the global coordinate -- so the two are independent statements.)
def pe_stat(tab, sel_regs, sel_info, read_first, opt, scoring_a):
    """bsw_pe_stat under the table: -> (pes, Trace, isize[4]); pe_py.pe_stat's loop with the rid test"""
    o = opt
    tab.check(o["l_pac"], 2 * o["l_pac"])
    tr = sp.Trace()
    pp.check_opt(o, len(read_first) - 1)
    L = pp.lists_of(o, sel_regs, sel_info, read_first)
    isize = [[], [], [], []]
    for p in range(len(L) // 2):
        a0, a1 = L[2 * p], L[2 * p + 1]
        if not a0 or not a1:
            tr.cnt["stat_empty"] += 1
            continue
        if any(pp.cal_sub(o, a, scoring_a) > 0.8 * a[0]["score"] for a in (a0, a1)):
            tr.cnt["stat_sub_skip"] += 1
            continue
        if tab.rid(a0[0]["rb"]) != tab.rid(a1[0]["rb"]):
            tr.cnt["stat_cross_rid"] += 1
            continue
        tr.cnt["stat_same_rid"] += 1
        d, dist = pp.infer_dir(o["l_pac"], a0[0]["rb"], a1[0]["rb"])
        if dist == 0:
            tr.cnt["stat_is_zero"] += 1
        elif dist > o["max_ins"]:
            tr.cnt["stat_far"] += 1
        else:
            tr.cnt["stat_kept"] += 1
            isize[d].append(dist)
    return pp.pestat_of_dirs(isize, tr), tr, isize


def mem_pair(tab, o, pes, a0, a1, p, scoring_a, gaps, tr):
    """pe_py.mem_pair on upstream's key: v entries are ((rid, relative forward position), y); the scan over
    earlier entries ends at the first one of another rid"""
    l_pac = o["l_pac"]
    v = []
    for r, a in enumerate((a0, a1)):
        for i, x in enumerate(a):
            st = 1 if x["rb"] >= l_pac else 0
            f = x["rb"] if not st else 2 * l_pac - 1 - x["rb"]
            k = tab.contig_of(f)
            v.append(((k, f - tab.off[k]), (x["score"] & 0xffffffff) << 32 | i << 2 | st << 1 | r))
    v.sort()
    id32 = ((o["id0"] >> 1) + p) & 0xffffffff
    t = (id32 << 8) & 0xffffffff
    t = t - (1 << 32) if t & 0x80000000 else t
    u = []
    last = [-1] * 4
    for i, ((ri, xi), yi) in enumerate(v):
        for r in (0, 1):
            d = pes[r << 1 | (yi >> 1 & 1)]
            which = r << 1 | ((yi & 1) ^ 1)
            if d["failed"] or last[which] < 0:
                continue
            for k in range(last[which], -1, -1):
                (rk, xk), yk = v[k]
                if (yk & 3) != which:
                    continue
                if rk != ri:
                    tr.cnt["pair_rid_break"] += 1
                    break
                dist = xi - xk
                if dist > d["high"]:
                    break
                if dist < d["low"]:
                    continue
                tr.cnt["pair_same_rid"] += 1
                ns = (dist - float(d["avg"])) / float(d["std"])
                e = 2. * math.erfc(abs(ns) * pp.M_SQRT1_2)
                lg = math.log(e) if e > 0 else -math.inf
                q = max(tr.trunc(float((yi >> 32) + (yk >> 32)) + .721 * lg * scoring_a + .499), 0)
                uy = k << 32 | i
                u.append((q << 32 | (sp.hash_64(uy ^ (t & pp.M64)) & 0xffffffff), uy))
        last[yi & 3] = i
    if not u:
        return 0, 0, 0, 0, None
    u.sort()
    k, i = u[-1][1] >> 32, u[-1][1] & 0xffffffff
    z = [0, 0]
    z[v[k][1] & 1] = (v[k][1] & 0xffffffff) >> 2
    z[v[i][1] & 1] = (v[i][1] & 0xffffffff) >> 2
    best = u[-1][0] >> 32
    sub = u[-2][0] >> 32 if len(u) > 1 else 0
    o_del, e_del, o_ins, e_ins = gaps
    tmp = max(scoring_a + o["b"], o_del + e_del, o_ins + e_ins)
    return len(u), best, sub, sum(1 for x, _ in u[:-1] if sub - (x >> 32) <= tmp), z


def pe_pair(tab, pes, sel_regs, sel_info, read_first, opt, mat, gaps):
    """bsw_pe_pair under the table: -> (sel_regs, sel_info, pairs, Trace).  pe_py.pe_pair's decision block reads
    no rid but in two places: its mem_pair (the one above runs in its place) and no_pairing's proper flag, which
    is taken back where the two tops -- the first regions of the lists as the call leaves them -- differ in rid"""
    tab.check(opt["l_pac"], 2 * opt["l_pac"])
    plain = pp.mem_pair
    pp.mem_pair = lambda o, pes_, a0, a1, p, a_sc, gaps_, tr: mem_pair(tab, o, pes_, a0, a1, p, a_sc, gaps_, tr)
    try:
        regs, info, pairs, tr = pp.pe_pair(pes, sel_regs, sel_info, read_first, opt, mat, gaps)
    finally:
        pp.mem_pair = plain
    for p in range(len(pairs)):
        if pairs[p]["paired"] == 0 and pairs[p]["proper"]:
            f0, f1 = int(read_first[2 * p]), int(read_first[2 * p + 1])
            if tab.rid(int(regs[f0]["rb"])) != tab.rid(int(regs[f1]["rb"])):
                tr.cnt["nopair_cross_rid"] += 1
                tr.cnt["proper"] -= 1
                pairs[p]["proper"] = 0
            else:
                tr.cnt["nopair_same_rid"] += 1
    return regs, info, pairs, tr


# ---------------------------------------------------------------- mem_matesw's window
def window(tab, o, d, r, arb, l_ms, tr=None):
    """matesw_py.window under the table: after the clamp to [0, 2 l_pac) the window is clipped to the segment of
    its midpoint (bns_fetch_seq), and a job runs only when that segment's contig is the anchor's and
    min_seed_len bases are left"""
    l_pac = o["l_pac"]
    is_rev, is_larger = (r >> 1) != (r & 1), not r >> 1
    if not is_rev:
        rb = arb + d["low"] if is_larger else arb - d["high"]
        re = (arb + d["high"] if is_larger else arb - d["low"]) + l_ms
    else:
        rb = (arb + d["low"] if is_larger else arb - d["high"]) - l_ms
        re = arb + d["high"] if is_larger else arb - d["low"]
    rb, re = max(rb, 0), min(re, 2 * l_pac)
    if rb >= re:
        return rb, re, False
    b = tab.bounds()
    s = tab.seg((rb + re) >> 1)
    if tr is not None:
        tr.cnt["msw_clip" if rb < b[s] or re > b[s + 1] else "msw_whole"] += 1
    rb, re = max(rb, b[s]), min(re, b[s + 1])
    if (s if s < tab.n else 2 * tab.n - 1 - s) != tab.rid(arb):
        if tr is not None:
            tr.cnt["msw_other_rid"] += 1
        return rb, re, False
    if tr is not None:
        tr.cnt["msw_same_rid"] += 1
    return rb, re, re - rb >= o["min_seed_len"]


def mate_rescue(tab, pes, T, reads, read_off, read_len, sel_regs, sel_info, read_first, opt, mat, gaps, ksw_align2, jobs=None):
    """matesw_py.mate_rescue with the window above in place of its own"""
    import matesw_py as mp
    tab.check(opt["l_pac"], len(T))
    plain = mp.window
    mp.window = lambda o, d, r, arb, l_ms, tr=None: window(tab, o, d, r, arb, l_ms, tr)
    try:
        return mp.mate_rescue(pes, T, reads, read_off, read_len, sel_regs, sel_info, read_first, opt, mat, gaps, ksw_align2,
                              jobs=jobs)
    finally:
        mp.window = plain


# ---------------------------------------------------------------- records
def records(tab, T, reads, off, lens, sel_regs, sel_info, read_first, pairs, opt, mat, gaps, cigar_stride=16,
            md_stride=64):
    """rec_py.records under the table.  Which regions become records, flags, MAPQ, the mate fields and XA read
    no rid; two things do: a needed region that bridges a join is rejected (BSW_E_RANGE), and TLEN is 0 unless
    pos and mpos -- after cross-linking -- lie in one contig"""
    tab.check(opt["l_pac"], len(T))
    res = rq.records(T, reads, off, lens, sel_regs, sel_info, read_first, pairs, opt, mat, gaps, cigar_stride, md_stride)
    for g in res.aln_reg:
        if tab.crosses(int(sel_regs[g]["rb"]), int(sel_regs[g]["re"])):
            raise ValueError("BSW_E_RANGE: a needed region bridges a join")
        res.tr.cnt["same_seg"] += 1
    for p in res.recs:
        if p["aln"] >= 0 and p["m_aln"] >= 0:               # both CIGARs exist: upstream's TLEN branch
            if tab.rid(int(p["pos"])) == tab.rid(int(p["mpos"])):
                res.tr.cnt["tlen_same_rid"] += 1
            else:
                res.tr.cnt["tlen_cross_rid"] += 1
                p["tlen"] = 0
    return res


# ---------------------------------------------------------------- text
def sam_text(tab, res, reads, off, lens, names, quals, opt, paired):
    """rec_py.sam_text under the table: opt["rname"] is not read"""
    soft = bool(opt["flags"] & rq.SOFTCLIP)
    cnt = res.tr.cnt

    def place(pos):
        k = tab.rid(int(pos))
        rel = int(pos) - tab.off[k] + 1
        return k, tab.names[k].decode("latin-1"), rel

    out, offs, total = [], [0], 0
    for i, p in enumerate(res.recs):
        r, which = int(p["read"]), int(p["which"])
        clip = "" if soft else ("H" if which else "S")
        n_cig = int(res.aln[p["aln"]]["n_cigar"]) if p["aln"] >= 0 else 0
        cg = res.cigar[p["aln"], :n_cig] if n_cig else []
        t = [names[r >> 1 if paired else r].decode("latin-1"), str(int(p["sam_flag"]))]
        rid = -1
        if p["pos"] >= 0:
            rid, nm, rel = place(p["pos"])
            if rel == 1:
                cnt["pos_one"] += 1
            if n_cig and rel - 1 + rq._rlen(cg) == tab.lens[rid]:
                cnt["pos_last"] += 1
            t += [nm, str(rel), str(int(p["mapq"])), rq._cigar(cg, clip) if n_cig else "*"]
        else:
            t += ["*", "0", "0", "*"]
        if p["mpos"] >= 0:
            mrid, mnm, mrel = place(p["mpos"])
            cnt["rnext_eq" if mrid == rid else "rnext_name"] += 1
            t += ["=" if mrid == rid else mnm, str(mrel), str(int(p["tlen"]))]
        else:
            t += ["*", "0", "0"]
        l = int(lens[r])
        qb, qe = 0, l
        seq = reads[int(off[r]):int(off[r]) + l]
        ql = None if quals is None else quals[int(off[r]):int(off[r]) + l]
        if n_cig and which and not soft:
            c5 = int(cg[0]) >> 4 if (int(cg[0]) & 15) in (3, 4) else 0
            c3 = int(cg[-1]) >> 4 if (int(cg[-1]) & 15) in (3, 4) else 0
            if p["is_rev"]:
                qe -= c5
                qb += c3
            else:
                qb += c5
                qe -= c3
        if not p["is_rev"]:
            t.append("".join("ACGTN"[int(c)] for c in seq[qb:qe]))
            t.append("*" if ql is None else bytes(ql[qb:qe]).decode("latin-1"))
        else:
            t.append("".join("TGCAN"[int(c)] for c in seq[qb:qe][::-1]))
            t.append("*" if ql is None else bytes(ql[qb:qe][::-1]).decode("latin-1"))
        if n_cig:
            a = res.aln[p["aln"]]
            t.append(f"NM:i:{int(a['NM'])}")
            t.append("MD:Z:" + bytes(res.md[p["aln"], :int(a["md_len"])]).decode())
        if p["m_aln"] >= 0:
            m = res.aln[p["m_aln"]]
            t.append("MC:Z:" + rq._cigar(res.cigar[p["m_aln"], :int(m["n_cigar"])], clip))
        t.append(f"AS:i:{int(p['score'])}")
        if p["sub"] >= 0:
            t.append(f"XS:i:{int(p['sub'])}")
        if not p["flag"] & 0x100:
            f0 = int(res.rec_first[r])
            others = [res.recs[f0 + j] for j in range(int(p["n_list"])) if j != which and not res.recs[f0 + j]["flag"] & 0x100]
            if others:
                s = "SA:Z:"
                for q in others:
                    a = res.aln[q["aln"]]
                    k, nm, rel = place(a["pos"])
                    cnt["sa_same_rname" if k == rid else "sa_other_rname"] += 1
                    s += (f"{nm},{rel},{'+-'[int(a['is_rev'])]},"
                          f"{rq._cigar(res.cigar[q['aln'], :int(a['n_cigar'])], '')},{int(q['mapq'])},{int(a['NM'])};")
                t.append(s)
        if p["xa_n"] > 0:
            s = "XA:Z:"
            for j in range(int(p["xa_first"]), int(p["xa_first"]) + int(p["xa_n"])):
                a = res.aln[j]
                k, nm, rel = place(a["pos"])
                cnt["xa_same_rname" if k == rid else "xa_other_rname"] += 1
                s += f"{nm},{'+-'[int(a['is_rev'])]}{rel},{rq._cigar(res.cigar[j, :int(a['n_cigar'])], '')},{int(a['NM'])};"
            t.append(s)
        line = ("\t".join(t) + "\n").encode("latin-1")
        out.append(line)
        total += len(line)
        offs.append(total)
    return b"".join(out), np.array(offs, dtype=np.int64)
