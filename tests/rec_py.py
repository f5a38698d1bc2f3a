"""Pure-Python restatement of mem_reg2sam, mem_gen_alt, mem_aln2sam and the output block of
mem_sam_pe as include/bsw_rec.h states them -- TEST INFRASTRUCTURE (tests/test_rec.py).  The lists
are pe_py's (regsel_py's fields), the alignments reg2aln_py's (the CPU oracle's ksw_global2
underneath); record selection, the primary switch, XA membership, cross-linking, TLEN and the text
are written out here.  Every call reports the branches taken."""

import numpy as np

import pe_py as pp
import reg2aln_py as rp
import regsel_py as sp

SOFTCLIP, NO_MULTI, KEEP_SUPP_MAPQ = 1, 2, 4

REC_DTYPE = np.dtype([("pos", np.int64), ("mpos", np.int64), ("tlen", np.int64), ("read", np.int32), ("reg", np.int32),
                      ("aln", np.int32), ("which", np.int32), ("n_list", np.int32), ("flag", np.int32),
                      ("sam_flag", np.int32), ("is_rev", np.int32), ("mapq", np.int32), ("score", np.int32),
                      ("sub", np.int32), ("m_is_rev", np.int32), ("m_aln", np.int32), ("xa_first", np.int32),
                      ("xa_n", np.int32), ("reserved", np.int32)])

DEFAULT_OPT = dict(l_pac=0, w=100, T=30, max_XA_hits=5, XA_drop_ratio=0.8, mask_level=0.5, flags=0, rname="ref")

# every data branch the restatement counts (options are inputs, not branches): the pipeline set reaches all
BRANCHES = ("rec_mapped", "rec_unmapped", "rec_fwd", "rec_rev", "rec_supp", "supp_capped", "secondary_skip",
            "paired_branch", "nopair_branch", "recomputed", "switch", "xa_member", "xa_record", "xa_below_ratio",
            "xa_dropped_many", "proper", "improper", "mate_unmapped", "takes_mate_pos", "tlen_pos", "tlen_neg",
            "tlen_zero", "mc", "clipped")


def rec_opt(**kw):
    o = dict(DEFAULT_OPT)
    o.update(kw)
    return o


def check_opt(o, n_reads, paired):
    if n_reads < 0 or (paired and n_reads & 1) or o["l_pac"] <= 0 or o["w"] < 0 or o["max_XA_hits"] < 0:
        raise ValueError("BSW_E_INVAL")
    if not 1 <= len(o["rname"].encode()) <= 63:
        raise ValueError("BSW_E_INVAL: rname")


def _overlaps(o, x, y):
    """PRIMARY MARKING step 4's test (bsw_sel.h)"""
    b_max, e_min = max(x["qb"], y["qb"]), min(x["qe"], y["qe"])
    if e_min <= b_max:
        return False
    min_l = min(x["qe"] - x["qb"], y["qe"] - y["qb"])
    return bool(np.float32(e_min - b_max) >= np.float32(min_l) * np.float32(o["mask_level"]))


def secondary_all(o, a, tr=None):
    """a list's secondary_all: secondary itself, but for a region bsw_pe_pair* marked -2 the first earlier
    region with secondary == -1 that passes the overlap test"""
    out = []
    for i, x in enumerate(a):
        s = x["secondary"]
        if s == -2:
            if tr is not None:
                tr.cnt["recomputed"] += 1
            s = -1
            for j in range(i):
                if a[j]["secondary"] == -1 and _overlaps(o, a[j], x):
                    s = j
                    break
        out.append(s)
    return out


def carried_secondary_all(opt_pe, sel_regs, sel_info, read_first, mat, gaps):
    """what upstream carries: secondary_all = secondary as bsw_pe_pair*'s step 1 (the second primary marking)
    leaves it, before the pair decision overwrites the chosen region's secondary -- for the lists that go
    INTO the pair call; returned in the order the pair call leaves them (the order after that marking)"""
    L = pp.lists_of(opt_pe, sel_regs, sel_info, read_first)
    out = []
    for r, a in enumerate(L):
        a = pp._remark(opt_pe, a, r, int(mat[0]), gaps, sp.Trace())
        out += [x["secondary"] for x in a]
    return out


def plan_read(o, a, pair, e, tr):
    """one read -> (its records as dicts(k, flag, mapq, which, n_list, xa), without alignments yet)"""
    T, fl = o["T"], o["flags"]
    sa = secondary_all(o, a, tr)
    recs = []
    if pair is not None and pair["paired"]:
        tr.cnt["paired_branch"] += 1
        z = int(pair["z"][e])
        if not 0 <= z < len(a):
            raise ValueError("BSW_E_RANGE: z")
        k = sa[z]
        if k >= 0:
            tr.cnt["switch"] += 1
            sa = [z if (s == k or j == k) else s for j, s in enumerate(sa)]
            sa[z] = -1
        recs.append(dict(k=z, flag=(0x40 << e) | 0x1 | (0x2 if pair["proper"] else 0), mapq=int(pair["mapq"][e])))
    else:
        if pair is not None:
            tr.cnt["nopair_branch"] += 1
        extra = 0 if pair is None else ((0x41 if e == 0 else 0x81) | (0x2 if pair["proper"] else 0))
        for k, x in enumerate(a):
            if x["score"] < T:
                continue
            if x["secondary"] >= 0:
                tr.cnt["secondary_skip"] += 1
                continue
            f, mq = extra, x["mapq"]
            if recs:
                f |= 0x10000 if fl & NO_MULTI else 0x800
                if not fl & KEEP_SUPP_MAPQ and mq > recs[0]["mapq"]:
                    tr.cnt["supp_capped"] += 1
                    mq = recs[0]["mapq"]
            recs.append(dict(k=k, flag=f, mapq=mq))
        if not recs:
            recs.append(dict(k=-1, flag=extra | 0x4, mapq=0))
    ratio = float(np.float32(o["XA_drop_ratio"]))

    def pri(i):
        k = sa[i]
        if k >= 0 and a[i]["score"] >= a[k]["score"] * ratio:
            return k
        if k >= 0:
            tr.cnt["xa_below_ratio"] += 1
        return -1
    pris = [pri(i) for i in range(len(a))]
    for l, rec in enumerate(recs):
        rec["which"], rec["n_list"] = l, len(recs)
        mem = [i for i in range(len(a)) if pris[i] == rec["k"]] if rec["k"] >= 0 else []
        if len(mem) > o["max_XA_hits"]:
            tr.cnt["xa_dropped_many"] += 1
            mem = []
        rec["xa"] = mem
    return recs


class Result:
    pass


def _rlen(words):
    return sum(int(w) >> 4 for w in words if (int(w) & 15) in (0, 2))


def records(T, reads, off, lens, sel_regs, sel_info, read_first, pairs, opt, mat, gaps, cigar_stride=16, md_stride=64,
            dp=None):
    """the library's bsw_records: -> Result(recs, rec_first, aln, aln_reg, cigar, md, tr); raises ValueError
    where the library returns BSW_E_INVAL / BSW_E_RANGE"""
    o = opt
    n_reads = len(read_first) - 1
    check_opt(o, n_reads, pairs is not None)
    if cigar_stride < 1 or md_stride < 1:
        raise ValueError("BSW_E_INVAL: strides")
    tr = sp.Trace()
    L = pp.lists_of(dict(l_pac=o["l_pac"]), sel_regs, sel_info, read_first)
    mat = [int(v) for v in mat]
    kw = {} if dp is None else dict(dp=dp)
    recs, rec_first, aln, aln_reg, cig, mds = [], [0], [], [], [], []
    for r, a in enumerate(L):
        pair = None if pairs is None else pairs[r >> 1]
        read = reads[int(off[r]):int(off[r]) + int(lens[r])]
        for rec in plan_read(o, a, pair, r & 1, tr):
            d = dict(read=r, reg=-1, aln=-1, which=rec["which"], n_list=rec["n_list"], flag=rec["flag"], mapq=rec["mapq"],
                     pos=-1, is_rev=0, score=0, sub=0, xa_first=0, xa_n=0)
            need = ([rec["k"]] if rec["k"] >= 0 else []) + rec["xa"]
            for j, k in enumerate(need):
                g = int(read_first[r]) + k
                f, cg, md, _ = rp.reg2aln_one(T, o["l_pac"], read, sel_regs[g], mat, gaps, o["w"], cigar_stride,
                                              md_stride, **kw)
                if f["flags"] & rp.REJECTED:
                    raise ValueError("BSW_E_RANGE: a needed region is rejected")
                if f["flags"] & rp.OVERFLOW:
                    raise ValueError("BSW_E_RANGE: stride overflow")
                if j == 0:
                    x = a[k]
                    d.update(reg=g, aln=len(aln), pos=f["pos"], is_rev=f["is_rev"], score=x["score"],
                             sub=max(x["sub"], x["csub"]), xa_first=len(aln) + 1, xa_n=len(rec["xa"]))
                    tr.cnt["rec_mapped"] += 1
                    tr.cnt["rec_rev" if f["is_rev"] else "rec_fwd"] += 1
                    if rec["which"]:
                        tr.cnt["rec_supp"] += 1
                    if rec["xa"]:
                        tr.cnt["xa_record"] += 1
                    if (cg[0] & 15) == 3 or (cg[-1] & 15) == 3:
                        tr.cnt["clipped"] += 1
                else:
                    tr.cnt["xa_member"] += 1
                aln.append(f)
                aln_reg.append(g)
                cig.append(cg)
                mds.append(md)
            if rec["k"] < 0:
                tr.cnt["rec_unmapped"] += 1
            recs.append(d)
        rec_first.append(len(recs))
    # mem_aln2sam's cross-linking
    for d in recs:
        flag = d["flag"]
        p_map = d["aln"] >= 0
        m = None
        if pairs is not None:
            m = recs[rec_first[d["read"] ^ 1]]              # the other end's first record: list[z], or unmapped
            flag |= 0x1
            tr.cnt["proper" if flag & 0x2 else "improper"] += 1
        if not p_map:
            flag |= 0x4
        pos, is_rev, mpos, m_rev, m_aln = d["pos"], d["is_rev"], -1, 0, -1
        if m is not None:
            m_map = m["aln"] >= 0
            if m_map:
                mpos, m_rev, m_aln = aln[m["aln"]]["pos"], aln[m["aln"]]["is_rev"], m["aln"]
            else:
                flag |= 0x8
                tr.cnt["mate_unmapped"] += 1
            if not p_map and m_map:
                pos, is_rev = mpos, m_rev
                tr.cnt["takes_mate_pos"] += 1
            if not m_map and p_map:
                mpos, m_rev = pos, is_rev
        if is_rev:
            flag |= 0x10
        if m_rev:
            flag |= 0x20
        tlen = 0
        if p_map and m_aln >= 0:
            p0 = pos + (_rlen(cig[d["aln"]]) - 1 if is_rev else 0)
            p1 = mpos + (_rlen(cig[m_aln]) - 1 if m_rev else 0)
            tlen = -(p0 - p1 + (1 if p0 > p1 else -1 if p0 < p1 else 0))
            tr.cnt["tlen_pos" if tlen > 0 else "tlen_neg" if tlen < 0 else "tlen_zero"] += 1
        if m_aln >= 0:
            tr.cnt["mc"] += 1
        d["out"] = dict(pos=pos, is_rev=is_rev, mpos=mpos, m_is_rev=m_rev, m_aln=m_aln, tlen=tlen, flag=flag,
                        sam_flag=(flag & 0xffff) | (0x100 if flag & 0x10000 else 0))
    res = Result()
    res.recs = np.zeros(len(recs), dtype=REC_DTYPE)
    for i, d in enumerate(recs):
        d.update(d.pop("out"))
        for f in REC_DTYPE.names:
            res.recs[i][f] = d.get(f, 0)
    res.rec_first = np.array(rec_first, dtype=np.int32)
    n = len(aln)
    res.aln = np.zeros(n, dtype=rp.ALN_DTYPE)
    res.aln_reg = np.array(aln_reg, dtype=np.int32)
    res.cigar = np.zeros((n, cigar_stride), dtype=np.uint32)
    res.md = np.zeros((n, md_stride), dtype=np.uint8)
    for i in range(n):
        for f, v in aln[i].items():
            res.aln[i][f] = v
        res.cigar[i, :len(cig[i])] = cig[i]
        res.md[i, :len(mds[i])] = np.frombuffer(mds[i], np.uint8)
    res.tr = tr
    return res


def stats_of(res):
    """the counters bsw_rec_last_stats reports after a records call"""
    r = res.recs
    return dict(n_rec=len(r), n_unmapped=int((r["aln"] < 0).sum()), n_supp=int((r["which"] > 0).sum()),
                n_xa=int(r["xa_n"].sum()), n_aln=len(res.aln), n_overflow=0)


# ---------------------------------------------------------------- text
def _cigar(words, clip):
    return "".join(f"{int(w) >> 4}{clip if (int(w) & 15) in (3, 4) and clip else 'MIDSH'[int(w) & 15]}" for w in words)


def sam_text(res, reads, off, lens, names, quals, opt, paired):
    """the library's bsw_sam_text: -> (text bytes, text_off int64 [n_rec + 1]); names: one bytes object per
    read (single-end) or per pair; quals: bytes parallel to reads, or None"""
    o = opt
    rname = o["rname"]
    soft = bool(o["flags"] & SOFTCLIP)
    out, offs = [], [0]
    total = 0
    for i, p in enumerate(res.recs):
        r = int(p["read"])
        which = int(p["which"])
        clip = "" if soft else ("H" if which else "S")
        n_cig = int(res.aln[p["aln"]]["n_cigar"]) if p["aln"] >= 0 else 0
        cg = res.cigar[p["aln"], :n_cig] if n_cig else []
        t = [names[r >> 1 if paired else r].decode("latin-1"), str(int(p["sam_flag"]))]
        if p["pos"] >= 0:
            t += [rname, str(int(p["pos"]) + 1), str(int(p["mapq"])), _cigar(cg, clip) if n_cig else "*"]
        else:
            t += ["*", "0", "0", "*"]
        if p["mpos"] >= 0:
            t += ["=", str(int(p["mpos"]) + 1), str(int(p["tlen"]))]
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
            t.append("MC:Z:" + _cigar(res.cigar[p["m_aln"], :int(m["n_cigar"])], clip))
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
                    s += (f"{rname},{int(a['pos']) + 1},{'+-'[int(a['is_rev'])]},"
                          f"{_cigar(res.cigar[q['aln'], :int(a['n_cigar'])], '')},{int(q['mapq'])},{int(a['NM'])};")
                t.append(s)
        if p["xa_n"] > 0:
            s = "XA:Z:"
            for j in range(int(p["xa_first"]), int(p["xa_first"]) + int(p["xa_n"])):
                a = res.aln[j]
                s += f"{rname},{'+-'[int(a['is_rev'])]}{int(a['pos']) + 1},{_cigar(res.cigar[j, :int(a['n_cigar'])], '')},{int(a['NM'])};"
            t.append(s)
        line = ("\t".join(t) + "\n").encode("latin-1")
        out.append(line)
        total += len(line)
        offs.append(total)
    return b"".join(out), np.array(offs, dtype=np.int64)
