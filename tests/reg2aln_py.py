"""Pure-Python restatement of mem_reg2aln -> bwa_gen_cigar2 as include/bsw_aln.h states it --
TEST INFRASTRUCTURE (tests/test_reg2aln.py).  The DP is the CPU oracle's ksw_global2
(oracle/ksw_global_ref.c) by default; the band loop, the no-DP shortcut, the strand reversal,
NM / MD, the deletion squeeze, the clips and pos are written out here.  Every region reports
the branches it took, so a test can require that its inputs reach all of them.
"""

import numpy as np

REJECTED, NODP, OVERFLOW = 1, 2, 4
BRANCHES = ("rejected", "gapfree", "dp", "pass2", "pass3", "cap_break", "min_w_reg", "squeeze_lead",
            "squeeze_trail", "clip5", "clip3", "fwd", "rev")

ALN_DTYPE = np.dtype([("pos", np.int64), ("is_rev", np.int32), ("n_cigar", np.int32), ("NM", np.int32),
                      ("score", np.int32), ("w", np.int32), ("n_pass", np.int32), ("md_len", np.int32),
                      ("flags", np.int32)])


def infer_bw(l1, l2, score, a, q, r):
    if l1 == l2 and l1 * a - score < (q + r - a) * 2:
        return 0
    w = int(float(min(l1, l2) * a - score - q) / r + 2.0)
    return max(w, abs(l1 - l2))


def gen_cigar_band(lq, rlen, w_, a, o_del, e_del, o_ins, e_ins):
    """bsw_gen_cigar_band (include/bsw_global.h)"""
    max_ins = int(float(((lq + 1) >> 1) * a - o_ins) / e_ins + 1.0)
    max_del = int(float(((lq + 1) >> 1) * a - o_del) / e_del + 1.0)
    max_gap = max(max_ins, max_del, 1)
    w = min((max_gap + abs(rlen - lq) + 1) >> 1, w_)
    return max(w, abs(rlen - lq) + 3)


def _oracle_dp(q, t, mat, o_del, e_del, o_ins, e_ins, w):
    import oracle
    return oracle.ksw_global2(q, t, mat, o_del, e_del, o_ins, e_ins, w)


def gen_cigar2(T, l_pac, query, rb, re, w_, mat, gaps, dp=_oracle_dp):
    """-> (score, [(op, len)], NM, MD bytes, no_dp); the caller has applied the reject test"""
    a = mat[0]
    rev = l_pac > 0 and rb >= l_pac
    q = [int(c) for c in query]
    t = [int(c) for c in T[rb:re]]
    if rev:
        q.reverse()
        t.reverse()
    lq, rl = len(q), len(t)
    if lq == rl and w_ == 0:
        score, cig, nodp = sum(mat[t[i] * 5 + q[i]] for i in range(lq)), [(0, lq)], True
    else:
        score, cig = dp(q, t, mat, *gaps, gen_cigar_band(lq, rl, w_, a, *gaps))
        nodp = False
    letters = "TGCAN" if rev else "ACGTN"
    md, x, y, u, n_mm, n_gap = [], 0, 0, 0, 0, 0
    for k, (op, ln) in enumerate(cig):
        if op == 0:
            for i in range(ln):
                if q[x + i] != t[y + i]:
                    md.append(str(u) + letters[t[y + i]])
                    n_mm += 1
                    u = 0
                else:
                    u += 1
            x += ln
            y += ln
        elif op == 2:
            if 0 < k < len(cig) - 1:
                md.append(str(u) + "^" + "".join(letters[t[y + i]] for i in range(ln)))
                u = 0
                n_gap += ln
            y += ln
        else:
            x += ln
            n_gap += ln
    md.append(str(u))
    return score, cig, n_mm + n_gap, "".join(md).encode(), nodp


def reg2aln_one(T, l_pac, read, reg, mat, gaps, W, cigar_stride, md_stride, dp=_oracle_dp):
    """One region (mapping with qb, qe, rb, re, truesc, w) of `read` -> (fields dict, cigar words,
    MD bytes, set of branches).  Raises ValueError where the library returns BSW_E_RANGE."""
    qb, qe, rb, re, truesc, w_reg = (int(reg[f]) for f in ("qb", "qe", "rb", "re", "truesc", "w"))
    l_query, a = len(read), mat[0]
    br = set()
    if rb < 0 or re < 0 or qe - qb <= 0 or rb >= re or (l_pac > 0 and rb < l_pac and re > l_pac):
        br.add("rejected")
        return (dict(pos=-1, is_rev=0, n_cigar=0, NM=-1, score=0, w=0, n_pass=1, md_len=0, flags=REJECTED),
                [], b"", br)
    if qb < 0 or qe > l_query or re > len(T) or re - rb > 32767 or qe - qb > 32767:
        raise ValueError("region outside its read or the text")
    o_del, e_del, o_ins, e_ins = gaps
    w2 = max(infer_bw(qe - qb, re - rb, truesc, a, o_del, e_del), infer_bw(qe - qb, re - rb, truesc, a, o_ins, e_ins))
    if w2 > W:
        w2 = min(w2, w_reg)
        br.add("min_w_reg")
    i, last_sc = 0, -(1 << 30)
    while True:
        w2 = min(w2, W << 2)
        score, cig, nm, md, nodp = gen_cigar2(T, l_pac, read[qb:qe], rb, re, w2, mat, gaps, dp)
        w_last = w2
        if score == last_sc or w2 == W << 2:
            if w2 == W << 2 and score != last_sc:
                br.add("cap_break")
            i += 1
            break
        last_sc = score
        w2 <<= 1
        i += 1
        if not (i < 3 and score < truesc - a):
            break
    n_pass = i
    br.add("gapfree" if nodp else "dp")
    if n_pass >= 2:
        br.add("pass2")
    if n_pass >= 3:
        br.add("pass3")
    is_rev = l_pac > 0 and rb >= l_pac
    br.add("rev" if is_rev else "fwd")
    flags = NODP if nodp else 0
    out = dict(score=score, w=w_last, n_pass=n_pass)
    pos = 2 * l_pac - re if is_rev else rb
    fin = list(cig)
    if fin[0][0] == 2:
        pos += fin[0][1]
        fin = fin[1:]
        br.add("squeeze_lead")
    elif fin[-1][0] == 2:
        fin = fin[:-1]
        br.add("squeeze_trail")
    if qb != 0 or qe != l_query:
        clip5 = l_query - qe if is_rev else qb
        clip3 = qb if is_rev else l_query - qe
        if clip5:
            fin = [(3, clip5)] + fin
            br.add("clip5")
        if clip3:
            fin = fin + [(3, clip3)]
            br.add("clip3")
    if len(cig) > cigar_stride or len(fin) > cigar_stride:
        out.update(pos=-1, is_rev=0, n_cigar=-1, NM=-1, md_len=-1, flags=flags | OVERFLOW)
        return out, [], b"", br
    md_len = 0 if md_stride == 0 else (len(md) if len(md) <= md_stride else -1)
    if md_len < 0:
        flags |= OVERFLOW
    out.update(pos=pos, is_rev=int(is_rev), n_cigar=len(fin), NM=nm, md_len=md_len, flags=flags)
    return out, [(ln << 4) | op for op, ln in fin], (md if md_len > 0 else b""), br


def reg2aln(T, l_pac, reads, read_off, read_len, regs, reg_read, mat, gaps, W, cigar_stride=16, md_stride=64,
            dp=_oracle_dp):
    """Batch form with the library's output layout: (aln ALN_DTYPE, cigar [n, cigar_stride], md
    [n, md_stride] or None, per-region branch sets)."""
    n = len(regs)
    aln = np.zeros(n, dtype=ALN_DTYPE)
    cigar = np.zeros((n, cigar_stride), dtype=np.uint32)
    md = np.zeros((n, md_stride), dtype=np.uint8) if md_stride > 0 else None
    branches = []
    mat = [int(v) for v in mat]
    for k in range(n):
        rd = int(reg_read[k])
        if not 0 <= rd < len(read_len):
            r = regs[k]
            if not (r["rb"] < 0 or r["re"] < 0 or r["qe"] - r["qb"] <= 0 or r["rb"] >= r["re"] or
                    (l_pac > 0 and r["rb"] < l_pac and r["re"] > l_pac)):
                raise ValueError("read index out of range")
            rd = 0
        read = reads[int(read_off[rd]):int(read_off[rd]) + int(read_len[rd])] if len(read_len) else reads[:0]
        f, cg, m, br = reg2aln_one(T, l_pac, read, regs[k], mat, gaps, W, cigar_stride, md_stride, dp)
        for name, v in f.items():
            aln[k][name] = v
        cigar[k, :len(cg)] = cg
        if md is not None and len(m):
            md[k, :len(m)] = np.frombuffer(m, np.uint8)
        branches.append(br)
    return aln, cigar, md, branches


def branch_counts(branches):
    return {b: sum(b in s for s in branches) for b in BRANCHES}


def cigar_str(words):
    return "".join(f"{int(w) >> 4}{'MIDS'[int(w) & 15]}" for w in words)
