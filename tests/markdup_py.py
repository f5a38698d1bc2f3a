"""The duplicate-marking rules of include/bsw_markdup.h restated by brute force: every candidate is compared with every
other (numpy tables of all pairs of members); nothing is sorted, no key is packed, and no code is shared with the serial
model tools/markdup_model.cpp or with the kernels.  Also the builders of hand-made inputs: a Case holds the arrays that
bsw_mark_duplicates* takes.  A plain module, not a test."""

import re
from types import SimpleNamespace

import numpy as np

import bsw

DUP_PAIR, DUP_FRAG, DUP_FRAG_BY_PAIR = 1, 2, 3
OPS = "MIDSH"
MAX_L_PAC, MAX_CONTIGS = 1 << 39, (1 << 23) - 1
SCORE_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- builders
def R(pos, rev=0, cigar="8M", quals=b"55555555", extra=(), flag=0):
    """a mapped read: its first record at pos on strand rev; extra: further records (pos, rev, cigar, flag bits,
    sam_flag bits) of the same read"""
    return SimpleNamespace(pos=pos, rev=rev, cigar=cigar, quals=quals, extra=tuple(extra), flag=flag)


def U(quals=b"55555555", pos=-1, rev=0):
    """an unmapped read (pos: what cross-linking gave it)"""
    return SimpleNamespace(pos=pos, rev=rev, cigar=None, quals=quals, extra=(), flag=0)


def N(quals=b"55555555"):
    """a read that has no record at all"""
    return SimpleNamespace(pos=-1, rev=0, cigar=None, quals=quals, extra=(), flag=0, no_record=True)


def cigar_words(text):
    return [int(n) << 4 | OPS.index(op) for n, op in re.findall(r"(\d+)([MIDSH])", text)]


def make_case(reads, paired, l_pac=1 << 20, min_qual=15, ctg=None, stride=8, with_quals=True, lead=0, gap=b""):
    """the arrays of one call.  lead: bytes in front of the first read's quals; gap: bytes between two reads' quals
    (so that reads begin on any byte and have neighbours)"""
    recs, first, alns, cig, off, lens, q = [], [0], [], [], [], [], bytearray(b"~" * lead)
    max_stride_rows = False
    for i, rd in enumerate(reads):
        off.append(len(q))
        lens.append(len(rd.quals))
        q += rd.quals + gap
        specs = [] if getattr(rd, "no_record", False) else [(rd.pos, rd.rev, rd.cigar, rd.flag, rd.flag)] + list(rd.extra)
        for which, (pos, rev, cg, fl, sfl) in enumerate(specs):
            # bsw_rec_t in field order: pos mpos tlen read reg aln which n_list flag sam_flag is_rev mapq score sub m_is_rev
            # m_aln xa_first xa_n reserved
            if cg is None:
                recs.append((pos, -1, 0, i, -1, -1, which, len(specs), fl | 4, sfl | 4, rev, 0, 0, 0, 0, -1, 0, 0, 0))
                continue
            words = cigar_words(cg)
            assert 0 < len(words) <= stride
            max_stride_rows = True
            strand = 16 if rev else 0
            recs.append((pos, -1, 0, i, len(alns), len(alns), which, len(specs), fl | strand, sfl | strand, rev, 0, 0, 0, 0, -1, 0, 0, 0))
            alns.append((pos, rev, len(words), 0, 0, 0, 0, 0, 0))
            cig.append(words + [0] * (stride - len(words)))
        first.append(len(recs))
    if max_stride_rows:
        cig = [row + [0] * (stride - len(row)) for row in cig]
    return SimpleNamespace(
        recs=np.array(recs, bsw.REC_DTYPE) if recs else np.zeros(0, bsw.REC_DTYPE), rec_first=np.array(first, np.int32),
        aln=np.array(alns, bsw.ALN_DTYPE) if alns else np.zeros(0, bsw.ALN_DTYPE),
        cigar=np.array(cig, np.uint32).reshape(len(cig), stride), read_off=np.array(off, np.int64), read_len=np.array(lens, np.int32),
        quals=np.frombuffer(bytes(q), np.uint8).copy() if with_quals else None, paired=bool(paired), l_pac=l_pac,
        min_qual=min_qual, flags=0, ctg=None if ctg is None else [int(x) for x in ctg], stride=stride, n_reads=len(reads))


# ---------------------------------------------------------------- the rules
def check(c):
    """0, -22 (BSW_E_INVAL) or -34 (BSW_E_RANGE): what the header says of the inputs"""
    n = c.n_reads
    if not 0 < c.l_pac <= MAX_L_PAC or c.min_qual < 0 or c.flags or c.stride < 1 or (c.paired and n % 2):
        return -22
    if c.ctg is not None and (sum(c.ctg) != c.l_pac or not 0 < len(c.ctg) <= MAX_CONTIGS):
        return -22
    if n == 0:
        return 0
    f = [int(x) for x in c.rec_first]
    if f[0] != 0 or f[-1] != len(c.recs) or any(b < a for a, b in zip(f, f[1:])):
        return -34
    for i in range(n):
        if c.quals is not None and (c.read_off[i] < 0 or c.read_len[i] < 0 or int(c.read_off[i]) + int(c.read_len[i]) > len(c.quals)):
            return -34
        for k in range(f[i], f[i + 1]):
            if c.recs["read"][k] != i or not -1 <= c.recs["aln"][k] < len(c.aln):
                return -34
        if f[i + 1] > f[i] and not c.recs["flag"][f[i]] & 4:
            r = c.recs[f[i]]
            if r["aln"] < 0 or not 0 <= r["pos"] < c.l_pac or not 0 < c.aln["n_cigar"][r["aln"]] <= c.stride:
                return -34
            if not -(1 << 31) <= end_of(c, i)[1] < (1 << 40) - (1 << 31):
                return -34
    return 0


def _rid(c, pos):
    if c.ctg is None:
        return 0
    start = 0
    for k, n in enumerate(c.ctg):
        if start <= pos < start + n:
            return k
        start += n
    raise AssertionError("pos outside the table")


def end_of(c, i):
    """(rid, u, s) of candidate read i, or None"""
    f0, f1 = int(c.rec_first[i]), int(c.rec_first[i + 1])
    if f1 == f0 or c.recs["flag"][f0] & 4:
        return None
    r = c.recs[f0]
    ops = [(int(w) >> 4, int(w) & 15) for w in c.cigar[r["aln"]][:c.aln["n_cigar"][r["aln"]]]]
    pos, rev = int(r["pos"]), int(r["is_rev"])
    if not rev:
        u = pos - (ops[0][0] if ops[0][1] in (3, 4) else 0)
    else:
        u = pos + sum(n for n, op in ops if op in (0, 2)) - 1 + (ops[-1][0] if ops[-1][1] in (3, 4) else 0)
    return _rid(c, pos), u, 1 if rev else 0


def score_of(c, i):
    if c.quals is None:
        return 0
    q = c.quals[int(c.read_off[i]):int(c.read_off[i]) + int(c.read_len[i])].astype(np.int64) - 33
    return min(int(q[q >= c.min_qual].sum()), SCORE_MAX)


class _Couples:
    """the couples (i, j) of members with equal keys, for the members i of `rows` against every member j: a table of
    booleans where many keys are equal, index lists where few are"""

    def __init__(self, rows, n, eq=None, a=None, j=None):
        self.rows, self.n, self.eq, self.a, self.j = rows, n, eq, a, j

    def any(self, fn):
        """per member i of rows: some j with an equal key has fn(j, i)"""
        if self.eq is not None:
            return (self.eq & fn(np.arange(self.n)[None, :], self.rows[:, None])).any(axis=1)
        out = np.zeros(len(self.rows), bool)
        out[self.a[fn(self.j, self.rows[self.a])]] = True
        return out

    def members(self):
        return self.eq.sum(axis=1) if self.eq is not None else np.bincount(self.a, minlength=len(self.rows))


def _equal_members(cols, chunk=1024):
    """every member meets every other on the first column of the key; the further columns are compared where the
    columns before them agreed"""
    n = len(cols[0])
    for b in range(0, n, chunk):
        rows = np.arange(b, min(b + chunk, n))
        eq = cols[0][rows, None] == cols[0][None, :]
        if eq.sum() > 16 * len(rows):
            for col in cols[1:]:
                eq &= col[rows, None] == col[None, :]
            yield _Couples(rows, n, eq=eq)
            continue
        a, j = np.nonzero(eq)
        for col in cols[1:]:
            keep = col[rows[a]] == col[j]
            a, j = a[keep], j[keep]
        yield _Couples(rows, n, a=a, j=j)


def mark(c):
    """(the records afterwards, dup uint8 [n_reads], the counters of bsw_markdup_stats_t that the rules define)"""
    n = c.n_reads
    ends = [end_of(c, i) for i in range(n)]
    score = [score_of(c, i) for i in range(n)]
    dup = np.zeros(n, np.uint8)
    st = dict(n_cand=sum(e is not None for e in ends), n_pair_cand=0, n_dup_pairs=0, n_dup_frag=0, n_dup_frag_by_pair=0,
              n_pair_sets=0, n_end_sets=0, n_flagged=0)
    in_pair = np.zeros(n, bool)
    if c.paired:
        pairs = [p for p in range(n // 2) if ends[2 * p] is not None and ends[2 * p + 1] is not None]
        st["n_pair_cand"] = len(pairs)
        if pairs:
            key = np.array([min(ends[2 * p], ends[2 * p + 1]) + max(ends[2 * p], ends[2 * p + 1]) for p in pairs], np.int64)
            sc = np.array([score[2 * p] + score[2 * p + 1] for p in pairs], np.int64)
            idx = np.array(pairs, np.int64)
            in_pair[2 * idx] = in_pair[2 * idx + 1] = True
            # member j beats member i: the higher score, then the lower index
            beats = lambda j, i: (sc[j] > sc[i]) | ((sc[j] == sc[i]) & (idx[j] < idx[i]))
            for cp in _equal_members([key[:, k] for k in (1, 4, 0, 2, 3, 5)]):
                lost = cp.any(beats)
                dup[2 * idx[cp.rows[lost]]] = dup[2 * idx[cp.rows[lost]] + 1] = DUP_PAIR
                st["n_dup_pairs"] += int(lost.sum())
                st["n_pair_sets"] += int((~lost & (cp.members() > 1)).sum())
    cand = [i for i in range(n) if ends[i] is not None]
    if cand:
        key = np.array([ends[i] for i in cand], np.int64)
        sc = np.array([score[i] for i in cand], np.int64)
        idx = np.array(cand, np.int64)
        frag = ~in_pair[idx]
        beats = lambda j, i: (sc[j] > sc[i]) | ((sc[j] == sc[i]) & (idx[j] < idx[i]))
        for cp in _equal_members([key[:, k] for k in (1, 0, 2)]):
            by_pair = cp.any(lambda j, i: ~frag[j] & (i == i))
            lost = cp.any(lambda j, i: frag[j] & beats(j, i))
            earlier = cp.any(lambda j, i: idx[j] < idx[i])
            mine = frag[cp.rows]
            dup[idx[cp.rows[mine]]] = np.where(by_pair[mine], DUP_FRAG_BY_PAIR, np.where(lost[mine], DUP_FRAG, 0))
            st["n_end_sets"] += int((~earlier & (cp.members() > 1)).sum())
        st["n_dup_frag"] = int((dup == DUP_FRAG).sum())
        st["n_dup_frag_by_pair"] = int((dup == DUP_FRAG_BY_PAIR).sum())
    recs = c.recs.copy()
    for k in range(len(recs)):
        on = dup[recs["read"][k]] != 0 and not recs["flag"][k] & 4
        for f in ("flag", "sam_flag"):
            recs[f][k] = recs[f][k] | 0x400 if on else recs[f][k] & ~0x400
        st["n_flagged"] += bool(on)
    return recs, dup, st
