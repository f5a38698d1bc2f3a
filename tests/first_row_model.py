"""Which first-row values does ksw_extend2 read late?  (Plain Python, small inputs only.)

A.1 fills the row buffer with the first row h0 - oe_ins - (j - 1) e_ins once.  A row reads slots
[beg, end) and writes slots <= end, and `end` grows by at most 2 a row (A.7), so a slot is read
with its first-row value still in it exactly when the band's right end moves two columns past
every slot written so far -- below the band edge i + w + 1, after the end shrank and grew back.

The wave kernel (bsw_wv.hip) holds a window of `win` columns and computes the first-row value of
a column when it slides in (`hin` for column `jn`).  `extend` is oracle/ksw_ext_ref.py's
transcription with two additions: it counts the reads of never-written slots j >= win whose
first-row value is positive, and `shift` puts the first-row value of column j + shift into
every slot j >= win -- what a wrong `jn` would do.  Outputs that change with `shift` are
outputs that depend on `hin`.
"""

from __future__ import annotations

import math


def extend(query, target, mat, o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, win, shift=0):
    """Returns ((score, tle, gtle, qle, gscore, max_off), late_reads)."""
    qlen, tlen = len(query), len(target)

    def first_row(j):
        return h0 if j == 0 else (max(h0 - (o_ins + e_ins) - (j - 1) * e_ins, 0) if j <= qlen else 0)

    H = [first_row(j) if j < win else first_row(j + shift) for j in range(qlen + 2)]
    E = [0] * (qlen + 2)
    maxsc = max(0, max(mat))
    w = min(w, max(int(math.trunc((qlen * maxsc + end_bonus - o_ins) / e_ins + 1.0)), 1))
    w = min(w, max(int(math.trunc((qlen * maxsc + end_bonus - o_del) / e_del + 1.0)), 1))
    best, best_i, best_j = h0, -1, -1
    max_ie, gscore, max_off = -1, -1, 0
    beg, end = 0, qlen
    written, late = -1, 0
    for i in range(tlen):
        row = mat[target[i] * 5: target[i] * 5 + 5]
        beg = max(beg, i - w)
        end = min(end, i + w + 1, qlen)
        h1 = max(h0 - (o_del + e_del * (i + 1)), 0) if beg == 0 else 0
        f = 0
        m = 0
        mj = -1
        for j in range(max(beg, written + 1, win), end):
            late += H[j] > 0
        for j in range(beg, end):
            M, e = H[j], E[j]
            H[j] = h1
            M = M + row[query[j]] if M != 0 else 0
            h = max(M, e, f)
            h1 = h
            if not (m > h):
                mj = j
            m = max(m, h)
            e = max(e - e_del, M - (o_del + e_del), 0)
            E[j] = e
            f = max(f - e_ins, M - (o_ins + e_ins), 0)
        H[end] = h1
        E[end] = 0
        written = max(written, end)
        if (end if beg < end else beg) == qlen:
            if not (gscore > h1):
                max_ie = i
            gscore = max(gscore, h1)
        if m == 0:
            break
        if m > best:
            best, best_i, best_j = m, i, mj
            max_off = max(max_off, abs(mj - i))
        elif zdrop > 0:
            di, dj = i - best_i, mj - best_j
            if di > dj:
                if best - m - (di - dj) * e_del > zdrop:
                    break
            elif best - m - (dj - di) * e_ins > zdrop:
                break
        j = beg
        while j < end and H[j] == 0 and E[j] == 0:
            j += 1
        beg = j
        j = end
        while j >= beg and H[j] == 0 and E[j] == 0:
            j -= 1
        end = min(j + 2, qlen)
    return (best, best_i + 1, max_ie + 1, best_j + 1, gscore, max_off), late
