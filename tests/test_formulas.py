"""Upstream's integer formulas as csrc/bsw_formulas.h states them once for the host builder and every
stage kernel: cal_max_gap, cigar_band, infer_bw, infer_dir.

CPU only: a small C++ program includes the internal header and the published include/bsw_global.h,
prints the four formulas over a fixed grid (asserting cigar_band == bsw_gen_cigar_band on the way),
and every printed value is compared with the Python restatements the suite already trusts
(reg2aln_py.infer_bw, reg2aln_py.gen_cigar_band, pe_py.infer_dir; cal_max_gap as include/bsw_ext.h
states it).  The published band is also printed from C, so the header is pinned under both compilers.
"""

import os
import subprocess

import pytest

import pe_py as pp
import reg2aln_py as rp
from conftest import ROOT
from stagekit import SCORINGS

LENS = (0, 1, 2, 19, 150, 151, 10000)
BANDS = (1, 100, 400)
L_PACS = (1, 1000)

GRID_LOOPS = """
    static const int lens[] = {0, 1, 2, 19, 150, 151, 10000}, bands[] = {1, 100, 400};
    static const int scorings[][5] = {%s};                  /* a, o_del, e_del, o_ins, e_ins */
    enum { NL = 7, NB = 3, NS = sizeof(scorings) / sizeof(scorings[0]) };
""" % ", ".join("{%d, %d, %d, %d, %d}" % (a, od, ed, oi, ei) for a, _, od, ed, oi, ei in SCORINGS)

CXX_SRC = """
#include <stdio.h>
#include <stdlib.h>
#include "bsw_formulas.h"
#include "bsw_global.h"
int main()
{""" + GRID_LOOPS + """
    for (int s = 0; s < NS; ++s) {
        const int a = scorings[s][0], od = scorings[s][1], ed = scorings[s][2], oi = scorings[s][3], ei = scorings[s][4];
        for (int w = 0; w < NB; ++w)
            for (int i = 0; i < NL; ++i) {
                printf("gap %d %d %d %d %d %d %d %d\\n", a, od, ed, oi, ei, bands[w], lens[i],
                       bsw::cal_max_gap(a, od, ed, oi, ei, bands[w], lens[i]));
                for (int k = 0; k < NL; ++k) {
                    const int band = bsw::cigar_band(a, od, ed, oi, ei, lens[i], lens[k], bands[w]);
                    if (band != bsw_gen_cigar_band(lens[i], lens[k], bands[w], a, od, ed, oi, ei)) {
                        fprintf(stderr, "cigar_band != bsw_gen_cigar_band at %d %d %d\\n", lens[i], lens[k], bands[w]);
                        return 1;
                    }
                    printf("band %d %d %d %d %d %d %d %d %d\\n", a, od, ed, oi, ei, lens[i], lens[k], bands[w], band);
                }
            }
        for (int i = 0; i < NL; ++i)
            for (int k = 0; k < NL; ++k) {
                const int m = (lens[i] < lens[k] ? lens[i] : lens[k]) * a;
                const int scores[] = {0, 1, m / 2, m - 7, m - 1, m};
                for (int c = 0; c < 6; ++c) {
                    printf("bw %d %d %d %d %d %d %d\\n", lens[i], lens[k], scores[c], a, od, ed,
                           bsw::infer_bw(lens[i], lens[k], scores[c], a, od, ed));
                    printf("bw %d %d %d %d %d %d %d\\n", lens[i], lens[k], scores[c], a, oi, ei,
                           bsw::infer_bw(lens[i], lens[k], scores[c], a, oi, ei));
                }
            }
    }
    static const long long l_pacs[] = {1, 1000};
    for (int p = 0; p < 2; ++p) {
        const long long L = l_pacs[p];
        const long long b[] = {0, L / 3, L - 1, L, L + L / 3, 2 * L - 1};
        for (int i = 0; i < 6; ++i)
            for (int k = 0; k < 6; ++k) {
                int64_t dist = -1;
                const int dir = bsw::infer_dir(L, b[i], b[k], dist);
                printf("dir %lld %lld %lld %d %lld\\n", L, b[i], b[k], dir, (long long)dist);
            }
    }
    return 0;
}
"""

C_SRC = """
#include <stdio.h>
#include "bsw_global.h"
int main(void)
{""" + GRID_LOOPS + """
    int s, w, i, k;
    for (s = 0; s < NS; ++s)
        for (w = 0; w < NB; ++w)
            for (i = 0; i < NL; ++i)
                for (k = 0; k < NL; ++k)
                    printf("band %d %d %d %d %d %d %d %d %d\\n", scorings[s][0], scorings[s][1], scorings[s][2],
                           scorings[s][3], scorings[s][4], lens[i], lens[k], bands[w],
                           bsw_gen_cigar_band(lens[i], lens[k], bands[w], scorings[s][0], scorings[s][1],
                                              scorings[s][2], scorings[s][3], scorings[s][4]));
    return 0;
}
"""


def _cal_max_gap(a, o_del, e_del, o_ins, e_ins, w, qlen):
    """gap(l) = min(max((l*a - o)/e + 1, 1), 2w), the larger of the two gap kinds (include/bsw_ext.h)"""
    l_del = int(float(qlen * a - o_del) / e_del + 1.0)
    l_ins = int(float(qlen * a - o_ins) / e_ins + 1.0)
    return min(max(l_del, l_ins, 1), w << 1)


def _run(tmp_path, cc, name, text, std):
    src, exe = tmp_path / name, tmp_path / (name + ".out")
    src.write_text(text)
    r = subprocess.run([cc, std, "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "bwa-mem2-arm_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [(ln.split()[0], [int(v) for v in ln.split()[1:]]) for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    d = tmp_path_factory.mktemp("formulas")
    return _run(d, "g++", "f.cpp", CXX_SRC, "-std=c++17"), _run(d, "gcc", "g.c", C_SRC, "-std=c11")


def _check(kind, v):
    if kind == "gap":
        return _cal_max_gap(*v[:7]) == v[7]
    if kind == "band":
        a, od, ed, oi, ei, lq, rlen, w_ = v[:8]
        return rp.gen_cigar_band(lq, rlen, w_, a, od, ed, oi, ei) == v[8]
    if kind == "bw":
        return rp.infer_bw(*v[:6]) == v[6]
    assert kind == "dir"
    return pp.infer_dir(*v[:3]) == (v[3], v[4])


def test_every_printed_value_matches_the_python_restatements(printed):
    cxx, c = printed
    bad = [(k, v) for k, v in cxx + c if not _check(k, v)]
    assert not bad, bad[:10]
    # the published header gives the same band under both compilers, on the same grid
    assert [v for k, v in cxx if k == "band"] == [v for k, v in c]


def test_the_grid_covers_what_it_is_meant_to(printed):
    cxx, _ = printed
    by = {k: [v for kk, v in cxx if kk == k] for k in ("gap", "band", "bw", "dir")}
    gaps = {(a, od, ed, oi, ei) for a, _, od, ed, oi, ei in SCORINGS}
    assert any(s[0] != 1 for s in gaps) and any(s[2] != s[4] for s in gaps)
    assert {tuple(v[:5]) for v in by["gap"]} == gaps == {tuple(v[:5]) for v in by["band"]}
    assert {(v[5], v[6]) for v in by["gap"]} == {(w, l) for w in BANDS for l in LENS}
    assert {(v[5], v[6], v[7]) for v in by["band"]} == {(lq, rl, w) for lq in LENS for rl in LENS for w in BANDS}
    assert {(v[0], v[1]) for v in by["bw"]} == {(l1, l2) for l1 in LENS for l2 in LENS}
    assert {tuple(v[3:6]) for v in by["bw"]} == {(a, o, e) for a, _, od, ed, oi, ei in SCORINGS for o, e in ((od, ed), (oi, ei))}
    assert any(v[6] == 0 for v in by["bw"]) and any(v[6] > abs(v[0] - v[1]) for v in by["bw"])   # both returns
    assert {v[0] for v in by["dir"]} == set(L_PACS)
    for L in L_PACS:
        b = {(v[1], v[2]) for v in by["dir"] if v[0] == L}
        edge = {L - 1, L, 2 * L - 1}
        assert edge <= {x for x, _ in b} and edge <= {y for _, y in b}
        assert any(x == y for x, y in b) and any(x < L <= y for x, y in b) and any(y < L <= x for x, y in b)
        assert any(x >= L and y >= L for x, y in b) and any(x < L and y < L for x, y in b)
    assert {v[3] for v in by["dir"]} == {0, 1, 2, 3}
