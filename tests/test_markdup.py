"""Duplicate marking on the GPU (include/bsw_markdup.h): bsw_mark_duplicates* against tests/markdup_py.py (the header's
rules restated by brute force: every candidate compared with every other) and against the serial model
tools/markdup_model.cpp, which runs the kernels' own per-read and per-pair functions on the CPU.

CPU: the restatement's answers derived by hand, one case per rule; the model (plain and under AddressSanitizer + UBSan,
as a stand-alone program) against the restatement on every case, on random sets and on every rejected input; the header
file, the exports, the invalid-argument cases, the binding.  GPU: the hand cases, the sizes at which the kernels can go
wrong, both sort routes, quals on every dword phase, errors that write nothing, and the pipeline device to device."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import bsw
import hiprt
import markdup_py as md
from conftest import ROOT
from markdup_py import N, R, U, make_case
from stagekit import declared, exported

HI, LO = b"IIIIIIII", b"55555555"           # 8 x 40 = 320, 8 x 20 = 160
COUNTERS = ("n_cand", "n_pair_cand", "n_dup_pairs", "n_dup_frag", "n_dup_frag_by_pair", "n_pair_sets", "n_end_sets", "n_flagged")


# ---------------------------------------------------------------- the hand cases: name -> (case, dup derived by hand)
_hand = {}


def hand_cases():
    if _hand:
        return _hand
    c = _hand
    fr = lambda q=LO: [R(100, 0, "8M", q), R(300, 1, "8M", q)]
    c["two_identical_pairs"] = (make_case(fr() + fr(), True), [0, 0, 1, 1])
    # 5S95M at 105 and 100M at 100: u = 100 both; the second pair scores higher
    c["leading_clip_same_u"] = (make_case([R(105, 0, "5S95M"), R(300, 1, "100M"), R(100, 0, "100M", HI), R(300, 1, "100M", HI)], True),
                                [1, 1, 0, 0])
    # reverse: 300 + 90 - 1 + 10 = 399 = 300 + 100 - 1
    c["reverse_trailing_clip"] = (make_case([R(100, 0, "50M"), R(300, 1, "90M10S"), R(100, 0, "50M"), R(300, 1, "100M")], True),
                                  [0, 0, 1, 1])
    # rlen counts D and not I: 40 + 5 + 45 = 90 -> u 389; with I alone 85 -> u 384
    c["reverse_D_and_I"] = (make_case([R(100, 0, "50M"), R(300, 1, "40M5D10I45M"), R(100, 0, "50M"), R(300, 1, "90M"),
                                       R(100, 0, "50M"), R(300, 1, "40M5I45M")], True), [0, 0, 1, 1, 0, 0])
    # FR (100 +, 349 -) against RF (100 -, 349 +): 51 + 50 - 1 = 100
    c["FR_against_RF"] = (make_case([R(100, 0, "50M"), R(300, 1, "50M"), R(51, 1, "50M"), R(349, 0, "50M")], True), [0, 0, 0, 0])
    c["same_lo_other_hi"] = (make_case([R(100, 0, "50M"), R(300, 1, "50M"), R(100, 0, "50M"), R(301, 1, "50M")], True), [0, 0, 0, 0])
    c["read1_read2_swapped"] = (make_case([R(100, 0, "50M"), R(300, 1, "50M"), R(300, 1, "50M"), R(100, 0, "50M")], True),
                                [0, 0, 1, 1])
    # a fragment at the pair's lo end (read 2) and one at its hi end (read 5), both scoring higher than the pair's reads
    c["fragment_by_pair_lo_and_hi"] = (make_case([R(100, 0, "50M"), R(300, 1, "50M"), R(100, 0, "50M", HI), U(), U(),
                                                  R(300, 1, "50M", HI)], True), [0, 0, 3, 0, 0, 3])
    c["fragment_only_set"] = (make_case([R(100, 0, "50M"), R(100, 0, "50M", HI), R(100, 0, "50M"), R(101, 0, "50M")], False),
                              [2, 0, 2, 0])
    c["mate_unmapped"] = (make_case([R(100, 0, "50M", HI), U(pos=100), R(100, 0, "50M"), U(pos=100)], True), [0, 0, 2, 0])
    c["both_unmapped"] = (make_case([U(), U(), U(), U()], True), [0, 0, 0, 0])
    c["supplementary_inherits"] = (make_case(fr(HI) + [R(100, 0, "8M", LO, extra=[(5000, 1, "4H4M", 0x800, 0x800)]), R(300, 1, "8M")],
                                             True), [0, 0, 1, 1])
    c["no_multi_inherits"] = (make_case(fr(HI) + [R(100, 0, "8M", LO, extra=[(5000, 0, "4S4M", 0x10000, 0x100)]), R(300, 1, "8M")],
                                        True), [0, 0, 1, 1])
    c["tie_to_lower_index"] = (make_case([R(100, 0, "50M"), R(100, 0, "50M")], False), [0, 2])
    # '/' is 14 and does not count: 0 against '0' = 15
    c["slash_and_zero"] = (make_case([R(100, 0, "50M", b"//////////"), R(100, 0, "50M", b"0!!!!!!!!!")], False), [2, 0])
    c["min_qual_14"] = (make_case([R(100, 0, "50M", b"//////////"), R(100, 0, "50M", b"0!!!!!!!!!")], False, min_qual=14), [0, 2])
    c["quals_null"] = (make_case([R(100, 0, "50M", LO), R(100, 0, "50M", HI)], False, with_quals=False), [0, 2])
    c["0x400_on_input_cleared"] = (make_case([R(100, 0, "50M", flag=0x400), R(200, 0, "50M", HI, extra=[(900, 0, "8M", 0xc00, 0xc00)])],
                                             False), [0, 0])
    c["bit_32"] = (make_case([R(5, 0, "50M", HI), R(5 + (1 << 32), 0, "50M", HI), R(5 + (1 << 32), 0, "50M")], False, l_pac=1 << 34),
                   [0, 0, 2])
    # 5S20M at the first base of contig 1 and 20M of contig 0: u = 995 both, the rids differ
    c["contig_start_clip"] = (make_case([R(1000, 0, "5S20M"), R(995, 0, "20M")], False, l_pac=3000, ctg=(1000, 1000, 1000)), [0, 0])
    # reads that have no record at all, the batch's last among them (its d_rec_first entry is n_rec): no candidates, and
    # their mates are fragments
    c["reads_without_records"] = (make_case([R(100, 0, "50M"), N(), N(), R(100, 0, "50M", HI), R(100, 0, "50M"), N()], True),
                                  [2, 0, 0, 0, 2, 0])
    c["no_record_at_all"] = (make_case([N(), N(), N(), N()], True), [0, 0, 0, 0])     # n_rec == 0, n_aln == 0: the arrays may be NULL
    return c


def _rng(seed):
    return np.random.default_rng(seed)


def random_case(seed, n_reads, paired, ctg=None, l_pac=1 << 20, span=40, with_quals=True):
    """coordinates from a few dozen values so that sets form; random clips, strands, quals; a few unmapped reads and
    further records"""
    r = _rng(seed)
    places = r.integers(50, l_pac - 200, span)
    reads = []
    for _ in range(n_reads):
        q = bytes(r.integers(33, 75, int(r.integers(1, 40))).astype(np.uint8))
        if r.random() < 0.1:
            reads.append(U(q))
            continue
        pos, rev = int(r.choice(places)) + int(r.integers(0, 3)), int(r.integers(0, 2))
        body = ["30M", "10M2D18M", "12M3I15M"][int(r.integers(0, 3))]
        cg = (f"{int(r.integers(1, 6))}S" if r.random() < 0.4 else "") + body + (f"{int(r.integers(1, 6))}S" if r.random() < 0.4 else "")
        extra = [(int(r.choice(places)), 1, "6H9M", 0x800, 0x800)] if r.random() < 0.1 else []
        reads.append(R(pos, rev, cg, q, extra, 0x400 if r.random() < 0.2 else 0))
    return make_case(reads, paired, l_pac=l_pac, ctg=ctg, lead=int(r.integers(0, 4)))


def random_cases():
    return {"se_300": random_case(1, 300, False), "pe_400": random_case(2, 400, True), "pe_no_quals": random_case(3, 200, True, with_quals=False),
            "pe_three_contigs": random_case(4, 300, True, ctg=(400000, 300000, (1 << 20) - 700000), span=25)}


def broken_cases():
    """(tag, case) that the stage answers with BSW_E_RANGE"""
    out = []

    def base():
        return make_case([R(100, 0, "8M"), R(300, 1, "8M", extra=[(700, 0, "4H4M", 0x800, 0x800)]), U(), R(100, 0, "4S4M")], True)
    c = base(); c.rec_first[2] = 1; out.append(("a decreasing rec_first", c))
    c = base(); c.rec_first[4] = 4; out.append(("a rec_first that does not end at n_rec", c))
    c = base(); c.rec_first[0] = 1; out.append(("a rec_first that does not start at 0", c))
    c = base(); c.recs["read"][2] = 0; out.append(("a record under another read", c))
    c = base(); c.recs["aln"][2] = len(c.aln); out.append(("aln == n_aln", c))
    c = base(); c.recs["aln"][3] = -2; out.append(("aln -2", c))
    c = base(); c.recs["aln"][0] = -1; out.append(("a candidate with aln -1", c))
    c = base(); c.aln["n_cigar"][0] = 0; out.append(("a candidate with n_cigar 0", c))
    c = base(); c.aln["n_cigar"][3] = -1; out.append(("a candidate with n_cigar -1", c))
    c = base(); c.read_len[3] += 1; out.append(("a read past the quals", c))
    c = base(); c.read_off[1] = -1; out.append(("a negative read offset", c))
    c = base(); c.read_off[2] = (1 << 63) - 4; out.append(("a read offset whose sum with the length wraps", c))
    # u = pos + rlen - 1 of a reverse end past the end word's 40 bits: 4,100 ops of 2^28 - 1 bases
    c = make_case([R(100, 1, "268435455M" * 4100), R(300, 0, "8M")], True, stride=4100)
    out.append(("a CIGAR whose rlen does not fit u", c))
    return out


# ---------------------------------------------------------------- CPU: the restatement's answers, derived by hand
@pytest.mark.parametrize("name", list(hand_cases()))
def test_restatement_and_model_give_the_hand_derived_answer(name, tmp_path_factory, tmp_path):
    c, want = hand_cases()[name]
    assert md.check(c) == 0
    recs, dup, st = md.mark(c)
    assert list(dup) == want, name
    rc, mrecs, mdup, _, err = run_model(model_bin(tmp_path_factory), tmp_path, c)         # the hand answer pins the code too
    assert rc == 0 and list(mdup) == want, (name, rc, err)
    assert mrecs.tobytes() == recs.tobytes(), name
    for k in range(len(recs)):
        on = want[recs["read"][k]] != 0 and not c.recs["flag"][k] & 4
        assert bool(recs["flag"][k] & 0x400) == on and bool(recs["sam_flag"][k] & 0x400) == on, (name, k)
        assert recs["flag"][k] & ~0x400 == c.recs["flag"][k] & ~0x400 and recs["sam_flag"][k] & ~0x400 == c.recs["sam_flag"][k] & ~0x400
    assert st["n_flagged"] == int(sum(bool(f & 0x400) for f in recs["flag"]))


def test_restatement_on_the_named_details():
    assert (md.DUP_PAIR, md.DUP_FRAG, md.DUP_FRAG_BY_PAIR) == (bsw.BSW_DUP_PAIR, bsw.BSW_DUP_FRAG, bsw.BSW_DUP_FRAG_BY_PAIR)
    assert (md.MAX_L_PAC, md.MAX_CONTIGS) == (1 << 39, (1 << 23) - 1)
    h = hand_cases()
    assert md.end_of(h["leading_clip_same_u"][0], 0) == md.end_of(h["leading_clip_same_u"][0], 2) == (0, 100, 0)
    assert md.end_of(h["reverse_trailing_clip"][0], 1) == md.end_of(h["reverse_trailing_clip"][0], 3) == (0, 399, 1)
    assert [md.end_of(h["reverse_D_and_I"][0], i)[1] for i in (1, 3, 5)] == [389, 389, 384]
    assert md.end_of(h["contig_start_clip"][0], 0) == (1, 995, 0) and md.end_of(h["contig_start_clip"][0], 1) == (0, 995, 0)
    assert [md.score_of(h["slash_and_zero"][0], i) for i in (0, 1)] == [0, 15]
    assert [md.score_of(h["min_qual_14"][0], i) for i in (0, 1)] == [140, 15]
    recs, _, st = md.mark(h["supplementary_inherits"][0])
    assert [int(f) & 0x400 for f in recs["sam_flag"]] == [0, 0, 0x400, 0x400, 0x400] and st["n_flagged"] == 3
    recs, _, _ = md.mark(h["no_multi_inherits"][0])
    assert int(recs["sam_flag"][3]) == 0x500 and int(recs["flag"][3]) == 0x10400
    recs, _, _ = md.mark(h["mate_unmapped"][0])
    assert [int(f) & 0x400 for f in recs["flag"]] == [0, 0, 0x400, 0]           # the unmapped mate stays unflagged
    recs, _, _ = md.mark(h["0x400_on_input_cleared"][0])
    assert [int(f) for f in recs["flag"]] == [0, 0, 0x800] and [int(f) for f in recs["sam_flag"]] == [0, 0, 0x800]
    st = md.mark(h["fragment_by_pair_lo_and_hi"][0])[2]
    assert (st["n_cand"], st["n_pair_cand"], st["n_dup_frag_by_pair"], st["n_end_sets"], st["n_pair_sets"]) == (4, 1, 2, 2, 0)
    for tag, c in broken_cases():
        assert md.check(c) == -34, tag


# ---------------------------------------------------------------- CPU: the serial model
_model = {}


def model_bin(tmp_path_factory, *flags):
    """tools/markdup_model.cpp, compiled once per set of flags: a stand-alone program"""
    if flags not in _model:
        exe = tmp_path_factory.mktemp("markdup") / "markdup_model"
        r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "bwa-mem2-arm_amd", "csrc"),
                            os.path.join(ROOT, "tools", "markdup_model.cpp"), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _model[flags] = str(exe)
    return _model[flags]


SAN = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")


def run_model(exe, tmp, c):
    """(returncode, recs, dup, the counters it prints, stderr)"""
    tmp = str(tmp)
    paths = {}
    for k in ("recs", "rec_first", "aln", "cigar", "read_off", "read_len", "quals"):
        a = getattr(c, k)
        if a is None:
            paths[k] = "-"
            continue
        paths[k] = os.path.join(tmp, k)
        np.ascontiguousarray(a).tofile(paths[k])
    paths["ctg"] = "-"
    if c.ctg is not None:
        paths["ctg"] = os.path.join(tmp, "ctg")
        np.array(c.ctg, np.int64).tofile(paths["ctg"])
    outs = [os.path.join(tmp, "out_recs"), os.path.join(tmp, "out_dup")]
    r = subprocess.run([exe] + [str(x) for x in (c.n_reads, len(c.recs), len(c.aln), c.stride, int(c.paired), c.l_pac, c.min_qual, c.flags)] +
                       [paths[k] for k in ("recs", "rec_first", "aln", "cigar", "read_off", "read_len", "quals", "ctg")] + outs,
                       capture_output=True, text=True)
    if r.returncode:
        return r.returncode, None, None, None, r.stderr
    w = r.stdout.split()
    return 0, np.fromfile(outs[0], bsw.REC_DTYPE), np.fromfile(outs[1], np.uint8), dict(zip(w[0::2], (int(x) for x in w[1::2]))), r.stderr


def same_marks(want, recs, dup, tag):
    wrecs, wdup, _ = want
    assert np.array_equal(dup, wdup), f"{tag}: dup differs at reads {np.flatnonzero(dup != wdup)[:8]}: want {wdup[dup != wdup][:8]} got {dup[dup != wdup][:8]}"
    for f in bsw.REC_DTYPE.names:
        bad = np.flatnonzero(wrecs[f] != recs[f])
        assert len(bad) == 0, f"{tag}: rec.{f} differs at {bad[:5]}: want {wrecs[f][bad[:5]]} got {recs[f][bad[:5]]}"


def _model_counters(cnt):
    return {"n_" + k if not k.startswith("n_") else k: v for k, v in cnt.items()}


@pytest.mark.parametrize("flags", [(), SAN], ids=["plain", "sanitized"])
def test_model_marks_as_the_restatement(tmp_path_factory, tmp_path, flags):
    exe = model_bin(tmp_path_factory, *flags)
    cases = {k: v[0] for k, v in hand_cases().items()}
    cases.update(random_cases())
    cases["no_reads"] = make_case([], True)
    for name, c in cases.items():
        rc, recs, dup, cnt, err = run_model(exe, tmp_path, c)
        assert rc == 0 and "runtime error" not in err and "Sanitizer" not in err, (name, rc, err)
        want = md.mark(c)
        same_marks(want, recs, dup, name)
        if name in hand_cases():
            assert list(dup) == hand_cases()[name][1], name
        cnt = _model_counters(cnt)
        assert {k: cnt[k] for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, name
    for tag, c in broken_cases():
        rc, _, _, _, err = run_model(exe, tmp_path, c)
        assert rc == 34 and "Sanitizer" not in err and "runtime error" not in err, (tag, rc, err)
    bad = make_case([R(100, 0, "8M")], False)
    for kw in (dict(l_pac=0), dict(l_pac=(1 << 39) + 1), dict(min_qual=-1), dict(flags=1), dict(paired=True), dict(ctg=[5, 6])):
        c = make_case([R(100, 0, "8M")], False)
        vars(c).update(kw)
        assert md.check(c) == -22 and run_model(exe, tmp_path, c)[0] == 22, kw
    assert md.check(bad) == 0


def test_model_takes_both_sort_routes(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for name, (c, route) in route_cases().items():
        rc, recs, dup, cnt, _ = run_model(exe, tmp_path, c)
        assert rc == 0 and cnt["pair_route"] == route, (name, cnt)
        same_marks(md.mark(c), recs, dup, name)


# ---------------------------------------------------------------- CPU: the header file and the binding
def test_library_exports_the_markdup_header():
    assert declared("bsw_markdup.h") == set(bsw.MARKDUP_SYMBOLS)
    assert declared("bsw_markdup.h") <= exported(), declared("bsw_markdup.h") - exported()
    others = (set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS) | set(bsw.MATESW_SYMBOLS) |
              set(bsw.REC_SYMBOLS) | set(bsw.CONTIGS_SYMBOLS) | set(bsw.BAM_SYMBOLS) | set(bsw.BGZF_SYMBOLS) | set(bsw.BAMSORT_SYMBOLS))
    assert not set(bsw.MARKDUP_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8
    assert (bsw.BSW_DUP_PAIR, bsw.BSW_DUP_FRAG, bsw.BSW_DUP_FRAG_BY_PAIR) == (1, 2, 3)


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_markdup_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_markdup.h"\n'
                   f"{sa}(sizeof(bsw_markdup_opt_t) == 16 && offsetof(bsw_markdup_opt_t, min_qual) == 8 && offsetof(bsw_markdup_opt_t, flags) == 12, \"opt\");\n"
                   f"{sa}(sizeof(bsw_markdup_stats_t) == 72 && offsetof(bsw_markdup_stats_t, n_flagged) == 32 && offsetof(bsw_markdup_stats_t, pair_route) == 44 && offsetof(bsw_markdup_stats_t, score_ms) == 52 && offsetof(bsw_markdup_stats_t, mark_ms) == 64, \"stats\");\n"
                   f"{sa}(BSW_MARKDUP_API == 1 && BSW_ABI_VERSION == 8 && BSW_DUP_PAIR == 1 && BSW_DUP_FRAG == 2 && BSW_DUP_FRAG_BY_PAIR == 3, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.MarkdupOpt) == 16 and bsw.MarkdupOpt.min_qual.offset == 8
    assert ctypes.sizeof(bsw.MarkdupStats) == 72 and bsw.MarkdupStats.n_flagged.offset == 32
    assert bsw.MarkdupStats.pair_route.offset == 44 and bsw.MarkdupStats.score_ms.offset == 52
    o = bsw.markdup_opt(1000)
    assert (o.l_pac, o.min_qual, o.flags) == (1000, 15, 0) and bsw.markdup_opt(5, min_qual=0).min_qual == 0


def test_resident_batch_knows_the_dup_buffer():
    import resident
    assert resident._row("dup") == (np.dtype(np.uint8), (), "n_reads")
    assert list(resident.DUP_LAYOUT) == ["dup"]
    assert not set(resident.DUP_LAYOUT) & (set(resident.LAYOUT) | set(resident.BAM_LAYOUT) | set(resident.BGZF_LAYOUT) | set(resident.SORT_LAYOUT))
    assert callable(resident.ResidentBatch.mark_duplicates)


def _calls(ctx, o, n_reads=2, n_rec=2, n_aln=2, stride=4, quals_len=8, paired=1, recs=True, first=True, aln=True, cigar=True,
           off=True, lens=True, dup=True):
    """(the host form's answer, the resident form's)"""
    Lb = bsw.hip_lib()
    P, B = bsw._ptr, ctypes.byref
    a = np.zeros(1024, np.uint8)
    pa = lambda on: P(a) if on else None
    args = (ctx, B(o) if o is not None else None, pa(recs), pa(first), n_rec, pa(aln), pa(cigar), stride, n_aln, pa(off), pa(lens),
            n_reads, P(a), quals_len, paired, pa(dup))
    return Lb.bsw_mark_duplicates(*args), Lb.bsw_mark_duplicates_resident(*args, None)


def test_invalid_arguments_need_no_device():
    Lb = bsw.hip_lib()
    assert Lb.bsw_markdup_last_stats(None, None) == -22
    fake = ctypes.c_void_p(1)                                    # never dereferenced: the checks come first
    good = bsw.markdup_opt(1000)
    inval = (-22, -22)
    assert _calls(None, good) == inval and _calls(fake, None) == inval
    for bad in (bsw.markdup_opt(0), bsw.markdup_opt(-5), bsw.markdup_opt((1 << 39) + 1), bsw.markdup_opt(1000, min_qual=-1),
                bsw.markdup_opt(1000, flags=1)):
        assert _calls(fake, bad) == inval
    for kw in (dict(n_reads=3), dict(n_reads=-2), dict(n_rec=-1), dict(n_aln=-1), dict(stride=0), dict(quals_len=-1), dict(recs=False),
               dict(first=False), dict(aln=False), dict(cigar=False), dict(off=False), dict(lens=False), dict(dup=False)):
        assert _calls(fake, good, **kw) == inval, kw


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng():
    e = bsw.Engine()
    yield e
    e.close()


_ctg_engines = {}


def engine_for(eng, c):
    """the module's engine, or one that holds the case's contig table"""
    if c.ctg is None:
        return eng
    key = tuple(c.ctg)
    if key not in _ctg_engines:
        e = _ctg_engines[key] = bsw.Engine()
        bsw.set_contigs(e, c.ctg, [f"c{k}" for k in range(len(c.ctg))])
    return _ctg_engines[key]


def _dev(a, pad=0):
    a = np.ascontiguousarray(a)
    raw = np.concatenate([np.frombuffer(a.tobytes(), np.uint8), np.zeros(max(pad, 1 if a.nbytes == 0 else 0), np.uint8)])
    return hiprt.DeviceBuffer.from_array(raw)


def gpu_mark(e, c, sentinel=0xA5):
    """bsw_mark_duplicates_resident over uploaded arrays and a sentinel-filled d_dup: (recs, dup); on an error the state
    afterwards is left in gpu_mark.last"""
    n = c.n_reads
    d = {k: _dev(getattr(c, k)) for k in ("recs", "rec_first", "aln", "cigar", "read_off", "read_len")}
    d_q = None if c.quals is None else _dev(c.quals)
    d_dup = hiprt.DeviceBuffer.from_array(np.full(n + 16, sentinel, np.uint8))
    o = bsw.markdup_opt(c.l_pac, min_qual=c.min_qual, flags=c.flags)
    try:
        null = lambda k: d[k].ptr if len(getattr(c, k)) else 0       # an array of no entries is passed as NULL
        bsw.mark_duplicates_resident(e, null("recs"), d["rec_first"].ptr, len(c.recs), null("aln"), null("cigar"), c.stride, len(c.aln),
                                     d["read_off"].ptr, d["read_len"].ptr, n, 0 if d_q is None else d_q.ptr,
                                     0 if c.quals is None else len(c.quals), c.paired, d_dup.ptr, o)
    finally:
        raw = d["recs"].download(np.zeros(max(c.recs.nbytes, 1), np.uint8))[:c.recs.nbytes]
        dup = d_dup.download(np.zeros(n + 16, np.uint8))
        gpu_mark.last = (np.frombuffer(raw.tobytes(), bsw.REC_DTYPE), dup)
    assert (dup[n:] == sentinel).all(), "bytes behind d_dup + n_reads were written"
    return gpu_mark.last[0], dup[:n]


def gpu_case(e, c, tag, exe=None, tmp=None):
    want = md.mark(c)
    recs, dup = gpu_mark(e, c)
    same_marks(want, recs, dup, tag)
    st = bsw.markdup_last_stats(e)
    assert {k: getattr(st, k) for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, tag
    assert st.n_reads == c.n_reads
    hrecs, hdup = bsw.mark_duplicates(e, c.recs, c.rec_first, c.aln, c.cigar, c.read_off, c.read_len, c.quals, c.paired,
                                      bsw.markdup_opt(c.l_pac, min_qual=c.min_qual))           # the host form
    same_marks(want, hrecs, hdup, tag + " (host form)")
    if exe is not None:
        rc, mrecs, mdup, cnt, _ = run_model(exe, tmp, c)
        assert rc == 0, tag
        same_marks((mrecs, mdup, None), recs, dup, tag + " (model)")
        assert (st.pair_key_bits, st.end_key_bits, st.pair_route, st.end_route) == (cnt["pair_bits"], cnt["end_bits"], cnt["pair_route"],
                                                                                    cnt["end_route"]), tag
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hand_cases()))
def test_gpu_hand_cases(eng, name, tmp_path_factory, tmp_path):
    c, want = hand_cases()[name]
    st = gpu_case(engine_for(eng, c), c, name, model_bin(tmp_path_factory), tmp_path)
    assert list(gpu_mark.last[1][:c.n_reads]) == want
    recs2, dup2 = gpu_mark(engine_for(eng, c), c)                  # the call can be repeated
    assert list(dup2) == want
    if c.quals is not None:
        assert st.score_ms > 0
    assert st.key_ms > 0 and st.mark_ms > 0


def _one_set(n_pairs, seed, same_score=False):
    r = _rng(seed)
    q = lambda: LO if same_score else bytes(r.integers(48, 75, 8).astype(np.uint8))
    return make_case([x for _ in range(n_pairs) for x in (R(1000, 0, "8M", q()), R(1300, 1, "8M", q()))], True)


def _small_sets(n_pairs, seed):
    """pairs in sets of 1-3, the sets' members scattered over the batch"""
    r = _rng(seed)
    place = []
    while len(place) < n_pairs:
        place += [len(place) * 7 + 50] * int(r.integers(1, 4))
    place = np.array(place[:n_pairs])[r.permutation(n_pairs)]
    q = r.integers(48, 75, (2 * n_pairs, 8)).astype(np.uint8)
    return make_case([x for p in range(n_pairs) for x in (R(int(place[p]), 0, "8M", bytes(q[2 * p])), R(int(place[p]) + 200, 1, "8M", bytes(q[2 * p + 1])))],
                     True)


_size = {}


def size_cases():
    if _size:
        return _size
    T = bsw.BAMSORT_SORT_TILE
    c = _size
    c["n_reads_0"] = make_case([], True)
    c["one_pair"] = _one_set(1, 1)
    c["two_pairs"] = _one_set(2, 2)
    for n in (63, 64, 65, 255, 256, 257, T + 1):
        c[f"one_set_{n}"] = _one_set(n, n)
    c["sets_1_to_3"] = _small_sets(3 * T + 5, 7)
    c["no_varying_bit"] = _one_set(70, 3, same_score=True)
    # one pair's lo end, then more fragments at its (rid, u, s) than one tile of the sort holds
    c["fragment_set_over_tiles"] = make_case([R(100, 0, "8M"), R(300, 1, "8M")] +
                                             [x for k in range(T + 100) for x in (R(100, 0, "8M", HI if k % 3 else LO), U())], True)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(size_cases()))
def test_gpu_sizes_at_which_the_kernels_can_go_wrong(eng, name, tmp_path_factory, tmp_path):
    c = size_cases()[name]
    st = gpu_case(eng, c, name, model_bin(tmp_path_factory), tmp_path)
    n = c.n_reads // 2
    if name.startswith("one_set_"):
        assert (st.n_pair_cand, st.n_dup_pairs, st.n_pair_sets) == (n, n - 1, 1)
    if name == "no_varying_bit":
        assert (st.pair_key_bits, st.pair_route, st.n_dup_pairs) == (0, bsw.MARKDUP_ROUTE_NONE, n - 1)
        assert list(gpu_mark.last[1][:4]) == [0, 0, 1, 1]
    if name == "n_reads_0":
        assert (st.n_cand, st.score_ms, st.key_ms, st.sort_ms, st.mark_ms) == (0, 0, 0, 0, 0)      # a valid call that runs nothing
    if name == "fragment_set_over_tiles":
        assert st.n_dup_frag_by_pair == bsw.BAMSORT_SORT_TILE + 100 and st.n_dup_frag == 0


_route = {}


def route_cases():
    """name -> (case, the pair sort's route): the same set structure over a small reference and spread over a 2^39-base
    table of 64 contigs, where the varying bits of two ends do not fit one word"""
    if _route:
        return _route
    for name, l_pac, ctg, route in (("fits_one_word", 1 << 20, None, bsw.MARKDUP_ROUTE_ONE),
                                    ("spread_over_2^39", 1 << 39, [1 << 33] * 64, bsw.MARKDUP_ROUTE_MULTI)):
        r, rp = _rng(11), _rng(12)                                # (the places from a stream of their own: the same sets in both)
        places = [(int(rp.integers(0, l_pac - 5000)), int(rp.integers(0, l_pac - 5000))) for _ in range(90)]
        reads = []
        for k in range(300):
            a, b = places[int(r.integers(0, len(places)))]
            q = [bytes(r.integers(40, 75, 12).astype(np.uint8)) for _ in range(2)]
            ends = [R(a, 0, "3S30M", q[0]), R(b, 1, "30M4S", q[1])]
            reads += ends[::-1] if k % 5 == 0 else ends
        _route[name] = (make_case(reads, True, l_pac=l_pac, ctg=ctg), route)
    return _route


@pytest.mark.gpu
def test_gpu_both_sort_routes(eng, tmp_path_factory, tmp_path):
    seen = {}
    for name, (c, route) in route_cases().items():
        st = gpu_case(engine_for(eng, c), c, name, model_bin(tmp_path_factory), tmp_path)
        assert st.pair_route == route, (name, st.pair_route, st.pair_key_bits)
        assert (st.pair_key_bits > 64) == (route == bsw.MARKDUP_ROUTE_MULTI) and st.n_dup_pairs > 50 and st.sort_ms > 0
        seen[name] = (st.n_dup_pairs, st.n_pair_sets)
    assert len(set(seen.values())) == 1                           # the same sets on both routes


@pytest.mark.gpu
def test_gpu_quals_on_every_dword_phase(eng):
    """reads at offsets 0..7 modulo 8 and of lengths 1, 3, 4, 5, 63, 64, 65, 151; the first and the last byte of a read at
    and around min_qual; the bytes between the reads ('~', 93) would change every sum if read"""
    lens = (1, 3, 4, 5, 63, 64, 65, 151)
    edge = [b"/", b"0", b"1"]                                     # 14, 15, 16
    seen = set()
    for lead in range(8):
        reads = []
        for k, n in enumerate(lens):
            for v in range(3):
                body = bytearray(b"5" * n)
                body[0:1] = edge[(k + v) % 3]
                body[-1:] = edge[(k + 2 * v + 1) % 3] if n > 1 else body[-1:]
                reads.append(R(100 + 10 * k, 0, "8M", bytes(body)))
        c = make_case(reads, False, lead=lead, gap=b"~")
        seen |= {(int(o) % 8, int(n)) for o, n in zip(c.read_off, c.read_len)}
        want = md.mark(c)
        recs, dup = gpu_mark(eng, c)
        same_marks(want, recs, dup, f"lead {lead}")
        assert want[2]["n_dup_frag"] == 2 * len(lens)
    assert seen == {(ph, n) for ph in range(8) for n in lens}       # every length began on every byte of 8


@pytest.mark.gpu
def test_gpu_errors_write_nothing(eng):
    for tag, c in broken_cases():
        with pytest.raises(bsw.BswError, match="-34"):
            gpu_mark(eng, c, sentinel=0x5A)
        recs, dup = gpu_mark.last
        assert (dup == 0x5A).all(), tag
        assert recs.tobytes() == c.recs.tobytes(), tag
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.mark_duplicates(eng, c.recs, c.rec_first, c.aln, c.cigar, c.read_off, c.read_len, c.quals, c.paired, bsw.markdup_opt(c.l_pac))
    c = hand_cases()["contig_start_clip"][0]
    with pytest.raises(bsw.BswError, match="-22"):               # a table is needed that sums to l_pac: this engine has none...
        gpu_mark(engine_for(eng, c), make_case([R(5, 0, "8M")], False, l_pac=2999))
    c, want = hand_cases()["fragment_by_pair_lo_and_hi"]
    assert list(gpu_mark(eng, c)[1]) == want                      # a valid call afterwards, on the same context


def _doubled(s, every=3):
    """the pipeline set of test_rec with every third pair emitted a second time and every sixth a third time, under
    other quals: (reads, off, lens, quals, mregs, minfo, mfirst, names)"""
    p, a = s.p, s.p.arr
    n_pairs = len(a["lens"]) // 2
    order = list(range(n_pairs)) + [q for q in range(n_pairs) if q % every == 0] + [q for q in range(n_pairs) if q % (2 * every) == 0]
    reads, quals, off, lens, regs, info, first = [], [], [], [], [], [], [0]
    r = _rng(5)
    at = 0
    for k, q in enumerate(order):
        for e in (2 * q, 2 * q + 1):
            o, n = int(a["off"][e]), int(a["lens"][e])
            reads.append(a["reads"][o:o + n])
            quals.append(s.quals[o:o + n] if k < n_pairs else r.integers(35, 74, n).astype(np.uint8))
            off.append(at)
            lens.append(n)
            at += n
            regs.append(p.mregs[p.mfirst[e]:p.mfirst[e + 1]])
            info.append(p.minfo[p.mfirst[e]:p.mfirst[e + 1]])
            first.append(first[-1] + int(p.mfirst[e + 1] - p.mfirst[e]))
    return (np.concatenate(reads), np.array(off, np.int64), np.array(lens, np.int32), np.concatenate(quals), np.concatenate(regs),
            np.concatenate(info), np.array(first, np.int32), [b"frag%d" % k for k in range(len(order))])


def _pipeline(e, s, ropt, l_pac, ctg, n_ref, tag):
    import bam_py as bp
    import bai_py as bi
    from resident import ResidentBatch
    reads, off, lens, quals, mregs, minfo, mfirst, names = _doubled(s)

    def run(mark):
        b = ResidentBatch(e, reads, off, lens, quals)
        b.put(mreg=mregs, minfo=minfo, mfirst=mfirst)
        b.pe_pair(s.p.pes, bsw.pe_opt(l_pac=l_pac))
        b.records(ropt)
        before = b.get("recs")
        st = b.mark_duplicates(bsw.markdup_opt(l_pac)) if mark else None
        b.sam_text(ropt, names, True)
        b.bam_records(ropt, None, True)
        b.bam_sort(n_ref)
        return b, before, st

    b, before, st = run(True)
    recs, dup = b.get("recs"), b.get("dup")
    c = make_case([], True, l_pac=l_pac, ctg=ctg, stride=b.stride["cigar"])
    c.recs, c.rec_first, c.aln, c.cigar, c.read_off, c.read_len, c.quals, c.n_reads = (before, b.get("rec_first"), b.get("aln"),
                                                                                     b.get("cigar"), off, lens, quals, len(lens))
    assert md.check(c) == 0
    want = md.mark(c)
    same_marks(want, recs, dup, tag)
    assert {k: getattr(st, k) for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, tag
    assert st.n_dup_pairs >= len(names) // 5 and st.n_flagged > 0, (tag, st.n_dup_pairs)
    on = (want[0]["flag"] & 0x400) != 0
    # the FLAG column of the text
    text, toff = b.get("text").tobytes(), b.get("text_off")
    lines = [text[toff[k]:toff[k + 1]] for k in range(len(recs))]
    assert [bool(int(x.split(b"\t")[1]) & 0x400) for x in lines] == list(on), tag
    # the flag field of every BAM block, unsorted and sorted
    bam, boff = b.get("bam").tobytes(), b.get("bam_off")
    blocks = bi.split(bam, boff)
    assert [bool(bp.fields(x[4:])["flag"] & 0x400) for x in blocks] == list(on), tag
    perm = b.get("bam_perm")
    sblocks = bi.split(b.get("sbam").tobytes(), b.get("sbam_off"))
    assert [bool(bp.fields(x[4:])["flag"] & 0x400) for x in sblocks] == [bool(on[k]) for k in perm], tag
    # every other byte equals the run without the stage
    b0, _, _ = run(False)
    text0, toff0 = b0.get("text").tobytes(), b0.get("text_off")
    for k, x in enumerate(lines):
        f = x.split(b"\t")
        f[1] = b"%d" % (int(f[1]) & ~0x400)
        assert b"\t".join(f) == text0[toff0[k]:toff0[k + 1]], (tag, k)
    blocks0 = bi.split(b0.get("bam").tobytes(), b0.get("bam_off"))
    for k, x in enumerate(blocks):
        y = bytearray(x)
        y[18 + 1] &= ~0x04 & 0xff                                # flag is the half-word at byte 18 of the block: 0x400 is bit 2 of byte 19
        assert bytes(y) == blocks0[k], (tag, k)
    assert np.array_equal(b0.get("bam_perm"), perm), tag          # the sort key does not read 0x400
    # the host-array form
    hrecs, hdup = bsw.mark_duplicates(e, before, c.rec_first, c.aln, c.cigar, off, lens, quals, True, bsw.markdup_opt(l_pac))
    assert np.array_equal(hdup, dup) and hrecs.tobytes() == recs.tobytes(), tag
    return st


@pytest.mark.gpu
def test_gpu_pipeline_marks_reach_text_and_bam_device_to_device(eng):
    """bsw_records_resident -> bsw_mark_duplicates_resident -> bsw_sam_text_resident / bsw_bam_records_resident ->
    bsw_bam_sort_resident on the same resident arrays"""
    from test_rec import rec_set
    s = rec_set()
    bsw.set_reference(eng, s.p.T)
    _pipeline(eng, s, bsw.rec_opt(**s.opt), int(s.p.l_pac), None, 1, "one reference")


def _free_join(p, near):
    """a forward coordinate at or behind `near` that no region of the pipeline set bridges (the reverse strand's regions
    mirrored), so that the set is a valid one under a table that joins two contigs there"""
    l_pac = int(p.l_pac)
    covered = np.zeros(l_pac + 1, bool)
    for rb, re_ in zip(p.mregs["rb"], p.mregs["re"]):
        lo, hi = (int(rb), int(re_)) if rb < l_pac else (2 * l_pac - int(re_), 2 * l_pac - int(rb))
        covered[max(lo - 200, 0):hi + 200] = True                # (and room for the clips around a region)
    return near + int(np.flatnonzero(~covered[near:])[0])


@pytest.mark.gpu
def test_gpu_pipeline_marks_under_three_contigs():
    from test_rec import rec_set
    s = rec_set()
    l_pac = int(s.p.l_pac)
    j1, j2 = _free_join(s.p, 8000), _free_join(s.p, 20000)
    lens = [j1, j2 - j1, l_pac - j2]
    e = bsw.Engine()
    bsw.set_reference(e, s.p.T)
    bsw.set_contigs(e, lens, ["c1", "chr_two", "3"])
    st = _pipeline(e, s, bsw.rec_opt(**s.opt), l_pac, lens, 3, "three contigs")
    assert st.n_dup_pairs > 0
    e.close()
