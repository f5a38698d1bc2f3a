"""Coordinate-sorted, indexed BAM on the GPU (include/bsw_bamsort.h): bsw_bam_sort* and bsw_bam_index* against
tests/bai_py.py (numpy's stable sort over the header's key; the header's index rules restated; an independent reader
that queries the index through SAMv1 section 5) and against the serial model tools/bamsort_model.cpp, which runs the
kernels' own per-record functions on the CPU.

CPU: known answers (reg2bin at its level boundaries, a .bai derived by hand); the reader against brute force on the
builder's output, so the oracle is checked before it judges the kernels; the model against bai_py on every case; the
header file; the invalid-argument cases.  GPU: the sort cases (bytes, offsets, permutation, sentinels, both forms, every
error), the index cases at three block sizes (bytes against the builder, queries against brute force), the capacity
protocol, and the pipeline set device to device, with and without a contig table."""

import ctypes
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bai_py as bi
import bam_py as bp
import bgzf_py as gz
import bsw
import hiprt
from conftest import ROOT
from resident import ResidentBatch
from stagekit import declared, exported
from test_bam import TAB3, _quals, _under_table
from test_rec import case_pe, rec_set

TILE = bsw.BAMSORT_PERM_TILE
BLOCK_BYTES = (64, 300, gz.MAX_BLOCK)


def _rng(seed):
    return np.random.default_rng(seed)


def _small(r, i, n_ref=3, span=50000):
    """a short record with a random place and a name that tells it apart"""
    rid = int(r.integers(-1, n_ref))
    return bi.record(rid, int(r.integers(0, span)) if rid >= 0 else -1, int(r.choice([0, 16, 99, 147])),
                     "20M" if rid >= 0 else (), b"q%d" % i, int(r.integers(0, 6)))


def _total_bytes(total, seed):
    """records of exactly `total` bytes together: short ones, then one whose tags fill what is left"""
    r, blocks, used = _rng(seed), [], 0
    while total - used > 400:
        blocks.append(_small(r, len(blocks)))
        used += len(blocks[-1])
    last = bi.record(1, 7, 0, "5M", b"fill", 0)
    blocks.append(bi.record(1, 7, 0, "5M", b"fill", 0, tags=b"XZZ" + b"f" * (total - used - len(last) - 4) + b"\0"))
    assert sum(len(b) for b in blocks) == total
    return blocks


_sort_cases = {}


def sort_cases():
    """name -> (blocks, n_ref)"""
    if _sort_cases:
        return _sort_cases
    c, r = _sort_cases, _rng(5)
    c["n0"] = ([], 1)
    c["n1"] = ([bi.record(0, 5, 0, "3M")], 1)
    c["n2"] = ([bi.record(0, 9, 0, "3M", b"b"), bi.record(0, 5, 16, "3M", b"a")], 1)
    c["all_equal"] = ([bi.record(0, 5, 0, "3M", b"n%d" % i) for i in range(50)], 2)
    c["all_unplaced"] = ([bi.record(-1, -1, 4, (), b"u%d" % (97 - i)) for i in range(40)], 2)
    c["ties_strand"] = ([bi.record(1, 100, 16 * ((i * 7) % 3 == 0), "4M", b"s%d" % i) for i in range(30)] +
                        [bi.record(1, 99 + i % 3, 16 * (i % 2), "4M", b"t%d" % i) for i in range(30)], 2)
    c["ties_name"] = ([bi.record(i % 2, 40, 16, "4M", b"name%d" % (60 - i)) for i in range(60)], 2)
    c["three_refs_reversed"] = ([bi.record(2 - i // 20, 1000 - 7 * (i % 20), 0, "9M", b"r%d" % i) for i in range(60)], 3)
    c["n_ref_70000"] = ([bi.record(rid, 10 + i, 0, "2M" if rid >= 0 else (), b"w%d" % i)
                         for i, rid in enumerate([69999, 65536, -1, 65535, 3, 65537, 65536, 0, -1, 65535])], 70000)
    c["pos_max"] = ([bi.record(0, 2 ** 31 - 2, 0, "1M", b"hi"), bi.record(-1, -1, 4, (), b"un"), bi.record(0, 0, 0, "1M", b"lo"),
                     bi.record(0, 2 ** 31 - 2, 16, "1M", b"hi2"), bi.record(0, 2 ** 31 - 3, 0, "1M", b"hi3")], 1)
    res = [bi.record(int(r.integers(0, 2)), int(r.integers(0, 300)), 0, "4M", b"x" * nl, ls) for nl in range(1, 9) for ls in range(8)]
    c["residues"] = ([res[i] for i in r.permutation(len(res))], 2)
    long_ = bi.record(1, 77, 0, [(1 + k % 3, "MID"[k % 3]) for k in range(600)], b"L" * 254, 4000)
    assert len(long_) > TILE
    c["long_block"] = ([_small(r, 0), _small(r, 1), long_, _small(r, 2), bi.record(0, 1, 0, "2M", b"first")], 3)
    for name, total in (("tile-1", TILE - 1), ("tile", TILE), ("tile+1", TILE + 1), ("3tiles+5", 3 * TILE + 5)):
        c[name] = (_total_bytes(total, total), 3)
    for n in (bsw.BAMSORT_SORT_TILE + 1, 3 * bsw.BAMSORT_SORT_TILE + 5):
        rr = _rng(n)
        c[f"n{n}"] = ([_small(rr, i, span=600) for i in range(n)], 3)
    return c


def _placed(rid, pos, cigar, name, flag=0, **kw):
    return bi.record(rid, pos, flag, cigar, name, 3, **kw)


_index_cases = {}


def index_cases():
    """name -> (blocks in the sort's order, ref_len)"""
    if _index_cases:
        return _index_cases
    c = {}
    c["ends_at_16384"] = ([_placed(0, 16384 - 50, "50M", b"a"), _placed(0, 16384 - 10, "5M5I5M", b"b")], [40000])
    c["pos_16383"] = ([_placed(0, 100, "5M", b"a"), _placed(0, 16383, "2M", b"b"), _placed(0, 16385, "2M", b"c")], [40000])
    c["levels"] = ([_placed(0, (1 << s) - 1, "2M", b"l%d" % s) for s in (14, 17, 20, 23, 26)] +
                   [_placed(0, 1 << 26, "3M", b"top", bin_field=12345)], [1 << 27])
    c["long_deletion"] = ([_placed(0, 1000, "10M40000D10M", b"d"), _placed(0, 1005, "4M", b"e"),
                           _placed(0, 30000, "2S6M", b"f")], [60000])
    c["gap"] = ([_placed(0, 100, "8M", b"a"), _placed(0, 100 + 100000 + 16384, "8M", b"b")], [200000])
    c["empty_middle_reference"] = ([_placed(0, 5, "8M", b"a"), _placed(0, 20000, "8M", b"b"), _placed(2, 7, "3M2N3M", b"c")],
                                   [30000, 5000, 900])
    c["placed_unmapped"] = ([_placed(0, 500, "10M", b"m", 0x49), _placed(0, 500, (), b"m", 0x85), _placed(0, 700, "10=2X", b"n")],
                            [1000])
    tail = [bi.record(-1, -1, 0x4D, (), b"u%d" % i, 5) for i in range(5)]
    c["unplaced_tail"] = ([_placed(1, 40, "6M", b"a"), _placed(1, 41, "6M", b"b", 16)] + tail, [100, 100])
    c["only_unplaced"] = (tail, [100, 200, 300])
    c["no_records"] = ([], [100, 200])
    c["one_base_refs"] = ([_placed(0, 0, "1M", b"a"), _placed(2, (1 << 29) - 1, "1M", b"z")], [1, 0, 1 << 29])
    # A and C in bin 4681, B (bin 585) between them in the file
    c["chunk_rule"] = ([_placed(0, 10, "5M", b"A"), _placed(0, 15, "20000M", b"B"), _placed(0, 20, "5M", b"C"),
                        _placed(0, 21, "5M", b"D")], [100000])
    r = _rng(9)
    many = [_placed(int(r.integers(0, 3)), int(r.integers(0, 70000)), f"{int(r.integers(1, 400))}M{int(r.integers(0, 2)) * 30000 + 1}N4M",
                    b"m%d" % i, int(r.choice([0, 16]))) for i in range(120)]
    c["many"] = (many + tail, [120000, 120000, 120000])
    for name, (blocks, ref_len) in c.items():
        _index_cases[name] = (bi.sort(blocks, len(ref_len))[0], ref_len)
    return _index_cases


def py_stream(blocks, bb, base=0):
    """bgzf_py's writer over the blocks: (stream, voff [n], end_voff) as bsw_bgzf* defines them"""
    data, off = bi.join(blocks)
    stream = gz.write(data, bb)
    starts = [b.off for b in gz.walk(stream)] + [len(stream)]
    voff = np.array([(base + starts[int(o) // bb]) << 16 | int(o) % bb for o in off[:-1]], np.int64)
    return stream, voff, (base + len(stream)) << 16


def regions(blocks, ref_len, seed, n_random=200, per_record=True):
    """(rid, beg, end): every record's extent, single bases on both sides of every window edge in use, whole
    references, a region past the last record, seeded random ones (n_random over all references).  per_record=False:
    the whole references, the region past the end and the random ones alone"""
    out, r = [], _rng(seed)
    last = {}
    for b in blocks:
        rid, beg, end, _ = bi.extent(b)
        if rid < 0:
            continue
        last[rid] = max(last.get(rid, 0), end)
        if not per_record:
            continue
        out.append((rid, beg, end))
        for w in range(beg >> 14, ((end - 1) >> 14) + 2):
            e = w << 14
            out += [(rid, e - 1, e)] if e > 0 else []
            out += [(rid, e, e + 1)]
    for rid, n in enumerate(ref_len):
        out += [(rid, 0, max(n, 1)), (rid, last.get(rid, 0) + 1000, last.get(rid, 0) + 1100)]
        for _ in range(n_random // len(ref_len) + 1):
            a = int(r.integers(0, max(n, 1)))
            out.append((rid, a, a + 1 + int(r.integers(0, max(n, 1)) * r.random() ** 4)))
    return sorted(set(out))


def check_queries(bai, stream, base, blocks, ref_len, seed, n_random=200, per_record=True):
    s, parsed, extents = bi.Stream(stream, base), bi.parse(bai), [bi.extent(b) for b in blocks]
    _, off = bi.join(blocks)
    hits = 0
    for rid, beg, end in regions(blocks, ref_len, seed, n_random, per_record):
        want = bi.brute(blocks, off, rid, beg, end, extents)
        assert bi.query(parsed, s, rid, beg, end) == want, (rid, beg, end)
        hits += len(want)
    return hits


# ---------------------------------------------------------------- CPU: known answers
def test_reg2bin_at_its_level_boundaries():
    assert bi.reg2bin(0, 1) == 4681 and bi.reg2bin(16383, 16384) == 4681 and bi.reg2bin(16384, 16385) == 4682
    assert bi.reg2bin(16383, 16385) == 585 and bi.reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73
    assert bi.reg2bin((1 << 20) - 1, (1 << 20) + 1) == 9 and bi.reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1
    assert bi.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0 and bi.reg2bin(0, 1 << 29) == 0
    assert bi.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767 == 37448
    assert bi.reg2bin(-1, 0) == 4680                                 # (what bsw_bam.h files for pos = -1)
    assert set(bi.reg2bins(0, 1)) == {0, 1, 9, 73, 585, 4681}
    assert 4682 in bi.reg2bins(16383, 16385) and 4681 in bi.reg2bins(16383, 16385)


def test_hand_derived_bai():
    """one reference of 20,000 bases, one record at pos 100 with 50M, voff v, end_voff e"""
    v, e = 0x1234 << 16 | 0x56, 0x2345 << 16
    want = (b"BAI\1" + struct.pack("<i", 1) +
            struct.pack("<i", 2) +                                   # n_bin: 4681 and the pseudo-bin
            struct.pack("<Ii", 4681, 1) + struct.pack("<QQ", v, e) +
            struct.pack("<Ii", 37450, 2) + struct.pack("<QQ", v, e) + struct.pack("<QQ", 1, 0) +
            struct.pack("<i", 1) + struct.pack("<Q", v) +            # n_intv, ioffset
            struct.pack("<Q", 0))                                    # n_no_coor
    assert len(want) == 8 + 4 + 24 + 40 + 12 + 8
    blocks = [bi.record(0, 100, 0, "50M", b"r", 50)]
    assert bi.build(blocks, [v], e, [20000]) == want
    refs, n_no_coor = bi.parse(want)
    assert n_no_coor == 0 and refs[0]["bins"] == {4681: [(v, e)]} and refs[0]["pseudo"] == ((v, e), (1, 0))
    assert refs[0]["ioffset"] == [v] and refs[0]["order"] == [4681, 37450]


def test_record_is_a_block_the_reader_accepts():
    b = bi.record(2, 77, 99, "3S10M2D5M", b"name", 18, mapq=30, next_rid=2, next_pos=200, tlen=150)
    assert bp.blocks(b) == [b[4:]] and bi.extent(b) == (2, 77, 77 + 17, 99)
    line = bp.decode(b, ["a", "b", "c"])[0].split("\t")
    assert line[:9] == ["name", "99", "c", "78", "30", "3S10M2D5M", "=", "201", "150"] and line[9] == "A" * 18
    assert bi.extent(bi.record(0, 5, 4))[:3] == (0, 5, 6) and bi.extent(bi.record(0, 5, 0, "4S3I"))[:3] == (0, 5, 6)


def test_sort_oracle_is_the_headers_key():
    blocks, n_ref = sort_cases()["n_ref_70000"]
    got, perm = bi.sort(blocks, n_ref)
    assert [bp.fields(b[4:])["refID"] for b in got] == [0, 3, 65535, 65535, 65536, 65536, 65537, 69999, -1, -1]
    assert list(perm) == [7, 4, 3, 9, 1, 6, 5, 0, 2, 8]
    got, perm = bi.sort(*sort_cases()["pos_max"])
    assert list(perm) == [2, 4, 0, 3, 1]
    got, perm = bi.sort(*sort_cases()["all_equal"])
    assert list(perm) == list(range(50))
    res = sort_cases()["residues"][0]
    assert {len(b) & 3 for b in res} == {0, 1, 2, 3} and {int(o) & 3 for o in bi.join(res)[1]} == {0, 1, 2, 3}
    assert {int(o) & 3 for o in bi.join(bi.sort(res, 2)[0])[1]} == {0, 1, 2, 3}


# ---------------------------------------------------------------- CPU: the reader against brute force, on the builder
@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_query_equals_brute_force_on_the_builders_index(bb):
    for name, (blocks, ref_len) in index_cases().items():
        stream, voff, end_voff = py_stream(blocks, bb, base=1000)
        bai = bi.build(blocks, voff, end_voff, ref_len)
        check_queries(bai, stream, 1000, blocks, ref_len, seed=len(name))


def _bins(bai, rid=0):
    return bi.parse(bai)[0][rid]


def test_builder_on_the_named_cases():
    ic = index_cases()
    build = lambda name, bb=300: bi.build(ic[name][0], *py_stream(ic[name][0], bb)[1:], ic[name][1])
    assert len(_bins(build("ends_at_16384"))["ioffset"]) == 1
    assert len(_bins(build("pos_16383"))["ioffset"]) == 2 and 585 in _bins(build("pos_16383"))["bins"]
    assert set(_bins(build("levels"))["bins"]) == {585, 73, 9, 1, 0, 4681 + 4096}
    r = _bins(build("long_deletion"))
    assert set(r["bins"]) == {585, 4681, 4682} and len(r["ioffset"]) == 3 and r["ioffset"][1] == r["ioffset"][0]
    r = _bins(build("gap"))
    assert len(r["ioffset"]) == 8 and r["ioffset"][0] < r["ioffset"][1] and len(set(r["ioffset"][1:])) == 1
    refs, _ = bi.parse(build("empty_middle_reference"))
    assert refs[1] == dict(bins={}, order=[], pseudo=None, ioffset=[]) and refs[2]["pseudo"][1] == (1, 0)
    assert _bins(build("placed_unmapped"))["pseudo"][1] == (2, 1)
    assert bi.parse(build("unplaced_tail"))[1] == 5 and bi.parse(build("only_unplaced"))[1] == 5
    assert build("no_records") == b"BAI\1" + struct.pack("<iiiiiQ", 2, 0, 0, 0, 0, 0)
    # the chunk rule: A and C in one compressed block with B between them: one chunk; across two blocks: two; D is
    # file-adjacent to C: it never starts a chunk
    assert [len(_bins(build("chunk_rule", bb))["bins"][4681]) for bb in BLOCK_BYTES] == [2, 1, 1]
    assert all(len(_bins(build("chunk_rule", bb))["bins"][585]) == 1 for bb in BLOCK_BYTES)


# ---------------------------------------------------------------- CPU: the serial model
_model = {}


def model_bin(tmp_path_factory, *flags):
    """tools/bamsort_model.cpp, compiled once per set of flags"""
    if flags not in _model:
        exe = tmp_path_factory.mktemp("bamsort") / "bamsort_model"
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "bwa-mem2-arm_amd", "csrc"),
                            os.path.join(ROOT, "tools", "bamsort_model.cpp"), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _model[flags] = str(exe)
    return _model[flags]


def _files(tmp, **arrays):
    paths = {}
    for k, a in arrays.items():
        paths[k] = os.path.join(tmp, k)
        with open(paths[k], "wb") as f:
            f.write(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return paths


def model_sort(exe, tmp, blocks, n_ref, data=None, off=None):
    """(returncode, sorted bytes, offsets, perm)"""
    d, o = bi.join(blocks)
    p = _files(str(tmp), bam=d if data is None else data, off=o if off is None else off)
    outs = [os.path.join(str(tmp), x) for x in ("out", "out_off", "perm")]
    r = subprocess.run([exe, "sort", str(n_ref), p["bam"], p["off"]] + outs, capture_output=True, text=True)
    if r.returncode:
        return r.returncode, None, None, None
    return 0, open(outs[0], "rb").read(), np.fromfile(outs[1], np.int64), np.fromfile(outs[2], np.int32)


def model_index(exe, tmp, blocks, voff, end_voff, ref_len):
    """(returncode, the .bai, the counters it prints)"""
    d, o = bi.join(blocks)
    p = _files(str(tmp), bam=d, off=o, voff=np.asarray(voff, np.int64), ref_len=np.asarray(ref_len, np.int32))
    out = os.path.join(str(tmp), "bai")
    r = subprocess.run([exe, "index", str(len(ref_len)), p["bam"], p["off"], p["voff"], str(end_voff), p["ref_len"], out],
                       capture_output=True, text=True)
    if r.returncode:
        return r.returncode, None, None
    w = r.stdout.split()
    return 0, open(out, "rb").read(), dict(zip(w[0::2], (int(x) for x in w[1::2])))


def _same_sort(blocks, n_ref, out, out_off, perm, tag):
    want, wperm = bi.sort(blocks, n_ref)
    wbytes, woff = bi.join(want)
    assert np.array_equal(perm, wperm), tag
    assert np.array_equal(out_off, woff), tag
    assert out == wbytes, tag


def test_model_sorts_as_the_oracle(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for name, (blocks, n_ref) in sort_cases().items():
        rc, out, out_off, perm = model_sort(exe, tmp_path, blocks, n_ref)
        assert rc == 0, name
        _same_sort(blocks, n_ref, out, out_off, perm, name)


def _broken_sort_inputs():
    """(tag, data, off, n_ref) that the sort answers with BSW_E_RANGE"""
    blocks = [bi.record(0, 50 - i, 0, "3M", b"e%d" % i) for i in range(6)]
    data, off = bi.join(blocks)
    out = []
    dec = off.copy()
    dec[3] = dec[2] - 1
    out.append(("decreasing offsets", data, dec, 1))
    shifted = off.copy()
    shifted[0] = 1
    out.append(("a first offset that is not 0", data, shifted, 1))
    bad = bytearray(data)
    bad[int(off[2])] ^= 1
    out.append(("a block_size that is not its span", bytes(bad), off, 1))
    tiny = struct.pack("<i", 28) + b"\0" * 28                      # block_size 28: the offsets span 32 bytes
    d2, o2 = bi.join(blocks[:2] + [tiny] + blocks[2:])
    out.append(("a block_size below 32", d2, o2, 1))
    for tag, rid, pos, n_ref in (("refID == n_ref", 2, 5, 2), ("refID -2", -2, 5, 2), ("pos -2", 0, -2, 2)):
        d3, o3 = bi.join(blocks + [bi.record(rid, pos, 0, "3M")])
        out.append((tag, d3, o3, n_ref))
    return out


def test_model_rejects_what_the_sort_rejects(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for tag, data, off, n_ref in _broken_sort_inputs():
        assert model_sort(exe, tmp_path, None or [], n_ref, data, off)[0] == 34, tag


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_model_indexes_as_the_oracle(tmp_path_factory, tmp_path, bb):
    exe = model_bin(tmp_path_factory)
    for name, (blocks, ref_len) in index_cases().items():
        _, voff, end_voff = py_stream(blocks, bb, base=77)
        rc, bai, cnt = model_index(exe, tmp_path, blocks, voff, end_voff, ref_len)
        assert rc == 0, name
        assert bai == bi.build(blocks, voff, end_voff, ref_len), name
        refs, n_no_coor = bi.parse(bai)
        assert cnt == dict(bins=sum(len(r["bins"]) for r in refs), chunks=sum(len(c) for r in refs for c in r["bins"].values()),
                           intv=sum(len(r["ioffset"]) for r in refs), no_coor=n_no_coor, bytes=len(bai)), name


def _broken_index_inputs():
    """(tag, blocks, voff, end_voff, ref_len) that the index answers with BSW_E_RANGE"""
    a, b, c = _placed(0, 10, "5M", b"a"), _placed(0, 20, "5M", b"b"), _placed(1, 5, "5M", b"c")
    v = lambda blocks: py_stream(blocks, 300)[1:]
    out = [("unsorted positions", [b, a, c], *v([b, a, c]), [100, 100]),
           ("unsorted references", [c, a], *v([c, a]), [100, 100]),
           ("placed behind unplaced", [bi.record(-1, -1, 4), a], *v([a, a]), [100, 100]),
           ("end > ref_len", [a, b], *v([a, b]), [24, 100]),
           ("ref_len > 2^29", [a, b], *v([a, b]), [100, (1 << 29) + 1]),
           ("placed at pos -1", [bi.record(0, -1, 0, "5M"), a], *v([a, a]), [100, 100])]
    voff, end_voff = v([a, b, c])
    out.append(("decreasing voff", [a, b, c], voff[[0, 2, 1]], end_voff, [100, 100]))
    out.append(("voff above end_voff", [a, b, c], voff, int(voff[2]) - 1, [100, 100]))
    over = bytearray(_placed(0, 30, "5M", b"o"))
    over[16:18] = struct.pack("<H", 3000)                            # n_cigar_op: the words would overrun the block
    out.append(("a CIGAR that overruns its block", [a, bytes(over)], *v([a, bytes(over)]), [100, 100]))
    return out


def test_model_rejects_what_the_index_rejects(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for tag, blocks, voff, end_voff, ref_len in _broken_index_inputs():
        assert model_index(exe, tmp_path, blocks, voff, end_voff, ref_len)[0] == 34, tag


# ---------------------------------------------------------------- CPU: the header file
def test_library_exports_the_bamsort_header():
    assert declared("bsw_bamsort.h") == set(bsw.BAMSORT_SYMBOLS)
    assert declared("bsw_bamsort.h") <= exported(), declared("bsw_bamsort.h") - exported()
    others = (set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS) | set(bsw.MATESW_SYMBOLS) |
              set(bsw.REC_SYMBOLS) | set(bsw.CONTIGS_SYMBOLS) | set(bsw.BAM_SYMBOLS) | set(bsw.BGZF_SYMBOLS))
    assert not set(bsw.BAMSORT_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_bamsort_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_bamsort.h"\n'
                   f"{sa}(sizeof(bsw_bamsort_opt_t) == 8 && offsetof(bsw_bamsort_opt_t, flags) == 4, \"opt\");\n"
                   f"{sa}(sizeof(bsw_bamsort_stats_t) == 64 && offsetof(bsw_bamsort_stats_t, n_bytes) == 8 && offsetof(bsw_bamsort_stats_t, key_ms) == 16 && offsetof(bsw_bamsort_stats_t, index_ms) == 28 && offsetof(bsw_bamsort_stats_t, n_intv) == 40 && offsetof(bsw_bamsort_stats_t, bai_bytes) == 56, \"stats\");\n"
                   f"{sa}(BSW_BAMSORT_API == 1 && BSW_ABI_VERSION == 8 && BSW_BAI_MAX_REF_LEN == 536870912 && BSW_BAI_PSEUDO_BIN == 37450, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.BamsortOpt) == 8 and bsw.BamsortOpt.flags.offset == 4
    assert ctypes.sizeof(bsw.BamsortStats) == 64 and bsw.BamsortStats.key_ms.offset == 16
    assert bsw.BamsortStats.n_intv.offset == 40 and bsw.BamsortStats.bai_bytes.offset == 56
    src = open(os.path.join(ROOT, "bwa-mem2-arm_amd", "csrc", "bsw_bamsort_k.h")).read()
    assert f"kPermTile = {TILE};" in src                            # the tile the binding names for the tests


def test_resident_batch_knows_the_sorted_buffers():
    import resident
    assert resident._row("sbam") == (np.dtype(np.uint8), (), "sbam")
    assert resident._row("sbam_off") == (np.dtype(np.int64), (), "sbam_off")
    assert resident._row("bam_perm") == (np.dtype(np.int32), (), "bam_perm")
    assert resident._row("bai") == (np.dtype(np.uint8), (), "bai")
    assert list(resident.SORT_LAYOUT) == ["sbam", "sbam_off", "bam_perm", "bai"]
    assert not set(resident.SORT_LAYOUT) & (set(resident.LAYOUT) | set(resident.BAM_LAYOUT) | set(resident.BGZF_LAYOUT))
    assert callable(ResidentBatch.bam_sort) and callable(ResidentBatch.bam_index)
    import inspect
    assert inspect.signature(ResidentBatch.bgzf).parameters["src"].default == "bam"


def _sort_calls(ctx, o, n_rec=2, out_cap=128, bam=True, off=True, out=True, out_off=True, perm=True, shift=0, same=False,
                host=True):
    """(the host form's answer, the resident form's); host=False: the resident form alone (its pointers are device
    addresses: what it refuses in them, the host form would go on to use)"""
    Lb = bsw.hip_lib()
    P, B = bsw._ptr, ctypes.byref
    a_bam, a_off = np.zeros(128, np.uint8), np.zeros(4, np.int64)
    a_out, a_oo, a_perm = np.zeros(136, np.uint8), np.zeros(4, np.int64), np.zeros(4, np.int32)
    p_out = ctypes.c_void_p((a_bam if same else a_out).ctypes.data + shift) if out else None
    args = (ctx, B(o) if o is not None else None, P(a_bam) if bam else None, P(a_off) if off else None, n_rec,
            p_out, out_cap, P(a_oo) if out_off else None, P(a_perm) if perm else None)
    return Lb.bsw_bam_sort(*args) if host else None, Lb.bsw_bam_sort_resident(*args, None)


def _index_calls(ctx, o, n_rec=2, bai_cap=64, end_voff=1 << 20, ref_len=(100,), bam=True, off=True, voff=True, bai=True, nby=True,
                 shift=0, host=True):
    Lb = bsw.hip_lib()
    P, B = bsw._ptr, ctypes.byref
    a_bam, a_off, a_voff, a_bai = np.zeros(128, np.uint8), np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(72, np.uint8)
    a_len = None if ref_len is None else np.array(ref_len, np.int32)
    n_bytes = ctypes.c_int64(0)
    args = (ctx, B(o) if o is not None else None, None if a_len is None else P(a_len), P(a_bam) if bam else None,
            P(a_off) if off else None, n_rec, P(a_voff) if voff else None, end_voff,
            ctypes.c_void_p(a_bai.ctypes.data + shift) if bai else None, bai_cap, B(n_bytes) if nby else None)
    return Lb.bsw_bam_index(*args) if host else None, Lb.bsw_bam_index_resident(*args, None)


def test_invalid_arguments_need_no_device():
    Lb = bsw.hip_lib()
    assert Lb.bsw_bamsort_last_stats(None, None) == -22
    fake = ctypes.c_void_p(1)                                    # never dereferenced: the checks come first
    good = bsw.bamsort_opt(1)
    inval = (-22, -22)
    assert _sort_calls(None, good) == inval and _sort_calls(fake, None) == inval
    for bad in (bsw.bamsort_opt(0), bsw.bamsort_opt(-3), bsw.bamsort_opt(1, flags=1)):
        assert _sort_calls(fake, bad) == inval and _index_calls(fake, bad) == inval
    for kw in (dict(n_rec=-1), dict(out_cap=-1), dict(bam=False), dict(off=False), dict(out=False), dict(out_off=False),
               dict(perm=False)):
        assert _sort_calls(fake, good, **kw) == inval, kw
    assert _sort_calls(fake, good, shift=1, host=False)[1] == -22              # a misaligned d_out
    assert _sort_calls(fake, good, same=True, host=False)[1] == -22            # d_out == d_bam
    assert _sort_calls(fake, good, same=True, shift=-64, out_cap=128, host=False)[1] == -22       # d_bam inside d_out's room
    assert _index_calls(None, good) == inval and _index_calls(fake, None) == inval
    for kw in (dict(n_rec=-1), dict(bai_cap=-1), dict(end_voff=-1), dict(ref_len=None), dict(bam=False), dict(off=False),
               dict(voff=False), dict(bai=False), dict(nby=False)):
        assert _index_calls(fake, good, **kw) == inval, kw
    assert _index_calls(fake, good, shift=2, host=False)[1] == -22             # a misaligned d_bai
    # a reference longer than the binning scheme holds is found on the host as well
    assert _index_calls(fake, good, ref_len=((1 << 29) + 1,)) == (-34, -34)
    assert _index_calls(fake, good, ref_len=(-1,)) == (-34, -34)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng():
    e = bsw.Engine()
    yield e
    e.close()


def _resident_sort(eng, data, off, n_ref, out_cap=None, pad=16):
    """bsw_bam_sort_resident into a sentinel-filled buffer: (out with its pad, out_off, perm, the input read back)"""
    n, n_rec = len(data), len(off) - 1
    d_in = hiprt.DeviceBuffer.from_array(np.frombuffer(data + b"\0", np.uint8))
    d_off = hiprt.DeviceBuffer.from_array(np.ascontiguousarray(off, np.int64))
    d_out, d_oo, d_perm = hiprt.DeviceBuffer(n + pad), hiprt.DeviceBuffer(8 * (n_rec + 1)), hiprt.DeviceBuffer(4 * max(n_rec, 1))
    d_out.upload(np.full(n + pad, 0xA5, np.uint8))
    d_oo.upload(np.full(n_rec + 1, -7, np.int64))
    d_perm.upload(np.full(max(n_rec, 1), -7, np.int32))
    try:
        bsw.bam_sort_resident(eng, d_in.ptr, d_off.ptr, n_rec, d_out.ptr, n if out_cap is None else out_cap, d_oo.ptr, d_perm.ptr,
                              bsw.bamsort_opt(n_ref))
    finally:
        got = (d_out.download(np.zeros(n + pad, np.uint8)), d_oo.download(np.zeros(n_rec + 1, np.int64)),
               d_perm.download(np.zeros(max(n_rec, 1), np.int32))[:n_rec], d_in.download(np.zeros(n + 1, np.uint8))[:n].tobytes())
        _resident_sort.last = got
    return got


def _gpu_sort_case(eng, name):
    blocks, n_ref = sort_cases()[name]
    data, off = bi.join(blocks)
    raw, out_off, perm, back = _resident_sort(eng, data, off, n_ref)
    if blocks:
        _same_sort(blocks, n_ref, raw[:len(data)].tobytes(), out_off, perm, name)
    assert (raw[len(data):] == 0xA5).all(), f"{name}: bytes behind d_out + n_bytes were written"
    assert back == data, f"{name}: the input changed"
    st = bsw.bamsort_last_stats(eng)
    assert (st.n_rec, st.n_bytes if blocks else 0) == (len(blocks), len(data)), name
    host = bsw.bam_sort(eng, data, off, n_ref)                     # the host form equals the resident form
    assert host[0] == raw[:len(data)].tobytes() and np.array_equal(host[2], perm), name
    if blocks:                                                     # (n_rec == 0 runs nothing: no offset is written)
        assert np.array_equal(host[1], out_off), name
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n0", "n1", "n2", "all_equal", "all_unplaced", "ties_strand", "ties_name", "three_refs_reversed",
                                  "n_ref_70000", "pos_max", "residues", "long_block"])
def test_gpu_sort_cases(eng, name):
    st = _gpu_sort_case(eng, name)
    if name in ("all_equal", "all_unplaced", "n1"):
        assert st.key_bits == 0                                   # no bit varies: stability is the whole answer
    if name == "n0":
        assert (st.key_ms, st.sort_ms, st.copy_ms) == (0, 0, 0)   # a valid call that runs nothing
    elif name != "n1":
        assert st.key_ms > 0 and st.copy_ms > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tile-1", "tile", "tile+1", "3tiles+5"])
def test_gpu_sort_total_bytes_around_the_permute_tile(eng, name):
    _gpu_sort_case(eng, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [bsw.BAMSORT_SORT_TILE + 1, 3 * bsw.BAMSORT_SORT_TILE + 5])
def test_gpu_sort_more_than_one_sort_tile(eng, n):
    _gpu_sort_case(eng, f"n{n}")


@pytest.mark.gpu
def test_gpu_sort_output_on_every_dword_phase(eng):
    """the same records behind 0..3 bytes of another record, so that every block's start moves through a dword"""
    base, n_ref = sort_cases()["residues"]
    for k in range(4):
        blocks = [bi.record(0, 0, 0, "1M", b"z" * (1 + k))] + base
        data, off = bi.join(blocks)
        raw, out_off, perm, _ = _resident_sort(eng, data, off, n_ref)
        _same_sort(blocks, n_ref, raw[:len(data)].tobytes(), out_off, perm, f"shift {k}")


@pytest.mark.gpu
def test_gpu_sort_errors_write_nothing(eng):
    untouched = lambda got, n: (got[0] == 0xA5).all() and (got[1] == -7).all() and (got[2] == -7).all()
    for tag, data, off, n_ref in _broken_sort_inputs():
        with pytest.raises(bsw.BswError, match="-34"):
            _resident_sort(eng, data, off, n_ref)
        assert untouched(_resident_sort.last, len(data)), tag
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.bam_sort(eng, data, off, n_ref)
    blocks, n_ref = sort_cases()["residues"]
    data, off = bi.join(blocks)
    with pytest.raises(bsw.BswError, match="-34"):               # out_cap < n_bytes
        _resident_sort(eng, data, off, n_ref, out_cap=len(data) - 1)
    assert untouched(_resident_sort.last, len(data))
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.bam_sort(eng, data, off, n_ref, out_cap=len(data) - 1)
    with pytest.raises(bsw.BswError, match="-22"):               # n_ref <= 0
        _resident_sort(eng, data, off, 0)
    # d_out overlapping d_bam: the same buffer; and a d_out whose room starts in front of d_bam and reaches into it
    n, n_rec = len(data), len(off) - 1
    d = hiprt.DeviceBuffer(2 * n + 64)
    half = (n + 3) // 4 * 4
    img = np.full(2 * n + 64, 0xA5, np.uint8)
    img[half:half + n] = np.frombuffer(data, np.uint8)
    d_off = hiprt.DeviceBuffer.from_array(off)
    d_oo, d_perm = hiprt.DeviceBuffer(8 * (n_rec + 1)), hiprt.DeviceBuffer(4 * n_rec)
    for out_at, cap in ((half, n), (half - 8, n), (half + 8, n), (0, half + 1)):
        d.upload(img)
        with pytest.raises(bsw.BswError, match="-22"):
            bsw.bam_sort_resident(eng, d.ptr + half, d_off.ptr, n_rec, d.ptr + out_at, cap, d_oo.ptr, d_perm.ptr, bsw.bamsort_opt(n_ref))
        assert np.array_equal(d.download(np.zeros(2 * n + 64, np.uint8)), img), (out_at, cap)
    with pytest.raises(bsw.BswError, match="-22"):               # a misaligned d_out
        bsw.bam_sort_resident(eng, d.ptr + half, d_off.ptr, n_rec, d.ptr + 1, n, d_oo.ptr, d_perm.ptr, bsw.bamsort_opt(n_ref))
    _gpu_sort_case(eng, "residues")                               # after the errors


def _device_index(eng, blocks, ref_len, bb, base=0, sorted_input=True):
    """the blocks through bsw_bgzf_resident (their virtual offsets) and bsw_bam_index_resident: (stream, voff, end_voff, bai)"""
    data, off = bi.join(blocks)
    n, n_rec = len(data), len(blocks)
    o = bsw.bgzf_opt(block_bytes=bb, base_coffset=base)
    nb = bsw.bgzf_blocks(n, o)
    d_in = hiprt.DeviceBuffer.from_array(np.frombuffer(data + b"\0", np.uint8))
    d_off = hiprt.DeviceBuffer.from_array(off)
    cap = bsw.bgzf_bound(n, o)
    d_z, d_blk, d_voff = hiprt.DeviceBuffer(cap), hiprt.DeviceBuffer(8 * (nb + 1)), hiprt.DeviceBuffer(8 * max(n_rec, 1))
    _, n_z = bsw.bgzf_resident(eng, d_in.ptr if n else 0, n, d_off.ptr if n_rec else 0, n_rec, d_z.ptr, cap, d_blk.ptr, nb + 1,
                               d_voff.ptr if n_rec else 0, o)
    stream = d_z.download(np.zeros(max(n_z, 1), np.uint8))[:n_z].tobytes()
    voff = d_voff.download(np.zeros(max(n_rec, 1), np.int64))[:n_rec]
    end_voff = (base + int(d_blk.download(np.zeros(nb + 1, np.int64))[nb])) << 16
    args = (eng, ref_len, d_in.ptr, d_off.ptr, n_rec, d_voff.ptr, end_voff)
    with pytest.raises(bsw.BswError, match="-34") as ei:         # the capacity protocol: no room says what is needed
        bsw.bam_index_resident(*args, 0, 0)
    need = ei.value.needed
    d_bai = hiprt.DeviceBuffer(need + 16)
    d_bai.upload(np.full(need + 16, 0xA5, np.uint8))
    assert bsw.bam_index_resident(*args, d_bai.ptr, need) == need
    raw = d_bai.download(np.zeros(need + 16, np.uint8))
    assert (raw[need:] == 0xA5).all(), "bytes behind d_bai + n_bytes were written"
    return stream, voff, end_voff, raw[:need].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_gpu_index_cases(eng, bb, tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for name, (blocks, ref_len) in index_cases().items():
        stream, voff, end_voff, bai = _device_index(eng, blocks, ref_len, bb, base=4096)
        assert gzip.decompress(stream) == bi.join(blocks)[0] if blocks else stream == b"", name
        assert bai == bi.build(blocks, voff, end_voff, ref_len), name
        refs, n_no_coor = bi.parse(bai)
        st = bsw.bamsort_last_stats(eng)
        assert (st.n_bins, st.n_chunks, st.n_intv, st.n_no_coor, st.bai_bytes) == (
            sum(len(r["bins"]) for r in refs), sum(len(c) for r in refs for c in r["bins"].values()),
            sum(len(r["ioffset"]) for r in refs), n_no_coor, len(bai)), name
        assert st.index_ms > 0, name
        rc, mbai, _ = model_index(exe, tmp_path, blocks, voff, end_voff, ref_len)     # the kernels and their serial model
        assert rc == 0 and mbai == bai, name
        check_queries(bai, stream, 4096, blocks, ref_len, seed=len(name))
        host = bsw.bam_index(eng, *bi.join(blocks), voff, end_voff, ref_len)           # the host form
        assert host == bai, name
        if name == "chunk_rule":
            assert len(refs[0]["bins"][4681]) == (2 if bb == 64 else 1) and len(refs[0]["bins"][585]) == 1
        if name == "levels":
            assert set(refs[0]["bins"]) == {585, 73, 9, 1, 0, 4681 + 4096}   # (the block's own bin field, 12345, is not read)
        if name == "gap":
            assert len(refs[0]["ioffset"]) == 8 and len(set(refs[0]["ioffset"][1:])) == 1
        if name == "placed_unmapped":
            assert refs[0]["pseudo"][1] == (2, 1)


@pytest.mark.gpu
def test_gpu_index_rejects_and_the_capacity_protocol(eng):
    for tag, blocks, voff, end_voff, ref_len in _broken_index_inputs():
        with pytest.raises(bsw.BswError, match="-34") as ei:
            bsw.bam_index(eng, *bi.join(blocks), voff, end_voff, ref_len, bai_cap=4096)
        assert ei.value.needed == 0, tag                          # (no capacity answer: the input is refused)
    for tag, data, off, n_ref in _broken_sort_inputs():          # everything the sort rejects in a block
        n_rec = len(off) - 1
        with pytest.raises(bsw.BswError, match="-34"):
            bsw.bam_index(eng, data, off, np.arange(n_rec, dtype=np.int64) << 16, n_rec << 16, [100] * n_ref, bai_cap=4096)
    blocks, ref_len = index_cases()["many"]
    stream, voff, end_voff, want = _device_index(eng, blocks, ref_len, 300)
    with pytest.raises(bsw.BswError, match="-34") as ei:         # one byte short, host form
        bsw.bam_index(eng, *bi.join(blocks), voff, end_voff, ref_len, bai_cap=len(want) - 1)
    assert ei.value.needed == len(want)
    assert bsw.bam_index(eng, *bi.join(blocks), voff, end_voff, ref_len, bai_cap=len(want)) == want
    assert bsw.bam_index(eng, *bi.join(blocks), voff, end_voff, ref_len) == want       # twice: the same bytes


def _pipeline_checks(eng, b, n_ref, ref_len, header, ref_names, tag):
    """b holds "bam" / "bam_off": bam_sort -> bgzf(src="sbam") -> bam_index, and everything the issue asks of the result"""
    bam, boff = b.get("bam").tobytes(), b.get("bam_off")
    unsorted = bi.split(bam, boff)
    assert b.bam_sort(n_ref) == len(bam)
    sbam, soff, perm = b.get("sbam").tobytes(), b.get("sbam_off"), b.get("bam_perm")
    blocks = bi.split(sbam, soff)
    want, wperm = bi.sort(unsorted, n_ref)
    assert np.array_equal(perm, wperm) and blocks == want, tag
    assert [unsorted[i] for i in perm] == blocks and sorted(unsorted) == sorted(blocks), tag
    keys = [(n_ref if r < 0 else r, p + 1, f & 16) for r, p, _, f in map(bi.extent, blocks)]
    assert keys == sorted(keys) and len(set(keys)) > 1, tag
    hz, _, _ = bsw.bgzf(eng, header)
    seen_chunks = set()
    for bb in (600, gz.MAX_BLOCK):
        bo = bsw.bgzf_opt(block_bytes=bb, base_coffset=len(hz), flags=bsw.BGZF_EOF)
        nb, n_z = b.bgzf(bo, src="sbam")
        z, voff, blk = b.get("bgzf").tobytes(), b.get("bgzf_voff"), b.get("bgzf_blk")
        whole = gzip.decompress(hz + z)
        assert whole == header + sbam, tag
        assert len(bp.decode(whole[len(header):], ref_names)) == len(blocks), tag
        n_bai = b.bam_index(ref_len, base_coffset=len(hz))
        bai = b.get("bai").tobytes()
        end_voff = (len(hz) + int(blk[nb])) << 16
        assert len(bai) == n_bai and bai == bi.build(blocks, voff, end_voff, ref_len), tag
        assert check_queries(bai, z, len(hz), blocks, ref_len, seed=bb, n_random=100 * len(ref_len), per_record=False) > 0, tag
        seen_chunks.add(bsw.bamsort_last_stats(eng).n_chunks)
    assert b.bgzf(bsw.bgzf_opt(block_bytes=600))[0] == -(-len(bam) // 600)        # the default source is still "bam"
    assert gzip.decompress(b.get("bgzf").tobytes()) == bam
    return seen_chunks


@pytest.mark.gpu
def test_gpu_pipeline_sorted_and_indexed_device_to_device(eng):
    """bsw_records_resident -> bsw_bam_records_resident -> bsw_bam_sort_resident -> bsw_bgzf_resident ->
    bsw_bam_index_resident on the same resident arrays"""
    s = rec_set()
    p, a = s.p, s.p.arr
    bsw.set_reference(eng, p.T)
    o = bsw.rec_opt(**s.opt)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], s.quals)
    b.put(mreg=p.mregs, minfo=p.minfo, mfirst=p.mfirst)
    b.pe_pair(p.pes, bsw.pe_opt(l_pac=p.l_pac))
    b.records(o)
    b.bam_records(o, s.names, True)
    header = bsw.bam_header(eng, o, b"@HD\tVN:1.6\tSO:coordinate\n")
    _pipeline_checks(eng, b, 1, [int(p.l_pac)], header, [s.opt["rname"]], "one reference")


@pytest.mark.gpu
def test_gpu_pipeline_sorted_and_indexed_under_three_contigs():
    eng = bsw.Engine()
    bsw.set_contigs(eng, TAB3.lens, TAB3.names)
    c = case_pe()
    res = _under_table(c)
    reads, off, lens = res.arrays[:3]
    o = bsw.rec_opt(**res.opt)
    bam, boff = bsw.bam_records(eng, res.recs, res.rec_first, res.aln, res.cigar, res.md, reads, off, lens, c.names, _quals(reads),
                                o, True)
    b = ResidentBatch(eng, reads, off, lens)
    b.put(bam=np.frombuffer(bam, np.uint8), bam_off=boff)
    header = bsw.bam_header(eng, o, b"@HD\tVN:1.6\tSO:coordinate\n")
    _pipeline_checks(eng, b, len(TAB3.lens), [int(x) for x in TAB3.lens], header, TAB3.names, "three contigs")
    assert len({bi.extent(x)[0] for x in bi.split(bam, boff)} - {-1}) > 1
    eng.close()
