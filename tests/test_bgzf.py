"""BGZF on the GPU (include/bsw_bgzf.h): bsw_bgzf* against Python's zlib and gzip as independent decoders
(tests/bgzf_py.py), and the encoder's serial model (tools/bgzf_model.cpp: the kernel's own per-strip and per-block
functions, run on the CPU).

CPU: the walker and its reference writer; the header file; the invalid-argument cases; the model over the input table;
its code lengths at the length limits; its CRC combine.  GPU: the same table through bsw_bgzf, every case twice
(determinism), through the walker and gzip.decompress, and byte for byte against the model; the capacity protocol; the
pipeline set device to device with the records' virtual offsets."""

import ctypes
import gzip
import os
import struct
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import bam_py as bp
import bgzf_py as gz
import bsw
import contigs_py as cp
import hiprt
from conftest import ROOT
from resident import ResidentBatch
from stagekit import declared, exported
from test_bam import TAB3, _lines, _quals, _under_table
from test_rec import RNAME, case_pe, rec_set

BB = gz.MAX_BLOCK
LENGTHS = {BB: (0, 1, 2, 3, 254, 255, 256, BB - 1, BB, BB + 1, 2 * BB + 7),
           600: (0, 1, 2, 3, 254, 255, 256, 599, 600, 601, 1207)}
RUNS = (3, 4, 257, 258, 259, 260, 516)
_inputs = {}


def _rng(seed):
    return np.random.default_rng(seed)


def _fib_bytes():
    """bytes over 24 values, shuffled, one block: Fibonacci frequencies 1, 1, 2 .. 17711 for 22 of them (46,367 bytes: 24
    Fibonacci numbers are more than a block), the rest on two more.  The unlimited Huffman tree is over 20 deep."""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    f += [10000, BB - sum(f) - 10000]
    a = np.concatenate([np.full(n, 10 + 9 * i, np.uint8) for i, n in enumerate(f)])
    assert len(a) == BB and len(f) == 24
    _rng(11).shuffle(a)
    return a.tobytes()


def inputs():
    """name -> (bytes, block_bytes): the issue's table but the length series (LENGTHS)"""
    if not _inputs:
        r = _rng(7)
        rnd = lambda n: r.integers(0, 256, n, dtype=np.uint8).tobytes()
        runs = rnd(40)
        for k in RUNS:
            runs += b"z" * k + rnd(41)
        _inputs["runs"] = (runs, BB)
        _inputs["runs600"] = (runs, 600)
        _inputs["ff"] = (b"\xff" * BB, BB)
        copy = rnd(20000)
        for d in (32768, 32769, 40000):
            _inputs[f"dist{d}"] = (copy + rnd(d - 20000) + copy, BB)
        _inputs["random"] = (rnd(BB), BB)
        _inputs["four"] = (r.choice(np.array([3, 17, 99, 200], dtype=np.uint8), BB).tobytes(), BB)
        _inputs["a"] = (b"a", BB)
        _inputs["ab"] = (b"ab", BB)
        _inputs["distinct300"] = (bytes(range(256)) + bytes(range(0, 88, 2)), BB)
        _inputs["fib24"] = (_fib_bytes(), BB)
    return _inputs


def _length_data(n):
    return _rng(n).integers(0, 8, n, dtype=np.uint8).tobytes()


def _check_stream(out, data, block_bytes, eof, forms=None, tag=""):
    """walker + gzip.decompress + the cuts; returns the data blocks"""
    blocks = gz.data_blocks(gz.walk(out, forms=forms, eof=eof))
    if out:
        assert gzip.decompress(out) == data, tag
    else:
        assert data == b"" and not eof, tag
    assert [len(b.data) for b in blocks] == [min(block_bytes, len(data) - at) for at in range(0, len(data), block_bytes)], tag
    return blocks


# ---------------------------------------------------------------- CPU: the walker tests itself
def test_walker_accepts_the_reference_writer():
    for name, (data, bb) in inputs().items():
        for level in (1, 0):
            _check_stream(gz.write(data, bb, level, eof=True), data, bb, True, tag=name)
    for bb, lens in LENGTHS.items():
        for n in lens:
            for eof in (False, True):
                _check_stream(gz.write(_length_data(n), bb, 1, eof), _length_data(n), bb, eof, tag=f"{n} at {bb}")
    assert gz.write(b"", eof=True) == gz.EOF and gz.write(b"") == b""
    stored = gz.write(inputs()["random"][0], level=0)
    assert len(stored) == BB + 31 and gz.walk(stored, forms=(1, 0, 0))[0].btype == gz.STORED


def test_walker_rejects_broken_streams():
    data = _length_data(1500)
    good = gz.write(data, 600, eof=True)
    blocks = gz.walk(good, eof=True)
    assert len(blocks) == 4
    b1 = blocks[1]
    crc = bytearray(good)
    crc[b1.off + b1.size - 8] ^= 1                               # a flipped CRC byte
    with pytest.raises(ValueError, match="CRC32"):
        gz.walk(bytes(crc))
    bsize = bytearray(good)
    bsize[b1.off + 16] ^= 4                                      # a wrong BSIZE
    with pytest.raises(ValueError, match="BSIZE|header"):
        gz.walk(bytes(bsize))
    noextra = bytearray(good)                                    # a plain gzip member: no extra field
    plain = gzip.compress(data[:600], mtime=0)
    with pytest.raises(ValueError, match="header"):
        gz.walk(plain)
    noextra[b1.off + 3] = 0
    with pytest.raises(ValueError, match="header|BSIZE"):
        gz.walk(bytes(noextra))
    with pytest.raises(ValueError, match="EOF"):
        gz.walk(good[:-28], eof=True)
    with pytest.raises(ValueError, match="EOF"):
        gz.walk(good, eof=False)
    with pytest.raises(ValueError, match="block types"):
        gz.walk(gz.write(data, 600, level=0), forms=(0, 0, 3))
    isize = bytearray(good)
    isize[b1.off + b1.size - 4] ^= 1
    with pytest.raises(ValueError, match="ISIZE"):
        gz.walk(bytes(isize))


# ---------------------------------------------------------------- CPU: the header file
def test_library_exports_the_bgzf_header():
    assert declared("bsw_bgzf.h") == set(bsw.BGZF_SYMBOLS)
    assert declared("bsw_bgzf.h") <= exported(), declared("bsw_bgzf.h") - exported()
    others = (set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS) |
              set(bsw.MATESW_SYMBOLS) | set(bsw.REC_SYMBOLS) | set(bsw.CONTIGS_SYMBOLS) | set(bsw.BAM_SYMBOLS))
    assert not set(bsw.BGZF_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_bgzf_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_bgzf.h"\n'
                   f"{sa}(sizeof(bsw_bgzf_opt_t) == 24 && offsetof(bsw_bgzf_opt_t, flags) == 8 && offsetof(bsw_bgzf_opt_t, base_coffset) == 16, \"opt\");\n"
                   f"{sa}(sizeof(bsw_bgzf_stats_t) == 40 && offsetof(bsw_bgzf_stats_t, n_in) == 16 && offsetof(bsw_bgzf_stats_t, deflate_ms) == 32 && offsetof(bsw_bgzf_stats_t, pack_ms) == 36, \"stats\");\n"
                   f"{sa}(BSW_BGZF_API == 1 && BSW_ABI_VERSION == 8 && BSW_BGZF_MAX_BLOCK == 65280 && BSW_BGZF_EOF == 1, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.BgzfOpt) == 24 and bsw.BgzfOpt.base_coffset.offset == 16
    assert ctypes.sizeof(bsw.BgzfStats) == 40 and bsw.BgzfStats.n_in.offset == 16 and bsw.BgzfStats.pack_ms.offset == 36
    o = bsw.bgzf_opt()
    assert (o.level, o.block_bytes, o.flags, o.base_coffset) == (1, 0xff00, 0, 0)


def test_resident_batch_knows_the_bgzf_buffers():
    import resident
    assert resident._row("bgzf") == (np.dtype(np.uint8), (), "bgzf")
    assert resident._row("bgzf_blk") == (np.dtype(np.int64), (), "bgzf_blk")
    assert resident._row("bgzf_voff") == (np.dtype(np.int64), (), "bgzf_voff")
    assert not set(resident.BGZF_LAYOUT) & (set(resident.LAYOUT) | set(resident.BAM_LAYOUT))
    assert callable(ResidentBatch.bgzf)


def _lib_calls(ctx, o, n_in=8, n_rec=1, out_cap=64, blk_cap=4, inp=True, out=True, blk=True, rec=True, voff=True, nb=True,
               nby=True):
    Lb = bsw.hip_lib()
    P, B = bsw._ptr, ctypes.byref
    a_in, a_rec = np.zeros(8, np.uint8), np.zeros(4, np.int64)
    a_out, a_blk, a_voff = np.zeros(72, np.uint8), np.zeros(8, np.int64), np.zeros(4, np.int64)
    n_blocks, n_bytes = ctypes.c_int32(0), ctypes.c_int64(0)
    args = (ctx, B(o) if o is not None else None, P(a_in) if inp else None, n_in, P(a_rec) if rec else None, n_rec,
            P(a_out) if out else None, out_cap, P(a_blk) if blk else None, blk_cap,
            P(a_voff) if voff else None, B(n_blocks) if nb else None, B(n_bytes) if nby else None)
    host = Lb.bsw_bgzf(*args)
    return (host, Lb.bsw_bgzf_resident(*args, None)), n_blocks.value


def test_invalid_arguments_need_no_device():
    Lb = bsw.hip_lib()
    assert Lb.bsw_bgzf_last_stats(None, None) == -22
    Lb.bsw_bgzf_opt_default(None)                                # (ignored)
    fake = ctypes.c_void_p(1)                                    # never dereferenced: the checks come first
    good = bsw.bgzf_opt()
    inval = (-22, -22)
    assert _lib_calls(None, good)[0] == inval
    assert _lib_calls(fake, None)[0] == inval
    for kw in (dict(n_in=-1), dict(n_rec=-1), dict(out_cap=-1), dict(blk_cap=-1), dict(inp=False), dict(out=False),
               dict(blk=False), dict(rec=False), dict(voff=False), dict(nb=False), dict(nby=False)):
        assert _lib_calls(fake, good, **kw)[0] == inval, kw
    for bad in (dict(block_bytes=0), dict(block_bytes=0xff01), dict(block_bytes=-5), dict(level=2), dict(level=-1),
                dict(flags=2), dict(flags=0x80000001)):
        assert _lib_calls(fake, bsw.bgzf_opt(**bad))[0] == inval, bad
    # a short blk_cap is a capacity, found on the host as well: -34 with the blocks needed
    rc, nblk = _lib_calls(fake, bsw.bgzf_opt(block_bytes=3), blk_cap=3)
    assert rc == (-34, -34) and nblk == 3


# ---------------------------------------------------------------- CPU: the serial model
_model = {}


def model_bin(tmp_path_factory):
    """tools/bgzf_model.cpp, compiled once"""
    if not _model:
        exe = tmp_path_factory.mktemp("bgzf") / "bgzf_model"
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "bwa-mem2-arm_amd", "csrc"),
                            os.path.join(ROOT, "tools", "bgzf_model.cpp"), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _model["x"] = str(exe)
    return _model["x"]


def model_stream(exe, tmp, data, block_bytes=BB, level=1, eof=False):
    """the model's stream for these bytes and its (n_stored, n_fixed, n_dynamic)"""
    src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, "--block-bytes", str(block_bytes), "--level", str(level)] + (["--eof"] if eof else []) +
                       [src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    assert w[0::2] == ["blocks", "stored", "fixed", "dynamic", "in", "out"]
    v = [int(x) for x in w[1::2]]
    out = open(dst, "rb").read()
    assert v[0] == v[1] + v[2] + v[3] and v[4] == len(data) and v[5] == len(out)
    return out, tuple(v[1:4])


# what the table's inputs have to give, whoever encodes them (the model on the CPU, the kernel on the GPU)
def _check_table_case(name, data, out, forms):
    if name == "ff":                                             # 256 strips of one literal-or-match each
        assert len(out) < 0.02 * len(data), len(out)
    if name == "random":
        assert forms == (1, 0, 0) and len(out) == len(data) + 31
    if name == "four":
        # a Huffman code over 4 literals and end-of-block: 2.25 bits a byte = 0.283; zlib level 1 0.333, zlib's best
        # with fixed codes 0.425: 0.40 is out of reach of fixed codes
        assert forms == (0, 0, 1) and len(out) < 0.40 * len(data), len(out)
    if name == "fib24":
        assert forms == (0, 0, 1)


def test_model_over_the_input_table(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for name, (data, bb) in inputs().items():
        out, forms = model_stream(exe, tmp_path, data, bb)
        _check_stream(out, data, bb, False, forms, name)
        _check_table_case(name, data, out, forms)
        again, _ = model_stream(exe, tmp_path, data, bb)
        assert again == out, name
        out0, forms0 = model_stream(exe, tmp_path, data, bb, level=0, eof=True)
        blocks = _check_stream(out0, data, bb, True, forms0, name + " level 0")
        assert forms0 == (len(blocks), 0, 0) and len(out0) == len(data) + 31 * len(blocks) + 28


def test_model_lengths_cuts_and_the_empty_call(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    for bb, lens in LENGTHS.items():
        for n in lens:
            data = _length_data(n)
            for eof in (False, True):
                out, forms = model_stream(exe, tmp_path, data, bb, eof=eof)
                _check_stream(out, data, bb, eof, forms, f"{n} bytes at {bb}")
                if n == 0:
                    assert out == (gz.EOF if eof else b"") and forms == (0, 0, 0)


def _kraft(lens):
    return sum(Fraction(1, 2 ** x) for x in lens if x)


def _model_lengths(exe, limit, freq):
    r = subprocess.run([exe, "--lengths", str(limit)] + [str(f) for f in freq], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lens = [int(x) for x in r.stdout.split()]
    assert len(lens) == len(freq) and all((x > 0) == (f > 0) for x, f in zip(lens, freq))
    return lens


def test_model_code_lengths_at_the_limits(tmp_path_factory):
    exe = model_bin(tmp_path_factory)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for limit, freq in ((15, fib), (7, fib[:19]), (15, [5, 9]), (15, [1] * 286), (15, [0, 0, 3, 0, 1, 0, 7]),
                        (7, [0, 4, 0, 0, 9, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 30])):
        lens = _model_lengths(exe, limit, freq)
        assert max(lens) <= limit and _kraft(lens) == 1, (limit, lens)
        # a rarer symbol never has the shorter code
        used = sorted((f, -x) for f, x in zip(freq, lens) if f)
        assert [x for _, x in used] == sorted(x for _, x in used), (limit, lens)
    assert _model_lengths(exe, 15, [5, 9]) == [1, 1]
    assert sorted(set(_model_lengths(exe, 15, [1] * 286))) == [8, 9]
    # one used symbol: the one-code case, a single code of one bit
    assert _model_lengths(exe, 15, [0, 0, 7, 0]) == [0, 0, 1, 0]
    assert _model_lengths(exe, 15, [3]) == [1]
    # within the limit the lengths are Huffman's: the cost equals that of a tree built here
    import heapq
    freq = [40, 30, 12, 9, 5, 2, 1, 1]
    h = list(freq)
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    assert sum(f * x for f, x in zip(freq, _model_lengths(exe, 15, freq))) == cost


def test_model_crc_combine_is_zlibs(tmp_path_factory, tmp_path):
    exe = model_bin(tmp_path_factory)
    data = _rng(3).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    src = tmp_path / "crc"
    for total in (0, 1, 255, 256, 1000):
        src.write_bytes(data[:total])
        for k in (0, 1, 254, 255, 256):
            if k > total:
                continue
            r = subprocess.run([exe, "--crc-split", str(k), str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert int(r.stdout, 16) == zlib.crc32(data[:total]), (total, k)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng():
    e = bsw.Engine()
    yield e
    e.close()


def _gpu(eng, data, tag, **kw):
    """bsw_bgzf twice (byte-equal), through the walker and gzip.decompress; the stats"""
    o = bsw.bgzf_opt(**kw)
    out, blk, _ = bsw.bgzf(eng, data, o)
    st = bsw.bgzf_last_stats(eng)
    forms = (st.n_stored, st.n_fixed, st.n_dynamic)
    eof = bool(o.flags & bsw.BGZF_EOF)
    blocks = _check_stream(out, data, o.block_bytes, eof, forms, tag)
    assert list(blk) == [b.off for b in blocks] + [len(out) - (28 if eof else 0)], tag
    assert (st.n_blocks, st.n_in, st.n_out) == (len(blocks), len(data), len(out)), tag
    assert st.deflate_ms > 0 and (st.pack_ms > 0) == (len(out) > 0), tag
    if o.level == 0:
        assert forms == (len(blocks), 0, 0) and len(out) == len(data) + 31 * len(blocks) + (28 if eof else 0), tag
    again, blk2, _ = bsw.bgzf(eng, data, o)
    assert again == out and np.array_equal(blk, blk2), f"{tag}: two runs differ"
    return out, forms


@pytest.mark.gpu
@pytest.mark.parametrize("bb", sorted(LENGTHS))
def test_gpu_lengths_cuts_and_the_empty_call(eng, bb):
    for n in LENGTHS[bb]:
        data = _length_data(n)
        for flags in (0, bsw.BGZF_EOF):
            out, forms = _gpu(eng, data, f"{n} bytes at {bb}, flags {flags}", block_bytes=bb, flags=flags)
            if n == 0:
                assert out == (gz.EOF if flags else b"") and forms == (0, 0, 0)
    _gpu(eng, _length_data(LENGTHS[bb][-1]), f"level 0 at {bb}", block_bytes=bb, level=0, flags=bsw.BGZF_EOF)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["runs", "runs600", "ff", "dist32768", "dist32769", "dist40000", "random", "four", "a", "ab",
                                  "distinct300", "fib24"])
def test_gpu_input_table(eng, name, tmp_path_factory, tmp_path):
    data, bb = inputs()[name]
    out, forms = _gpu(eng, data, name, block_bytes=bb)
    print(f"{name}: {len(data)} -> {len(out)} bytes, (stored, fixed, dynamic) {forms}")
    _check_table_case(name, data, out, forms)
    # the kernel and its serial model give the same bytes
    want, wforms = model_stream(model_bin(tmp_path_factory), tmp_path, data, bb)
    assert forms == wforms and out == want, name
    _gpu(eng, data, name + " level 0", block_bytes=bb, level=0)


@pytest.mark.gpu
def test_gpu_capacity_protocol_and_no_write_past_the_end(eng):
    data = _length_data(1207) + inputs()["runs"][0]
    o = bsw.bgzf_opt(block_bytes=600, flags=bsw.BGZF_EOF)
    want, wblk, _ = bsw.bgzf(eng, data, o)
    n, nb = len(want), len(wblk) - 1
    assert nb == -(-len(data) // 600)
    # host form: one byte short says what is needed and leaves the block starts; a short blk_cap says the blocks
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.bgzf(eng, data, o, out_cap=n - 1)
    assert ei.value.needed == n and np.array_equal(ei.value.blk_off[:nb + 1], wblk)
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.bgzf(eng, data, o, blk_cap=nb)
    assert ei.value.n_blocks == nb
    assert bsw.bgzf(eng, data, o, out_cap=n)[0] == want
    # resident form, a sentinel behind the end; the output starts on every byte of a dword in turn (block starts do)
    d_in = hiprt.DeviceBuffer.from_array(np.frombuffer(data, np.uint8))
    d_out, d_blk = hiprt.DeviceBuffer(n + 16), hiprt.DeviceBuffer(8 * (nb + 1))
    fill = np.full(n + 16, 0xA5, np.uint8)
    for cap in (n + 16, n):
        d_out.upload(fill)
        assert bsw.bgzf_resident(eng, d_in.ptr, len(data), 0, 0, d_out.ptr, cap, d_blk.ptr, nb + 1, 0, o) == (nb, n)
        raw = d_out.download(np.zeros(n + 16, np.uint8))
        assert raw[:n].tobytes() == want and (raw[n:] == 0xA5).all()
        assert np.array_equal(d_blk.download(np.zeros(nb + 1, np.int64)), wblk)
    assert {int(x) & 3 for x in wblk} == {0, 1, 2, 3}
    d_out.upload(fill)
    d_blk.upload(np.zeros(nb + 1, np.int64))
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.bgzf_resident(eng, d_in.ptr, len(data), 0, 0, d_out.ptr, n - 1, d_blk.ptr, nb + 1, 0, o)
    assert ei.value.needed == n and (d_out.download(np.zeros(n + 16, np.uint8)) == 0xA5).all()     # nothing written
    assert np.array_equal(d_blk.download(np.zeros(nb + 1, np.int64)), wblk)
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.bgzf_resident(eng, d_in.ptr, len(data), 0, 0, d_out.ptr, n, d_blk.ptr, nb, 0, o)
    assert ei.value.n_blocks == nb
    with pytest.raises(bsw.BswError, match="-22"):                # a misaligned output
        bsw.bgzf_resident(eng, d_in.ptr, len(data), 0, 0, d_out.ptr + 1, n, d_blk.ptr, nb + 1, 0, o)
    # a record offset outside the input
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.bgzf(eng, data, o, rec_off=np.array([0, len(data) + 1, len(data)], np.int64))
    assert bsw.bgzf(eng, data, o)[0] == want                     # after the errors


def _check_voffs(stream, base, bam, boff, voff, bb):
    """every record's virtual offset names a block of the stream and lands on the record's block_size field; returns
    (records that start on a cut, records that straddle one)"""
    blocks = gz.data_blocks(gz.walk(stream))
    starts = {b.off for b in blocks}
    on_cut = straddle = 0
    assert len(voff) == len(boff) - 1
    for i, v in enumerate(voff):
        assert (int(v) >> 16) - base in starts, i
        k, u = gz.voff_lands(stream, blocks, v, base)
        assert k * bb + u == boff[i], i
        field = (blocks[k].data[u:] + (blocks[k + 1].data if k + 1 < len(blocks) else b""))[:4]
        assert struct.unpack("<i", field)[0] == boff[i + 1] - boff[i] - 4, i
        assert field == bam[boff[i]:boff[i] + 4]
        on_cut += u == 0 and i > 0
        straddle += boff[i] // bb != (boff[i + 1] - 1) // bb
    return on_cut, straddle


@pytest.mark.gpu
def test_gpu_pipeline_set_device_to_device_with_virtual_offsets(eng):
    """bsw_pe_pair_resident -> bsw_records_resident -> bsw_bam_records_resident -> bsw_bgzf_resident on the same resident
    arrays, the header block compressed by the host form in front"""
    s = rec_set()
    p, a = s.p, s.p.arr
    bsw.set_reference(eng, p.T)
    o = bsw.rec_opt(**s.opt)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], s.quals)
    b.put(mreg=p.mregs, minfo=p.minfo, mfirst=p.mfirst)
    b.pe_pair(p.pes, bsw.pe_opt(l_pac=p.l_pac))
    b.records(o)
    n_bam = b.bam_records(o, s.names, True)
    bam, boff = b.get("bam").tobytes(), b.get("bam_off")
    assert len(bam) == n_bam and bp.decode(bam, [RNAME]) == _lines(s.text)
    header = bsw.bam_header(eng, o, b"@HD\tVN:1.6\n")
    hz, hblk, _ = bsw.bgzf(eng, header)
    assert len(hblk) == 2
    on_cut = straddle = 0
    # 600; and a cut on which the third record starts
    for bb, base in ((600, 0), (600, len(hz)), (int(boff[2]), len(hz))):
        assert 1 <= bb <= BB
        bo = bsw.bgzf_opt(block_bytes=bb, base_coffset=base, flags=bsw.BGZF_EOF)
        nb, n_bytes = b.bgzf(bo)
        z, blk, voff = b.get("bgzf").tobytes(), b.get("bgzf_blk"), b.get("bgzf_voff")
        st = bsw.bgzf_last_stats(eng)
        assert nb == -(-len(bam) // bb) and len(z) == n_bytes and len(blk) == nb + 1 and blk[nb] == n_bytes - 28
        blocks = _check_stream(z, bam, bb, True, (st.n_stored, st.n_fixed, st.n_dynamic), f"pipeline at {bb}")
        assert list(blk[:-1]) == [x.off for x in blocks]
        whole = gzip.decompress(hz + z)
        assert whole == header + bam
        assert bp.decode(whole[len(header):], [RNAME]) == _lines(s.text)
        c, t = _check_voffs(z, base, bam, boff, voff, bb)
        on_cut, straddle = on_cut + c, straddle + t
        nb2, _ = b.bgzf(bo)                                      # determinism, device to device
        assert b.get("bgzf").tobytes() == z and np.array_equal(b.get("bgzf_voff"), voff)
    assert on_cut > 0 and straddle > 0


@pytest.mark.gpu
def test_gpu_virtual_offsets_under_three_contigs():
    """the same chain under TAB3's contig table: bsw_bam_records -> bsw_bgzf with the blocks' offsets, behind the table's
    header block"""
    eng = bsw.Engine()
    bsw.set_contigs(eng, TAB3.lens, TAB3.names)
    c = case_pe()
    res = _under_table(c)
    reads, off, lens = res.arrays[:3]
    q = _quals(reads)
    o = bsw.rec_opt(**res.opt)
    bam, boff = bsw.bam_records(eng, res.recs, res.rec_first, res.aln, res.cigar, res.md, reads, off, lens, c.names, q, o, True)
    text, _ = cp.sam_text(TAB3, res, reads, off, lens, c.names, q, res.opt, True)
    header = bsw.bam_header(eng, o, b"@HD\tVN:1.6\n")
    assert header == bp.header(res.opt, b"@HD\tVN:1.6\n", TAB3)
    hz, _, _ = bsw.bgzf(eng, header)
    bb = int(boff[1])                                            # the second record starts on a cut
    z, blk, voff = bsw.bgzf(eng, bam, bsw.bgzf_opt(block_bytes=bb, base_coffset=len(hz), flags=bsw.BGZF_EOF), rec_off=boff)
    whole = gzip.decompress(hz + z)
    assert whole == header + bam and bp.decode(whole[len(header):], TAB3.names) == _lines(text)
    on_cut, _ = _check_voffs(z, len(hz), bam, boff, voff, bb)
    assert on_cut > 0
    eng.close()
