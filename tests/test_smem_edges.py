"""SMEM seeding edge by edge (csrc/bsw_fmi.hip smem_kernel): the branches and
bounds of the walk that tests/test_fmi.py's random 151 / 250-bp reads do not reach.

  1. min_seed_len at kt - 1 .. kt + 2 (kt = the k-mer table's depth): the switch between stored and
     virtual entries (smem1's `keep_len >= kt`, seed_strategy1's `min_len > kt`) at equality, with
     the counts-only table on and off (BSW_FMI_STAB=0, the form taken when its allocation fails).
  2. reads of 1 .. 40 bases and an N at each of the first 21 offsets: KPre::init's clamps.
  3. table depth 15 (the 3 Gb default; BSW_FMI_KTAB=16 is clamped to it) and 13 against the oracle.
  4. reads of 32,766 / 32,767 bases: 15-bit ends of the packed entries, the switch to 32-B ones.
  5. chunked launches (BSW_SMEM_SCRATCH_MB=1): the n0 > 0 path, a last chunk shorter than a wave.
  6. a read longer than max_len through the device API.

Every GPU test compares Fmi.collect_intv (or the device API) with oracle.FmiRef.collect_intv for
exact equality of the counts and of every interval of every read.  Each input family has a CPU-only
test_inputs_* companion that proves from the oracle alone that the inputs reach what they claim.
The oracle's outputs are computed once per (family, options) and shared.
"""
import ctypes
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import bsw
import oracle
from test_fmi import _compare, _long_runs_ref, repetitive_ref, sample_reads

gpu = pytest.mark.gpu

WIDE = bsw.FMI_GPU_BUILD | bsw.FMI_WIDE
FORMS = {"narrow": 0, "wide_packed": WIDE, "wide_plain": WIDE | bsw.FMI_PLAIN_ENT}
BSW_MAX_LEN = 32767
E_RANGE = -34


def _batch(rd):
    """(reads, off, len) of a list of reads"""
    lens = np.array([len(r) for r in rd], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return np.concatenate(rd).astype(np.uint8), off, lens


def _spans(out, cnt, i):
    v = out[i, :cnt[i]]["info"]
    return (v >> np.uint64(32)).astype(np.int64), (v & np.uint64(0xffffffff)).astype(np.int64)


def _ents(kt):
    return (4 ** (kt + 1) - 4) // 3


_base_bytes = {}


def _build(ref, flags, kt, monkeypatch, stab=True, ask=None):
    """the index of ref with a kt-level k-mer table (BSW_FMI_KTAB=ask, kt when None), the depth
    checked through info().device_bytes against a BSW_FMI_KTAB=0 build of the same reference and
    flags: 16 B per entry, and 4 B more with the counts-only copy"""
    ask = kt if ask is None else ask
    key = (ref.tobytes(), flags)
    if key not in _base_bytes:
        monkeypatch.setenv("BSW_FMI_KTAB", "0")
        f0 = bsw.Fmi(ref, flags=flags)
        _base_bytes[key] = f0.info().device_bytes
        f0.close()
    monkeypatch.setenv("BSW_FMI_KTAB", str(ask))
    if stab:
        monkeypatch.delenv("BSW_FMI_STAB", raising=False)
    else:
        monkeypatch.setenv("BSW_FMI_STAB", "0")
    f = bsw.Fmi(ref, flags=flags)
    assert f.info().device_bytes - _base_bytes[key] == _ents(kt) * (20 if stab else 16), (ask, kt, stab)
    return f


# ------------------------------------------------------------------ family 1: depth boundaries

CAP1 = 1024


@functools.lru_cache(maxsize=None)
def _ref60():
    ref = _long_runs_ref(60_000, 11)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _oref60():
    return oracle.FmiRef(_ref60())


@functools.lru_cache(maxsize=None)
def _reads1(n=1500):
    return sample_reads(_ref60(), n, 151, 13, p_n=0.01)


@functools.lru_cache(maxsize=None)
def _want1(msl, pass3, n=1500, split_width=50):
    kw = dict(min_seed_len=msl, split_width=split_width)
    if not pass3:
        kw["max_mem_intv"] = 0
    out, cnt = _oref60().collect_intv(*_reads1(n), cap=CAP1, opt=oracle.mem_opt(**kw), nthreads=8)
    out.setflags(write=False)
    cnt.setflags(write=False)
    return kw, out, cnt


def test_inputs_depth_boundaries():
    """At every min_seed_len of 4 .. 9 (kt - 1 .. kt + 2 for kt = 5, 7) the oracle's outputs hold
    intervals of length exactly min_seed_len and min_seed_len + 1 -- the lengths on either side of
    the stored / virtual switch -- with and without pass 3 (the fewest: 47 of length 5 at
    min_seed_len 5 and 54 of length 4 at 4, where nearly every 4- or 5-mer still extends; 150 to
    60,000 elsewhere), and no read reaches the cap (the largest count, at min_seed_len 4, is 682)."""
    reads, off, lens = _reads1()
    for msl in range(4, 10):
        for pass3 in (True, False):
            _, out, cnt = _want1(msl, pass3)
            assert cnt.max() < CAP1
            ln = np.concatenate([np.subtract(*_spans(out, cnt, i)[::-1]) for i in range(len(lens))])
            assert ln.min() >= msl
            n0, n1 = int((ln == msl).sum()), int((ln == msl + 1).sum())
            print(f"min_seed_len {msl} pass3 {pass3}: max count {cnt.max()}, length k {n0}, k + 1 {n1}")
            assert n0 >= 30 and n1 >= 30, (msl, pass3, n0, n1)
    assert _want1(4, True)[2].max() == 682


@gpu
@pytest.mark.parametrize("text", [True, False], ids=["text_mode", "blocks_only"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("stab", [True, False], ids=["stab", "stab_off"])
@pytest.mark.parametrize("kt", [5, 7])
def test_gpu_min_seed_len_at_table_depth(kt, stab, form, text, monkeypatch):
    """min_seed_len = kt - 1, kt, kt + 1, kt + 2: a length-kt entry is a mask bit only when nothing
    that short can be output; counts-only loads only below the shortest output."""
    f = _build(_ref60(), FORMS[form] | (0 if text else bsw.FMI_NO_TEXT), kt, monkeypatch, stab)
    reads, off, lens = _reads1()
    for msl in (kt - 1, kt, kt + 1, kt + 2):
        for pass3 in (True, False):
            kw, o_out, o_cnt = _want1(msl, pass3)
            assert o_cnt.max() < CAP1
            g_out, g_cnt = f.collect_intv(reads, off, lens, cap=CAP1, opt=bsw.mem_opt(**kw))
            _compare(o_out, o_cnt, g_out, g_cnt)
    f.close()


# ------------------------------------------------------------------ family 2: short reads, N offsets

CAP2 = 256
MSL2 = (1, 3, 7, 8)


@functools.lru_cache(maxsize=None)
def _short_reads():
    """320 reads: every length 1 .. 40 x 8, cut from the reference without substitutions, every
    other one from the reverse strand, two of each eight with one N; 21 reads of 40 bases with an
    N at offset 0 .. 20; a single base, two bases, and `N A`.  Returns (reads, off, len)."""
    ref = _ref60()
    rng = np.random.default_rng(29)
    rd = []
    for L in range(1, 41):
        for j in range(8):
            p = int(rng.integers(0, len(ref) - L))
            r = ref[p:p + L].copy()
            if j & 1:
                r = (3 - r[::-1]).astype(np.uint8)
            if j >= 6:
                r[int(rng.integers(0, L))] = 4
            rd.append(r)
    for p in range(21):
        r = ref[7000 + 50 * p:7040 + 50 * p].copy()
        r[p] = 4
        rd.append(r)
    rd += [np.array([1], np.uint8), np.array([3, 0], np.uint8), np.array([4, 0], np.uint8)]
    return _batch(rd)


@functools.lru_cache(maxsize=None)
def _want2(msl):
    out, cnt = _oref60().collect_intv(*_short_reads(), cap=CAP2, opt=oracle.mem_opt(min_seed_len=msl))
    out.setflags(write=False)
    cnt.setflags(write=False)
    return out, cnt


def test_inputs_short_reads():
    """At least 250 of the 320 short reads produce intervals at every min_seed_len used, the reads
    start at every offset mod 4 (KPre::init reads aligned dwords and shifts), every N-offset read
    but the one whose N leaves fewer than min_seed_len bases produces some, and no count reaches
    the cap."""
    reads, off, lens = _short_reads()
    assert len(lens) == 344 and sorted(set(lens[:320])) == list(range(1, 41))
    assert set(int(o) % 4 for o in off) == {0, 1, 2, 3}
    assert [int(np.nonzero(reads[off[320 + p]:off[320 + p] + 40] == 4)[0][0]) for p in range(21)] == list(range(21))
    for msl in MSL2:
        out, cnt = _want2(msl)
        assert cnt.max() < CAP2
        # reads shorter than min_seed_len cannot produce anything: 8 reads per length
        some = int((cnt[:320] > 0).sum())
        print(f"min_seed_len {msl}: {some} of 320 short reads with output, max count {cnt.max()}")
        assert some >= 250 and some <= 8 * (41 - msl)
        assert (cnt[320:341] > 0).all()
    assert _want2(1)[1][341] > 0 and _want2(1)[1][342] > 0 and _want2(1)[1][343] > 0


@gpu
@pytest.mark.parametrize("form", ["narrow", "wide_packed"])
def test_gpu_short_reads_and_n_offsets(form, monkeypatch):
    f = _build(_ref60(), FORMS[form], 7, monkeypatch)
    reads, off, lens = _short_reads()
    for msl in MSL2:
        o_out, o_cnt = _want2(msl)
        assert o_cnt.max() < CAP2
        g_out, g_cnt = f.collect_intv(reads, off, lens, cap=CAP2, opt=bsw.mem_opt(min_seed_len=msl))
        _compare(o_out, o_cnt, g_out, g_cnt)
    f.close()


# ------------------------------------------------------------------ family 3: depth 15 and the clamp

MSL3 = (14, 15, 16, 19)


@functools.lru_cache(maxsize=None)
def _want3(msl):
    return _want1(msl, True, split_width=10)


def test_inputs_deep_tables():
    """Reads of family 1 at min_seed_len 14, 15, 16 and 19 (kt - 1, kt, kt + 1 for 15 levels; past
    both depths): outputs of length exactly min_seed_len and min_seed_len + 1 exist at each, and
    four reads in five have an output, i.e. a match that ran past KPre's 16-base register window."""
    reads, off, lens = _reads1()
    for msl in MSL3:
        _, out, cnt = _want3(msl)
        assert cnt.max() < CAP1
        ln = np.concatenate([np.subtract(*_spans(out, cnt, i)[::-1]) for i in range(len(lens))])
        n0, n1 = int((ln == msl).sum()), int((ln == msl + 1).sum())
        print(f"min_seed_len {msl}: max count {cnt.max()}, length k {n0}, k + 1 {n1}, reads with output "
              f"{int((cnt > 0).sum())}")
        assert n0 > 0 and n1 > 0 and (cnt > 0).sum() > 1200


@gpu
@pytest.mark.parametrize("form,ask,kt", [("wide_packed", 16, 15), ("narrow", 13, 13)])
def test_gpu_deep_tables_equal_oracle(form, ask, kt, monkeypatch):
    """BSW_FMI_KTAB=16 builds 15 levels (the clamp; 22.9 GB of entries + 5.7 GB of counts), the
    depth a 3 Gb genome runs at: KPre's 16-base window has one base to spare and the masks use
    their highest legal bit.  Narrow at 13.  == the oracle at min_seed_len 14, 15, 16, 19.
    Measured on an MI355X: the 15 levels over this 60 kb (cache-resident) index build in 0.13 s and
    the whole wide case takes 0.20 s (narrow at 13: 0.01 s and 0.07 s), so the wide case stays at 15."""
    t = time.perf_counter()
    f = _build(_ref60(), FORMS[form], kt, monkeypatch, ask=ask)
    print(f"{form}: building {kt} levels (and the table-less index before it) took {time.perf_counter() - t:.2f} s")
    reads, off, lens = _reads1()
    for msl in MSL3:
        kw, o_out, o_cnt = _want3(msl)
        assert o_cnt.max() < CAP1
        g_out, g_cnt = f.collect_intv(reads, off, lens, cap=CAP1, opt=bsw.mem_opt(**kw))
        _compare(o_out, o_cnt, g_out, g_cnt)
    f.close()


# ------------------------------------------------------------------ family 4: 32K reads

CAP4 = 8192


@functools.lru_cache(maxsize=None)
def _ref120():
    ref = repetitive_ref(120_000, 23)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _oref120():
    return oracle.FmiRef(_ref120())


def _long_read(ref, L, seed):
    """L bases of the reference with 2% substitutions and 0.1% N"""
    rng = np.random.default_rng(seed)
    p = int(rng.integers(0, len(ref) - L))
    r = ref[p:p + L].copy()
    m = rng.random(L) < 0.02
    r[m] = (r[m] + rng.integers(1, 4, int(m.sum()))) % 4
    r[rng.random(L) < 0.001] = 4
    return r.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _long_batch(L):
    """one read of L bases after 10 and before 10 ordinary 151-bp reads; the long read is read 10"""
    ref = _ref120()
    sr, so, sl = sample_reads(ref, 20, 151, 31)
    rd = [sr[so[i]:so[i] + sl[i]] for i in range(20)]
    return _batch(rd[:10] + [_long_read(ref, L, 37)] + rd[10:])


@functools.lru_cache(maxsize=None)
def _want4(L):
    out, cnt = _oref120().collect_intv(*_long_batch(L), cap=CAP4, nthreads=8)
    out.setflags(write=False)
    cnt.setflags(write=False)
    return out, cnt


def test_inputs_long_reads():
    """A read of 32,766 / 32,767 bases with 2% substitutions has ~650 mismatch-free stretches, two
    thirds of them >= 19 bases: the oracle gives well over 1,000 intervals, hundreds of them with
    ends past 16,383 (bit 14 of the packed entries' 15-bit end), the last within 20 bases of the
    read's end, all under the cap."""
    for L in (BSW_MAX_LEN - 1, BSW_MAX_LEN):
        reads, off, lens = _long_batch(L)
        assert lens[10] == L and lens.max() == L
        out, cnt = _want4(L)
        assert cnt.max() < CAP4
        b, e = _spans(out, cnt, 10)
        print(f"{L} bases: {cnt[10]} intervals, {int((e > 16383).sum())} ending past 16383, largest end {e.max()}")
        assert cnt[10] >= 1000 and (e > 16383).sum() >= 500
        assert L - 20 <= e.max() <= L


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [BSW_MAX_LEN - 1, BSW_MAX_LEN])
def test_gpu_long_reads_equal_oracle(L, form):
    f = bsw.Fmi(_ref120(), flags=FORMS[form])
    reads, off, lens = _long_batch(L)
    o_out, o_cnt = _want4(L)
    assert o_cnt.max() < CAP4
    g_out, g_cnt = f.collect_intv(reads, off, lens, cap=CAP4)
    _compare(o_out, o_cnt, g_out, g_cnt)
    # the packed 16-B entries hold ends below 2^15 - 1: the host switches at BSW_MAX_LEN
    want_entry = 32 if form == "wide_plain" or (form == "wide_packed" and L == BSW_MAX_LEN) else 16
    assert f.last_launch() == (1, want_entry)
    f.close()


@gpu
def test_gpu_read_past_max_len_is_refused():
    """32,768 bases on the host path: BSW_E_RANGE before any device work"""
    f = bsw.Fmi(_ref120())
    r = np.resize(_ref120(), BSW_MAX_LEN + 1)
    out = np.zeros((1, 4), dtype=bsw.BWTINTV_DTYPE)
    cnt = np.full(1, -1, np.int32)
    rc = bsw.hip_lib().bsw_mem_collect_intv(f._f, ctypes.byref(bsw.mem_opt()), bsw._ptr(r),
                                            bsw._ptr(np.zeros(1, np.int64)),
                                            bsw._ptr(np.array([BSW_MAX_LEN + 1], np.int32)), 1, bsw._ptr(out), 4,
                                            bsw._ptr(cnt))
    assert rc == E_RANGE and cnt[0] == -1
    with pytest.raises(bsw.BswError):
        f.collect_intv(r, np.zeros(1, np.int64), np.array([BSW_MAX_LEN + 1], np.int32), cap=4)
    f.close()


# ------------------------------------------------------------------ family 5: chunked launches


def _launches(n, max_len, entry, budget_mb=1):
    chunk = max(64, min(n, (budget_mb << 20) // (2 * (max_len + 1) * entry)))
    return -(-n // chunk), chunk


def test_library_exports_the_launch_header(tmp_path):
    """include/bsw_fmi_launch.h: declared == bsw.FMI_LAUNCH_SYMBOLS, exported, additive (bsw_fmi.h's
    own list and the ABI version are unchanged), compiles as C and C++, rejects null arguments."""
    from conftest import ROOT
    from stagekit import declared, exported
    assert declared("bsw_fmi_launch.h") == set(bsw.FMI_LAUNCH_SYMBOLS) <= exported()
    assert not set(bsw.FMI_LAUNCH_SYMBOLS) & set(bsw.ABI_SYMBOLS)
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8
    for cc, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / f"t.{ext}"
        src.write_text('#include "bsw_fmi_launch.h"\nint main(void) { int32_t a, b; return bsw_fmi_last_launch(0, &a, &b) == 0; }\n')
        r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    a = ctypes.c_int32()
    assert bsw.hip_lib().bsw_fmi_last_launch(None, ctypes.byref(a), ctypes.byref(a)) == -22


@functools.lru_cache(maxsize=None)
def _floor_batch():
    """130 reads, one of them (read 100, in the second launch) of BSW_MAX_LEN bases"""
    sr, so, sl = _reads1(700)
    rd = [sr[so[i]:so[i] + sl[i]] for i in range(129)]
    return _batch(rd[:100] + [_long_read(_ref60(), BSW_MAX_LEN, 41)] + rd[100:])


@functools.lru_cache(maxsize=None)
def _want5_floor():
    out, cnt = _oref60().collect_intv(*_floor_batch(), cap=CAP4, nthreads=8)
    out.setflags(write=False)
    cnt.setflags(write=False)
    return out, cnt


def test_inputs_chunked_launches():
    """The launch arithmetic of the chunking tests: 700 reads of 151 bases under a 1 MiB budget go
    in 4 launches of 16-B entries (215, 215, 215, 55: the last shorter than a wave) and 7 of 32-B
    entries (the last with 58); 130 reads with one of 32,767 bases hit the 64-read floor (64, 64, 2).
    Reads of every launch produce intervals, so a wrong read index or stride past the first chunk
    cannot pass."""
    assert _launches(700, 151, 16) == (4, 215) and 700 - 3 * 215 == 55
    assert _launches(700, 151, 32) == (7, 107) and 700 - 6 * 107 == 58
    assert _launches(130, BSW_MAX_LEN, 16) == (3, 64)
    assert _launches(700, 151, 16, budget_mb=16384) == (1, 700)
    _, out, cnt = _want1(19, True, 700, 10)
    assert cnt.max() < CAP1
    for chunk in (215, 107):
        for n0 in range(0, 700, chunk):
            assert (cnt[n0:n0 + chunk] > 0).sum() >= min(chunk, 700 - n0) // 2, (chunk, n0)
    # neighbouring reads differ, so reading read r - 1 or r + 1 for r would show
    assert all(not np.array_equal(out[i], out[i + 1]) for i in range(699) if cnt[i] > 0)
    reads, off, lens = _floor_batch()
    assert len(lens) == 130 and lens[100] == BSW_MAX_LEN
    fo, fc = _want5_floor()
    assert fc.max() < CAP4 and fc[100] >= 1000
    assert all((fc[a:b] > 0).sum() >= (b - a) // 2 for a, b in ((0, 64), (64, 128), (128, 130)))


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_gpu_chunked_launches_equal_oracle(form, monkeypatch):
    monkeypatch.delenv("BSW_SMEM_SCRATCH_MB", raising=False)
    f = bsw.Fmi(_ref60(), flags=FORMS[form])
    reads, off, lens = _reads1(700)
    kw, o_out, o_cnt = _want1(19, True, 700, 10)
    assert o_cnt.max() < CAP1
    entry = 32 if form == "wide_plain" else 16
    one_out, one_cnt = f.collect_intv(reads, off, lens, cap=CAP1, opt=bsw.mem_opt(**kw))
    assert f.last_launch() == (1, entry)
    monkeypatch.setenv("BSW_SMEM_SCRATCH_MB", "1")
    g_out, g_cnt = f.collect_intv(reads, off, lens, cap=CAP1, opt=bsw.mem_opt(**kw))
    want_launches = _launches(len(lens), int(lens.max()), entry)[0]
    assert want_launches == (7 if form == "wide_plain" else 4)
    assert f.last_launch() == (want_launches, entry)
    _compare(o_out, o_cnt, g_out, g_cnt)
    assert np.array_equal(one_cnt, g_cnt) and np.array_equal(one_out, g_out)
    # values below 1 count as 1
    monkeypatch.setenv("BSW_SMEM_SCRATCH_MB", "0")
    z_out, z_cnt = f.collect_intv(reads, off, lens, cap=CAP1, opt=bsw.mem_opt(**kw))
    assert f.last_launch() == (want_launches, entry)
    assert np.array_equal(z_cnt, g_cnt) and np.array_equal(z_out, g_out)
    f.close()


@gpu
def test_gpu_chunk_floor_of_64_reads(monkeypatch):
    """one read of 32,767 bases makes the budget's share less than one read: launches of 64 reads
    (64, 64, 2) over 64 MiB of scratch"""
    f = bsw.Fmi(_ref60())
    reads, off, lens = _floor_batch()
    o_out, o_cnt = _want5_floor()
    assert o_cnt.max() < CAP4
    monkeypatch.setenv("BSW_SMEM_SCRATCH_MB", "1")
    g_out, g_cnt = f.collect_intv(reads, off, lens, cap=CAP4)
    assert f.last_launch() == (3, 16) == (_launches(130, BSW_MAX_LEN, 16)[0], 16)
    _compare(o_out, o_cnt, g_out, g_cnt)
    f.close()


def _device_call(f, reads, off, lens, max_len, cap, opt=None, own_stream=False):
    """bsw_mem_collect_intv_device over uploaded copies -> (rc, intervals, counts)"""
    import hiprt
    n = len(lens)
    d_reads, d_off, d_len = (hiprt.DeviceBuffer.from_array(a) for a in (reads, off, lens))
    d_mems = hiprt.DeviceBuffer.from_array(np.zeros((n, cap), dtype=bsw.BWTINTV_DTYPE))
    d_cnt = hiprt.DeviceBuffer.from_array(np.full(n, -1, np.int32))
    stream = ctypes.c_void_p()
    if own_stream:
        hiprt.rt().hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        hiprt.rt().hipStreamDestroy.argtypes = [ctypes.c_void_p]
        hiprt.check(hiprt.rt().hipStreamCreate(ctypes.byref(stream)))
    try:
        rc = f.collect_intv_device(d_reads.ptr, d_off.ptr, d_len.ptr, n, max_len, d_mems.ptr, cap, d_cnt.ptr, opt=opt,
                                   stream=stream.value or 0)
    finally:
        if own_stream:
            hiprt.check(hiprt.rt().hipStreamDestroy(stream))
    g_out = d_mems.download(np.zeros((n, cap), dtype=bsw.BWTINTV_DTYPE))
    g_cnt = d_cnt.download(np.zeros(n, dtype=np.int32))
    return rc, g_out, g_cnt


@gpu
def test_gpu_chunked_device_api_on_a_callers_stream(monkeypatch):
    f = bsw.Fmi(_ref60(), flags=WIDE)
    reads, off, lens = _reads1(700)
    kw, o_out, o_cnt = _want1(19, True, 700, 10)
    monkeypatch.setenv("BSW_SMEM_SCRATCH_MB", "1")
    rc, g_out, g_cnt = _device_call(f, reads, off, lens, 151, CAP1, opt=bsw.mem_opt(**kw), own_stream=True)
    assert rc == 0 and f.last_launch() == (4, 16)
    _compare(o_out, o_cnt, g_out, g_cnt)
    f.close()


# ------------------------------------------------------------------ family 6: a read past max_len


@functools.lru_cache(maxsize=None)
def _overlong_batch():
    """63 reads of 30 .. 100 bases and, as read 40, one of 151"""
    sr, so, sl = _reads1(700)
    rng = np.random.default_rng(43)
    rd = [sr[so[i]:so[i] + int(rng.integers(30, 101))] for i in range(63)]
    rd[5], rd[6] = rd[5][:100], rd[6][:30]
    return _batch(rd[:40] + [sr[so[63]:so[63] + 151]] + rd[40:])


@functools.lru_cache(maxsize=None)
def _want6():
    return _oref60().collect_intv(*_overlong_batch(), cap=CAP2, nthreads=8)


def test_inputs_overlong_read():
    """one read of 151 bases among 63 of at most 100 (the bound itself included); the oracle, which
    has no max_len, finds intervals in it and in most of the others"""
    reads, off, lens = _overlong_batch()
    assert len(lens) == 64 and lens[40] == 151 and np.delete(lens, 40).max() == 100
    out, cnt = _want6()
    assert cnt.max() < CAP2 and cnt[40] > 0 and (np.delete(cnt, 40) > 0).sum() >= 40


@gpu
@pytest.mark.parametrize("form", ["narrow", "wide_packed"])
def test_gpu_device_api_read_past_max_len(form):
    """max_len = 100 with a 151-base read: BSW_E_RANGE, that read's count 0, every other read exact"""
    f = bsw.Fmi(_ref60(), flags=FORMS[form])
    reads, off, lens = _overlong_batch()
    o_out, o_cnt = _want6()
    rc, g_out, g_cnt = _device_call(f, reads, off, lens, 100, CAP2)
    assert rc == E_RANGE and g_cnt[40] == 0
    keep = np.arange(64) != 40
    _compare(o_out[keep], o_cnt[keep], g_out[keep], g_cnt[keep])
    f.close()
