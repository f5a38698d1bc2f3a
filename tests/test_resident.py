"""ResidentBatch (bwa-mem2-arm_amd/py/resident.py): the device-to-device stage chain behind one object.

CPU: the module imports without a device, argument mistakes are ValueErrors before the library is loaded,
the layout table has the binding's item sizes, and the GPU tests' input reaches the rescue and the pairing.
GPU: on 32 pairs of 2 x 100 bp against a 20 kb reference, every stage's buffers == what the host-array
form of the same stage returns from the stage before's downloaded arrays; a pair nothing seeds; the capacity
errors; entering the chain from host arrays.
"""

import numpy as np
import pytest

import bsw
import hiprt
import resident
from resident import ResidentBatch
from stagekit import DEFAULT, RECORDS, fetch, got_aln, got_pair, got_text, mat_gaps

# bench.pe_reads' seed: the default 42 leaves the rescue without a region to add on this reference; 13 gives two
# (test_input_reaches_rescue_and_pairing)
READS_SEED = 13
RNAME = "chrR"


def _input():
    import bench
    ref = bench.seeding_reference(20_000)
    return (ref,) + bench.pe_reads(ref, 32, 100, seed=READS_SEED)


def _opts(l_pac):
    return dict(e=bsw.ext_opt(l_pac=l_pac), s=bsw.sel_opt(l_pac=l_pac), p=bsw.pe_opt(l_pac=l_pac), m=bsw.matesw_opt(l_pac=l_pac),
                r=bsw.rec_opt(l_pac=l_pac, rname=RNAME))


# ---------------------------------------------------------------- CPU
def test_import_and_argument_checks_need_no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a library was loaded")

    class HostBuffer:                                        # stands in for device memory: no runtime behind it
        def __init__(self, nbytes):
            self.nbytes, self.ptr = nbytes, 1

        def upload(self, a):
            pass

    monkeypatch.setattr(bsw, "hip_lib", boom)
    monkeypatch.setattr(hiprt, "rt", boom)
    reads, off, lens = np.zeros(200, np.uint8), np.array([0, 100]), np.array([100, 100])
    with pytest.raises(ValueError):
        ResidentBatch(None, reads, off, lens[:1])
    with pytest.raises(ValueError):
        ResidentBatch(None, reads, off, lens, quals=np.zeros(199, np.uint8))
    monkeypatch.setattr(hiprt, "DeviceBuffer", HostBuffer)
    b = ResidentBatch(None, reads, off, lens)
    assert b.n_reads == 2 and b.n["reads"] == 200
    for call in (lambda: b.chain2aln(None), lambda: b.select(None), lambda: b.pe_stat(None), lambda: b.matesw(None, None),
                 lambda: b.pe_pair(None, None), lambda: b.reg2aln(None), lambda: b.records(None),
                 lambda: b.sam_text(None, [b"x"], True), lambda: b.get("sreg")):
        with pytest.raises(ValueError, match="buffer yet"):
            call()
    for kw in (dict(nosuch=lens), dict(off=off[:1]), dict(sreg=np.zeros(3, bsw.ALNREG_DTYPE), sinfo=np.zeros(2, bsw.SELINFO_DTYPE)),
               dict(cigar=np.zeros(4, np.uint32))):
        with pytest.raises(ValueError):
            b.put(**kw)
    b.put(seeds=np.zeros(3, bsw.SEED_DTYPE), sr=np.zeros(3, np.int32), sc=np.zeros(3, np.int32),
          regs=np.zeros(3, bsw.ALNREG_DTYPE), ext=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="csub"):
        b.select(None, csub=np.zeros(2, np.int32))
    b.put(sreg=np.zeros(1, bsw.ALNREG_DTYPE), sread=np.zeros(1, np.int32), sinfo=np.zeros(1, bsw.SELINFO_DTYPE),
          sfirst=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="pairs"):           # paired records before pe_pair
        b.records(None)
    with pytest.raises(ValueError, match="into"):
        b.reg2aln(None, into="mine")


def test_layout_table_has_the_binding_item_sizes():
    want = dict(seeds=bsw.SEED_DTYPE, regs=bsw.ALNREG_DTYPE, sreg=bsw.ALNREG_DTYPE, mreg=bsw.ALNREG_DTYPE,
                sinfo=bsw.SELINFO_DTYPE, minfo=bsw.SELINFO_DTYPE, pairs=bsw.PAIR_DTYPE, aln=bsw.ALN_DTYPE, recs=bsw.REC_DTYPE)
    for name, (dtype, strides, key) in resident.LAYOUT.items():
        dt = np.dtype(dtype)
        assert dt.itemsize == (want[name].itemsize if name in want else {"off": 8, "name_off": 8, "text_off": 8, "reads": 1,
                                                                         "quals": 1, "md": 1, "names": 1, "text": 1}.get(name, 4)), name
        assert (dt == want[name]) if name in want else dt.names is None, name
        assert strides == ({"cigar": ("cigar",), "md": ("md",)}.get(name, ())) and isinstance(key, str)
    assert resident._row("all.cigar") == (np.dtype(np.uint32), ("all.cigar",), "all.aln")
    assert set(x for names in resident.LISTS.values() for x in names if x) <= set(resident.LAYOUT)


def test_input_reaches_rescue_and_pairing():
    """the oracle front end and the restatements on the GPU tests' input: the rescue adds a region, pairs pair"""
    import matesw_py as mp
    import oracle
    import pe_py as pp
    import regsel_py as sp
    from test_memchain import _oracle_front, _two_strand
    from test_regsel import _select
    ref, reads, off, lens = _input()
    T, L = _two_strand(ref), len(ref)
    mat, gaps = mat_gaps(DEFAULT)
    f, mems, cnt, seeds, sr, sc = _oracle_front(ref, reads, off, lens, cap=256)
    regs, ext = oracle.chain2aln(oracle.make_params(), bsw.ext_opt(l_pac=L), T, reads, off, lens, seeds, sr, sc)
    arr = dict(reads=reads, off=off, lens=lens, seeds=seeds, sr=sr, sc=sc, regs=regs, ext=ext)
    sregs, _, sinfo, first, _ = _select(T, arr, opt=sp.sel_opt(l_pac=L))
    popt = pp.pe_opt(l_pac=L)
    pes, _, _ = pp.pe_stat(sregs, sinfo, first, popt, 1)
    m = mp.mate_rescue(pes, T, reads, off, lens, sregs, sinfo, first, mp.matesw_opt(l_pac=L), mat, gaps, oracle.ksw_align2)
    pairs = pp.pe_pair(pes, m[0], m[2], m[3], popt, mat, gaps)[2]
    assert len(m[0]) > len(sregs) and (m[2]["src"] == -1).sum() >= 1 and pairs["paired"].sum() >= 1


# ---------------------------------------------------------------- GPU
class Chain:
    """the full chain on one batch, each stage's outputs kept as downloaded"""

    def __init__(self):
        self.ref, self.reads, self.off, self.lens = _input()
        self.T = np.concatenate([self.ref, 3 - self.ref[::-1]]).astype(np.uint8)
        self.o = o = _opts(len(self.ref))
        self.names = [b"pair%02d" % i for i in range(len(self.lens) // 2)]
        self.quals = (33 + (np.arange(len(self.reads)) * 7) % 41).astype(np.uint8)
        self.fmi = bsw.Fmi(self.ref)
        self.eng = bsw.Engine()
        bsw.set_reference(self.eng, self.T)
        self.b = b = self.batch()
        self.seeds_host = b.seed_and_chain(self.fmi)
        self.seeds = tuple(b.get(x) for x in ("seeds", "sr", "sc"))
        b.chain2aln(o["e"])
        self.regs, self.ext = b.get("regs"), b.get("ext")
        self.k = b.select(o["s"])
        self.sel = fetch(b, *b.lists[0])
        self.pes = b.pe_stat(o["p"])
        self.m = b.matesw(self.pes, o["m"])
        self.msw = fetch(b, *b.lists[0])
        b.pe_pair(self.pes, o["p"])
        self.paired = got_pair(b)
        b.reg2aln(o["e"], into="all.aln")                    # (records writes "aln": rows are compared whole below)
        self.aln = got_aln(b, "all.aln")
        self.n_rec, self.n_aln = b.records(o["r"])
        self.rec = fetch(b, *RECORDS)
        self.n_bytes = b.sam_text(o["r"], self.names, True)
        self.text = got_text(b)

    def batch(self):
        return ResidentBatch(self.eng, self.reads, self.off, self.lens, self.quals)

    def close(self):
        self.eng.close()
        self.fmi.close()


@pytest.fixture(scope="module")
def chain():
    c = Chain()
    yield c
    c.close()


def _bytes_equal(want, got, tag):
    assert len(want) == len(got), tag
    for i, (w, g) in enumerate(zip(want, got)):
        w = np.ascontiguousarray(w)
        assert w.dtype == g.dtype and w.shape == g.shape and w.tobytes() == g.tobytes(), f"{tag}: array {i}"


@pytest.mark.gpu
def test_gpu_full_chain_is_the_host_array_forms(chain):
    c, eng, o = chain, chain.eng, chain.o
    rd = (c.reads, c.off, c.lens)
    _bytes_equal(c.seeds_host, c.seeds, "seeds")
    assert len(c.seeds[0]) > 0
    _bytes_equal(bsw.chain2aln(eng, c.T, *rd, *c.seeds, o["e"]), (c.regs, c.ext), "chain2aln")
    _bytes_equal(bsw.regs_select(eng, *rd, *c.seeds, c.regs, c.ext, o["s"]), c.sel, "select")
    assert c.k == len(c.sel[0]) > 0
    sregs, sread, sinfo, sfirst = c.sel
    assert bsw.pe_stat(eng, sregs, sinfo, sfirst, o["p"]).tobytes() == c.pes.tobytes() and c.pes[1]["failed"] == 0
    _bytes_equal(bsw.matesw(eng, c.pes, *rd, sregs, sinfo, sfirst, o["m"]), c.msw, "matesw")
    mregs, mread, minfo, mfirst = c.msw
    assert c.m == len(mregs) > c.k and (minfo["src"] == -1).sum() >= 1           # a rescued region
    _bytes_equal(bsw.pe_pair(eng, c.pes, mregs, minfo, mfirst, o["p"]), c.paired, "pe_pair")
    pregs, pinfo, pairs = c.paired
    assert pairs["paired"].sum() >= 1 and np.array_equal(c.b.get("mread"), mread)
    _bytes_equal(bsw.reg2aln(eng, *rd, pregs, mread, o["e"]), c.aln, "reg2aln")
    _bytes_equal(bsw.records(eng, *rd, pregs, pinfo, mfirst, pairs, o["r"]), c.rec, "records")
    recs, rfirst, aln, aln_reg, cig, md = c.rec
    assert (c.n_rec, c.n_aln) == (len(recs), len(aln)) and c.n_rec >= len(c.lens)
    text, toff = bsw.sam_text(eng, recs, rfirst, aln, cig, md, *rd, c.names, c.quals, o["r"], True)
    assert text == c.text[0] and np.array_equal(toff, c.text[1]) and c.n_bytes == len(text) > 0
    assert text.count(b"\n") == c.n_rec


@pytest.mark.gpu
def test_gpu_single_pair_nothing_seeds(chain, monkeypatch):
    c, eng, o = chain, chain.eng, chain.o
    asked = []
    init = hiprt.DeviceBuffer.__init__
    monkeypatch.setattr(hiprt.DeviceBuffer, "__init__", lambda self, nbytes: (asked.append(nbytes), init(self, nbytes))[1])
    reads = np.random.default_rng(5).integers(0, 4, 200).astype(np.uint8)
    off, lens = np.array([0, 100], np.int64), np.array([100, 100], np.int32)
    rd = (reads, off, lens)
    b = ResidentBatch(eng, *rd)
    seeds = b.seed_and_chain(c.fmi)
    b.chain2aln(o["e"])
    k = b.select(o["s"])
    pes = b.pe_stat(o["p"])
    m = b.matesw(pes, o["m"])
    b.pe_pair(pes, o["p"])
    b.reg2aln(o["e"], into="all.aln")
    n_rec, n_aln = b.records(o["r"])
    n_bytes = b.sam_text(o["r"], [b"lonely"], True)
    assert (len(seeds[0]), k, m, n_rec, n_aln) == (0, 0, 0, 2, 0) and min(asked) >= 1, asked
    sel = bsw.regs_select(eng, *rd, *seeds, *bsw.chain2aln(eng, c.T, *rd, *seeds, o["e"]), o["s"])
    _bytes_equal(sel, tuple(b.get(x) for x in ("sreg", "sread", "sinfo", "sfirst")), "select")
    assert bsw.pe_stat(eng, sel[0], sel[2], sel[3], o["p"]).tobytes() == pes.tobytes()
    msw = bsw.matesw(eng, pes, *rd, sel[0], sel[2], sel[3], o["m"])
    _bytes_equal(msw, fetch(b, *b.lists[0]), "matesw")
    paired = bsw.pe_pair(eng, pes, msw[0], msw[2], msw[3], o["p"])
    _bytes_equal(paired, got_pair(b), "pe_pair")
    assert len(got_aln(b, "all.aln")[0]) == 0
    want = bsw.records(eng, *rd, paired[0], paired[1], msw[3], paired[2], o["r"])
    rec = fetch(b, *RECORDS)
    _bytes_equal(want, rec, "records")
    assert list(rec[0]["sam_flag"] & 4) == [4, 4] and list(rec[0]["aln"]) == [-1, -1]
    text, toff = bsw.sam_text(eng, *want[:3], *want[4:], *rd, [b"lonely"], None, o["r"], True)
    assert (text, n_bytes) == (got_text(b)[0], len(text)) and np.array_equal(toff, got_text(b)[1])
    assert text.startswith(b"lonely\t77\t*\t0\t0\t*\t")


@pytest.mark.gpu
def test_gpu_capacity_errors_then_the_default_capacities(chain):
    c, o = chain, chain.o
    b = c.batch()
    b.seed_and_chain(c.fmi)
    b.chain2aln(o["e"])
    b.select(o["s"])
    pes = b.pe_stat(o["p"])
    with pytest.raises(bsw.BswError, match="-34") as ei:
        b.matesw(pes, o["m"], cap=1)
    assert ei.value.needed == c.m and b.lists[0][0] == "sreg"            # the selection's lists stay current
    assert b.matesw(pes, o["m"]) == c.m
    _bytes_equal(c.msw, fetch(b, *b.lists[0]), "matesw after the error")
    b.pe_pair(pes, o["p"])
    assert b.records(o["r"]) == (c.n_rec, c.n_aln)
    with pytest.raises(bsw.BswError, match="-34") as ei:
        b.sam_text(o["r"], c.names, True, cap=c.n_bytes - 1)
    assert ei.value.needed == c.n_bytes
    assert b.sam_text(o["r"], None, True) == c.n_bytes                   # (the names of the call before)
    assert got_text(b)[0] == c.text[0] and np.array_equal(got_text(b)[1], c.text[1])
    _bytes_equal(c.rec, fetch(b, *RECORDS), "records")


@pytest.mark.gpu
def test_gpu_reentry_from_host_arrays(chain):
    """the selection's four arrays put into a fresh batch.  Pairing them as they are gives the full chain's pairs
    wherever the rescue left both lists of a pair as they were (it did not everywhere: the input is chosen so that
    it adds a region); with the rescue between, as in the full chain, every pair is the full chain's."""
    c, o = chain, chain.o
    sregs, sread, sinfo, sfirst = c.sel
    mregs, _, minfo, mfirst = c.msw
    b = c.batch()
    b.put(sreg=sregs, sread=sread, sinfo=sinfo, sfirst=sfirst)
    pes = b.pe_stat(o["p"])
    assert pes.tobytes() == c.pes.tobytes()
    b.pe_pair(pes, o["p"])
    _bytes_equal(bsw.pe_pair(c.eng, pes, sregs, sinfo, sfirst, o["p"]), got_pair(b), "pairs of the selection")
    same = [p for p in range(len(c.lens) // 2)
            if sregs[sfirst[2 * p]:sfirst[2 * p + 2]].tobytes() == mregs[mfirst[2 * p]:mfirst[2 * p + 2]].tobytes() and
            sinfo[sfirst[2 * p]:sfirst[2 * p + 2]].tobytes() == minfo[mfirst[2 * p]:mfirst[2 * p + 2]].tobytes() and
            list(np.diff(sfirst[2 * p:2 * p + 3])) == list(np.diff(mfirst[2 * p:2 * p + 3]))]
    assert 0 < len(same) < len(c.lens) // 2
    have, want = b.get("pairs"), c.paired[2]
    assert all(have[p].tobytes() == want[p].tobytes() for p in same)
    b.put(sreg=sregs, sread=sread, sinfo=sinfo, sfirst=sfirst)           # (the pairing updated them in place)
    assert b.matesw(b.pe_stat(o["p"]), o["m"]) == c.m
    b.pe_pair(pes, o["p"])
    _bytes_equal(c.paired, got_pair(b), "pairs behind the rescue")
