"""BAM records (include/bsw_bam.h): the records of bsw_records* as uncompressed BAM alignment blocks.

CPU: the restatement (tests/bam_py.py) decoded by its independent reader is rec_py's text line for line, on
test_rec's hand cases and pipeline set, under every option flag, with and without quals; known answers derived by
hand from the SAM specification (one whole mapped paired record, the unmapped record, reg2bin, the integer tag
types, the header block); the header's symbols and layouts; the argument checks that need no device.
GPU: bsw_bam_records* == the restatement in every byte and offset.  Byte parity with htslib rests on the
specification as bsw_bam.h restates it and on the known answers: no htslib, samtools or sample BAM file is at hand.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import bam_py as bp
import bsw
import contigs_py as cp
import rec_py as rq
import reg2aln_py as rp
from conftest import ROOT
from resident import ResidentBatch
from stagekit import DEFAULT, declared, exported, got_text, mat_gaps, same_text
from test_matesw import L, REF, T, MsBatch, reg, rnd
from test_rec import HAND, RNAME, Case, case_pe, case_supp, case_xa, ext_set, rec_set, rv

FLAGS = (rq.SOFTCLIP, rq.NO_MULTI, rq.KEEP_SUPP_MAPQ, 7)
# three contigs over test_matesw's text: case_pe's improper pair (1000 / 25000), case_supp's two parts (5000 / 9000)
# and case_xa's members (7000 .. 9000) lie on both sides of a join, no region of them across one
TAB3 = cp.Table((8000, 12000, L - 20000), ("c1", "chr_two", "3"))


def _quals(reads):
    return (33 + (np.arange(len(reads)) * 5) % 60).astype(np.uint8)


def _lines(text):
    return text.decode("latin-1").split("\n")[:-1]


def _paired(c):
    return c.pairs is not None


# ---------------------------------------------------------------- CPU: the reader gives the pinned text back
def _roundtrip(res, reads, off, lens, names, opt, paired, tag, tab=None):
    for quals in (_quals(reads), None):
        if tab is None:
            text, _ = rq.sam_text(res, reads, off, lens, names, quals, opt, paired)
        else:
            text, _ = cp.sam_text(tab, res, reads, off, lens, names, quals, opt, paired)
        bam, boff = bp.encode(res, reads, off, lens, names, quals, opt, paired, tab)
        assert len(boff) == len(res.recs) + 1 and boff[-1] == len(bam), tag
        ref_names = [opt["rname"]] if tab is None else tab.names
        got, want = bp.decode(bam, ref_names), _lines(text)
        assert len(got) == len(want), tag
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{tag}, quals {quals is not None}, record {i}"
        for i, b in enumerate(bp.blocks(bam)):                   # the offsets are the blocks'
            assert boff[i + 1] - boff[i] == 4 + len(b), tag


@pytest.mark.parametrize("name", sorted(HAND))
def test_decoded_blocks_are_the_text_hand_cases(name):
    for flags in (0,) + FLAGS:
        c = HAND[name]()
        w = c.run(flags=flags)
        reads, off, lens = w.arrays[:3]
        _roundtrip(w, reads, off, lens, c.names, w.opt, _paired(c), f"{name} flags {flags}")


def test_decoded_blocks_are_the_text_pipeline_set():
    s = rec_set()
    a = s.p.arr
    _roundtrip(s.res, a["reads"], a["off"], a["lens"], s.names, s.opt, True, "pipeline set")


def _under_table(c, tab=TAB3):
    """a test_rec case under a contig table: contigs_py's records (TLEN 0 across contigs) and text"""
    w = c.run()
    reads, off, lens, regs, info, first = w.arrays
    mat, gaps = mat_gaps(DEFAULT)
    opt = dict(w.opt)
    res = cp.records(tab, T, reads, off, lens, regs, info, first, c.pairs, opt, mat, gaps)
    res.opt, res.arrays = opt, w.arrays
    return res


def test_decoded_blocks_are_the_text_under_three_contigs():
    seen = set()
    for mk in (case_pe, case_supp, case_xa):
        c = mk()
        res = _under_table(c)
        reads, off, lens = res.arrays[:3]
        _roundtrip(res, reads, off, lens, c.names, res.opt, _paired(c), mk.__name__, TAB3)
        bam, _ = bp.encode(res, reads, off, lens, c.names, None, res.opt, _paired(c), TAB3)
        for b in bp.blocks(bam):
            f = bp.fields(b)
            if f["refID"] >= 0 and f["next_refID"] >= 0 and f["refID"] != f["next_refID"]:
                seen.add("mate")
        for line in bp.decode(bam, TAB3.names):
            rname = line.split("\t")[2]
            for t in line.split("\t")[11:]:
                if t[:5] in ("SA:Z:", "XA:Z:") and any(e.split(",")[0] != rname for e in t[5:-1].split(";")):
                    seen.add(t[:2])
    assert seen == {"mate", "SA", "XA"}


# ---------------------------------------------------------------- CPU: known answers, by hand from the specification
NIB = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}                  # SAMv1 4.2: `=ACMGRSVTWYHKDBN` -> [0, 15]


def _pack(seq):
    """SEQ as the specification packs it: the first base in the high nibble, a trailing low nibble 0"""
    v = [NIB[c] for c in seq] + [0]
    return bytes(v[i] << 4 | v[i + 1] for i in range(0, len(seq), 2))


def _pe_with_quals():
    c = case_pe()
    reads = c.run().arrays[0]
    return Case(c.batch, c.pairs, _quals(reads))


def test_one_mapped_paired_record_byte_for_byte():
    c = _pe_with_quals()
    w = c.run()
    reads, off, lens = w.arrays[:3]
    seq = "".join("ACGT"[int(x)] for x in REF[1000:1100])
    qual = bytes(c.quals[:100])
    # the line this block has to say (test_rec pins it field by field)
    assert w.lines[0] == f"q0\t99\tchrT\t1001\t60\t100M\t=\t1401\t500\t{seq}\t{qual.decode()}\tNM:i:0\tMD:Z:100\tMC:Z:100M\tAS:i:100\tXS:i:0"
    want = bytes.fromhex(
        "d8000000"       # block_size: 32 fixed + 3 name + 4 CIGAR + 50 SEQ + 100 QUAL + 27 tags = 216
        "00000000"       # refID: the one reference
        "e8030000"       # pos: POS 1001 is 1-based -> 1000
        "03"             # l_read_name: `q0` + NUL
        "3c"             # mapq 60
        "4912"           # bin: [1000, 1100) lies in one 16 kb bin -> 4681 + (1000 >> 14) = 4681 = 0x1249
        "0100"           # n_cigar_op
        "6300"           # flag 99
        "64000000"       # l_seq 100
        "00000000"       # next_refID: RNEXT `=`
        "78050000"       # next_pos: PNEXT 1401 -> 1400
        "f4010000"       # tlen 500
        "713000"         # read_name
        "40060000"       # 100M: 100 << 4 | 0
    ) + _pack(seq) + bytes(q - 33 for q in qual) + (
        b"NMC\x00"       # NM:i:0: 0 fits uint8
        b"MDZ100\x00"
        b"MCZ100M\x00"
        b"ASC\x64"       # AS:i:100
        b"XSC\x00")
    assert len(want) == 4 + 216
    bam, boff = bp.encode(w, reads, off, lens, c.names, c.quals, w.opt, True)
    assert bam[:boff[1]] == want


def test_the_fully_unmapped_record():
    c = _pe_with_quals()
    w = c.run()
    reads, off, lens = w.arrays[:3]
    assert w.lines[9].startswith("q4\t77\t*\t0\t0\t*\t*\t0\t0\t") and w.lines[9].endswith("\tAS:i:0\tXS:i:0")
    seq = "".join("ACGT"[int(x)] for x in rnd(seed=7))
    bam, boff = bp.encode(w, reads, off, lens, c.names, None, w.opt, True)
    want = bytes.fromhex(
        "c1000000"       # block_size: 32 + 3 + 0 + 50 + 100 + 8 = 193
        "ffffffff"       # refID -1
        "ffffffff"       # pos -1
        "03" "00"        # l_read_name, mapq
        "4812"           # bin: reg2bin(-1, 0) = 4681 + (-1 >> 14) = 4680 = 0x1248
        "0000"           # n_cigar_op
        "4d00"           # flag 77
        "64000000"       # l_seq
        "ffffffff" "ffffffff"    # next_refID, next_pos
        "00000000"       # tlen
        "713400"         # `q4` + NUL
    ) + _pack(seq) + b"\xff" * 100 + b"ASC\x00XSC\x00"          # no quals: 0xFF, l_seq times
    assert bam[boff[9]:boff[10]] == want
    f = bp.fields(bam[boff[9] + 4:boff[10]])
    assert (f["bin"], f["refID"], f["pos"], f["next_refID"], f["next_pos"]) == (4680, -1, -1, -1, -1)


def test_reg2bin_known_values():
    assert bp.reg2bin(0, 1) == 4681 and bp.reg2bin(16383, 16384) == 4681 and bp.reg2bin(16384, 16385) == 4682
    assert bp.reg2bin(16383, 16385) == 585 and bp.reg2bin(0, 1 << 29) == 0 and bp.reg2bin(-1, 0) == 4680


def test_integer_tag_types_at_their_boundaries():
    assert bp.int_tag("NM", 255) == b"NMC\xff"
    assert bp.int_tag("NM", 256) == b"NMS\x00\x01"
    assert bp.int_tag("AS", 65535) == b"ASS\xff\xff"
    assert bp.int_tag("AS", 65536) == b"ASI\x00\x00\x01\x00"
    assert bp.int_tag("XS", -1) == b"XSc\xff"
    assert bp.int_tag("AS", -128) == b"ASc\x80" and bp.int_tag("AS", -129) == b"ASs\x7f\xff"
    assert bp.int_tag("AS", -32768) == b"ASs\x00\x80" and bp.int_tag("AS", -32769) == b"ASi\xff\x7f\xff\xff"


def test_header_block_bytes():
    opt = rq.rec_opt(l_pac=L, rname=RNAME)
    # no table: one reference, opt's name and length (30000 = 0x7530)
    assert bp.header(opt) == b"BAM\x01" + bytes.fromhex("00000000" "01000000" "05000000") + b"chrT\x00" + bytes.fromhex("30750000")
    text = b"@HD\tVN:1.6\n"
    want = (b"BAM\x01" + bytes.fromhex("0b000000") + text + bytes.fromhex("03000000") +
            bytes.fromhex("03000000") + b"c1\x00" + bytes.fromhex("401f0000") +          # 8000
            bytes.fromhex("08000000") + b"chr_two\x00" + bytes.fromhex("e02e0000") +     # 12000
            bytes.fromhex("02000000") + b"3\x00" + bytes.fromhex("10270000"))            # 10000
    assert bp.header(opt, text, TAB3) == want
    with pytest.raises(ValueError, match="INVAL"):
        bp.header(rq.rec_opt(l_pac=L - 1, rname=RNAME), b"", TAB3)
    with pytest.raises(ValueError, match="RANGE"):
        bp.header(rq.rec_opt(l_pac=2 ** 31, rname=RNAME))


# ---------------------------------------------------------------- CPU: the header file
def test_library_exports_the_bam_header():
    assert declared("bsw_bam.h") == set(bsw.BAM_SYMBOLS)
    assert declared("bsw_bam.h") <= exported(), declared("bsw_bam.h") - exported()
    others = (set(bsw.ABI_SYMBOLS) | set(bsw.ALN_SYMBOLS) | set(bsw.SEL_SYMBOLS) | set(bsw.PE_SYMBOLS) |
              set(bsw.MATESW_SYMBOLS) | set(bsw.REC_SYMBOLS) | set(bsw.CONTIGS_SYMBOLS))
    assert not set(bsw.BAM_SYMBOLS) & others
    assert len(bsw.ABI_SYMBOLS) == 45 and bsw.hip_lib().bsw_abi_version() == 8


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_bam_header_layouts_compile(tmp_path, cc, ext):
    sa = "_Static_assert" if ext == "c" else "static_assert"
    src = tmp_path / f"t.{ext}"
    src.write_text('#include <stddef.h>\n#include "bsw_bam.h"\n'
                   f"{sa}(sizeof(bsw_bam_stats_t) == 24 && offsetof(bsw_bam_stats_t, n_bytes) == 8 && offsetof(bsw_bam_stats_t, len_ms) == 16 && offsetof(bsw_bam_stats_t, write_ms) == 20, \"stats\");\n"
                   f"{sa}(sizeof(bsw_rec_t) == 88 && sizeof(bsw_rec_opt_t) == 96, \"rec\");\n"
                   f"{sa}(BSW_BAM_API == 1 && BSW_REC_API == 1 && BSW_ABI_VERSION == 8 && BSW_BAM_MAX_NAME == 254, \"api\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(bsw.BamStats) == 24 and bsw.BamStats.n_bytes.offset == 8 and bsw.BamStats.write_ms.offset == 20


def test_resident_batch_knows_the_bam_buffers():
    import resident
    assert resident._row("bam") == (np.dtype(np.uint8), (), "bam")
    assert resident._row("bam_off") == (np.dtype(np.int64), (), "bam_off")
    assert not set(resident.BAM_LAYOUT) & set(resident.LAYOUT)
    assert callable(ResidentBatch.bam_records)


def _lib_calls(ctx, o, n_reads=2, paired=True, cs=16, ms=64, cap=8):
    Lb = bsw.hip_lib()
    first, reads = np.zeros(n_reads + 2, dtype=np.int32), np.zeros(8, np.uint8)
    off, lens = np.zeros(max(n_reads, 1), np.int64), np.zeros(max(n_reads, 1), np.int32)
    recs, aln = np.zeros(4, dtype=bsw.REC_DTYPE), np.zeros(4, dtype=bsw.ALN_DTYPE)
    cig, md = np.zeros(64, np.uint32), np.zeros(256, np.uint8)
    noff, boff, bam = np.zeros(4, np.int64), np.zeros(8, np.int64), np.zeros(8, np.uint8)
    nb = ctypes.c_int64(0)
    P, B = bsw._ptr, ctypes.byref
    return (Lb.bsw_bam_records(ctx, B(o), P(recs), P(first), 0, P(aln), P(cig), cs, P(md), ms, 0, P(reads), P(off), P(lens),
                               n_reads, P(reads), P(noff), None, int(paired), P(bam), P(boff), cap, B(nb)),
            Lb.bsw_bam_records_resident(ctx, B(o), P(recs), P(first), 0, P(aln), P(cig), cs, P(md), ms, 0, P(reads), P(off),
                                        P(lens), n_reads, P(reads), P(noff), None, int(paired), P(bam), P(boff), cap,
                                        B(nb), None))


def test_invalid_arguments_need_no_device():
    Lb = bsw.hip_lib()
    assert Lb.bsw_bam_last_stats(None, None) == -22
    fake = ctypes.c_void_p(1)                                # never dereferenced: the checks come first
    good = bsw.rec_opt(l_pac=L, rname=RNAME)
    inval = (-22, -22)
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L)) == inval                        # no rname
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname="x" * 64)) == inval        # unterminated
    assert _lib_calls(fake, bsw.rec_opt(l_pac=L, rname=RNAME, flags=8)) == inval
    assert _lib_calls(fake, good, n_reads=3) == inval                             # odd with pairs
    assert _lib_calls(fake, good, cs=0) == inval
    assert _lib_calls(fake, good, ms=0) == inval
    assert _lib_calls(fake, good, cap=-1) == inval
    assert _lib_calls(None, good) == inval
    out, nb = np.zeros(64, np.uint8), ctypes.c_int64(0)
    P, B = bsw._ptr, ctypes.byref
    assert Lb.bsw_bam_header(None, B(good), None, 0, P(out), 64, B(nb)) == -22
    assert Lb.bsw_bam_header(fake, B(bsw.rec_opt(l_pac=L)), None, 0, P(out), 64, B(nb)) == -22
    assert Lb.bsw_bam_header(fake, B(good), None, -1, P(out), 64, B(nb)) == -22
    assert Lb.bsw_bam_header(fake, B(good), None, 0, P(out), -1, B(nb)) == -22
    assert Lb.bsw_bam_header(fake, B(good), None, 0, P(out), 64, None) == -22
    assert Lb.bsw_bam_header(fake, B(good), None, 3, P(out), 64, B(nb)) == -22    # a length without a text


# ---------------------------------------------------------------- GPU
def _gpu_bam(eng, res, reads, off, lens, names, quals, opt, paired, tag, tab=None):
    """bsw_bam_records on the restatement's records and alignments (the host form takes them as inputs) against
    the restatement's blocks"""
    want, woff = bp.encode(res, reads, off, lens, names, quals, opt, paired, tab)
    got = bsw.bam_records(eng, res.recs, res.rec_first, res.aln, res.cigar, res.md, reads, off, lens, names, quals,
                          bsw.rec_opt(**opt), paired)
    same_text(want, woff, got, tag)
    st = bsw.bam_last_stats(eng)
    assert st.n_bytes == len(want) and st.n_rec == len(res.recs) and st.len_ms > 0 and (st.write_ms > 0) == (len(want) > 0), tag
    return want, woff


@pytest.mark.gpu
def test_gpu_hand_sets_and_option_flags():
    eng = bsw.Engine()
    for name, mk in sorted(HAND.items()):
        for flags in (0,) + FLAGS:
            c = mk()
            w = c.run(flags=flags)
            reads, off, lens = w.arrays[:3]
            for quals in (_quals(reads), None):
                _gpu_bam(eng, w, reads, off, lens, c.names, quals, w.opt, _paired(c), f"{name} flags {flags}")
    eng.close()


def _length_case(quals):
    """reads of 1 .. 300 bases on both strands, mapped and not; names of every length 1 .. 8 and one of 254"""
    b = MsBatch()
    for n in (1, 2, 31, 32, 33, 151, 300):
        r, rb, re_ = rv(4000, 4000 + n)
        b.reads += [REF[3000:3000 + n], r, rnd(n, seed=n)]
        b.ends += [[reg(3000, 40, qb=0, qe=n, mapq=n % 61)], [reg(rb, 40, qb=0, qe=n, mapq=n % 61)], []]
    c = Case(b, None, _quals(np.concatenate(b.reads)) if quals else None)
    c.names = [b"N" * (1 + i % 8) for i in range(len(b.reads))]
    c.names[-2] = b"x" * 254
    return c


@pytest.mark.gpu
def test_gpu_read_and_name_lengths():
    eng = bsw.Engine()
    for quals in (True, False):
        c = _length_case(quals)
        w = c.run()
        assert len(w.recs) == 21 and (w.recs["aln"] >= 0).sum() == 14
        reads, off, lens = w.arrays[:3]
        want, woff = _gpu_bam(eng, w, reads, off, lens, c.names, c.quals, w.opt, False, f"lengths quals={quals}")
        d = np.diff(woff)
        assert d.max() > 512                                     # a record that flushes its window more than once
        assert {int(x) & 3 for x in woff[:-1]} == {0, 1, 2, 3} and {int(x) & 3 for x in d} == {0, 1, 2, 3}
        assert bp.decode(want, [RNAME]) == w.lines
    c.names[0] = b"y" * 255                                      # one more than l_read_name holds
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.bam_records(eng, w.recs, w.rec_first, w.aln, w.cigar, w.md, reads, off, lens, c.names, None, bsw.rec_opt(**w.opt),
                        False)
    eng.close()


_enc = {}


def _set_blocks():
    """the pipeline set's blocks, encoded once"""
    if not _enc:
        s = rec_set()
        a = s.p.arr
        _enc["x"] = bp.encode(s.res, a["reads"], a["off"], a["lens"], s.names, s.quals, s.opt, True)
    return _enc["x"]


@pytest.mark.gpu
def test_gpu_record_counts():
    s = rec_set()
    a, w = s.p.arr, s.res
    bam, boff = _set_blocks()
    eng = bsw.Engine()
    o = bsw.rec_opt(**s.opt)
    for npairs in (0, 1, 63, 64, 65, 257):
        nr = 2 * npairs
        nrec = int(w.rec_first[nr])
        nal = int(max((w.recs["aln"][:nrec] + 1 + w.recs["xa_n"][:nrec]).max(initial=0), 0))
        got = bsw.bam_records(eng, w.recs[:nrec], w.rec_first[:nr + 1], w.aln[:nal], w.cigar[:nal], w.md[:nal],
                              a["reads"][:nr * 150], a["off"][:nr], a["lens"][:nr], s.names[:npairs], s.quals[:nr * 150], o, True)
        same_text(bam[:int(boff[nrec])], boff[:nrec + 1], got, f"{npairs} pairs")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("read_len", [5, 6, 7, 8])
def test_gpu_exact_record_counts_around_one_block(read_len):
    """exactly 0, 1, 63, 64 and 65 records (64 = the records of a block at 4 lanes per record; 128 and 129: two full
    blocks, and a last block of one record behind them): hand-built single-end records, one per read, names of
    1 .. 8 bytes so that the block's two ends and the shared dwords fall on every offset mod 4"""
    eng = bsw.Engine()
    opt = rq.rec_opt(l_pac=L, rname=RNAME)
    for n in (0, 1, 63, 64, 65, 128, 129):
        rows = [(100 + 7 * i, i % 3, 50 + i, i % 5 - 1, 0) for i in range(n)]
        res, reads, off, lens, _ = _hand_result(rows, read_len=read_len)
        names = [b"n" * (1 + (i * 3 + n) % 8) for i in range(n)]
        quals = _quals(reads) if n % 2 else None
        if n == 0:                                               # (no write kernel: its event pair brackets nothing)
            got = bsw.bam_records(eng, res.recs, res.rec_first, res.aln, res.cigar, res.md, reads, off, lens, names, quals,
                                  bsw.rec_opt(**opt), False)
            assert got[0] == b"" and list(got[1]) == [0]
            continue
        want, woff = _gpu_bam(eng, res, reads, off, lens, names, quals, opt, False, f"{n} records of {read_len}")
        assert len(woff) == n + 1
        if n >= 63:
            assert {int(x) & 3 for x in woff[1:]} == {0, 1, 2, 3}
    eng.close()


@pytest.mark.gpu
def test_gpu_pipeline_set_device_to_device_text_and_bam_of_one_batch():
    """bsw_pe_pair_resident -> bsw_records_resident -> bsw_sam_text_resident and bsw_bam_records_resident on the same
    resident arrays, the names uploaded once"""
    s = rec_set()
    p, a = s.p, s.p.arr
    bam, boff = _set_blocks()
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    o = bsw.rec_opt(**s.opt)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], s.quals)
    b.put(mreg=p.mregs, minfo=p.minfo, mfirst=p.mfirst)
    b.pe_pair(p.pes, bsw.pe_opt(l_pac=p.l_pac))
    b.records(o)
    assert b.sam_text(o, s.names, True) == len(s.text)
    assert b.bam_records(o, None, True) == len(bam)              # cap=None: the size from a call with no room
    same_text(s.text, s.text_off, got_text(b), "device to device: text")
    same_text(bam, boff, (b.get("bam").tobytes(), b.get("bam_off")), "device to device: bam")
    st = bsw.bam_last_stats(eng)
    assert st.n_rec == len(s.res.recs) and st.n_bytes == len(bam)
    assert bp.decode(b.get("bam").tobytes(), [RNAME]) == _lines(s.text)
    # the sentinel: a buffer of needed + 16 bytes keeps its last 16
    n = len(bam)
    b.put(bam=np.full(n + 16, 0xA5, np.uint8))
    assert b.bam_records(o, None, True, cap=n + 16) == n
    raw = b.buf["bam"].download(np.zeros(n + 16, np.uint8))
    assert raw[:n].tobytes() == bam and (raw[n:] == 0xA5).all()
    # capacity: one byte short says what is needed and leaves the offsets; the exact capacity succeeds
    b.put(bam=np.full(n + 16, 0xA5, np.uint8), bam_off=np.zeros(len(boff), np.int64))
    with pytest.raises(bsw.BswError, match="-34") as ei:
        b.bam_records(o, None, True, cap=n - 1)
    assert ei.value.needed == n and np.array_equal(b.get("bam_off"), boff)
    assert (b.buf["bam"].download(np.zeros(n + 16, np.uint8)) == 0xA5).all()     # nothing written
    assert b.bam_records(o, None, True, cap=n) == n
    raw = b.buf["bam"].download(np.zeros(n + 16, np.uint8))
    assert raw[:n].tobytes() == bam and (raw[n:] == 0xA5).all()
    eng.close()


@pytest.mark.gpu
def test_gpu_single_end_from_regs_select_resident():
    p = ext_set()
    a = p.arr
    nr_all = len(a["lens"])
    opt = rq.rec_opt(l_pac=p.l_pac, rname=RNAME)
    res = rq.records(p.T, a["reads"], a["off"], a["lens"], p.regs, p.info, p.first, None, opt, p.mat, p.gaps)
    names = [f"r{i}".encode() for i in range(nr_all)]
    quals = (40 + np.arange(len(a["reads"])) % 30).astype(np.uint8)
    bam, boff = bp.encode(res, a["reads"], a["off"], a["lens"], names, quals, opt, False)
    eng = bsw.Engine()
    bsw.set_reference(eng, p.T)
    b = ResidentBatch(eng, a["reads"], a["off"], a["lens"], quals)
    b.put(seeds=a["seeds"], sr=a["sr"], sc=a["sc"])
    b.chain2aln(p.eopt)
    b.select(bsw.sel_opt(l_pac=p.l_pac))
    b.records(bsw.rec_opt(**opt), paired=False)
    b.bam_records(bsw.rec_opt(**opt), names, False, cap=len(bam) + 5)
    same_text(bam, boff, (b.get("bam").tobytes(), b.get("bam_off")), "single-end")
    eng.close()


def _hand_result(rows, read_len=4):
    """one single-end record of its own read per row of (pos, NM, AS, XS, tlen): records and alignments as
    bsw_records* would leave them, built by hand"""
    n = len(rows)
    res = rq.Result()
    res.recs = np.zeros(n, dtype=rq.REC_DTYPE)
    res.aln = np.zeros(n, dtype=rp.ALN_DTYPE)
    res.cigar = np.zeros((n, 2), np.uint32)
    res.md = np.zeros((n, 4), np.uint8)
    res.rec_first = np.arange(n + 1, dtype=np.int32)
    for i, (pos, nm, as_, xs, tlen) in enumerate(rows):
        r, a = res.recs[i], res.aln[i]
        r["pos"], r["mpos"], r["tlen"], r["read"], r["reg"], r["aln"], r["n_list"] = pos, pos, tlen, i, i, i, 1
        r["flag"] = r["sam_flag"] = 0x1
        r["mapq"], r["score"], r["sub"], r["m_aln"], r["xa_first"] = 7, as_, xs, -1, i + 1
        a["pos"], a["n_cigar"], a["NM"], a["score"], a["md_len"] = pos, 1, nm, as_, 1
        res.cigar[i, 0] = read_len << 4
        res.md[i, 0] = ord("0") + read_len
    reads = np.tile(np.array([0, 1, 2, 3, 4, 7], np.uint8), n * read_len // 6 + 1)[:n * read_len].copy()
    off, lens = np.arange(n, dtype=np.int64) * read_len, np.full(n, read_len, np.int32)
    return res, reads, off, lens, [f"h{i}".encode() for i in range(n)]


@pytest.mark.gpu
def test_gpu_hand_built_records_tag_types_and_int32_limits():
    vals = (0, 255, 256, 65535, 65536, -1, -128, -129, -32768, -32769, 2 ** 31 - 1, -2 ** 31)
    rows = [(100 + i, v, 0, 0, 0) for i, v in enumerate(vals)]                        # NM
    rows += [(200 + i, 0, v, -1, -500 - i) for i, v in enumerate(vals)]               # AS; no XS; a negative tlen
    rows += [(300 + i, 0, 0, v, 0) for i, v in enumerate(vals) if v >= 0]             # XS is printed when >= 0
    rows += [(2 ** 31 - 1, 0, 0, 0, 2 ** 31 - 1), (5, 0, 0, 0, -2 ** 31)]             # the last values that fit
    big = 2 ** 33
    opt = rq.rec_opt(l_pac=big, rname=RNAME)
    eng = bsw.Engine()
    res, reads, off, lens, names = _hand_result(rows, read_len=5)
    want, woff = _gpu_bam(eng, res, reads, off, lens, names, None, opt, False, "hand-built")
    lines = bp.decode(want, [RNAME])
    assert lines[1].split("\t")[11] == "NM:i:255" and want[woff[1]:woff[2]].count(b"NMC\xff") == 1
    assert want[woff[2]:woff[3]].count(b"NMS\x00\x01") == 1 and want[woff[4]:woff[5]].count(b"NMI\x00\x00\x01\x00") == 1
    assert lines[12].split("\t")[8] == "-500" and lines[12 + 5].split("\t")[-1] == "AS:i:-1"
    # what int32 cannot hold: BSW_E_RANGE, nothing written
    for bad in ((2 ** 31, 0, 0, 0, 0), (7, 0, 0, 0, 2 ** 31), (7, 0, 0, 0, -2 ** 31 - 1)):
        res, reads, off, lens, names = _hand_result(rows[:3] + [bad] + rows[3:6])
        with pytest.raises(ValueError, match="RANGE"):
            bp.encode(res, reads, off, lens, names, None, opt, False)
        b = ResidentBatch(eng, reads, off, lens)
        b.put(recs=res.recs, rec_first=res.rec_first, aln=res.aln, cigar=res.cigar, md=res.md,
              bam=np.full(4096, 0xA5, np.uint8))
        with pytest.raises(bsw.BswError, match="-34"):
            b.bam_records(bsw.rec_opt(**opt), names, False, cap=4096)
        assert (b.buf["bam"].download(np.zeros(4096, np.uint8)) == 0xA5).all(), bad
    eng.close()


@pytest.mark.gpu
def test_gpu_three_contigs_and_the_header_block():
    eng = bsw.Engine()
    opt = rq.rec_opt(l_pac=L, rname=RNAME)
    assert bsw.bam_header(eng, bsw.rec_opt(**opt)) == bp.header(opt)
    bsw.set_contigs(eng, TAB3.lens, TAB3.names)
    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    assert bsw.bam_header(eng, bsw.rec_opt(**opt), text) == bp.header(opt, text, TAB3)
    with pytest.raises(bsw.BswError, match="-22"):               # the table does not sum to l_pac
        bsw.bam_header(eng, bsw.rec_opt(l_pac=L - 1, rname=RNAME))
    out, nb = np.zeros(8, np.uint8), ctypes.c_int64(0)
    assert bsw.hip_lib().bsw_bam_header(eng._ctx, ctypes.byref(bsw.rec_opt(**opt)), None, 0, bsw._ptr(out), 8,
                                        ctypes.byref(nb)) == -34
    assert nb.value == len(bp.header(opt, b"", TAB3)) and not out.any()
    for mk in (case_pe, case_supp, case_xa):
        c = mk()
        res = _under_table(c)
        reads, off, lens = res.arrays[:3]
        q = _quals(reads)
        want, _ = _gpu_bam(eng, res, reads, off, lens, c.names, q, res.opt, _paired(c), f"table {mk.__name__}", TAB3)
        text, _ = cp.sam_text(TAB3, res, reads, off, lens, c.names, q, res.opt, _paired(c))
        assert bp.decode(want, TAB3.names) == _lines(text)
    with pytest.raises(bsw.BswError, match="-22"):
        bsw.bam_records(eng, res.recs, res.rec_first, res.aln, res.cigar, res.md, reads, off, lens, c.names, None,
                        bsw.rec_opt(l_pac=L - 1, rname=RNAME), _paired(c))
    bsw.set_contigs(eng)
    # a reference too long for l_ref
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.bam_header(eng, bsw.rec_opt(l_pac=2 ** 31, rname=RNAME))
    eng.close()


@pytest.mark.gpu
def test_gpu_capacity_and_range_errors_host_form():
    c = case_pe()
    w = c.run()
    reads, off, lens = w.arrays[:3]
    o = bsw.rec_opt(**w.opt)
    want, woff = bp.encode(w, reads, off, lens, c.names, None, w.opt, True)
    eng = bsw.Engine()
    args = (w.rec_first, w.aln, w.cigar, w.md, reads, off, lens, c.names, None, o, True)
    with pytest.raises(bsw.BswError, match="-34") as ei:
        bsw.bam_records(eng, w.recs, *args, bam_cap=len(want) - 1)
    assert ei.value.needed == len(want) and np.array_equal(ei.value.bam_off, woff)
    same_text(want, woff, bsw.bam_records(eng, w.recs, *args, bam_cap=len(want)), "exact capacity")
    bad = w.recs.copy()
    bad[0]["aln"] = len(w.aln)
    with pytest.raises(bsw.BswError, match="-34"):
        bsw.bam_records(eng, bad, *args)
    same_text(want, woff, bsw.bam_records(eng, w.recs, *args), "after the errors")
    eng.close()
