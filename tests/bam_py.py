"""Pure-Python restatement of the BAM alignment blocks and the header block as include/bsw_bam.h states
them -- TEST INFRASTRUCTURE (tests/test_bam.py), numpy and the standard library only.

  encode    rec_py's Result (or contigs_py's, with its table) -> the blocks and their offsets
  decode    an independent reader, written from the header's table: blocks -> SAM lines.  decode(encode(x))
            has to be rec_py.sam_text(x) (contigs_py.sam_text under a table) line for line, which ties this
            restatement to the text that is already pinned
  header    the uncompressed header block

[SPEC-RECALL: SAMv1 section 4.2, htslib's sam_parse1 for the integer tag types]: no htslib, samtools or sample
BAM file is at hand; the known answers of test_bam.py are derived by hand from the specification."""

import struct

import numpy as np

import rec_py as rq

INT32_MAX = 2 ** 31 - 1
MAX_NAME = 254
NIBBLE = "=ACMGRSVTWYHKDBN"           # SAMv1: the base of a 4-bit code


def reg2bin(beg, end):
    """SAMv1 section 5.3: the bin of the 0-based half-open [beg, end); 14-bit smallest bin, 5 levels"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def int_tag(tag, v):
    """an integer tag with the smallest type that holds v, as the text parser picks it"""
    if v >= 0:
        t, f = ("C", "<B") if v <= 0xff else ("S", "<H") if v <= 0xffff else ("I", "<I")
    else:
        t, f = ("c", "<b") if v >= -128 else ("s", "<h") if v >= -32768 else ("i", "<i")
    return tag.encode() + t.encode() + struct.pack(f, v)


def _z_tag(tag, s):
    return tag.encode() + b"Z" + s + b"\0"


def _place(tab, pos):
    """(rid, offset) of a global forward position"""
    if tab is None:
        return 0, 0
    k = tab.rid(int(pos))
    return k, tab.off[k]


def _ref_name(tab, opt, pos):
    return opt["rname"].encode() if tab is None else tab.names[_place(tab, pos)[0]]


def _cigar_text(words):
    return "".join(f"{int(w) >> 4}{'MIDSH'[int(w) & 15]}" for w in words).encode()


def encode(res, reads, off, lens, names, quals, opt, paired, contigs=None):
    """the library's bsw_bam_records: -> (bytes, bam_off int64 [n_rec + 1]); raises ValueError where the
    library returns BSW_E_RANGE"""
    tab = contigs
    soft = bool(opt["flags"] & rq.SOFTCLIP)
    out, offs, total = [], [0], 0
    for p in res.recs:
        r, which = int(p["read"]), int(p["which"])
        name = names[r >> 1 if paired else r]
        if len(name) > MAX_NAME:
            raise ValueError("BSW_E_RANGE: name")
        if not -2 ** 31 <= int(p["tlen"]) <= INT32_MAX:
            raise ValueError("BSW_E_RANGE: tlen")
        n_cig = int(res.aln[p["aln"]]["n_cigar"]) if p["aln"] >= 0 else 0
        cg = [int(w) for w in res.cigar[p["aln"], :n_cig]] if n_cig else []
        rid = mrid = pos = mpos = -1
        if p["pos"] >= 0:
            rid, base = _place(tab, p["pos"])
            pos = int(p["pos"]) - base
        if p["mpos"] >= 0:
            mrid, base = _place(tab, p["mpos"])
            mpos = int(p["mpos"]) - base
        if pos > INT32_MAX or mpos > INT32_MAX:
            raise ValueError("BSW_E_RANGE: pos")
        # the clip letter the text prints: S for record 0, H for the others, as stored under SOFTCLIP
        ops = []
        for w in cg:
            op = w & 15
            if op >= 3:
                op = (4 if op == 3 else 5) if soft else (5 if which else 4)
            ops.append((w >> 4) << 4 | op)
        l = int(lens[r])
        qb, qe = 0, l
        if n_cig and which and not soft:
            c5 = cg[0] >> 4 if (cg[0] & 15) >= 3 else 0
            c3 = cg[-1] >> 4 if (cg[-1] & 15) >= 3 else 0
            qb, qe = (c3, l - c5) if p["is_rev"] else (c5, l - c3)
        seq = [min(int(c), 4) for c in reads[int(off[r]) + qb:int(off[r]) + qe]]
        ql = None if quals is None else [int(q) for q in quals[int(off[r]) + qb:int(off[r]) + qe]]
        if p["is_rev"]:
            seq = [3 - c if c < 4 else 4 for c in seq[::-1]]
            ql = None if ql is None else ql[::-1]
        nib = [(1, 2, 4, 8, 15)[c] for c in seq] + [0]
        packed = bytes(nib[2 * i] << 4 | nib[2 * i + 1] for i in range((len(seq) + 1) // 2))
        qbytes = b"\xff" * len(seq) if ql is None else bytes((q - 33) & 0xff for q in ql)
        end = pos + (rq._rlen(cg) if n_cig else 1)
        body = struct.pack("<iiBBHHHiiii", rid, pos, len(name) + 1, int(p["mapq"]) if p["pos"] >= 0 else 0,
                           reg2bin(pos, end) & 0xffff, n_cig, int(p["sam_flag"]), len(seq), mrid, mpos, int(p["tlen"]))
        body += name + b"\0" + struct.pack(f"<{len(ops)}I", *ops) + packed + qbytes
        clip = "" if soft else ("H" if which else "S")
        if n_cig:
            a = res.aln[p["aln"]]
            body += int_tag("NM", int(a["NM"])) + _z_tag("MD", bytes(res.md[p["aln"], :int(a["md_len"])]))
        if p["m_aln"] >= 0:
            m = res.aln[p["m_aln"]]
            body += _z_tag("MC", rq._cigar(res.cigar[p["m_aln"], :int(m["n_cigar"])], clip).encode())
        body += int_tag("AS", int(p["score"]))
        if p["sub"] >= 0:
            body += int_tag("XS", int(p["sub"]))
        if not p["flag"] & 0x100:
            f0 = int(res.rec_first[r])
            s = b""
            for j in range(int(p["n_list"])):
                q = res.recs[f0 + j]
                if j == which or q["flag"] & 0x100:
                    continue
                a = res.aln[q["aln"]]
                s += b"%s,%d,%s,%s,%d,%d;" % (_ref_name(tab, opt, a["pos"]), int(a["pos"]) - _place(tab, a["pos"])[1] + 1,
                                               b"+-"[int(a["is_rev"]):][:1], _cigar_text(res.cigar[q["aln"], :int(a["n_cigar"])]),
                                               int(q["mapq"]), int(a["NM"]))
            if s:
                body += _z_tag("SA", s)
        if p["xa_n"] > 0:
            s = b""
            for j in range(int(p["xa_first"]), int(p["xa_first"]) + int(p["xa_n"])):
                a = res.aln[j]
                s += b"%s,%s%d,%s,%d;" % (_ref_name(tab, opt, a["pos"]), b"+-"[int(a["is_rev"]):][:1],
                                          int(a["pos"]) - _place(tab, a["pos"])[1] + 1,
                                          _cigar_text(res.cigar[j, :int(a["n_cigar"])]), int(a["NM"]))
            body += _z_tag("XA", s)
        out.append(struct.pack("<i", len(body)) + body)
        total += 4 + len(body)
        offs.append(total)
    return b"".join(out), np.array(offs, dtype=np.int64)


# ---------------------------------------------------------------- the reader
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def blocks(data):
    """the alignment blocks of a stream of them, each without its block_size"""
    out, at = [], 0
    while at < len(data):
        (n,) = struct.unpack_from("<i", data, at)
        assert n >= 32 and at + 4 + n <= len(data), f"block_size {n} at byte {at} of {len(data)}"
        out.append(data[at + 4:at + 4 + n])
        at += 4 + n
    return out


def fields(block):
    """the fixed fields of one block (without block_size) as a dict"""
    keys = ("refID", "pos", "l_read_name", "mapq", "bin", "n_cigar_op", "flag", "l_seq", "next_refID", "next_pos", "tlen")
    return dict(zip(keys, struct.unpack_from("<iiBBHHHiiii", block, 0)))


def decode(data, ref_names):
    """uncompressed alignment blocks -> the SAM lines a reader prints for them (samtools view's conventions: `=`
    for an RNEXT equal to RNAME, `*` for no reference, no CIGAR and absent qualities)"""
    names = [s.decode("latin-1") if isinstance(s, bytes) else s for s in ref_names]
    lines = []
    for b in blocks(data):
        f = fields(b)
        at = 32
        qname = b[at:at + f["l_read_name"] - 1].decode("latin-1")
        assert b[at + f["l_read_name"] - 1] == 0, "read_name is not NUL-terminated"
        at += f["l_read_name"]
        cig = struct.unpack_from(f"<{f['n_cigar_op']}I", b, at)
        at += 4 * f["n_cigar_op"]
        n = f["l_seq"]
        packed = b[at:at + (n + 1) // 2]
        at += (n + 1) // 2
        seq = "".join(NIBBLE[packed[i >> 1] >> 4 if i % 2 == 0 else packed[i >> 1] & 15] for i in range(n))
        assert n % 2 == 0 or packed[-1] & 15 == 0, "the unused nibble is not 0"
        qual = b[at:at + n]
        at += n
        t = [qname, str(f["flag"]), names[f["refID"]] if f["refID"] >= 0 else "*", str(f["pos"] + 1), str(f["mapq"]),
             "".join(f"{w >> 4}{'MIDNSHP=X'[w & 15]}" for w in cig) or "*"]
        t += ["*" if f["next_refID"] < 0 else "=" if f["next_refID"] == f["refID"] else names[f["next_refID"]],
              str(f["next_pos"] + 1), str(f["tlen"]), seq,
              "*" if n and all(q == 0xff for q in qual) else bytes(q + 33 for q in qual).decode("latin-1")]
        while at < len(b):
            tag, ty = b[at:at + 2].decode(), chr(b[at + 2])
            at += 3
            if ty == "Z":
                e = b.index(b"\0", at)
                t.append(f"{tag}:Z:{b[at:e].decode('latin-1')}")
                at = e + 1
            else:
                (v,) = struct.unpack_from(_INT[ty], b, at)
                at += struct.calcsize(_INT[ty])
                t.append(f"{tag}:i:{v}")
        assert at == len(b), "the tags overrun the block"
        lines.append("\t".join(t))
    return lines


# ---------------------------------------------------------------- the header block
def header(opt, sam_text=b"", contigs=None):
    """the library's bsw_bam_header"""
    if contigs is None:
        refs = [(opt["rname"].encode(), int(opt["l_pac"]))]
    else:
        if contigs.sum != opt["l_pac"]:
            raise ValueError("BSW_E_INVAL: l_pac is not the sum of the contig lengths")
        refs = list(zip(contigs.names, contigs.lens))
    if any(l > INT32_MAX for _, l in refs):
        raise ValueError("BSW_E_RANGE: a reference longer than INT32_MAX")
    out = b"BAM\1" + struct.pack("<i", len(sam_text)) + sam_text + struct.pack("<i", len(refs))
    for name, l in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", l)
    return out
