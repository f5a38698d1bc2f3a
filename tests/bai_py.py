"""Coordinate sort and the .bai in Python (include/bsw_bamsort.h) -- TEST INFRASTRUCTURE (tests/test_bamsort.py), numpy
and the standard library only.

  record   a minimal valid BAM alignment block from a few fields
  sort     the header's key over numpy's stable sort -> blocks, offsets, permutation
  build    the header's index rules restated -> the .bai file's bytes
  parse    the file back into its parts
  query    an independent reader that follows SAMv1 section 5 from the query's side: candidate bins (reg2bins), their
           chunks, the linear index as a floor, a seek by virtual offset into the BGZF stream, records read to the
           chunk's end.  It shares no code with build beyond reg2bin's scheme.
  brute    the records that overlap a region, by looking at every record

[SPEC-RECALL: SAMv1 section 4.2, 5.1.1, 5.2, 5.3]: no htslib, samtools or sample index is at hand."""

import struct

import numpy as np

import bam_py as bp
import bgzf_py as gz

OPS = "MIDNSHP=X"
REF_OPS = {0, 2, 3, 7, 8}            # M D N = X consume the reference
PSEUDO_BIN = 37450
reg2bin = bp.reg2bin


def cigar_words(cigar):
    """"10M40000D10M" or [(10, "M"), ...] -> the uint32 words"""
    if isinstance(cigar, str):
        out, num = [], ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                out.append((int(num), ch))
                num = ""
        cigar = out
    return [n << 4 | OPS.index(op) for n, op in cigar]


def record(rid, pos, flag=0, cigar=(), name=b"r", l_seq=0, mapq=0, next_rid=-1, next_pos=-1, tlen=0, tags=b"", bin_field=None):
    """one alignment block with its block_size; SEQ all A, QUAL 0xff.  bin_field: the bin the block carries (the index
    has to ignore it); None: the specification's"""
    words = cigar_words(cigar)
    rlen = sum(w >> 4 for w in words if (w & 15) in REF_OPS)
    if bin_field is None:
        bin_field = reg2bin(pos, pos + (rlen if rlen else 1)) & 0xffff
    body = struct.pack("<iiBBHHHiiii", rid, pos, len(name) + 1, mapq, bin_field, len(words), flag, l_seq, next_rid, next_pos, tlen)
    body += name + b"\0" + struct.pack(f"<{len(words)}I", *words) + b"\x11" * ((l_seq + 1) // 2) + b"\xff" * l_seq + tags
    return struct.pack("<i", len(body)) + body


def join(blocks):
    """blocks -> (bytes, off int64 [n + 1])"""
    off = np.zeros(len(blocks) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in blocks])
    return b"".join(blocks), off


def split(data, off):
    return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def extent(block):
    """(refID, beg, end, flag) of a block (with its block_size)"""
    f = bp.fields(block[4:])
    at = 36 + f["l_read_name"]
    words = struct.unpack_from(f"<{f['n_cigar_op']}I", block, at)
    rlen = sum(w >> 4 for w in words if (w & 15) in REF_OPS)
    return f["refID"], f["pos"], f["pos"] + (rlen if rlen else 1), f["flag"]


def sort(blocks, n_ref):
    """-> (sorted blocks, perm): the key (refID < 0 ? n_ref : refID, pos + 1, flag & 0x10), stable"""
    if not blocks:
        return [], np.zeros(0, np.int32)
    f = [bp.fields(b[4:]) for b in blocks]
    rid = np.array([n_ref if x["refID"] < 0 else x["refID"] for x in f], np.int64)
    pos = np.array([x["pos"] + 1 for x in f], np.int64)
    rev = np.array([x["flag"] & 0x10 for x in f], np.int64)
    perm = np.lexsort((rev, pos, rid))              # stable; the last key is the primary one
    return [blocks[i] for i in perm], perm.astype(np.int32)


def build(blocks, voff, end_voff, ref_len):
    """the .bai of sorted blocks with virtual offsets voff [n] and end_voff behind the last"""
    n_ref = len(ref_len)
    vend = [int(v) for v in voff[1:]] + [int(end_voff)]
    refs = [dict(bins={}, lin={}, first=None, last=None, mapped=0, unmapped=0) for _ in range(n_ref)]
    n_no_coor = 0
    for i, b in enumerate(blocks):
        rid, beg, end, flag = extent(b)
        if rid < 0:
            n_no_coor += 1
            continue
        assert 0 <= beg and end <= ref_len[rid], "BSW_E_RANGE"
        R = refs[rid]
        v = int(voff[i])
        if R["first"] is None:
            R["first"] = v
        R["last"] = vend[i]
        R["unmapped" if flag & 4 else "mapped"] += 1
        chunks = R["bins"].setdefault(reg2bin(beg, end), [])
        if chunks and not (v >> 16) > (chunks[-1][2] >> 16):
            chunks[-1][1] = chunks[-1][2] = vend[i]
        else:
            chunks.append([v, vend[i], vend[i]])     # beg, end, vend of the last member
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            R["lin"][w] = min(R["lin"].get(w, v), v)
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for R in refs:
        has = R["first"] is not None
        out += struct.pack("<i", len(R["bins"]) + (1 if has else 0))
        for b in sorted(R["bins"]):
            out += struct.pack("<Ii", b, len(R["bins"][b]))
            for c in R["bins"][b]:
                out += struct.pack("<QQ", c[0], c[1])
        if has:
            out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["first"], R["last"], R["mapped"], R["unmapped"])
        n_intv = max(R["lin"]) + 1 if R["lin"] else 0
        out += struct.pack("<i", n_intv)
        nxt, vals = None, []
        for w in range(n_intv - 1, -1, -1):
            nxt = R["lin"].get(w, nxt)
            vals.append(nxt)
        out += struct.pack(f"<{n_intv}Q", *vals[::-1])
    return out + struct.pack("<Q", n_no_coor)


def parse(bai):
    """-> (refs, n_no_coor); a ref: dict(bins {bin: [(beg, end)]} without the pseudo-bin, order [bins as filed],
    pseudo ((beg, end), (n_mapped, n_unmapped)) or None, ioffset [n_intv])"""
    assert bai[:4] == b"BAI\1", bai[:4]
    (n_ref,) = struct.unpack_from("<i", bai, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", bai, at)
        at += 4
        R = dict(bins={}, order=[], pseudo=None, ioffset=[])
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            R["order"].append(b)
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and R["pseudo"] is None
                R["pseudo"] = (chunks[0], chunks[1])
            else:
                assert b not in R["bins"] and b < PSEUDO_BIN - 1 and n_chunk > 0
                R["bins"][b] = chunks
        (n_intv,) = struct.unpack_from("<i", bai, at)
        at += 4
        R["ioffset"] = list(struct.unpack_from(f"<{n_intv}Q", bai, at))
        at += 8 * n_intv
        refs.append(R)
    (n_no_coor,) = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai), f"{len(bai) - at - 8} bytes behind n_no_coor"
    return refs, n_no_coor


# ---------------------------------------------------------------- the reader
def reg2bins(beg, end):
    """SAMv1 section 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class Stream:
    """a BGZF stream of alignment blocks, walked once: virtual offset -> position in the uncompressed bytes"""

    def __init__(self, stream, base_coffset=0):
        blocks = gz.data_blocks(gz.walk(stream))
        self.at, self.data, total = {}, b"".join(b.data for b in blocks), 0
        for b in blocks:
            self.at[b.off + base_coffset] = (total, len(b.data))
            total += len(b.data)
        self.at[len(stream) - (len(gz.EOF) if stream.endswith(gz.EOF) else 0) + base_coffset] = (total, 0)

    def pos(self, voff):
        start, size = self.at[int(voff) >> 16]      # KeyError: no block starts there
        assert (int(voff) & 0xffff) <= size, "a virtual offset behind its block"
        return start + (int(voff) & 0xffff)


def query(bai, stream, rid, beg, end):
    """positions in the uncompressed bytes of the records that overlap [beg, end) of reference rid, found through the
    index alone.  bai: the file's bytes, or what parse made of them; stream: a Stream."""
    refs, _ = parse(bai) if isinstance(bai, (bytes, bytearray)) else bai
    R = refs[rid]
    w = beg >> 14
    floor = R["ioffset"][w] if w < len(R["ioffset"]) else None
    if floor is None:
        return []                                    # no record reaches the window of beg or any behind it
    found = set()
    for b in reg2bins(beg, end):
        for cb, ce in R["bins"].get(b, ()):
            if ce <= floor:
                continue
            p, stop = stream.pos(cb), stream.pos(ce)
            while p < stop:
                (size,) = struct.unpack_from("<i", stream.data, p)
                f = bp.fields(stream.data[p + 4:p + 36])
                words = struct.unpack_from(f"<{f['n_cigar_op']}I", stream.data, p + 36 + f["l_read_name"])
                rlen = sum(x >> 4 for x in words if (x & 15) in REF_OPS)
                if f["refID"] == rid and f["pos"] < end and f["pos"] + max(rlen, 1) > beg:
                    found.add(p)
                p += 4 + size
            assert p == stop, "a chunk ends inside a record"
    return sorted(found)


def brute(blocks, off, rid, beg, end, extents=None):
    """the same by looking at every record: their offsets.  extents: [extent(b) for b in blocks], when the caller
    asks more than once"""
    out = []
    for i, (r, rb, re_, _) in enumerate(extents if extents is not None else map(extent, blocks)):
        if r == rid and rb < end and re_ > beg:
            out.append(int(off[i]))
    return out
