"""ResidentBatch: the device arrays of one batch of reads and the resident stage chain over them,

    seeds -> chain2aln -> select -> pe_stat -> matesw -> pe_pair -> reg2aln / records -> sam_text / bam_records -> bgzf
    (duplicates marked: records -> mark_duplicates -> sam_text / bam_records)
    (coordinate-sorted and indexed: bam_records -> bam_sort -> bgzf(src="sbam") -> bam_index)

Plumbing for tests and tools, like bsw.py: every stage method is one bsw.*_resident call on the buffers the
stage before left in HBM.  Importing this module loads no library and touches no device.
"""

from __future__ import annotations

import ctypes

import numpy as np

import bsw
import hiprt

# buffer name -> (dtype, row shape: the names of the strides a row has, the count that trims it).
# Every allocation is sized from this table; a dotted name ("all.aln") has the layout of its last part
# and counts of its own ("all.aln").  ("bam" / "bam_off" are not here: BAM_LAYOUT below; _row reads both.)
LAYOUT = {
    "reads": (np.uint8, (), "reads"), "quals": (np.uint8, (), "reads"),
    "off": (np.int64, (), "n_reads"), "lens": (np.int32, (), "n_reads"), "frac_rep": (np.float32, (), "n_reads"),
    "seeds": (bsw.SEED_DTYPE, (), "seeds"), "sr": (np.int32, (), "seeds"), "sc": (np.int32, (), "seeds"),
    "csub": (np.int32, (), "seeds"), "regs": (bsw.ALNREG_DTYPE, (), "seeds"), "ext": (np.int32, (), "seeds"),
    # the selection's lists and the rescue's: (regs, read, info, first)
    "sreg": (bsw.ALNREG_DTYPE, (), "sreg"), "sread": (np.int32, (), "sreg"), "sinfo": (bsw.SELINFO_DTYPE, (), "sreg"),
    "sfirst": (np.int32, (), "first"),
    "mreg": (bsw.ALNREG_DTYPE, (), "mreg"), "mread": (np.int32, (), "mreg"), "minfo": (bsw.SELINFO_DTYPE, (), "mreg"),
    "mfirst": (np.int32, (), "first"),
    "pairs": (bsw.PAIR_DTYPE, (), "pairs"),
    "aln": (bsw.ALN_DTYPE, (), "aln"), "cigar": (np.uint32, ("cigar",), "aln"), "md": (np.uint8, ("md",), "aln"),
    "aln_reg": (np.int32, (), "aln"),
    "recs": (bsw.REC_DTYPE, (), "recs"), "rec_first": (np.int32, (), "first"),
    "names": (np.uint8, (), "names"), "name_off": (np.int64, (), "name_off"),
    "text": (np.uint8, (), "text"), "text_off": (np.int64, (), "text_off"),
}
# the BAM form of the records (bsw_bam.h), rows of the same shape in a table of their own: LAYOUT's entries and
# their item sizes are pinned one by one (tests/test_resident.py)
BAM_LAYOUT = {"bam": (np.uint8, (), "bam"), "bam_off": (np.int64, (), "bam_off")}
# the BGZF form of the BAM blocks (bsw_bgzf.h), in a table of its own likewise
BGZF_LAYOUT = {"bgzf": (np.uint8, (), "bgzf"), "bgzf_blk": (np.int64, (), "bgzf_blk"), "bgzf_voff": (np.int64, (), "bgzf_voff")}
# the coordinate-sorted blocks and their index (bsw_bamsort.h), in a table of its own likewise
SORT_LAYOUT = {"sbam": (np.uint8, (), "sbam"), "sbam_off": (np.int64, (), "sbam_off"), "bam_perm": (np.int32, (), "bam_perm"),
               "bai": (np.uint8, (), "bai")}
# the reads' duplicate marks (bsw_markdup.h), in a table of its own likewise
DUP_LAYOUT = {"dup": (np.uint8, (), "n_reads")}
FIXED = ("reads", "n_reads", "first")           # counts the constructor sets for good
# (regs, read, info, first) as the extension, the selection and the rescue leave them
LISTS = {"c": ("regs", "sr", None, None), "s": ("sreg", "sread", "sinfo", "sfirst"), "m": ("mreg", "mread", "minfo", "mfirst")}


def _row(name):
    """(dtype, stride keys, count key) of a buffer name"""
    pre, dot, base = name.rpartition(".")
    table = next((t for t in (LAYOUT, BAM_LAYOUT, BGZF_LAYOUT, SORT_LAYOUT, DUP_LAYOUT) if base in t), None)
    if table is None:
        raise ValueError(f"no buffer named '{name}'")
    dtype, strides, key = table[base]
    return np.dtype(dtype), tuple(pre + dot + s for s in strides), pre + dot + key


class ResidentBatch:
    """buf[name]: hiprt.DeviceBuffer, n[key]: the counts (n["sreg"], n["mreg"], n["aln"], ...), stride: the CIGAR
    and MD row lengths.  The current lists (regs, read, info, first) are those of the last stage that left
    regions: chain2aln (one region per seed, no info), select, then matesw, whose outputs replace the selection's;
    pe_stat, pe_pair, reg2aln and records read whichever are current (cur: "c", "s" or "m"; it may be set, to
    read an earlier stage's lists again)."""

    def __init__(self, engine, reads, read_off, read_len, quals=None):
        self.read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        self.read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        if len(self.read_off) != len(self.read_len):
            raise ValueError(f"{len(self.read_off)} read offsets for {len(self.read_len)} read lengths")
        if quals is not None and len(quals) != len(reads):
            raise ValueError("quals are not parallel to reads")
        self.engine, self.n_reads = engine, len(self.read_len)
        self.buf, self.stride, self.cur = {}, {}, "c"
        self.n = {"reads": len(reads), "n_reads": self.n_reads, "first": self.n_reads + 1}
        self.put(reads=reads, off=self.read_off, lens=self.read_len, **({} if quals is None else {"quals": quals}))

    # ---------------------------------------------------------------- buffers
    def alloc(self, name, count):
        """buf[name] with room for count rows (at least one): allocated only when missing or smaller.  Strided
        rows (CIGAR, MD) are filled only in part by the kernels: they are zeroed here, once."""
        dtype, strides, _ = _row(name)
        nbytes = max(count, 1) * dtype.itemsize
        for s in strides:
            nbytes *= max(self.stride[s], 1)
        b = self.buf.get(name)
        if b is None or b.nbytes < nbytes:
            b = self.buf[name] = hiprt.DeviceBuffer(nbytes)
            if strides:
                hiprt.check(hiprt.rt().hipMemset(ctypes.c_void_p(b.ptr), 0, nbytes))
        return b

    def put(self, **arrays):
        """upload host arrays as named buffers and set their counts"""
        host, counts = {}, {}
        for name, a in arrays.items():
            dtype, strides, key = _row(name)
            a = host[name] = np.ascontiguousarray(a, dtype=dtype)
            if a.ndim != 1 + len(strides) or len(a) != (self.n[key] if key in FIXED else counts.setdefault(key, len(a))):
                raise ValueError(f"put({name}): shape {a.shape} does not fit '{key}'")
        for name, a in host.items():
            self.stride.update(zip(_row(name)[1], a.shape[1:]))
            self.cur = {"regs": "c", "sreg": "s", "mreg": "m"}.get(name, self.cur)
            b = self.alloc(name, len(a))
            if a.nbytes:
                b.upload(a)
        self.n.update(counts)

    def get(self, name):
        """download one buffer, trimmed to its count, with the table's dtype and shape"""
        dtype, strides, key = _row(name)
        self._have("get", name)
        out = np.zeros((self.n[key],) + tuple(self.stride[s] for s in strides), dtype=dtype)
        return self.buf[name].download(out) if out.nbytes else out

    def _have(self, stage, *names):
        for name in names:
            if name not in self.buf:
                raise ValueError(f"{stage}: no {name!r} buffer yet: run the stage that leaves it, or put() it")

    def _p(self, *names):
        return [self.buf[x].ptr for x in names]

    @property
    def lists(self):
        """names of the current (regs, read, info, first) and their count"""
        names = LISTS[self.cur]
        return names, self.n.get(_row(names[0])[2])

    # ---------------------------------------------------------------- stages
    def seed_and_chain(self, fmi, cap=256, mopt=None, copt=None):
        """bsw.seed_and_chain over the resident reads; adopts its buffers.  Returns its host (seeds, sr, sc)."""
        host, dev, (d_off, d_len) = bsw.seed_and_chain(fmi, self.buf["reads"], self.read_off, self.read_len, cap, mopt, copt)
        self.buf.update(seeds=dev[0], sr=dev[1], sc=dev[2], off=d_off, lens=d_len)
        self.n["seeds"] = len(host[0])
        return host

    def chain2aln(self, eopt):
        self._have("chain2aln", "seeds", "sr", "sc")
        ns = self.n["seeds"]
        out = [self.alloc(x, ns).ptr for x in ("regs", "ext")]
        bsw.chain2aln_resident(self.engine, *self._p("reads", "off", "lens"), self.n_reads, *self._p("seeds", "sr", "sc"), ns,
                               *out, eopt)
        self.cur = "c"

    def select(self, sopt, csub=None, frac_rep=None) -> int:
        """the selection's lists become the current ones; csub / frac_rep: host arrays per seed / per read"""
        self._have("select", "seeds", "sr", "sc", "regs", "ext")
        ns = self.n["seeds"]
        if csub is not None and len(csub) != ns:
            raise ValueError(f"select: {len(csub)} csub for {ns} seeds")
        self.put(**{k: v for k, v in (("csub", csub), ("frac_rep", frac_rep)) if v is not None})
        out = [self.alloc(x, ns).ptr for x in ("sreg", "sread", "sinfo")] + [self.alloc("sfirst", self.n_reads + 1).ptr]
        k = bsw.regs_select_resident(self.engine, *self._p("reads", "off", "lens"), self.n_reads,
                                     *self._p("seeds", "sr", "sc", "regs", "ext"), ns, *out, ns, sopt,
                                     d_csub=0 if csub is None else self.buf["csub"].ptr,
                                     d_frac_rep=0 if frac_rep is None else self.buf["frac_rep"].ptr)
        self.n["sreg"], self.cur = k, "s"
        return k

    def pe_stat(self, popt):
        (regs, _, info, first), k = self.lists
        self._have("pe_stat", regs, info, first)
        return bsw.pe_stat_resident(self.engine, *self._p(regs, info, first), self.n_reads, k, popt)

    def matesw(self, pes, mopt, cap=None) -> int:
        """reads the selection's lists; afterwards the rescue's outputs are the current lists"""
        self._have("matesw", "sreg", "sinfo", "sfirst")
        k = self.n["sreg"]
        cap = k + 4 * mopt.max_matesw * self.n_reads if cap is None else cap
        out = [self.alloc(x, cap).ptr for x in ("mreg", "mread", "minfo")] + [self.alloc("mfirst", self.n_reads + 1).ptr]
        m = bsw.matesw_resident(self.engine, pes, *self._p("reads", "off", "lens"), self.n_reads,
                                *self._p("sreg", "sinfo", "sfirst"), k, *out, cap, mopt)
        self.n["mreg"], self.cur = m, "m"
        return m

    def pe_pair(self, pes, popt):
        """updates the current regs and info in place (their read column stays valid), writes pairs"""
        (regs, _, info, first), k = self.lists
        self._have("pe_pair", regs, info, first)
        self.n["pairs"] = self.n_reads // 2
        bsw.pe_pair_resident(self.engine, pes, *self._p(regs, info, first), self.n_reads, k,
                             self.alloc("pairs", self.n["pairs"]).ptr, popt)

    def _rows(self, pre, cigar_stride, md_stride):
        """a change of stride gives up the old rows: what lies between the new ones would not be zero"""
        for s, v in (("cigar", cigar_stride), ("md", md_stride)):
            if self.stride.get(pre + s) != v:
                self.stride[pre + s] = v
                self.buf.pop(pre + s, None)

    def reg2aln(self, eopt, cigar_stride=16, md_stride=64, into="aln"):
        """every current region -> into ("aln", or "x.aln" for outputs of its own: "x.aln", "x.cigar", "x.md")"""
        (regs, read, _, _), k = self.lists
        self._have("reg2aln", regs, read)
        pre = into[:-len("aln")]
        if not into.endswith("aln") or (pre and not pre.endswith(".")):
            raise ValueError(f"reg2aln: into='{into}' is neither 'aln' nor 'x.aln'")
        self._rows(pre, cigar_stride, md_stride)
        aln, cig, md = (self.alloc(pre + x, k).ptr for x in ("aln", "cigar", "md"))
        self.n[into] = k
        bsw.reg2aln_resident(self.engine, *self._p("reads", "off", "lens"), self.n_reads, *self._p(regs, read), k, aln, cig,
                             cigar_stride, md if md_stride else 0, md_stride, eopt)

    def records(self, ropt, cigar_stride=16, md_stride=64, paired=True):
        (regs, _, info, first), k = self.lists
        self._have("records", regs, info, first, *(("pairs",) if paired else ()))
        self._rows("", cigar_stride, md_stride)
        rc = self.n_reads + k
        out = [self.alloc("recs", rc).ptr, self.alloc("rec_first", self.n_reads + 1).ptr, rc] + \
              [self.alloc(x, k).ptr for x in ("aln", "aln_reg", "cigar")] + [cigar_stride, self.alloc("md", k).ptr, md_stride, k]
        self.n["recs"], self.n["aln"] = bsw.records_resident(
            self.engine, *self._p("reads", "off", "lens"), self.n_reads, *self._p(regs, info, first), k,
            self.buf["pairs"].ptr if paired else 0, *out, ropt)
        return self.n["recs"], self.n["aln"]

    def mark_duplicates(self, dopt, paired=True):
        """between records() and sam_text() / bam_records(): 0x400 set or cleared on "recs" in place, the reads' marks
        in "dup" (bsw.BSW_DUP_*).  Returns bsw.markdup_last_stats."""
        self._have("mark_duplicates", "recs", "rec_first", "aln", "cigar")
        quals = self.buf.get("quals")
        bsw.mark_duplicates_resident(self.engine, *self._p("recs", "rec_first"), self.n["recs"], *self._p("aln", "cigar"),
                                     self.stride["cigar"], self.n["aln"], *self._p("off", "lens"), self.n_reads,
                                     0 if quals is None else quals.ptr, 0 if quals is None else self.n["reads"], paired,
                                     self.alloc("dup", self.n_reads).ptr, dopt)
        return bsw.markdup_last_stats(self.engine)

    def _records_out(self, stage, fn, out, ropt, names, paired, cap):
        """call 2 in either form: fn = bsw.sam_text_resident into "text" / "text_off", or bsw.bam_records_resident
        into "bam" / "bam_off" """
        self._have(stage, "recs", "rec_first", "aln", "cigar", "md")
        if names is not None:
            if len(names) != (self.n_reads // 2 if paired else self.n_reads):
                raise ValueError(f"{stage}: {len(names)} names for {self.n_reads} reads, paired={paired}")
            nm, nm_off = bsw._names_host(names)
            self.put(names=nm, name_off=nm_off)
        self._have(stage, "names", "name_off")
        n_rec = self.n["recs"]
        toff = self.alloc(out + "_off", n_rec + 1).ptr

        def call(d_text, cap):
            return fn(self.engine, *self._p("recs", "rec_first"), n_rec, *self._p("aln", "cigar"),
                      self.stride["cigar"], self.buf["md"].ptr, self.stride["md"], self.n["aln"],
                      *self._p("reads", "off", "lens"), self.n_reads, *self._p("names", "name_off"),
                      self.buf["quals"].ptr if "quals" in self.buf else 0, paired, d_text, toff, cap, ropt)

        if cap is None:
            try:
                cap = call(0, 0)
            except bsw.BswError as e:
                if getattr(e, "needed", -1) <= 0:
                    raise
                cap = e.needed
        self.n[out], self.n[out + "_off"] = call(self.alloc(out, cap).ptr, cap), n_rec + 1
        return self.n[out]

    def sam_text(self, ropt, names, paired, cap=None) -> int:
        """names: a list of bytes (one per read, or per pair), uploaded; None: the names of the call before.
        cap=None: one call with no room that says how many bytes are needed, then the call with exactly those."""
        return self._records_out("sam_text", bsw.sam_text_resident, "text", ropt, names, paired, cap)

    def bam_records(self, ropt, names, paired, cap=None) -> int:
        """the same records as BAM alignment blocks ("bam", "bam_off"); names=None reuses the uploaded names, so
        text and BAM of one batch come from one upload"""
        return self._records_out("bam_records", bsw.bam_records_resident, "bam", ropt, names, paired, cap)

    def bam_sort(self, n_ref) -> int:
        """the BAM blocks ("bam", "bam_off") in coordinate order: "sbam", "sbam_off" and "bam_perm", the input index of
        every output record.  Returns the bytes."""
        self._have("bam_sort", "bam", "bam_off")
        n_in, n_rec = self.n["bam"], self.n["bam_off"] - 1
        out, off, perm = self.alloc("sbam", n_in).ptr, self.alloc("sbam_off", n_rec + 1).ptr, self.alloc("bam_perm", n_rec).ptr
        bsw.bam_sort_resident(self.engine, self.buf["bam"].ptr, self.buf["bam_off"].ptr, n_rec, out, n_in, off, perm,
                              bsw.bamsort_opt(n_ref))
        self.n["sbam"], self.n["sbam_off"], self.n["bam_perm"] = n_in, n_rec + 1, n_rec
        return n_in

    def bgzf(self, bopt, cap=None, src="bam"):
        """the BAM blocks (src: "bam" with "bam_off", or the sorted "sbam" with "sbam_off") as BGZF blocks: "bgzf", the
        block starts "bgzf_blk" and the records' virtual offsets "bgzf_voff".  cap=None: room for every block stored.
        Returns (n_blocks, n_bytes)."""
        if src not in ("bam", "sbam"):
            raise ValueError(f"bgzf: src='{src}' is neither 'bam' nor 'sbam'")
        self._have("bgzf", src, src + "_off")
        n_in, n_rec = self.n[src], self.n[src + "_off"] - 1
        nb = bsw.bgzf_blocks(n_in, bopt)
        cap = bsw.bgzf_bound(n_in, bopt) if cap is None else cap
        out, blk, voff = self.alloc("bgzf", cap).ptr, self.alloc("bgzf_blk", nb + 1).ptr, self.alloc("bgzf_voff", n_rec).ptr
        nb, n_bytes = bsw.bgzf_resident(self.engine, self.buf[src].ptr, n_in, self.buf[src + "_off"].ptr, n_rec, out, cap,
                                        blk, nb + 1, voff, bopt)
        self.n["bgzf"], self.n["bgzf_blk"], self.n["bgzf_voff"] = n_bytes, nb + 1, n_rec
        return nb, n_bytes

    def bam_index(self, ref_len, base_coffset=0) -> int:
        """the .bai ("bai") of the sorted blocks behind bgzf(bopt, src="sbam"); base_coffset: that call's.  Reads the
        one entry of "bgzf_blk" that end_voff needs.  Returns the bytes."""
        self._have("bam_index", "sbam", "sbam_off", "bgzf_blk", "bgzf_voff")
        n_rec, nb1 = self.n["sbam_off"] - 1, self.n["bgzf_blk"]
        if self.n["bgzf_voff"] != n_rec:
            raise ValueError("bam_index: the virtual offsets are not those of the sorted blocks: run bgzf(bopt, src='sbam')")
        last = np.zeros(1, np.int64)
        hiprt.check(hiprt.rt().hipMemcpy(ctypes.c_void_p(last.ctypes.data), ctypes.c_void_p(self.buf["bgzf_blk"].ptr + 8 * (nb1 - 1)),
                                         8, hiprt.D2H))
        end_voff = (base_coffset + int(last[0])) << 16
        args = (self.engine, ref_len, self.buf["sbam"].ptr, self.buf["sbam_off"].ptr, n_rec, self.buf["bgzf_voff"].ptr, end_voff)
        try:
            cap = bsw.bam_index_resident(*args, 0, 0)
        except bsw.BswError as e:
            if getattr(e, "needed", -1) <= 0:
                raise
            cap = e.needed
        self.n["bai"] = bsw.bam_index_resident(*args, self.alloc("bai", cap).ptr, cap)
        return self.n["bai"]
