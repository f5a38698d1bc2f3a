#!/usr/bin/env python3
"""The record stage (include/bsw_rec.h) on paired reads in the style of bench.py::pe_reads: --pairs
fragments (2 x 150 bp, insert 400-600) against a --ref-mb reference, taken through the resident front
end (bsw_mem_collect_intv_device -> bsw_mem_chain_device -> bsw_chain2aln_resident).  Legs alternating
in one process, --reps times each:
  (a) bsw_regs_select_resident   -- the yardstick of the helper kernels (it also renews the arrays the
                                    pair call updates in place); then stat and pair, untimed
  (b) bsw_reg2aln_resident over ALL of the reads' regions -- the only route to the records' CIGARs
                                    without this stage
  (c) bsw_records_resident       -- aln_ms beside (b), helper_ms beside (a)
  (d) bsw_sam_text_resident      -- its kernels' bytes/s
  (e) a device-to-device hipMemcpy of the same byte count
  (f) bsw_bam_records_resident   -- the same records as BAM alignment blocks (include/bsw_bam.h): len_ms, write_ms
  (g) a device-to-device hipMemcpy of the BAM byte count
Prints one JSON line (and writes it to --out).  --only-new: just (c) and (d) (for a kernel trace); --only-out: just
(d) and (f) with their copies (the lanes-per-record sweeps, BSW_HIP_LIB names the library under test; a kernel trace).
--bgzf: the BGZF legs (include/bsw_bgzf.h) over the BAM bytes of (f), alternating:
  (f) (g) as above, the yardsticks of the same process
  (h) bsw_bgzf_resident at block_bytes 0xff00 and (i) at 32,640: deflate_ms, pack_ms, bytes out, blocks per form
  (j) hipMemcpy device -> pinned host of the BAM bytes; (k) of (h)'s compressed bytes
and, on the host, Python's zlib at levels 1 and 6 over --zlib-chunks chunks of 0xff00 bytes spread over the BAM bytes,
beside this encoder's blocks of the same chunks.

--sort: the coordinate sort and the index (include/bsw_bamsort.h) over the same BAM bytes, alternating:
  (f) (g) as above: the write kernel that builds these bytes from scratch, and the device copy that is the floor
  (s) bsw_bam_sort_resident: key_ms, sort_ms, copy_ms (lengths, scan, the permute kernel)
  (t) bsw_bgzf_resident on the sorted blocks and (u) on the unsorted ones: time and bytes
  (x) bsw_bam_index_resident: index_ms, the index's size
and, as context on the host, numpy's stable argsort over the same keys (its order has to be the device's).

--markdup: duplicate marking (include/bsw_markdup.h) on the same fragments with a share d of them emitted a second time
under fresh quals, for d = 0 and d = 0.1, each through the front end and bsw_records_resident; alternating:
  (m) bsw_mark_duplicates_resident: wall time, score_ms, key_ms, sort_ms, mark_ms
  (s) bsw_bam_sort_resident over the batch's BAM blocks: as many 64-bit keys, twice the bytes moved
  (q) a device-to-device hipMemcpy of the quals bytes, beside score_ms
and, for d = 0.1, d_dup against tests/markdup_py.py on a sample of 20,000 pairs taken with their whole sets.

    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --out profiles/rec/bench.json
    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --only-out --out profiles/bam/bench.json
    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 5 --bgzf --out profiles/bgzf/bench.json
    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 5 --sort --out profiles/bamsort/bench.json
    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 5 --markdup --out profiles/markdup/bench.json
"""

import argparse
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem2-arm_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import bsw  # noqa: E402
import hiprt  # noqa: E402
from resident import ResidentBatch  # noqa: E402
from bench import pe_reads  # noqa: E402
from reg2aln_bench import spread, timed  # noqa: E402


def bgzf_legs(args, eng, b, bam_bytes, bam, copy_bam, log):
    """the --bgzf legs over b's BAM bytes; returns the JSON fields"""
    rt = hiprt.rt()
    big, half = bsw.bgzf_opt(), bsw.bgzf_opt(block_bytes=32640)
    cap = bsw.bgzf_bound(bam_bytes, half)
    nb_big, z_big = b.bgzf(big, cap=cap)                         # warm-up; the sizes
    st_big = bsw.bgzf_last_stats(eng)
    blk_big = b.get("bgzf_blk")
    nb_half, z_half = b.bgzf(half, cap=cap)
    st_half = bsw.bgzf_last_stats(eng)
    pinned = ctypes.c_void_p()
    hiprt.check(rt.hipHostMalloc(ctypes.byref(pinned), ctypes.c_size_t(bam_bytes), ctypes.c_uint(0)))

    def d2h(name, nbytes):
        def run():
            hiprt.check(rt.hipMemcpy(pinned, ctypes.c_void_p(b.buf[name].ptr), nbytes, hiprt.D2H))
        return run

    d2h("bam", bam_bytes)()
    tf, f_write, tg, th, ti, tj, tk = [], [], [], [], [], [], []
    h_def, h_pack, i_def, i_pack = [], [], [], []
    for _ in range(args.reps):
        tf.append(timed(bam))
        f_write.append(bsw.bam_last_stats(eng).write_ms)
        tg.append(timed(copy_bam))
        ti.append(timed(lambda: b.bgzf(half, cap=cap)))
        st = bsw.bgzf_last_stats(eng)
        i_def.append(st.deflate_ms)
        i_pack.append(st.pack_ms)
        th.append(timed(lambda: b.bgzf(big, cap=cap)))           # (last: (k) copies its bytes)
        st = bsw.bgzf_last_stats(eng)
        h_def.append(st.deflate_ms)
        h_pack.append(st.pack_ms)
        tj.append(timed(d2h("bam", bam_bytes)))
        tk.append(timed(d2h("bgzf", z_big)))
    hiprt.check(rt.hipHostFree(pinned))
    # the yardstick: zlib per chunk on the host, and this encoder's blocks of the same chunks
    data = b.get("bam")
    pick = np.unique(np.linspace(0, nb_big - 1, min(args.zlib_chunks, nb_big)).astype(np.int64))
    raw = z1 = z6 = ours = 0
    for k in pick:
        chunk = data[k * 0xff00:(k + 1) * 0xff00].tobytes()
        raw += len(chunk)
        z1 += len(zlib.compress(chunk, 1)) - 6 + 26              # (the zlib wrapper's 6 bytes for a block's 26)
        z6 += len(zlib.compress(chunk, 6)) - 6 + 26
        ours += int(blk_big[k + 1] - blk_big[k])
    log(f"bgzf: {bam_bytes} -> {z_big} bytes at 0xff00, {z_half} at 32640; sample of {len(pick)} chunks: zlib-1 {z1}, zlib-6 {z6}, ours {ours}")

    def forms(st):
        return {"blocks": st.n_blocks, "stored": st.n_stored, "fixed": st.n_fixed, "dynamic": st.n_dynamic}

    med = lambda v: spread(v)["median"]  # noqa: E731
    return {"bam_bytes": int(bam_bytes),
            "f_bam_s": spread(tf), "f_bam_write_ms": spread(f_write), "g_memcpy_d2d_bam_s": spread(tg),
            "h_bgzf_ff00_bytes": int(z_big), "h_bgzf_ff00_ratio": round(z_big / bam_bytes, 4), "h_bgzf_ff00_forms": forms(st_big),
            "h_bgzf_ff00_s": spread(th), "h_bgzf_ff00_deflate_ms": spread(h_def), "h_bgzf_ff00_pack_ms": spread(h_pack),
            "h_bgzf_ff00_deflate_gb_per_s": round(bam_bytes / (med(h_def) * 1e-3) / 1e9, 1),
            "i_bgzf_32640_bytes": int(z_half), "i_bgzf_32640_ratio": round(z_half / bam_bytes, 4),
            "i_bgzf_32640_forms": forms(st_half), "i_bgzf_32640_s": spread(ti), "i_bgzf_32640_deflate_ms": spread(i_def),
            "i_bgzf_32640_pack_ms": spread(i_pack),
            "j_d2h_pinned_bam_s": spread(tj), "j_d2h_pinned_bam_gb_per_s": round(bam_bytes / med(tj) / 1e9, 1),
            "k_d2h_pinned_bgzf_s": spread(tk),
            "compress_plus_copy_s": round(med(th) + med(tk), 6), "copy_uncompressed_s": round(med(tj), 6),
            "zlib_sample": {"chunks": int(len(pick)), "raw_bytes": int(raw), "zlib1_bytes": int(z1), "zlib6_bytes": int(z6),
                            "bgzf_bytes": int(ours), "zlib1_ratio": round(z1 / raw, 4), "zlib6_ratio": round(z6 / raw, 4),
                            "bgzf_ratio": round(ours / raw, 4), "bgzf_over_zlib1": round(ours / z1, 3)}}


def sort_legs(args, eng, b, bam_bytes, bam, copy_bam, l_pac, log):
    """the --sort legs over b's BAM bytes (one reference of l_pac bases); returns the JSON fields"""
    big = bsw.bgzf_opt(flags=bsw.BGZF_EOF)
    cap = bsw.bgzf_bound(bam_bytes, big)
    ref_len = [l_pac]
    b.bam_sort(1)                                                # warm-up; the sizes
    n_rec = b.n["bam_perm"]
    nb, z_sorted = b.bgzf(big, cap=cap, src="sbam")
    bai_bytes = b.bam_index(ref_len)
    st_x = bsw.bamsort_last_stats(eng)
    end_voff = int(b.get("bgzf_blk")[nb]) << 16
    _, z_unsorted = b.bgzf(big, cap=cap, src="bam")

    def index():
        # (the virtual offsets are those of the last bgzf call: the sorted blocks')
        bsw.bam_index_resident(eng, ref_len, b.buf["sbam"].ptr, b.buf["sbam_off"].ptr, n_rec, b.buf["bgzf_voff"].ptr, end_voff,
                               b.buf["bai"].ptr, bai_bytes)

    tf, f_write, tg, ts, tt, tu, tx = [], [], [], [], [], [], []
    key_ms, sort_ms, copy_ms, index_ms, t_def, u_def = [], [], [], [], [], []
    for _ in range(args.reps):
        tf.append(timed(bam))
        f_write.append(bsw.bam_last_stats(eng).write_ms)
        tg.append(timed(copy_bam))
        ts.append(timed(lambda: b.bam_sort(1)))
        st = bsw.bamsort_last_stats(eng)
        key_ms.append(st.key_ms)
        sort_ms.append(st.sort_ms)
        copy_ms.append(st.copy_ms)
        tu.append(timed(lambda: b.bgzf(big, cap=cap, src="bam")))
        u_def.append(bsw.bgzf_last_stats(eng).deflate_ms)
        tt.append(timed(lambda: b.bgzf(big, cap=cap, src="sbam")))
        t_def.append(bsw.bgzf_last_stats(eng).deflate_ms)
        tx.append(timed(index))
        index_ms.append(bsw.bamsort_last_stats(eng).index_ms)
    # the host's context: numpy's stable argsort over the same keys; its order is the device's
    data, boff = b.get("bam"), b.get("bam_off")
    at = boff[:-1, None] + np.arange(4)[None, :]
    rid = data[at + 4].copy().view("<i4")[:, 0].astype(np.int64)
    pos = data[at + 8].copy().view("<i4")[:, 0].astype(np.int64)
    rev = (data[boff[:-1] + 18] >> 4 & 1).astype(np.int64)
    key = np.where(rid < 0, 1, rid) << 33 | (pos + 1) << 1 | rev
    t0 = time.perf_counter()
    order = np.argsort(key, kind="stable")
    t_np = time.perf_counter() - t0
    if not np.array_equal(order.astype(np.int32), b.get("bam_perm")):
        raise SystemExit("the device's permutation is not numpy's stable argsort over the same keys")
    log(f"sort: {n_rec} records, {bam_bytes} bytes; bgzf {z_unsorted} unsorted, {z_sorted} sorted; .bai {bai_bytes} bytes")
    med = lambda v: spread(v)["median"]  # noqa: E731
    return {"bam_bytes": int(bam_bytes), "records": int(n_rec), "key_bits": int(st_x.key_bits),
            "f_bam_s": spread(tf), "f_bam_write_ms": spread(f_write),
            "g_memcpy_d2d_bam_s": spread(tg), "g_memcpy_d2d_bam_ms_median": round(med(tg) * 1e3, 3),
            "s_bam_sort_s": spread(ts), "s_key_ms": spread(key_ms), "s_sort_ms": spread(sort_ms), "s_copy_ms": spread(copy_ms),
            "s_copy_gb_per_s": round(bam_bytes / (med(copy_ms) * 1e-3) / 1e9, 1),
            "s_copy_over_f_write_median": round(med(copy_ms) / med(f_write), 3),
            "s_copy_over_g_memcpy_median": round(med(copy_ms) * 1e-3 / med(tg), 3),
            "t_bgzf_sorted_s": spread(tt), "t_bgzf_sorted_deflate_ms": spread(t_def), "t_bgzf_sorted_bytes": int(z_sorted),
            "u_bgzf_unsorted_s": spread(tu), "u_bgzf_unsorted_deflate_ms": spread(u_def), "u_bgzf_unsorted_bytes": int(z_unsorted),
            "x_bam_index_s": spread(tx), "x_index_ms": spread(index_ms), "x_bai_bytes": int(bai_bytes),
            "x_bins": int(st_x.n_bins), "x_chunks": int(st_x.n_chunks), "x_intv": int(st_x.n_intv),
            "host_numpy_stable_argsort_s": round(t_np, 4)}


def end_words(recs, rec_first, aln, cigar):
    """per read (rid 0, u, s) as one integer, -1 for a read that is no candidate: numpy over the downloaded arrays, used
    only to close the checked sample over its sets (the verdict on the sample is tests/markdup_py.py's)"""
    first = recs[rec_first[:-1].clip(max=len(recs) - 1)]
    cand = (rec_first[1:] > rec_first[:-1]) & (first["flag"] & 4 == 0)
    a = first["aln"].clip(min=0)
    cg, nc = cigar[a], aln["n_cigar"][a]
    op, ln = (cg & 15).astype(np.int64), (cg >> 4).astype(np.int64)
    live = np.arange(cg.shape[1])[None, :] < nc[:, None]
    rlen = (ln * (live & ((op == 0) | (op == 2)))).sum(axis=1)
    lead = np.where((op[:, 0] == 3) | (op[:, 0] == 4), ln[:, 0], 0)
    last = np.take_along_axis(cg, (nc.clip(min=1) - 1)[:, None].astype(np.int64), axis=1)[:, 0].astype(np.int64)
    trail = np.where((last & 15 == 3) | (last & 15 == 4), last >> 4, 0)
    rev = first["is_rev"] != 0
    u = np.where(rev, first["pos"] + rlen - 1 + trail, first["pos"] - lead)
    return np.where(cand, (u + (1 << 31)) << 1 | rev, -1)


def check_sample(b, l_pac, quals, off, lens, dup, n_sample, log):
    """d_dup against tests/markdup_py.py on the first n_sample pairs, taken with every pair that shares an end with them"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import markdup_py as md
    recs, rec_first, aln, cigar = b.get("recs"), b.get("rec_first"), b.get("aln"), b.get("cigar")
    recs = recs.copy()
    recs["flag"] &= ~0x400                                        # (the stage has run: its input is the records without the mark)
    recs["sam_flag"] &= ~0x400
    w = end_words(recs, rec_first, aln, cigar)
    n_pairs = len(w) // 2
    mine = w[:2 * n_sample]
    hit = np.isin(w, mine[mine >= 0])
    pairs = np.flatnonzero(hit[0::2] | hit[1::2] | (np.arange(n_pairs) < n_sample))
    reads = np.stack([2 * pairs, 2 * pairs + 1], axis=1).ravel()
    counts = (rec_first[1:] - rec_first[:-1])[reads]
    sub_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = np.concatenate([np.arange(rec_first[r], rec_first[r + 1]) for r in reads])
    sub = recs[idx]
    sub["read"] = np.repeat(np.arange(len(reads)), counts)
    c = md.make_case([], True, l_pac=l_pac, stride=cigar.shape[1])
    c.recs, c.rec_first, c.aln, c.cigar, c.read_off, c.read_len, c.quals, c.n_reads = (sub, sub_first, aln, cigar, off[reads], lens[reads],
                                                                                     quals, len(reads))
    assert md.check(c) == 0
    want = md.mark(c)[1]
    keep = np.flatnonzero(pairs < n_sample)
    keep = np.stack([2 * keep, 2 * keep + 1], axis=1).ravel()
    got = dup[reads][keep]
    if not np.array_equal(got, want[keep]):
        raise SystemExit(f"d_dup differs from tests/markdup_py.py at {int((got != want[keep]).sum())} reads of the sample")
    log(f"sample: {n_sample} pairs within {len(pairs)} (their sets), {int((got != 0).sum())} duplicate reads, == tests/markdup_py.py")
    return {"sample_pairs": int(n_sample), "sample_pairs_with_sets": int(len(pairs)), "sample_dup_reads": int((got != 0).sum())}


def markdup_legs(args, eng, fmi, ref, reads, off, lens, l_pac, share, log):
    """the --markdup legs with a share of the fragments emitted a second time under fresh quals; returns the JSON fields"""
    n_pairs = len(lens) // 2
    extra = np.arange(0, n_pairs, int(round(1 / share)))[:int(share * n_pairs)] if share > 0 else np.zeros(0, np.int64)
    ends = np.stack([2 * extra, 2 * extra + 1], axis=1).ravel()
    if len(ends):
        more = np.concatenate([reads[off[e]:off[e] + lens[e]] for e in ends])
        off = np.concatenate([off, len(reads) + np.concatenate([[0], np.cumsum(lens[ends])[:-1]])]).astype(np.int64)
        lens = np.concatenate([lens, lens[ends]]).astype(np.int32)
        reads = np.concatenate([reads, more])
    quals = (33 + (np.arange(len(reads)) * 7) % 41).astype(np.uint8)
    if len(ends):                                                 # fresh quals for the second copies
        quals[off[2 * n_pairs]:] = np.random.default_rng(3).integers(35, 74, len(reads) - int(off[2 * n_pairs]))
    n = len(lens)
    opt, sopt, popt = bsw.ext_opt(w=args.w, l_pac=l_pac), bsw.sel_opt(w=args.w, l_pac=l_pac), bsw.pe_opt(l_pac=l_pac)
    ropt, dopt = bsw.rec_opt(w=args.w, l_pac=l_pac, rname="chrS"), bsw.markdup_opt(l_pac)
    b = ResidentBatch(eng, reads, off, lens, quals=quals)
    b.seed_and_chain(fmi)
    b.chain2aln(opt)
    b.select(sopt)
    b.pe_pair(b.pe_stat(popt), popt)
    b.records(ropt)
    b.bam_records(ropt, [b"frag%08d" % i for i in range(n // 2)], True)
    d_copy = hiprt.DeviceBuffer(len(reads))

    def copy_quals():
        hiprt.check(hiprt.rt().hipMemcpy(ctypes.c_void_p(d_copy.ptr), ctypes.c_void_p(b.buf["quals"].ptr), len(reads), hiprt.D2D))
        hiprt.synchronize()

    mark = lambda: b.mark_duplicates(dopt)  # noqa: E731
    sort = lambda: b.bam_sort(1)  # noqa: E731
    mark(), sort(), copy_quals()                                  # warm-up
    tm, ts, tq, groups = [], [], [], {k: [] for k in ("score_ms", "key_ms", "sort_ms", "mark_ms")}
    for _ in range(args.reps):
        tm.append(timed(mark))
        st = bsw.markdup_last_stats(eng)
        for k in groups:
            groups[k].append(getattr(st, k))
        ts.append(timed(sort))
        tq.append(timed(copy_quals))
    dup = b.get("dup")
    out = {"share": share, "pairs": n // 2, "reads": n, "records": int(b.n["recs"]), "quals_bytes": int(len(reads)),
           "stats": {k: int(getattr(st, k)) for k in ("n_cand", "n_pair_cand", "n_dup_pairs", "n_dup_frag", "n_dup_frag_by_pair",
                                                      "n_pair_sets", "n_end_sets", "n_flagged", "pair_key_bits", "end_key_bits",
                                                      "pair_route", "end_route")},
           "m_mark_duplicates_s": spread(tm), **{"m_" + k: spread(v) for k, v in groups.items()},
           "s_bam_sort_s": spread(ts), "s_bam_bytes": int(b.n["bam"]), "q_memcpy_d2d_quals_s": spread(tq),
           "m_over_s_median": round(spread(tm)["median"] / spread(ts)["median"], 3),
           "score_ms_over_q_median": round(spread(groups["score_ms"])["median"] * 1e-3 / spread(tq)["median"], 3)}
    log(f"markdup d={share}: {out['stats']}")
    if share > 0:
        out.update(check_sample(b, l_pac, quals, off, lens, dup, min(20000, n_pairs), log))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-mb", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--only-out", action="store_true")
    ap.add_argument("--bgzf", action="store_true")
    ap.add_argument("--sort", action="store_true")
    ap.add_argument("--markdup", action="store_true")
    ap.add_argument("--shares", default="0,0.1", help="--markdup: the shares of fragments emitted twice")
    ap.add_argument("--zlib-chunks", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    log = lambda m: print(f"[rec_bench] {m}", file=sys.stderr, flush=True)  # noqa: E731
    ref = bsw.synth_reference(args.ref_mb * 1_000_000, seed=7)
    nb = ref > 3
    ref[nb] = np.random.default_rng(1).integers(0, 4, int(nb.sum()), dtype=np.uint8)
    reads, off, lens = pe_reads(ref, args.pairs, args.read_len, seed=42)
    n = len(lens)
    T = np.concatenate([ref, (3 - ref[::-1])]).astype(np.uint8)
    l_pac = len(ref)
    t0 = time.perf_counter()
    fmi = bsw.Fmi(ref)
    log(f"index of {len(ref)} bases built in {time.perf_counter() - t0:.1f} s")
    eng = bsw.Engine()
    bsw.set_reference(eng, T)
    if args.markdup:
        out = {"tool": "rec_bench", "legs": "markdup", "lib": os.path.basename(bsw.HIP_LIB), "read_len": args.read_len,
               "ref_mb": args.ref_mb, "reps": args.reps,
               "runs": [markdup_legs(args, eng, fmi, ref, reads, off, lens, l_pac, d, log) for d in map(float, args.shares.split(","))]}
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        eng.close()
        fmi.close()
        return
    opt = bsw.ext_opt(w=args.w, l_pac=l_pac)
    sopt = bsw.sel_opt(w=args.w, l_pac=l_pac)
    popt = bsw.pe_opt(l_pac=l_pac)
    ropt = bsw.rec_opt(w=args.w, l_pac=l_pac, rname="chrS")
    b = ResidentBatch(eng, reads, off, lens, quals=(33 + (np.arange(len(reads)) * 7) % 41).astype(np.uint8))
    names = [b"frag%08d" % i for i in range(n // 2)]
    ns = len(b.seed_and_chain(fmi)[1])
    b.chain2aln(opt)
    log(f"{n} reads -> {ns} region slots (skipped seeds included)")

    def select():
        b.select(sopt)

    def stat_pair():
        b.pe_pair(b.pe_stat(popt), popt)

    select()
    stat_pair()
    k = b.n["sreg"]

    def all_regions():
        # writes arrays of its own: the records' alignments stay what (c) left for (d)
        b.reg2aln(opt, into="all.aln")

    def records():
        b.records(ropt)

    records()                                                # warm-up, and the size of the text
    n_bytes = b.sam_text(ropt, names, True)                  # (the sizing call, then one with exactly that room)
    d_copy = hiprt.DeviceBuffer(n_bytes)

    def text():
        return b.sam_text(ropt, None, True, cap=n_bytes)

    def copy():
        hiprt.check(hiprt.rt().hipMemcpy(ctypes.c_void_p(d_copy.ptr), ctypes.c_void_p(b.buf["text"].ptr), n_bytes, hiprt.D2D))
        hiprt.synchronize()

    # (--only-new stays (c) and (d): its kernel trace holds no BAM kernel)
    bam_bytes = 0 if args.only_new else b.bam_records(ropt, None, True)     # (the names of the text call)
    d_copy_bam = None if args.only_new else hiprt.DeviceBuffer(bam_bytes)

    def bam():
        return b.bam_records(ropt, None, True, cap=bam_bytes)

    def copy_bam():
        hiprt.check(hiprt.rt().hipMemcpy(ctypes.c_void_p(d_copy_bam.ptr), ctypes.c_void_p(b.buf["bam"].ptr), bam_bytes,
                                         hiprt.D2D))
        hiprt.synchronize()

    all_regions()
    text()
    copy()
    if not args.only_new:
        bam()
        copy_bam()
    ta, tb, tc, td, te, b_ms, c_aln, c_help, d_ms = [], [], [], [], [], [], [], [], []
    tf, tg, f_len, f_write = [], [], [], []

    def out_legs():
        td.append(timed(text))
        d_ms.append(bsw.rec_last_stats(eng).text_ms)
        te.append(timed(copy))
        tf.append(timed(bam))
        bs = bsw.bam_last_stats(eng)
        f_len.append(bs.len_ms)
        f_write.append(bs.write_ms)
        tg.append(timed(copy_bam))

    def out_json():
        n_rec = bsw.bam_last_stats(eng).n_rec
        f_ms = [x + y for x, y in zip(f_len, f_write)]
        return {"records": n_rec, "text_bytes": int(n_bytes), "text_bytes_per_record": round(n_bytes / max(n_rec, 1), 1),
                "bam_bytes": int(bam_bytes), "bam_bytes_per_record": round(bam_bytes / max(n_rec, 1), 1),
                "d_text_s": spread(td), "d_text_kernel_ms": spread(d_ms),
                "d_text_kernels_gb_per_s": round(n_bytes / (spread(d_ms)["median"] * 1e-3) / 1e9, 1),
                "e_memcpy_d2d_s": spread(te), "e_memcpy_d2d_gb_per_s": round(n_bytes / spread(te)["median"] / 1e9, 1),
                "f_bam_s": spread(tf), "f_bam_len_ms": spread(f_len), "f_bam_write_ms": spread(f_write),
                "f_bam_kernel_ms": spread(f_ms),
                "f_bam_kernels_gb_per_s": round(bam_bytes / (spread(f_ms)["median"] * 1e-3) / 1e9, 1),
                "f_bam_over_d_text_median": round(spread(f_ms)["median"] / spread(d_ms)["median"], 3),
                "g_memcpy_d2d_bam_s": spread(tg), "g_memcpy_d2d_bam_gb_per_s": round(bam_bytes / spread(tg)["median"] / 1e9, 1)}

    if args.bgzf or args.sort:
        out = {"tool": "rec_bench", "legs": "bgzf" if args.bgzf else "sort", "lib": os.path.basename(bsw.HIP_LIB), "pairs": n // 2,
               "reads": n, "read_len": args.read_len, "ref_mb": args.ref_mb}
        out.update(bgzf_legs(args, eng, b, bam_bytes, bam, copy_bam, log) if args.bgzf else
                   sort_legs(args, eng, b, bam_bytes, bam, copy_bam, l_pac, log))
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        eng.close()
        fmi.close()
        return
    if args.only_out:
        for _ in range(args.reps):
            out_legs()
        out = {"tool": "rec_bench", "legs": "out", "lib": os.path.basename(bsw.HIP_LIB), "pairs": n // 2, "reads": n,
               "read_len": args.read_len, "ref_mb": args.ref_mb}
        out.update(out_json())
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        eng.close()
        fmi.close()
        return
    for _ in range(args.reps):
        if args.only_new:
            select()
        else:
            ta.append(timed(select))
        stat_pair()
        if not args.only_new:
            tb.append(timed(all_regions))
            a = bsw.aln_last_stats(eng)
            b_ms.append(a.dp_ms + a.helper_ms)
        tc.append(timed(records))
        st = bsw.rec_last_stats(eng)
        c_aln.append(st.aln_ms)
        c_help.append(st.helper_ms)
        if args.only_new:
            td.append(timed(text))
            d_ms.append(bsw.rec_last_stats(eng).text_ms)
        else:
            out_legs()
    st = bsw.rec_last_stats(eng)
    out = {"tool": "rec_bench", "pairs": n // 2, "reads": n, "read_len": args.read_len, "ref_mb": args.ref_mb,
           "regions": int(k), "records": st.n_rec, "unmapped": st.n_unmapped, "supplementary": st.n_supp, "xa_members": st.n_xa,
           "regions_aligned": st.n_aln, "text_bytes": int(n_bytes), "bytes_per_record": round(n_bytes / max(st.n_rec, 1), 1),
           "c_records_s": spread(tc), "c_records_aln_ms": spread(c_aln), "c_records_helper_ms": spread(c_help),
           "d_text_s": spread(td), "d_text_kernel_ms": spread(d_ms),
           "d_text_kernels_gb_per_s": round(n_bytes / (spread(d_ms)["median"] * 1e-3) / 1e9, 1)}
    if not args.only_new:
        out.update(out_json())
        out.update({"a_regs_select_s": spread(ta), "b_reg2aln_all_regions_s": spread(tb),
                    "b_reg2aln_all_regions_kernel_ms": spread(b_ms),
                    "c_helper_over_a_median": round(spread(c_help)["median"] * 1e-3 / spread(ta)["median"], 3),
                    "c_aln_over_b_median": round(spread(c_aln)["median"] / spread(b_ms)["median"], 3)})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    fmi.close()


if __name__ == "__main__":
    main()
