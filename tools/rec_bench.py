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

    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --out profiles/rec/bench.json
    python tools/rec_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --only-out --out profiles/bam/bench.json
"""

import argparse
import ctypes
import json
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-mb", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--only-out", action="store_true")
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
