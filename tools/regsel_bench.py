#!/usr/bin/env python3
"""Region selection (include/bsw_sel.h) on the workload of tools/reg2aln_bench.py: --reads 151 bp
reads taken through the GPU front end (bsw_mem_collect_intv_device -> bsw_mem_chain_device ->
bsw_chain2aln_resident).  Three things, alternating in one process, --reps times each:
  (a) bsw_reg2aln_resident over ALL region slots        -- what a caller could do before
  (b) bsw_regs_select_resident alone
  (c) (b) followed by bsw_reg2aln_resident over its survivors
Prints one JSON line (and writes it to --out).  --only-new: just (b) (for a kernel trace).

    python tools/regsel_bench.py --reads 1000000 --ref-mb 16 --reps 7 --out profiles/regsel/bench.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem2-arm_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bsw  # noqa: E402
from resident import ResidentBatch  # noqa: E402
from reg2aln_bench import make_reads, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=151)
    ap.add_argument("--ref-mb", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--cigar-stride", type=int, default=16)
    ap.add_argument("--md-stride", type=int, default=64)
    ap.add_argument("--p-sub", type=float, default=0.01)
    ap.add_argument("--p-n", type=float, default=0.001)
    ap.add_argument("--indel-frac", type=float, default=0.1)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    log = lambda m: print(f"[regsel_bench] {m}", file=sys.stderr, flush=True)  # noqa: E731
    ref = bsw.synth_reference(args.ref_mb * 1_000_000, seed=7)
    nb = ref > 3
    ref[nb] = np.random.default_rng(1).integers(0, 4, int(nb.sum()), dtype=np.uint8)
    reads, off, lens = make_reads(ref, args.reads, args.read_len, 42, args.p_sub, args.p_n, args.indel_frac)
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
    b = ResidentBatch(eng, reads, off, lens)
    ns = len(b.seed_and_chain(fmi)[1])
    b.chain2aln(opt)
    log(f"{n} reads -> {ns} region slots (skipped seeds included)")
    cs, ms = args.cigar_stride, args.md_stride

    def aln(cur):
        """over the extension's region slots ("c") or the selection's survivors ("s")"""
        b.cur = cur
        b.reg2aln(opt, cs, ms)

    def select():
        return b.select(sopt)

    def both():
        select()
        aln("s")

    k = select()                                             # warm-up: buffers grown, code loaded
    if not args.only_new:
        aln("c")
        aln("s")
    ta, tb, tc, hs, ds = [], [], [], [], []
    for _ in range(args.reps):
        if not args.only_new:
            ta.append(timed(lambda: aln("c")))
        tb.append(timed(select))
        st = bsw.sel_last_stats(eng)
        hs.append(st.helper_ms)
        ds.append(st.dp_ms)
        if not args.only_new:
            tc.append(timed(both))
    st = bsw.sel_last_stats(eng)
    info = b.get("sinfo")
    out = {"tool": "regsel_bench", "reads": n, "read_len": args.read_len, "ref_mb": args.ref_mb, "w": args.w,
           "p_sub": args.p_sub, "p_n": args.p_n, "indel_frac": args.indel_frac, "cigar_stride": cs, "md_stride": ms,
           "region_slots": ns, "regions_in": st.n_regs_in, "survivors": k, "redundant": st.n_redundant,
           "identical": st.n_identical, "patch_tried": st.n_patch_tried, "patch_ok": st.n_patch_ok,
           "patch_ratio": st.n_patch_ratio, "dp_jobs": st.n_dp, "rounds": st.rounds,
           "secondary": int((info["secondary"] >= 0).sum()), "mapq_mean": round(float(info["mapq"].mean()), 3) if k else 0,
           "b_select_s": spread(tb), "select_helper_kernel_ms": spread(hs), "select_dp_kernel_ms": spread(ds),
           "select_reads_per_s": round(n / spread(tb)["median"])}
    if not args.only_new:
        a, c = spread(ta)["median"], spread(tc)["median"]
        out.update({"a_reg2aln_all_slots_s": spread(ta), "c_select_then_reg2aln_survivors_s": spread(tc),
                    "c_over_a_median": round(c / a, 3)})
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
