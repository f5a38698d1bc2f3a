#!/usr/bin/env python3
"""The paired-end stage (include/bsw_pe.h) on paired reads in the style of bench.py::pe_reads:
--pairs fragments (2 x 150 bp, insert 400-600) against a --ref-mb reference, taken through the GPU
front end (bsw_mem_collect_intv_device -> bsw_mem_chain_device -> bsw_chain2aln_resident).  Three
legs, alternating in one process, --reps times each:
  (a) bsw_regs_select_resident   -- the stage before, as the yardstick (it also renews the arrays
                                    (c) updates in place)
  (b) bsw_pe_stat_resident
  (c) bsw_pe_pair_resident under (b)'s pes
Prints one JSON line (and writes it to --out).  --only-new: just (b) and (c) (for a kernel trace).

    python tools/pe_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --out profiles/pe/bench.json
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
sys.path.insert(0, ROOT)
import bsw  # noqa: E402
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    log = lambda m: print(f"[pe_bench] {m}", file=sys.stderr, flush=True)  # noqa: E731
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
    b = ResidentBatch(eng, reads, off, lens)
    ns = len(b.seed_and_chain(fmi)[1])
    b.chain2aln(opt)
    log(f"{n} reads -> {ns} region slots (skipped seeds included)")
    state = {}

    def select():
        state["k"] = b.select(sopt)

    def stat():
        state["pes"] = b.pe_stat(popt)

    def pair():
        b.pe_pair(state["pes"], popt)

    select()                                                 # warm-up: buffers grown, code loaded
    stat()
    pair()
    ta, tb, tc, kb, kc = [], [], [], [], []
    for _ in range(args.reps):
        if args.only_new:
            select()
        else:
            ta.append(timed(select))
        tb.append(timed(stat))
        kb.append(bsw.pe_last_stats(eng).kernel_ms)
        tc.append(timed(pair))
        kc.append(bsw.pe_last_stats(eng).kernel_ms)
    st = bsw.pe_last_stats(eng)
    first, pairs = b.get("sfirst"), b.get("pairs")
    per = np.diff(first)
    pes = state["pes"]
    out = {"tool": "pe_bench", "pairs": n // 2, "reads": n, "read_len": args.read_len, "ref_mb": args.ref_mb,
           "insert": [400, 600], "region_slots": ns, "regions": int(state["k"]),
           "pairs_one_region_per_end_or_fewer": int(((per[0::2] <= 1) & (per[1::2] <= 1)).sum()),
           "longest_list": int(per.max()),
           "pes": [{f: (float(pes[d][f]) if f in ("avg", "std") else int(pes[d][f])) for f in bsw.PESTAT_DTYPE.names}
                   for d in range(4)],
           "pairing_tried": st.n_pairing_tried, "paired": st.n_paired, "multi": st.n_multi,
           "unpaired_preferred": st.n_unpaired_preferred, "proper": st.n_proper,
           "mean_u_n": round(st.n_u / max(st.n_pairing_tried, 1), 4),
           "mapq_mean": round(float(pairs["mapq"].mean()), 3),
           "b_stat_s": spread(tb), "b_stat_kernel_ms": spread(kb), "c_pair_s": spread(tc), "c_pair_kernel_ms": spread(kc)}
    if not args.only_new:
        a = spread(ta)["median"]
        out.update({"a_regs_select_s": spread(ta), "b_over_a_median": round(spread(tb)["median"] / a, 3),
                    "c_over_a_median": round(spread(tc)["median"] / a, 3)})
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
