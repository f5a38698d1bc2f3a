#!/usr/bin/env python3
"""The mate-rescue stage (include/bsw_matesw.h) on paired reads in the style of bench.py::pe_reads:
--pairs fragments (2 x 150 bp, insert 400-600) against a --ref-mb reference, a fraction --f of the
mates made unseedable (a substitution every 13 to 16 bases: no exact 19-mer), taken through the GPU
front end (bsw_mem_collect_intv_device -> bsw_mem_chain_device -> bsw_chain2aln_resident ->
bsw_regs_select_resident -> bsw_pe_stat_resident).  Legs, alternating in one process, --reps times:
  (m) bsw_matesw_resident
  (a) bsw_pe_pair_resident over the same reads (on a copy of the selected arrays)
  (b) bsw_ksw_align2_device over the stage's own jobs, rebuilt on the host as ONE batch: the floor of
      the Smith-Waterman part (sw_ms / (b) is what the rounds cost)
Prints one JSON line per --f (and writes them to --out).  --only-new: just (m) (for a kernel trace).

    python tools/matesw_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --f 0,0.02,0.2 --out profiles/matesw/bench.json
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
import hiprt  # noqa: E402
from resident import ResidentBatch  # noqa: E402
from bench import pe_reads  # noqa: E402
from reg2aln_bench import spread, timed  # noqa: E402


def unseedable(reads, n_pairs, L, f, seed=21):
    """a substitution every 13 to 16 bases in one mate of a fraction f of the pairs"""
    rng = np.random.default_rng(seed)
    R = reads.reshape(-1, L)
    hit = np.flatnonzero(rng.random(n_pairs) < f)
    rows = 2 * hit + rng.integers(0, 2, len(hit))
    for r in rows:
        pos = np.cumsum(rng.integers(13, 17, L // 13 + 1)) - int(rng.integers(1, 13))
        pos = pos[(pos >= 0) & (pos < L)]
        R[r, pos] = (R[r, pos] + rng.integers(1, 4, len(pos))) % 4
    return len(rows)


def host_jobs(T, l_pac, reads, off, lens, regs, first, pes, mo, a):
    """the first round's jobs of every pair, as the specification builds them (the later rounds' jobs
    depend on results; round 1 holds nearly all of them on this data) -> (pairs, ref, qer)"""
    pr, rbuf, qbuf = [], [], []
    ro = qo = 0
    RB = regs["rb"].tolist()
    failed, lows, highs = ([int(pes[d][f]) for d in range(4)] for f in ("failed", "low", "high"))
    first = first.tolist()
    for p in range(len(lens) // 2):
        for e in (0, 1):
            fb, fe = first[2 * p + e], first[2 * p + e + 1]
            if fb == fe:
                continue
            ms = 2 * p + 1 - e
            mb, me = first[ms], first[ms + 1]
            arb = RB[fb]
            skip = list(failed)
            for k in range(mb, me):
                b2 = RB[k]
                r1, r2 = arb >= l_pac, b2 >= l_pac
                p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
                d = (0 if r1 == r2 else 1) ^ (0 if p2 > arb else 3)
                if lows[d] <= abs(p2 - arb) <= highs[d]:
                    skip[d] = 1
            l_ms = int(lens[ms])
            q = reads[off[ms]:off[ms] + l_ms]
            for r in range(4):
                if skip[r]:
                    continue
                is_rev, larger = (r >> 1) != (r & 1), not r >> 1
                lo, hi = lows[r], highs[r]
                if not is_rev:
                    rb, re = (arb + lo if larger else arb - hi), (arb + hi if larger else arb - lo) + l_ms
                else:
                    rb, re = (arb + lo if larger else arb - hi) - l_ms, (arb + hi if larger else arb - lo)
                rb, re = max(rb, 0), min(re, 2 * l_pac)
                if rb < re:
                    if (rb + re) >> 1 < l_pac:
                        re = min(re, l_pac)
                    else:
                        rb = max(rb, l_pac)
                if rb >= re or re - rb < mo.min_seed_len:
                    continue
                xtra = 0x40000 | 0x80000 | (0x10000 if l_ms * a < 250 else 0) | mo.min_seed_len * a
                pr.append((ro, qo, len(pr), re - rb, l_ms, xtra))
                rbuf.append(T[rb:re])
                qbuf.append(np.where(q < 4, 3 - q, 4)[::-1] if is_rev else q)
                ro += re - rb
                qo += l_ms
            break                                            # (the first end that has a list: round 1)
    pairs = np.zeros(len(pr), dtype=bsw.SEQPAIR_DTYPE)
    for i, (idr, idq, id_, l1, l2, h0) in enumerate(pr):
        pairs[i]["idr"], pairs[i]["idq"], pairs[i]["id"], pairs[i]["len1"], pairs[i]["len2"], pairs[i]["h0"] = idr, idq, id_, l1, l2, h0
    cat = lambda v: np.concatenate(v).astype(np.uint8) if v else np.zeros(1, np.uint8)  # noqa: E731
    return pairs, cat(rbuf), cat(qbuf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-mb", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--f", default="0,0.02,0.2")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    log = lambda m: print(f"[matesw_bench] {m}", file=sys.stderr, flush=True)  # noqa: E731
    ref = bsw.synth_reference(args.ref_mb * 1_000_000, seed=7)
    nb = ref > 3
    ref[nb] = np.random.default_rng(1).integers(0, 4, int(nb.sum()), dtype=np.uint8)
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
    mo = bsw.matesw_opt(l_pac=l_pac)
    lines = []
    for f in [float(x) for x in args.f.split(",")]:
        reads, off, lens = pe_reads(ref, args.pairs, args.read_len, seed=42)
        n_mut = unseedable(reads, args.pairs, args.read_len, f)
        n = len(lens)
        b = ResidentBatch(eng, reads, off, lens)
        b.seed_and_chain(fmi)
        b.chain2aln(opt)
        k = b.select(sopt)
        pes = b.pe_stat(popt)
        log(f"f = {f}: {n} reads ({n_mut} mates unseedable) -> {k} regions; FR [{pes[1]['low']}, {pes[1]['high']}]")
        cap = k + 8 * n_mut + 1024
        h_sreg, first = b.get("sreg"), b.get("sfirst")
        pb = ResidentBatch(eng, reads, off, lens)            # the pairing updates in place: it gets lists of its own
        pb.put(sreg=h_sreg, sinfo=b.get("sinfo"), sfirst=first)
        state = {}

        def rescue():
            state["m"] = b.matesw(pes, mo, cap=cap)

        def pair():
            pb.pe_pair(pes, popt)

        rescue()
        st = bsw.matesw_last_stats(eng)
        out = {"tool": "matesw_bench", "f": f, "pairs": n // 2, "read_len": args.read_len, "ref_mb": args.ref_mb,
               "mates_unseedable": n_mut, "regions_in": int(k), "regions_out": int(state["m"]),
               **{x: getattr(st, x) for x in ("n_calls", "n_calls_all_skipped", "n_jobs", "n_jobs_u8", "n_short_window",
                                              "n_pushed", "n_redundant", "n_identical", "n_lists_changed", "rounds")}}
        jobs = None
        if not args.only_new:
            pair()
            if st.n_jobs:
                jp, jr, jq = host_jobs(T, l_pac, reads, off, lens, h_sreg, first, pes, mo, 1)
                jobs = (hiprt.DeviceBuffer.from_array(jp), hiprt.DeviceBuffer.from_array(jr),
                        hiprt.DeviceBuffer.from_array(jq), hiprt.DeviceBuffer(max(len(jp), 1) * bsw.KSWR_DTYPE.itemsize), len(jp))
                out["b_jobs_one_batch"] = len(jp)
                bsw.ksw_align2_device(eng, jobs[0].ptr, jobs[1].ptr, jobs[2].ptr, jobs[4], jobs[3].ptr)
        tm, ta, tb, sw, hp, kb = [], [], [], [], [], []
        for _ in range(args.reps):
            tm.append(timed(rescue))
            s = bsw.matesw_last_stats(eng)
            sw.append(s.sw_ms)
            hp.append(s.helper_ms)
            if args.only_new:
                continue
            ta.append(timed(pair))
            if jobs:
                tb.append(timed(lambda: bsw.ksw_align2_device(eng, jobs[0].ptr, jobs[1].ptr, jobs[2].ptr, jobs[4], jobs[3].ptr)))
                ms = bsw.mate_last_stats(eng)
                kb.append(ms.fwd_ms + ms.rev_ms)
        out.update({"m_matesw_s": spread(tm), "sw_ms": spread(sw), "helper_ms": spread(hp)})
        if ta:
            out.update({"a_pe_pair_s": spread(ta), "m_over_a_median": round(spread(tm)["median"] / spread(ta)["median"], 3)})
        if tb:
            out.update({"b_ksw_one_batch_s": spread(tb), "b_ksw_kernel_ms": spread(kb),
                        "sw_ms_over_b_kernel_ms": round(spread(sw)["median"] / max(spread(kb)["median"], 1e-9), 3)})
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    eng.close()
    fmi.close()


if __name__ == "__main__":
    main()
