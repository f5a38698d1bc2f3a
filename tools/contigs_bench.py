#!/usr/bin/env python3
"""What the contig table (include/bsw_contigs.h) costs, stage by stage.  --pairs fragments (2 x 150 bp,
insert 400-600, drawn anywhere on the text: some bridge a join) against a --ref-mb reference cut into
--contigs contigs of unequal length; a fraction --unseedable of the mates carries a substitution every 13 to
16 bases, so that the rescue has jobs.  The SMEM intervals are collected once (they read no table).  Then,
alternating in one process, --reps times each, under
  (a) no table     (b) a table of 1 contig     (c) the table of --contigs contigs
(set on the index and on the context), every stage behind the intervals, each on the one before:
  bsw_mem_chain_device, bsw_chain2aln_resident, bsw_regs_select_resident (wall), bsw_pe_stat_resident,
  bsw_matesw_resident, bsw_pe_pair_resident (kernel ms and wall), bsw_reg2aln_resident over ALL selected regions
  (kernel ms; arrays of its own), bsw_records_resident (aln_ms, helper_ms, wall), bsw_sam_text_resident
  (kernel ms, wall).
The setters allocate, which idles the device: after each switch of the table the whole chain runs once
untimed, so that no timed call pays for it.
Prints one JSON line per case (and writes them to --out).  --cases a: case (a) alone, without a call of the
setters -- the form that also runs on a tree from before the table, for the comparison with it.

    python tools/contigs_bench.py --pairs 1000000 --ref-mb 16 --reps 7 --out profiles/contigs/bench.json
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

STAGES = ("chain_s", "ext_s", "select_s", "stat_s", "stat_ms", "matesw_s", "matesw_ms", "pair_s", "pair_ms", "reg2aln_ms",
          "rec_s", "rec_aln_ms", "rec_helper_ms", "text_s", "text_ms")


def contig_lengths(total, n, seed=5):
    """n unequal lengths that sum to total, none below 2,000"""
    w = np.random.default_rng(seed).random(n) ** 2 + 0.02
    lens = np.maximum((w / w.sum() * total).astype(np.int64), 2000)
    lens[np.argmax(lens)] += total - lens.sum()
    assert lens.sum() == total and lens.min() >= 2000
    return lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-mb", type=int, default=16)
    ap.add_argument("--contigs", type=int, default=64)
    ap.add_argument("--unseedable", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    log = lambda m: print(f"[contigs_bench] {m}", file=sys.stderr, flush=True)  # noqa: E731
    ref = bsw.synth_reference(args.ref_mb * 1_000_000, seed=7)
    nb = ref > 3
    ref[nb] = np.random.default_rng(1).integers(0, 4, int(nb.sum()), dtype=np.uint8)
    l_pac = len(ref)
    clens = contig_lengths(l_pac, args.contigs)
    RL = args.read_len
    reads, off, lens = pe_reads(ref, args.pairs, RL, seed=42)
    n = len(lens)
    rows = reads.reshape(n, RL)
    hit = np.flatnonzero(np.random.default_rng(3).random(n // 2) < args.unseedable)
    cols, k0, i = [], 7, 0
    while k0 < RL:
        cols.append(k0)
        k0 += 13 + i % 4
        i += 1
    for c in cols:                                           # mate 2p + 1 of the chosen pairs
        v = rows[2 * hit + 1, c]
        rows[2 * hit + 1, c] = np.where(v < 4, (v + 1) % 4, v)
    T = np.concatenate([ref, (3 - ref[::-1])]).astype(np.uint8)
    t0 = time.perf_counter()
    fmi = bsw.Fmi(ref)
    log(f"index of {len(ref)} bases built in {time.perf_counter() - t0:.1f} s; {len(hit)} unseedable mates")
    eng = bsw.Engine()
    bsw.set_reference(eng, T)
    opt = bsw.ext_opt(w=args.w, l_pac=l_pac)
    sopt = bsw.sel_opt(w=args.w, l_pac=l_pac)
    popt = bsw.pe_opt(l_pac=l_pac)
    mopt = bsw.matesw_opt(l_pac=l_pac)
    ropt = bsw.rec_opt(w=args.w, l_pac=l_pac, rname="chrS")
    b = ResidentBatch(eng, reads, off, lens, quals=(33 + (np.arange(len(reads)) * 7) % 41).astype(np.uint8))
    names = [b"frag%08d" % i for i in range(n // 2)]
    d_reads, d_off, d_len = (b.buf[x] for x in ("reads", "off", "lens"))
    icap = 256
    d_mems, d_cnt = hiprt.DeviceBuffer(n * icap * bsw.BWTINTV_DTYPE.itemsize), hiprt.DeviceBuffer(n * 4)
    bsw._check(fmi.collect_intv_device(d_reads.ptr, d_off.ptr, d_len.ptr, n, RL, d_mems.ptr, icap, d_cnt.ptr))
    tables = {"a": None, "b": ([l_pac], ["chrS"]),
              "c": (clens, [("ctg%02d_" % i) + "x" * (i % 40) for i in range(len(clens))])}

    def use(case):
        if args.cases != "a":                                # (case (a) alone never names the setters)
            tb = tables[case] or ((), ())
            bsw.set_contigs(eng, *tb)
            fmi.set_contigs(tb[0])

    need = 0
    for case in args.cases:                                  # the seeds every case needs
        use(case)
        rc_, ns_ = fmi.mem_chain_device(d_len.ptr, n, d_mems.ptr, icap, d_cnt.ptr, 0, 0, 0, 0)
        assert rc_ in (0, -34), rc_
        need = max(need, ns_)
    S = need + 1024
    d_seeds, d_sr, d_sc = (b.alloc(x, S) for x in ("seeds", "sr", "sc"))
    cap = S + 8 * len(hit) + 1024                            # the rescue's output: the lists plus at most 4 per call
    st = {}

    def chain():
        rc_, st["ns"] = fmi.mem_chain_device(d_len.ptr, n, d_mems.ptr, icap, d_cnt.ptr, d_seeds.ptr, d_sr.ptr, d_sc.ptr, S)
        bsw._check(rc_)
        b.n["seeds"] = st["ns"]

    def extend():
        b.chain2aln(opt)

    def select():
        st["k"] = b.select(sopt)

    def stat():
        st["pes"] = b.pe_stat(popt)

    def rescue():
        st["m"] = b.matesw(st["pes"], mopt, cap=cap)

    def pair():
        b.pe_pair(st["pes"], popt)

    def all_regions():
        b.reg2aln(opt, into="all.aln")

    def records():
        b.records(ropt)

    def text(tcap):
        return b.sam_text(ropt, None, True, cap=tcap)

    front = (chain, extend, select, stat, rescue, pair, all_regions, records)

    size = {}
    for case in args.cases:                                  # the size of each case's text
        use(case)
        for f in front:
            f()
        size[case] = b.sam_text(ropt, names, True)
    b.alloc("text", max(size.values()) + 4)
    t = {c: {m: [] for m in STAGES} for c in args.cases}
    for _ in range(args.reps):
        for case in args.cases:
            use(case)
            for f in front:                                  # untimed: see the docstring
                f()
            text(size[case])
            x = t[case]
            x["chain_s"].append(timed(chain))
            x["ext_s"].append(timed(extend))
            x["select_s"].append(timed(select))
            x["stat_s"].append(timed(stat))
            x["stat_ms"].append(bsw.pe_last_stats(eng).kernel_ms)
            x["matesw_s"].append(timed(rescue))
            ms_ = bsw.matesw_last_stats(eng)
            x["matesw_ms"].append(ms_.sw_ms + ms_.helper_ms)
            x["pair_s"].append(timed(pair))
            ps = bsw.pe_last_stats(eng)
            x["pair_ms"].append(ps.kernel_ms)
            all_regions()
            a = bsw.aln_last_stats(eng)
            x["reg2aln_ms"].append(a.dp_ms + a.helper_ms)
            x["rec_s"].append(timed(records))
            rs = bsw.rec_last_stats(eng)
            x["rec_aln_ms"].append(rs.aln_ms)
            x["rec_helper_ms"].append(rs.helper_ms)
            x["text_s"].append(timed(text, size[case]))
            x["text_ms"].append(bsw.rec_last_stats(eng).text_ms)
            x["counts"] = {"seeds": int(st["ns"]), "selected": int(st["k"]), "after_rescue": int(st["m"]),
                           "matesw_jobs": ms_.n_jobs, "paired": ps.n_paired, "proper": ps.n_proper, "records": rs.n_rec,
                           "rejected_of_all_regions": a.n_rejected}
    lines = []
    for case in args.cases:
        o = {"tool": "contigs_bench", "tag": args.tag, "case": case,
             "contigs": 0 if case == "a" else 1 if case == "b" else len(clens), "pairs": n // 2, "read_len": RL,
             "ref_mb": args.ref_mb, "unseedable_mates": int(len(hit)), "text_bytes": int(size[case])}
        o.update(t[case]["counts"])
        o.update({m: spread(v) for m, v in t[case].items() if isinstance(v, list)})
        lines.append(json.dumps(o))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()
    fmi.close()


if __name__ == "__main__":
    main()
