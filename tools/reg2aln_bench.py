#!/usr/bin/env python3
"""regions/s of bsw_reg2aln_resident (include/bsw_aln.h) on the regions of --reads 151 bp reads
taken through the GPU front end (bsw_mem_collect_intv_device -> bsw_mem_chain_device ->
bsw_chain2aln_resident), against what a caller could do before it: bsw_ksw_global2_device over
host-prebuilt first-pass jobs of ALL those regions (job building and NM / MD excluded from its
time -- they ran on the host).  Both in one process, alternating, --reps times each; prints one
JSON line (and writes it to --out).  --only-new: just the new call (for a kernel trace).

    python tools/reg2aln_bench.py --reads 1000000 --ref-mb 16 --reps 7 --out profiles/reg2aln/bench.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem2-arm_amd", "py"))
import bsw  # noqa: E402
import hiprt  # noqa: E402
from resident import ResidentBatch  # noqa: E402


def make_reads(ref, n, L, seed, p_sub, p_n, indel_frac):
    """n reads of L bases from either strand: substitutions, N bases, and in indel_frac of the
    reads one insertion or deletion of 1..6 bases"""
    rng = np.random.default_rng(seed)
    st = rng.integers(0, len(ref) - L - 8, n)
    src = ref[st[:, None] + np.arange(L + 8)[None, :]]
    reads = src[:, :L].copy()
    for i in np.flatnonzero(rng.random(n) < indel_frac):
        p, g = int(rng.integers(20, L - 20)), int(rng.integers(1, 7))
        if rng.random() < 0.5:                               # deletion from the read
            reads[i] = np.concatenate([src[i, :p], src[i, p + g:L + g]])
        else:
            reads[i] = np.concatenate([src[i, :p], rng.integers(0, 4, g).astype(np.uint8), src[i, p:L - g]])
    flip = rng.random(n) < 0.5
    reads[flip] = (3 - reads[flip][:, ::-1]).astype(np.uint8)
    sub = rng.random(reads.shape) < p_sub
    reads[sub] = ((reads[sub] + rng.integers(1, 4, int(sub.sum()))) % 4).astype(np.uint8)
    reads[rng.random(reads.shape) < p_n] = 4
    return np.ascontiguousarray(reads).reshape(-1), np.arange(n, dtype=np.int64) * L, np.full(n, L, np.int32)


def infer_bw(l1, l2, score, a, q, r):
    w = np.trunc((np.minimum(l1, l2) * a - score - q) / r + 2.0).astype(np.int64)
    w = np.maximum(w, np.abs(l1 - l2))
    return np.where((l1 == l2) & (l1 * a - score < (q + r - a) * 2), 0, w)


def first_pass_jobs(T, l_pac, reads, off, regs, sr, W, a=1, o=6, e=1):
    """SeqPairs + code buffers of bwa_gen_cigar2's first pass for every non-rejected region"""
    rb, re, qb, qe = (regs[f].astype(np.int64) for f in ("rb", "re", "qb", "qe"))
    keep = np.flatnonzero(~((rb < 0) | (re < 0) | (qe - qb <= 0) | (rb >= re) | ((rb < l_pac) & (re > l_pac))))
    rb, re, qb, qe = rb[keep], re[keep], qb[keep], qe[keep]
    lq, rl = qe - qb, re - rb
    w2 = infer_bw(lq, rl, regs["truesc"][keep].astype(np.int64), a, o, e)
    w2 = np.where(w2 > W, np.minimum(w2, regs["w"][keep]), w2)
    w2 = np.minimum(w2, W << 2)
    mg = np.maximum(np.trunc((((lq + 1) >> 1) * a - o) / e + 1.0).astype(np.int64), 1)
    d = np.abs(rl - lq)
    band = np.maximum(np.minimum((mg + d + 1) >> 1, w2), d + 3)
    n, qs, ts = len(keep), int(lq.max()), int(rl.max())
    assert n * max(qs, ts) < 2 ** 31
    qbuf, tbuf = np.zeros((n, qs), np.uint8), np.zeros((n, ts), np.uint8)
    rev = rb >= l_pac
    r0 = off[sr[keep]]
    for a0 in range(0, n, 65536):
        s = slice(a0, min(n, a0 + 65536))
        k = np.arange(qs)[None, :]
        src = np.where(rev[s, None], (r0[s] + qe[s] - 1)[:, None] - k, (r0[s] + qb[s])[:, None] + k)
        ok = k < lq[s, None]
        qbuf[s][ok] = reads[np.where(ok, src, 0)][ok]
        k = np.arange(ts)[None, :]
        src = np.where(rev[s, None], (re[s] - 1)[:, None] - k, rb[s][:, None] + k)
        ok = k < rl[s, None]
        tbuf[s][ok] = T[np.where(ok, src, 0)][ok]
    pairs = np.zeros(n, dtype=bsw.SEQPAIR_DTYPE)
    pairs["idr"], pairs["idq"], pairs["id"] = np.arange(n) * ts, np.arange(n) * qs, np.arange(n)
    pairs["len1"], pairs["len2"], pairs["h0"] = rl, lq, band
    return pairs, tbuf.reshape(-1), qbuf.reshape(-1), int((w2 == 0).sum())


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "n": len(xs)}


def timed(f, *a):
    t = time.perf_counter()
    f(*a)
    return time.perf_counter() - t


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
    log = lambda m: print(f"[reg2aln_bench] {m}", file=sys.stderr, flush=True)  # noqa: E731
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
    b = ResidentBatch(eng, reads, off, lens)
    _, sr, _ = b.seed_and_chain(fmi)
    ns = len(sr)
    b.chain2aln(opt)                                         # its regions, one per seed, are the current lists
    log(f"{n} reads -> {ns} regions (skipped seeds included)")
    cs, ms = args.cigar_stride, args.md_stride

    def new_call():
        t = time.perf_counter()
        b.reg2aln(opt, cs, ms)
        return time.perf_counter() - t

    old_call = None
    if not args.only_new:
        regs = b.get("regs")
        t0 = time.perf_counter()
        pairs, tbuf, qbuf, n_w0 = first_pass_jobs(T, l_pac, reads, off, regs, sr, args.w)
        log(f"{len(pairs)} first-pass jobs built on the host in {time.perf_counter() - t0:.1f} s")
        d_pairs, d_t, d_q = (hiprt.DeviceBuffer.from_array(x) for x in (pairs, tbuf, qbuf))
        d_jc, d_jn = hiprt.DeviceBuffer(len(pairs) * cs * 4), hiprt.DeviceBuffer(len(pairs) * 4)

        def old_call():
            t = time.perf_counter()
            bsw.ksw_global2_device(eng, d_pairs.ptr, d_t.ptr, d_q.ptr, len(pairs), d_jc.ptr, cs, d_jn.ptr)
            return time.perf_counter() - t

    new_call()                                               # warm-up: buffers grown, code loaded
    if old_call:
        old_call()
    tn, to, hs, ds, gk = [], [], [], [], []
    for _ in range(args.reps):
        tn.append(new_call())
        st = bsw.aln_last_stats(eng)
        hs.append(st.helper_ms)
        ds.append(st.dp_ms)
        if old_call:
            to.append(old_call())
            gk.append(bsw.global_last_stats(eng).kernel_ms)
    st = bsw.aln_last_stats(eng)
    live = ns - st.n_rejected
    out = {"tool": "reg2aln_bench", "reads": n, "read_len": args.read_len, "ref_mb": args.ref_mb, "w": args.w,
           "p_sub": args.p_sub, "p_n": args.p_n, "indel_frac": args.indel_frac, "cigar_stride": cs, "md_stride": ms,
           "regions": ns, "rejected": st.n_rejected, "gapfree": st.n_gapfree, "dp_jobs_per_pass": list(st.n_dp),
           "gapfree_share_of_live": round(st.n_gapfree / max(live, 1), 4),
           "reg2aln_resident_s": spread(tn), "reg2aln_regions_per_s": round(ns / spread(tn)["median"]),
           "reg2aln_live_regions_per_s": round(live / spread(tn)["median"]),
           "helper_kernel_ms": spread(hs), "dp_kernel_ms": spread(ds)}
    if old_call:
        out.update({"comparator": "bsw_ksw_global2_device over host-prebuilt first-pass jobs of all live regions",
                    "comparator_jobs": len(pairs), "comparator_jobs_w0": n_w0, "comparator_s": spread(to),
                    "comparator_kernel_ms": spread(gk),
                    "comparator_regions_per_s": round(len(pairs) / spread(to)["median"]),
                    "speedup_median": round(spread(to)["median"] / spread(tn)["median"], 3)})
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
