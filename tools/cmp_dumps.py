"""Compare two bench.py dumps: every array equal.
   python tools/cmp_dumps.py <dump-a> <dump-b>
Two --dump outputs (<a>.rank0.npz vs <b>.rank0.npz): used to check that a pipelined c4mem step
(--pipeline P) writes exactly what the sequential step writes.  Two --dump-outputs directories
(DIR/<name>.npy): used to check that a kernel change leaves the timed step's outputs as they were."""
import os
import sys

import numpy as np

pa, pb = sys.argv[1:3]
if os.path.isdir(pa):
    names = sorted(f for f in os.listdir(pa) if f.endswith(".npy"))
    other = sorted(f for f in os.listdir(pb) if f.endswith(".npy"))
    a = {f: np.load(os.path.join(pa, f)) for f in names}
    bad = [f for f in names if f not in other or not np.array_equal(a[f], np.load(os.path.join(pb, f)))]
    bad += [f for f in other if f not in names]
    if not names:
        bad = ["(no arrays)"]
    print({k: tuple(v.shape) for k, v in a.items()}, "identical" if not bad else f"DIFFER in {bad}")
else:
    a, b = (np.load(f"{p}.rank0.npz") for p in (pa, pb))
    bad = [k for k in a.files if not np.array_equal(a[k], b[k])]
    print({k: int(a[k].shape[0]) for k in a.files}, "identical" if not bad else f"DIFFER in {bad}")
sys.exit(1 if bad else 0)
