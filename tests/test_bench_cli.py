"""bench.py's command line: a plain run times exactly --steps steps and carries none of the
--full legs; --dump-outputs writes the last timed step's outputs, equal to the CPU oracle."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bsw
import oracle
from conftest import ROOT


def test_dump_outputs_caps_and_samples_reproducibly(tmp_path, monkeypatch):
    """past the byte cap every array keeps the same seeded, ordered fraction of its rows; a
    structured array gives one float64 file per field"""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 3000)
    rec = np.zeros(4000, dtype=[("a", "<i4"), ("b", "<i8")])
    rec["a"] = np.arange(4000)
    rec["b"] = np.arange(4000, dtype=np.int64) + (1 << 40)
    mat = np.arange(8000, dtype=np.int32).reshape(4000, 2)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"rec": rec, "mat": mat})
    names = sorted(os.listdir(tmp_path / "x"))
    assert names == ["mat.npy", "rec.a.npy", "rec.b.npy"]
    got = {n: np.load(tmp_path / "x" / n) for n in names}
    assert all(np.array_equal(got[n], np.load(tmp_path / "y" / n)) for n in names)
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 8 * 3000
    rows = got["rec.a.npy"].astype(np.int64)
    assert len(rows) == 3000 // 4 and np.all(np.diff(rows) > 0)            # 4 columns in all: 3/4 of a quarter
    assert np.array_equal(got["rec.b.npy"], rows + float(1 << 40))         # the same rows of every array
    assert np.array_equal(got["mat.npy"], mat[rows].astype(np.float64))
    # under the cap: every row
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64_000_000)
    bench.dump_outputs(str(tmp_path / "z"), {"mat": mat})
    assert np.array_equal(np.load(tmp_path / "z" / "mat.npy"), mat.astype(np.float64))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    n, dump = 30_000, str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--pairs", str(n), "--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "int16"
    assert abs(line["value"] - n / line["ms_per_step"] / 1e3) <= 0.01 * line["value"]
    for k in ("cpu_baseline", "speedup_vs_cpu", "abi_inclusive", "abi_inclusive_value", "wide_kernel_comparison"):
        assert k not in line, k
    want, ref, qer = bsw.synth_batch(n)
    oracle.get_scores(oracle.make_params(), want, ref, qer, 100, nthreads=16)
    assert sorted(os.listdir(dump)) == sorted(f"{f}.npy" for f in bsw.OUT_FIELDS)
    for f in bsw.OUT_FIELDS:
        got = np.load(os.path.join(dump, f"{f}.npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want[f].astype(np.float64)), f
