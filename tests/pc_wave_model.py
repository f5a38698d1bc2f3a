"""The Python side of tests/pc_wave_model.c, the CPU model of the packed-column kernel's row loop with its
wave-level rules (left skip, left prune, right prune).  The C file is compiled
against the kernel's own rules header (bsw_pc_rules.h) and hands its values over through
pc_model_defaults(): no tunable's number is written here.

Redo lanes are recomputed with both prunes off, in waves of their own, in list order.  Per pair the model
returns the six outputs, the rows the lane ran (a redo lane's are those of its second run) and the redo mark;
per wave the NST figures named in WST.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pc_batches import default_order, qmax_class

# per-wave figures.  skipped: groups the skip and the left prune removed from the entered set.  cap_span: groups
# between the wave's clamped band end and its static band end, summed over the rows under a cap -- an upper bound of
# what the cap removes (the lazy edge may have dropped some of them anyway); what it removes is the difference in
# `entered` against a run with rprune=False.  clipped: lanes whose band end ever sat at the cap.  redo_item12:
# item 12's certificate (z-drop, or h1 == 0 in a left-pruned wave)
WST = ("rows", "entered", "skipped", "left_events", "redo", "right_events", "cap_span", "retreats",
       "redo_crossing", "redo_item12", "redo_final", "group_tests", "clipped")
NST = len(WST)

_HERE = os.path.dirname(os.path.abspath(__file__))
_RULES_DIR = os.path.join(_HERE, os.pardir, "bwa-mem2-arm_amd", "csrc")


class Cfg(ctypes.Structure):
    """cfg_t: the three rules' flags, then the schedule and the constants, by the names run() takes as keywords."""
    _fields_ = [(n, ctypes.c_int32) for n in ("skip", "prune", "rprune", "skip_mask", "skip_row", "scan_phase",
                                               "skip_qmin", "prune_qmin", "margin", "slack", "slack2", "k", "row0",
                                               "walk_mask", "rwin", "touched")]


_lib = None


def build(dirpath) -> ctypes.CDLL:
    """Compile the model into `dirpath` (a test's tmp_path) and load it; once per process."""
    global _lib
    if _lib is None:
        so = os.path.join(str(dirpath), "libpc_wave_model.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=c11", "-fPIC", "-shared", "-I", _RULES_DIR, "-o", so,
                        os.path.join(_HERE, "pc_wave_model.c")], check=True)
        _lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int32
        _lib.pc_model.argtypes = [P, P, P, P, I, P, P, I, I, I, P, P, P]
        _lib.pc_model.restype = None
        _lib.pc_model_defaults.argtypes = [P]
        _lib.pc_model_defaults.restype = None
    return _lib


def defaults(lib) -> Cfg:
    """The kernel's compiled-in switches, schedule and constants (bsw_pc_rules.h)."""
    cfg = Cfg()
    lib.pc_model_defaults(ctypes.byref(cfg))
    return cfg


def run(lib, params, pairs, ref, qer, w, order=None, skip=True, prune=True, rprune=True, threads=8, **over):
    """(outputs, rows per pair, redo mark per pair, per-wave figures [nw, NST]): `pairs` is not modified.
    `order` lists the lanes (wave v = order[64 v : 64 v + 64]; default: every pair, as given); pairs it leaves
    out keep their input fields and 0 rows.  A rule runs when its flag is set here and in the header.  `over`
    replaces the header's schedule and constants by Cfg's field names (margin=, slack=, skip_mask=, ...)."""
    cfg = defaults(lib)
    cfg.skip, cfg.prune, cfg.rprune = cfg.skip and skip, cfg.prune and prune, cfg.rprune and rprune
    for name, v in over.items():
        if name not in dict(Cfg._fields_) or name in ("skip", "prune", "rprune"):
            raise TypeError(f"run() got an unexpected keyword argument {name!r}")
        setattr(cfg, name, v)
    out = pairs.copy()
    idx = np.ascontiguousarray(np.arange(len(out)) if order is None else order, np.int32)
    n = len(idx)
    nw = (n + 63) // 64
    rows = np.zeros(len(out), np.int32)
    redo = np.zeros(len(out), np.uint8)
    wst = np.zeros((nw, NST), np.int64)
    ref = np.ascontiguousarray(ref, np.uint8)
    qer = np.ascontiguousarray(qer, np.uint8)
    step = max(1, (nw + threads - 1) // threads)

    def part(a):
        lib.pc_model(ctypes.byref(params), ctypes.byref(cfg), ctypes.c_void_p(out.ctypes.data),
                     ctypes.c_void_p(idx.ctypes.data), n, ctypes.c_void_p(ref.ctypes.data),
                     ctypes.c_void_p(qer.ctypes.data), w, a, min(nw, a + step), ctypes.c_void_p(rows.ctypes.data),
                     ctypes.c_void_p(redo.ctypes.data), ctypes.c_void_p(wst.ctypes.data))

    if nw:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(part, range(0, nw, step)))
    again = idx[redo[idx] != 0]
    if len(again):
        o2, r2, _, _ = run(lib, params, pairs, ref, qer, w, order=again, skip=skip, prune=False, rprune=False,
                           threads=threads, **over)
        out[again], rows[again] = o2[again], r2[again]
    return out, rows, redo, wst


def run_planned(lib, params, pairs, ref, qer, w, **kw):
    """As run(), with the lanes laid out as the engine lays them out: one launch per QMAX class over its slice
    of default_order() -- no wave holds pairs of two classes -- each class with a redo list of its own."""
    order = default_order(pairs, ref, qer)
    cls = qmax_class(pairs)[order]
    out, rows, redo, wsts = pairs.copy(), np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.uint8), []
    for c in np.unique(cls):
        sub = order[cls == c]
        o, r, d, wst = run(lib, params, pairs, ref, qer, w, order=sub, **kw)
        out[sub], rows[sub], redo[sub] = o[sub], r[sub], d[sub]
        wsts.append(wst)
    return out, rows, redo, np.concatenate(wsts) if wsts else np.zeros((0, NST), np.int64)


def totals(wst):
    """The per-wave figures summed, by name."""
    t = dict(zip(WST, (int(v) for v in wst.sum(0))))
    t["refused"] = t["group_tests"] - t["right_events"]      # group tests the walk stopped at
    return t
