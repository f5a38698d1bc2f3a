"""Group-path statistics of pc_kernel on the C2 batch (experiment; GPU box):
   BSW_HIP_LIB=bwa-mem2-arm_amd/lib/libbsw_hip_stats.so python tools/pc_stats.py
Prints rows, groups entered / FAST / masked-R / masked-L, lastpos scans, per wave and per row,
the early stop's scan rows and retired lanes per bound, the left prune's
(§3 item 12) non-zero groups passed over and redo lanes, and the right prune's (§3 item 13) events
(groups the cap's walk passed over), groups between the cap and the static band end, cap retreats and redo lanes by cause.
KERNEL8=2 runs the byte-plane form; H0_HI, QLEN and CELL_BITS give the other bench lines' batches
(bench.py --h0-hi / --qlen / --cell-bits)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem2-arm_amd", "py"))
import numpy as np  # noqa: E402
import hiprt  # noqa: E402
import bsw  # noqa: E402

cfg = bsw.synth_cfg(h0_hi=int(os.environ.get("H0_HI", "100")), qlen=int(os.environ.get("QLEN", "150")))
bits = int(os.environ.get("CELL_BITS", "16"))
pairs, ref, qer = bsw.synth_batch(int(os.environ.get("PAIRS", "1000000")), cfg=cfg)
d = [hiprt.DeviceBuffer.from_array(a) for a in (pairs, ref, qer)]
eng = bsw.Engine(kernel8=int(os.environ.get("KERNEL8", "1")))
L = bsw.hip_lib()
L.bsw_pc_stats.argtypes = [ctypes.c_void_p, ctypes.c_int]
NST = 19
st = (ctypes.c_ulonglong * NST)()
eng.get_scores_device(d[0].ptr, d[1].ptr, d[2].ptr, len(pairs), 100, bits)
L.bsw_pc_stats(st, 1)
eng.get_scores_device(d[0].ptr, d[1].ptr, d[2].ptr, len(pairs), 100, bits)
L.bsw_pc_stats(st, 0)
(rows, ent, fast, mr, ml, lp, waves, ue, scans, ret_s, ret_c, pruned, redo, rev, rcap, rret, rd_cross, rd_zdrop,
 rd_final) = (int(st[k]) for k in range(NST))
print(f"waves {waves} rows {rows} ({rows / waves:.1f}/wave)  groups entered {ent} ({ent / rows:.2f}/row)")
print(f"FAST {fast / ent:.3f}  masked-R {mr / ent:.3f}  masked-L {ml / ent:.3f}  lastpos rows {lp / rows:.3f}")
print(f"per row: entered {ent / rows:.2f}  FAST {fast / rows:.2f}  R {mr / rows:.3f}  L {ml / rows:.3f}")
print(f"uniform-end rows {ue / rows:.3f} (every live lane of the wave at the same band end)")
print(f"early stop: scan rows {scans} ({scans / waves:.2f}/wave)  lanes retired by the scalar bound {ret_s} "
      f"({ret_s / len(pairs):.3f}/pair)  by the per-cell bound {ret_c} ({ret_c / len(pairs):.3f}/pair)")
print(f"left prune: groups pruned {pruned} ({pruned / waves:.2f}/wave)  redo lanes {redo} ({redo / len(pairs):.5f}/pair)")
print(f"right prune: events {rev} ({rev / waves:.2f}/wave)  groups between the cap and the static band end {rcap} ({rcap / rows:.2f}/row: an upper bound of what the cap removes)  "
      f"retreats {rret} ({rret / waves:.2f}/wave)  redo lanes by cause: crossing {rd_cross}  item 12's certificate (z-drop or h1 == 0) {rd_zdrop}  "
      f"final {rd_final}")
print(f"kernel_ms {eng.last_stats().kernel_ms:.3f}")
