"""What runs between a step's plan and its DP kernel, from a rocprofv3 kernel trace of bench.py's default line.
   python tools/plan_span.py <..._kernel_trace.csv>
Per step (one plan_kernel dispatch each): the kernels from plan_kernel up to the first pc_kernel, their count
and summed duration without plan_kernel, and the span from plan_kernel's start to pc_kernel's start.  Traced
times carry the tracer's overhead: compare traces with traces."""
import csv
import sys
from collections import Counter

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
short = lambda n: n.split("(")[0].split("<")[0].split("::")[-1] if "trampoline" not in n else (
    "rocprim:" + n.split("wrapped_")[1].split("_config")[0])
steps, cur = [], None
for r in rows:
    name = r["Kernel_Name"]
    if "plan_kernel" in name:
        cur = [r]
    elif cur is not None:
        if "pc_kernel" in name:
            steps.append((cur, r))
            cur = None
        else:
            cur.append(r)
for k, (ks, dp) in enumerate(steps):
    t0 = int(ks[0]["Start_Timestamp"])
    between = ks[1:]
    dur = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in between)
    plan = int(ks[0]["End_Timestamp"]) - t0
    names = Counter(short(r["Kernel_Name"]) for r in between)
    print(f"step {k}: plan_kernel {plan / 1e3:.1f} us; {len(between)} kernels after it, {dur / 1e3:.1f} us summed; "
          f"plan start -> DP start {(int(dp['Start_Timestamp']) - t0) / 1e3:.1f} us")
    if k == len(steps) - 1:
        for n, c in names.items():
            d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in between if short(r["Kernel_Name"]) == n]
            print(f"    {c:3d} x {n}: {sum(d) / len(d) / 1e3:.1f} us each")
