#!/usr/bin/env python3
"""Summarises the phoneme-level front of every step (text encoder + duration predictor: from the step's first kernel through
durations_kernel) in a rocprofv3 --kernel-trace CSV: launches and kernel microseconds per step, and per (kernel, grid) the microseconds
per launch with sigma and n.  The first third of the steps is dropped as warm-up.  A step starts at the first embed_kernel or
col_proj_kernel behind the previous step's durations_kernel.
   python tools/trace_front.py <dir-with-*_kernel_trace.csv>"""
import csv, glob, os, re, statistics, sys
from collections import defaultdict


def main():
    d = sys.argv[1]
    f = max(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], None
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("sts::", "")
        if cur is None:
            if not (name.startswith("embed_kernel") or name.startswith("col_proj_kernel")):
                continue
            cur = []
        wg = [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]
        grid = "x".join(str(int(r[f"Grid_Size_{a}"]) // w) for a, w in zip("XYZ", wg))
        cur.append((f"{name} [{grid} wg {wg[0]}]", (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3,
                    int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        if name.startswith("durations_kernel"):
            steps.append(cur)
            cur = None
    steps = steps[len(steps) // 3:]
    if not steps:
        print("no complete step in the trace"); return
    n = [len(s) for s in steps]
    us = [sum(k[1] for k in s) for s in steps]
    span = [(s[-1][3] - s[0][2]) / 1e3 for s in steps]
    sd = lambda v: statistics.pstdev(v) if len(v) > 1 else 0.0
    print(f"{len(steps)} steps; front launches per step {statistics.mean(n):.1f} (min {min(n)}, max {max(n)}); "
          f"kernel us per step {statistics.mean(us):.1f} (sigma {sd(us):.1f}); span us per step {statistics.mean(span):.1f} (sigma {sd(span):.1f})")
    by = defaultdict(list)
    for s in steps:
        for k in s:
            by[k[0]].append(k[1])
    print(f"{'us/launch':>10s} {'sigma':>6s} {'n':>5s} {'per step':>8s}  kernel [workgroups]")
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{statistics.mean(v):10.2f} {sd(v):6.2f} {len(v):5d} {len(v) / len(steps):8.1f}  {k}")


if __name__ == "__main__":
    main()
