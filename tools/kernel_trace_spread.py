#!/usr/bin/env python3
"""Per-kernel launch durations of a rocprofv3 --kernel-trace run: n, mean, median, min and max in milliseconds for every rtd_*
kernel instance (and grid size) of the kernel_trace.csv files given -- the launch-to-launch spread that a difference between two
builds has to exceed.

Usage: python tools/kernel_trace_spread.py [--per-launch FILE KERNEL_SUBSTRING] OUT_DIR/**/*kernel_trace.csv
--per-launch: also write the durations (ms, in launch order, one per line) of the kernels whose name contains the substring, so that
two builds that ran the same program can be compared launch by launch (window i of one against window i of the other)."""
import collections
import csv
import re
import statistics
import sys

args = sys.argv[1:]
per_launch = None
if args and args[0] == "--per-launch":
    per_launch, args = (args[1], args[2]), args[3:]
acc = collections.defaultdict(list)
ordered = []
for path in args:
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"rtd_\w+(<[^>]*>)?", row.get("Kernel_Name", ""))
            if m:
                grid = row.get("Grid_Size") or row.get("Grid_Size_X") or "?"
                ms = (float(row["End_Timestamp"]) - float(row["Start_Timestamp"])) * 1e-6
                acc[(m.group(0).replace(", ", ","), grid)].append(ms)
                if per_launch and per_launch[1] in m.group(0):
                    ordered.append((float(row["Start_Timestamp"]), ms))
for (k, g), v in sorted(acc.items()):
    print(f"{k} grid={g} n={len(v)} mean={statistics.fmean(v):.4f} median={statistics.median(v):.4f} min={min(v):.4f} max={max(v):.4f} ms")
if per_launch:
    with open(per_launch[0], "w") as f:
        f.write("".join(f"{ms:.6f}\n" for _, ms in sorted(ordered)))
