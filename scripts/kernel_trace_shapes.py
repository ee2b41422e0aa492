#!/usr/bin/env python3
"""Summarize a rocprofv3 --kernel-trace CSV by launch shape: per (kernel, grid size, workgroup
size) the dispatches, their total and average duration, and (with --steps N: the bench's steps +
warmup) the time per step.  The per-dispatch trace is megabytes; this table is what profiles/
keeps of it.
    python3 scripts/kernel_trace_shapes.py out/x_kernel_trace.csv --steps 210 > profiles/x_shapes.csv"""
import argparse
import collections
import csv
import re
import sys


def short(name: str) -> str:
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*\)$", "", name)[:96]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=0, help="executes in the run (steps + warmup): adds us_per_step")
    args = ap.parse_args()
    agg = collections.defaultdict(lambda: [0, 0])
    for r in csv.DictReader(open(args.trace)):
        grid = r.get("Grid_Size") or "x".join(r.get(k, "1") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
        wg = r.get("Workgroup_Size") or "x".join(r.get(k, "1") for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"))
        a = agg[(short(r["Kernel_Name"]), grid, wg)]
        a[0] += 1
        a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "grid_size", "workgroup_size", "dispatches", "total_us", "avg_us"] + (["us_per_step"] if args.steps else []))
    for (name, grid, wg), (n, ns) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        row = [name, grid, wg, n, f"{ns / 1e3:.1f}", f"{ns / 1e3 / n:.2f}"]
        if args.steps:
            row.append(f"{ns / 1e3 / args.steps:.2f}")
        w.writerow(row)


if __name__ == "__main__":
    main()
