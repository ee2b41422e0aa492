#!/usr/bin/env python
"""Print a benchmark config's compiled plan: its describe() text and every tq_plan_query key
that needs no device.  CPU only (tq_plan_create compiles on the host; nothing is executed).

The tool for "did the planner change?": run it with two builds of the library and compare the
outputs byte for byte (stderr too when a dump knob such as TQ_S2_DUMP=1 is set).  It loads the
package next to it, so a copy under another checkout's scripts/ dumps that checkout's planner.

    python scripts/plan_dump.py C4 > new.txt
    python scripts/plan_dump.py C4 --group-hint 4 --min-chunks 64
    TQ_S2_REORDER=0 python scripts/plan_dump.py C3 --dtype complex128
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

# runtime counters (graph_builds, graph_launches, presplit_fallbacks, coop_timeouts) are left out
KEYS = (
    "n_slices", "out_numel", "arena_bytes", "table_bytes", "flops", "bytes_moved", "flops_once", "flops_slice",
    "bytes_once", "bytes_slice", "n_kernels", "n_ops_once", "n_gemm", "n_apply", "n_permute", "n_sweep",
    "n_sweep_gates", "n_sweep2", "n_launch_once", "n_launch_slice", "n_chain_launches", "n_coop_launches",
    "n_coop_ops", "n_presplit", "lanes", "group_hint", "min_chunks", "planes_gemm", "planes_active",
    "planes_bytes", "planes_ws_bytes", "planes_gemm_M", "planes_gemm_N", "planes_gemm_K", "planes_gemm_lda",
    "planes_gemm_ldb", "s2_programs", "n_s2_programs", "n_s2_block_gate_work", "n_s2_prog_gate_work",
)
# the whole program of a plan with sliced modes (what a call over every slice runs when fold_slices
# is 1); printed last, so the lines above stay comparable with builds that lack these keys
WHOLE_KEYS = (
    "fold_slices", "whole_bytes_moved", "whole_flops", "whole_arena_bytes", "whole_n_launch",
    "whole_n_s2_block_gate_work", "whole_n_s2_prog_gate_work",
)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", help="a circuits.config_task name: C1, C2, C3, C3d, C4, C4g, C4x4")
    ap.add_argument("--dtype", default="complex64", choices=["float32", "float64", "complex64", "complex128"])
    ap.add_argument("--group-hint", type=int, default=1, help='tq_plan_set "group_hint" (lockstep groups)')
    ap.add_argument("--min-chunks", type=int, default=0, help='tq_plan_set "min_chunks" (0: the default)')
    ap.add_argument("--batch", type=int, default=0, help="config_task batch (open qubits of the amplitude block)")
    args = ap.parse_args()

    import torch

    from tneq_qc_amd.circuits import config_task
    from tneq_qc_amd.expression import HipContractExpression

    task = config_task(args.config, batch=args.batch)
    expr = HipContractExpression(task.eq, *task.shapes, optimize=task.path, slices=task.sliced)
    plan = expr.plan(getattr(torch, args.dtype))
    if args.group_hint != 1:
        plan.set("group_hint", args.group_hint)
    if args.min_chunks:
        plan.set("min_chunks", args.min_chunks)
    print(f"# {args.config} {args.dtype} group_hint={args.group_hint} min_chunks={args.min_chunks} batch={args.batch}")
    print(plan.describe(), end="")
    for key in KEYS:
        print(f"{key} = {plan.query(key)}")
    for i in range(1, plan.query("n_s2_programs") + 1):
        print(f"n_s2_prog_passes_{i} = {plan.query(f'n_s2_prog_passes_{i}')}")
    for key in WHOLE_KEYS:
        print(f"{key} = {plan.query(key)}")
    # what the device reads (gather tables, descriptor blobs, launch fields), after the older keys
    for key in ("tables_digest", "whole_tables_digest"):
        print(f"{key} = {plan.query(key)}")


if __name__ == "__main__":
    main()
