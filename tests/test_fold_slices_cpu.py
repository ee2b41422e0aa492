"""The whole program of a sliced plan (tq_plan.h Plan::whole): a plan created with sliced modes
also holds the same network and path compiled with no sliced modes, and an execute call that
covers every slice runs that instead of the slice lanes when it costs no more (bytes, flops,
arena) and the sliced program's per-slice part holds no GEMM.  Compile-only (no GPU): which
configs fold, that the whole_* queries are those of a plan created without slices, that the
sliced program's description and keys do not move with the switch, and that the switch follows
the plan through a recompile and a clone.  Parity on the GPU: test_fold_slices_gpu.py."""
import functools

import pytest
import torch

from tneq_qc_amd.circuits import config_task
from tneq_qc_amd.expression import HipContractExpression

# keys that describe the sliced program (scripts/plan_dump.py prints the same set)
OLD_KEYS = (
    "n_slices", "out_numel", "arena_bytes", "table_bytes", "flops", "bytes_moved", "flops_once", "flops_slice",
    "bytes_once", "bytes_slice", "n_kernels", "n_ops_once", "n_gemm", "n_apply", "n_permute", "n_sweep",
    "n_sweep_gates", "n_sweep2", "n_launch_once", "n_launch_slice", "n_chain_launches", "lanes", "group_hint",
    "min_chunks", "planes_gemm", "planes_bytes", "s2_programs", "n_s2_block_gate_work", "n_s2_prog_gate_work",
)
# whole_* key -> the query it equals on a plan created with slices=()
WHOLE = {
    "whole_bytes_moved": "bytes_moved", "whole_flops": "flops", "whole_arena_bytes": "arena_bytes",
    "whole_n_s2_block_gate_work": "n_s2_block_gate_work", "whole_n_s2_prog_gate_work": "n_s2_prog_gate_work",
}


@functools.lru_cache(maxsize=None)
def _shared(cfg, min_chunks=0, sliced=True):
    """A plan the tests only query (compiled once)."""
    return _plan(cfg, min_chunks, sliced)


def _plan(cfg, min_chunks=0, sliced=True):
    t = config_task(cfg)
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced if sliced else ())
    p = e.plan(torch.complex64)
    if min_chunks:
        p.set("min_chunks", min_chunks)
    return e, p


@pytest.mark.parametrize("cfg,min_chunks", [("C4", 64), ("C4x4", 0), ("C3d", 0)])
def test_eligible_configs_fold(cfg, min_chunks):
    _, p = _shared(cfg, min_chunks)
    _, w = _shared(cfg, min_chunks, sliced=False)
    assert p.query("n_slices") > 1 and w.query("n_slices") == 1
    assert p.query("fold_slices") == 1
    for key, plain in WHOLE.items():
        assert p.query(key) == w.query(plain), key
        print(f"{cfg} {plain}: sliced {p.query(plain)}, whole {p.query(key)}")
    assert p.query("whole_n_launch") == w.query("n_launch_once") + w.query("n_launch_slice")
    # the costs the choice is made by
    for key in ("bytes_moved", "flops", "arena_bytes"):
        assert p.query("whole_" + key) <= p.query(key)
    assert p.query("folded_executes") == 0
    assert w.query("fold_slices") == 0 and w.query("whole_flops") == -1   # nothing to fold


@pytest.mark.parametrize("cfg", ["C3", "C4g"])
def test_other_configs_keep_the_lanes(cfg):
    _, p = _shared(cfg)
    assert p.query("fold_slices") == 0
    assert p.query("whole_flops") > 0   # compiled, not chosen
    if cfg == "C4g":   # ruled out by cost: the whole program's arena
        assert p.query("whole_arena_bytes") > p.query("arena_bytes")


def test_switch_keeps_the_sliced_program():
    _, p = _plan("C4", 64)
    on = p.describe(), [p.query(k) for k in OLD_KEYS]
    whole = [p.query(k) for k in WHOLE]
    p.set("fold_slices", 0)
    assert p.query("fold_slices") == 0
    assert (p.describe(), [p.query(k) for k in OLD_KEYS]) == on
    assert [p.query(k) for k in WHOLE] == whole
    assert p.query("lanes") == 8 and "lane-sum" in p.describe()
    p.set("fold_slices", 1)
    assert p.query("fold_slices") == 1
    assert (p.describe(), [p.query(k) for k in OLD_KEYS]) == on


def test_switch_survives_recompile_and_clone():
    _, p = _plan("C4")
    w128 = p.query("whole_n_s2_block_gate_work")
    p.set("fold_slices", 0)
    p.set("min_chunks", 64)
    assert p.query("fold_slices") == 0
    # the whole program follows the parent's min_chunks
    _, w = _shared("C4", 64, sliced=False)
    assert p.query("whole_n_s2_block_gate_work") == w.query("n_s2_block_gate_work") != w128
    c = p.clone()
    assert c.query("fold_slices") == 0 and c.query("whole_bytes_moved") == p.query("whole_bytes_moved")
    p.set("fold_slices", 1)
    p.set("group_hint", 2)
    assert p.query("fold_slices") == 1
    assert p.clone().query("fold_slices") == 1 and c.query("fold_slices") == 0
    # the pass-program switch reaches the whole program as well
    p.set("s2_programs", 0)
    assert p.query("whole_n_s2_prog_gate_work") == 0 and p.query("whole_n_s2_block_gate_work") > 0
    assert p.clone().query("whole_n_s2_prog_gate_work") == 0
