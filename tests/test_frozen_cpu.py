"""Frozen steps at compile time (no GPU: tq_plan_create / tq_plan_set_volatile only compile).

A plan told which inputs are volatile (tq_plan_set_volatile) marks every step whose subtree holds
no volatile and no sliced input frozen, gives the ops of those steps a schedule of their own in
front of the hoisted one and pins what the later schedules read of them.  The step classes are
recomputed here from the path; describe() tags every op, so each op's step range is checked
against them.

Networks: the 12-qubit cut brick wall with two sliced legs (closed qubits 0-3 left of the cut,
8-11 right of it), with and without deferred tails, and an unsliced 10-qubit line sweep in which
only q4's projector is volatile, so that the frozen / live boundary falls inside one sweep chain.
A sliced plan holds two programs (the slice lanes and the whole program, which has no sliced
input): frozen steps, left projectors volatile -- 31 of 52 in both programs with deferred tails;
without them 33 of 52 in the whole program and 32 in the sliced one (one step of the right half
reads a sliced leg); 34 of 55 for the 10-qubit sweep; 18 of 52 when all eight projectors are."""
import re

import pytest
import torch

from tneq_qc_amd.circuits import BrickWall, amplitude_task
from tneq_qc_amd.expression import HipContractExpression

KEYS = ["n_slices", "arena_bytes", "table_bytes", "flops", "bytes_moved", "flops_once", "flops_slice", "bytes_once",
        "bytes_slice", "n_ops_once", "n_kernels", "n_presplit", "lanes", "n_gemm", "n_apply", "n_permute", "n_sweep",
        "n_sweep_gates", "n_sweep2", "n_launch_once", "n_chain_launches", "n_coop_ops", "n_launch_slice",
        "planes_gemm", "planes_bytes", "n_s2_block_gate_work", "n_s2_prog_gate_work", "out_numel", "fold_slices",
        "whole_bytes_moved", "whole_flops", "whole_arena_bytes", "whole_n_launch", "whole_n_s2_block_gate_work"]
FROZEN_KEYS = ["n_ops_frozen", "n_launch_frozen", "bytes_frozen", "flops_frozen", "frozen_kept_bytes",
               "frozen_valid", "frozen_runs"]


def _task(name):
    if name == "defer":
        return amplitude_task(BrickWall(12, 6, 2), list(range(4, 8)), cut=6, n_slice=2, defer=(2, 2))
    if name == "plain":
        return amplitude_task(BrickWall(12, 6, 2), list(range(4, 8)), cut=6, n_slice=2)
    return amplitude_task(BrickWall(10, 8, 0), [])


def _proj(t):
    return {q: i for i, (kind, q) in enumerate(t.kinds) if kind == "proj"}


def _volatile(name, t, which):
    pr = _proj(t)
    if which == "all":
        return sorted(pr.values())
    return [pr[4]] if name == "line" else [pr[q] for q in range(4)]


def _plan(t, volatile="undeclared", dtype=torch.complex64):
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced)
    p = e.plan(dtype).clone()
    if volatile != "undeclared":
        p.set_volatile(volatile)
    return p


def _step_classes(t, volatile, sliced):
    """Per path step: frozen = no volatile and no sliced input in its subtree (the final step never)."""
    terms = t.eq.split("->")[0].split(",")
    live = [i in volatile or bool(set(s) & set(sliced)) for i, s in enumerate(terms)]
    for s, (x, y) in enumerate(t.path):
        live.append(live[x] or live[y] or s == len(t.path) - 1)
    return [not v for v in live[len(terms):]]


def _ops(describe):
    """(tag, first step, last step) of every op line of describe()."""
    out = []
    for line in describe.splitlines():
        m = re.match(r"\[(frozen|once|slice)\]\s+b\d (?:compose )?step (\d+)(?:\.\.(\d+))?", line)
        if m:
            a = int(m.group(2))
            out.append((m.group(1), a, int(m.group(3) or a)))
        else:
            assert line.startswith("#"), line
    return out


@pytest.mark.parametrize("name", ["defer", "plain", "line"])
def test_nothing_declared_is_the_parents_plan(name):
    t = _task(name)
    p0 = _plan(t)
    p1 = _plan(t, list(range(len(t.shapes))))    # every input, explicitly
    p2 = _plan(t, [0])
    p2.set_volatile(None)                        # ... and the default restored
    for p in (p1, p2):
        for k in KEYS:
            assert p.query(k) == p0.query(k), k
        assert p.describe() == p0.describe()
    for k in FROZEN_KEYS:
        assert p0.query(k) == 0 and p1.query(k) == 0, k
    assert "[frozen]" not in p0.describe() and "# frozen" not in p0.describe()
    with pytest.raises(ValueError):
        p0.set_volatile([len(t.shapes)])


@pytest.mark.parametrize("name,which,n_whole,n_sliced", [
    ("defer", "left", 31, 31), ("plain", "left", 33, 32), ("line", "left", 34, None),
    ("defer", "all", 18, 18), ("plain", "all", 18, 18)])
def test_frozen_ops_cover_frozen_steps_only(name, which, n_whole, n_sliced):
    t = _task(name)
    vol = _volatile(name, t, which)
    p, p0 = _plan(t, vol), _plan(t)
    n_steps = len(t.path)
    assert n_steps == (55 if name == "line" else 52)
    whole = _step_classes(t, vol, [])
    assert sum(whole) == n_whole
    fr = _step_classes(t, vol, t.sliced)
    assert sum(fr) == (n_whole if n_sliced is None else n_sliced)
    # every op: frozen steps only, or none (the program describe() shows has the sliced modes)
    ops = _ops(p.describe())
    covered = set()
    for tag, a, b in ops:
        assert all(fr[a:b + 1]) if tag == "frozen" else not any(fr[a:b + 1]), (tag, a, b)
        covered.update(range(a, b + 1))
    assert covered == set(range(n_steps))
    n_frozen = sum(tag == "frozen" for tag, _, _ in ops)
    assert p.query("n_ops_frozen") == n_frozen > 0
    assert p.query("n_ops_frozen") + p.query("n_ops_once") == p0.query("n_ops_once") + p.query("n_kernels") - p0.query("n_kernels")
    # the costs move between the tiers, a split chain adds its hand-over
    assert p.query("bytes_frozen") > 0 and p.query("flops_frozen") > 0
    assert p.query("bytes_once") < p0.query("bytes_once")
    assert p.query("bytes_slice") == p0.query("bytes_slice")
    assert p.query("n_launch_slice") == p0.query("n_launch_slice")
    # a frozen result that a live step reads is kept: every path step that reads a frozen result
    # of another step and is not frozen itself
    n_in = len(t.shapes)
    kept = {z for s, (x, y) in enumerate(t.path) if not fr[s] for z in (x, y) if z >= n_in and fr[z - n_in]}
    assert kept and p.query("frozen_kept_bytes") > 0
    last = {b for tag, _, b in ops if tag == "frozen"}
    assert {z - n_in for z in kept} <= last             # each is the result of a frozen op
    assert p.query("frozen_kept_bytes") >= len(kept) * 8   # complex64: 8 bytes per element at least
    assert p.query("frozen_valid") == 0 and p.query("frozen_runs") == 0
    # the schedule lists the frozen launches first
    sched = [l.split()[1] for l in p.describe().splitlines() if l.startswith(("# frozen", "# once", "# slice"))]
    assert sched == sorted(sched, key=["frozen", "once", "slice"].index)
    assert sched.count("frozen") >= p.query("n_launch_frozen") > 0    # (chain launches merge entries)
    if t.sliced:
        assert p.query("whole_n_ops_frozen") > 0 and p.query("whole_frozen_kept_bytes") > 0
        assert p.query("fold_slices") == p0.query("fold_slices") == 1


@pytest.mark.parametrize("name,which", [("defer", "left"), ("plain", "left"), ("line", "left"),
                                        ("defer", "all"), ("plain", "all")])
def test_launches_of_a_full_run(name, which):
    """A full run launches no more than the undeclared plan plus the chains that had to split:
    n_launch_frozen (what a full run launches on top of a live-only one) + n_launch_once <= the
    undeclared plan's n_launch_once + the split chains.  A full run zips the frozen and the hoisted
    schedule: a hoisted level that no frozen entry still to come conflicts with shares the launch
    of a frozen level, as the two halves' levels do in the undeclared plan (frozen + once |
    undeclared once + split chains: defer/left 1 + 3 | 3 + 1, plain/left 1 + 2 | 2 + 1, line/left
    2 + 3 | 4 + 1, defer/all 1 + 3 | 3 + 2, plain/all 1 + 2 | 2 + 2)."""
    t = _task(name)
    p, p0 = _plan(t, _volatile(name, t, which)), _plan(t)
    split = p.query("n_kernels") - p0.query("n_kernels")
    got = p.query("n_launch_frozen") + p.query("n_launch_once")
    print(f"{name}/{which}: {p.query('n_launch_frozen')} + {p.query('n_launch_once')} | "
          f"{p0.query('n_launch_once')} + {split}")
    assert got <= p0.query("n_launch_once") + split


def test_chain_splits_at_the_tier_boundary():
    """The 10-qubit sweep with only q4's projector volatile: a sweep chain of the undeclared plan
    that holds frozen steps followed by live ones becomes a frozen op and a live one."""
    t = _task("line")
    vol = _volatile("line", t, "left")
    fr = _step_classes(t, vol, [])
    mixed = [(a, b) for _, a, b in _ops(_plan(t).describe()) if any(fr[a:b + 1]) and not all(fr[a:b + 1])]
    assert mixed
    ops = _ops(_plan(t, vol).describe())
    for a, b in mixed:
        cut = a + fr[a:b + 1].index(False)
        assert all(fr[a:cut]) and not any(fr[cut:b + 1])
        assert ("frozen", a, cut - 1) in ops
        assert any(tag == "once" and x == cut for tag, x, _ in ops)


def test_clone_and_recompile_keep_the_classes():
    t = _task("defer")
    vol = _volatile("defer", t, "left")
    p = _plan(t, vol)
    want = [tag for tag, _, _ in _ops(p.describe())]
    frozen = {k: p.query(k) for k in FROZEN_KEYS + ["whole_n_ops_frozen", "whole_frozen_kept_bytes"]}
    c = p.clone()
    assert c.describe() == p.describe()
    for k, v in frozen.items():
        assert c.query(k) == v, k
    for key, val in (("min_chunks", 64), ("group_hint", 2)):
        c.set(key, val)
        assert c.query(key) == val
        assert [tag for tag, _, _ in _ops(c.describe())] == want
        assert c.query("n_ops_frozen") == frozen["n_ops_frozen"]
        assert c.query("whole_n_ops_frozen") == frozen["whole_n_ops_frozen"]
        assert c.clone().query("n_ops_frozen") == frozen["n_ops_frozen"]
    # declaring again after the other options keeps those
    c.set_volatile(_volatile("defer", t, "all"))
    assert c.query("min_chunks") == 64 and c.query("group_hint") == 2
    assert 0 < c.query("n_ops_frozen") < frozen["n_ops_frozen"]
