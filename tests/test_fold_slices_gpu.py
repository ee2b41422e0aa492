"""A call over every slice runs the plan's whole program (tq_plan.h Plan::whole; plan_run in
tq_plan_run.cpp) on the GPU: four small cut / sliced brick-wall networks whose per-slice parts
hold the op kinds a fold replaces (APPLY + PERMUTE + SWEEP2, a SWEEP2-only tail on 8 lanes, a
table SWEEP) and one whose per-slice part holds a GEMM, which must keep the slice lanes.  Per
network and dtype: the folded result against the slice lanes' (fold_slices 0) and both against
the exact oracle; a full-range call with accumulate; a partial range plus its complement after a
folded call on the same plan (both programs alive); graph and fold counters; a clone; which
program's arena is on the device.  A lockstep group of three plans, all folding and one not.
Then one headline block (C4, four in flight) folded against
not folded.

Bounds (relative to max |reference|): 1e-5 against the exact oracle for complex64 and 1e-12 for
complex128 (the parity tests' bounds), 2e-5 between two complex64 results (the project's
variant-vs-variant bound); between two complex128 results 2e-12, the sum of their two oracle
bounds."""
import numpy as np
import pytest
import torch

from oracle.contract_ref import contract_sliced
from tneq_qc_amd.circuits import BrickWall, amplitude_task, config_task
from tneq_qc_amd.expression import HipContractExpression, run_group
from tneq_qc_amd.sampling import BlockPipeline

pytestmark = pytest.mark.gpu

# (qubits, depth, open qubits [a, b), cut, sliced legs, defer, folds)
NETS = [
    (14, 8, (4, 10), 7, 2, None, 1),       # per-slice APPLY + PERMUTE + SWEEP2
    (14, 8, (4, 10), 7, 3, (6, 4), 1),     # SWEEP2-only tail, 8 lanes
    (16, 10, (4, 12), 8, 3, (8, 6), 1),    # per-slice table SWEEP
    (16, 10, (4, 12), 8, 3, "auto", 0),    # per-slice GEMM: not folded
]
REF_TOL = {torch.complex64: 1e-5, torch.complex128: 1e-12}
VAR_TOL = {torch.complex64: 2e-5, torch.complex128: 2e-12}


@pytest.fixture(scope="module")
def cases():
    """Per network: the task and its exact sliced sum (computed once)."""
    out = []
    for n, d, (a, b), cut, ns, defer, folds in NETS:
        t = amplitude_task(BrickWall(n, d, 1), list(range(a, b)), cut=cut, n_slice=ns, defer=defer)
        out.append((t, contract_sliced(t.eq, t.operands, t.sliced, t.path), folds))
    return out


def _expr(t, dtype, fold):
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced)
    p = e.plan(dtype, None, 0)
    p.set("fold_slices", fold)
    return e, p


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_fold_against_lanes_and_oracle(cases, k, dtype):
    t, ref, folds = cases[k]
    scale = np.abs(ref).max()
    ts = [torch.from_numpy(o).to("cuda:0", dtype) for o in t.operands]
    e, p = _expr(t, dtype, 1)
    e0, p0 = _expr(t, dtype, 0)
    n = e.n_slices
    assert n == 2 ** NETS[k][4]
    assert p.query("fold_slices") == folds and p0.query("fold_slices") == 0
    has_gemm = any("[slice]" in l and " GEMM " in l for l in p.describe().splitlines())
    assert has_gemm == (not folds)

    def err(x, y=ref):
        return float(np.abs(x.cpu().numpy() - y).max() / scale)

    # the full range, replayed: one graph, every call counted
    out = torch.empty(e.out_shape, dtype=dtype, device="cuda:0")
    for _ in range(3):
        e(*ts, out=out)
    assert p.query("graph_builds") == 1 and p.query("graph_launches") == 3
    assert p.query("folded_executes") == (3 if folds else 0)
    out0 = e0(*ts)
    assert p0.query("folded_executes") == 0
    d = err(out, out0.cpu().numpy())
    print(f"net {k} {dtype}: folded {err(out):.2e} lanes {err(out0):.2e} folded-lanes {d:.2e}")
    assert err(out) <= REF_TOL[dtype] and err(out0) <= REF_TOL[dtype]
    assert d <= VAR_TOL[dtype]
    # only the program that ran holds an arena
    if folds:
        assert p.query("resident_arena_bytes") == 0
        assert p.query("whole_resident_arena_bytes") == p.query("whole_arena_bytes") > 0
    else:
        assert p.query("resident_arena_bytes") == p.query("arena_bytes") > 0
        assert p.query("whole_resident_arena_bytes") == 0
    assert p0.query("resident_arena_bytes") == p0.query("arena_bytes") and p0.query("whole_resident_arena_bytes") == 0

    # accumulate on the full range: out + sum, folded as well (another graph key)
    acc = out.clone()
    e(*ts, out=acc, accumulate=True)
    assert p.query("graph_builds") == 2 and p.query("folded_executes") == (4 if folds else 0)
    assert float(np.abs(acc.cpu().numpy() - 2 * out.cpu().numpy()).max() / scale) <= VAR_TOL[dtype]

    # a partial range and its complement on the same plan: the slice lanes, beside the whole program
    part = torch.empty_like(out)
    for _ in range(2):
        e(*ts, out=part, slice_range=(1, n, 2))
        e(*ts, out=part, slice_range=(0, n, 2), accumulate=True)
    assert p.query("graph_builds") == 4 and p.query("graph_launches") == 8
    assert p.query("folded_executes") == (4 if folds else 0)
    assert p.query("resident_arena_bytes") == p.query("arena_bytes")
    assert err(part) <= REF_TOL[dtype]
    assert err(part, out.cpu().numpy()) <= VAR_TOL[dtype]
    # ... and the folded call still replays its graph
    before = out.cpu().numpy()
    e(*ts, out=out)
    assert p.query("graph_builds") == 4
    assert err(out, before) <= VAR_TOL[dtype]

    # a clone: its own device state, the same result
    c = p.clone()
    assert c.query("fold_slices") == folds and c.query("folded_executes") == 0
    outc = torch.empty_like(out)
    c.execute([x.data_ptr() for x in ts], outc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.query("folded_executes") == folds
    assert err(outc, before) <= VAR_TOL[dtype]
    c.release_now()


def test_switch_is_fixed_at_the_first_execute(cases):
    t, _, _ = cases[1]
    e, p = _expr(t, torch.complex64, 1)
    e(*[torch.from_numpy(o).to("cuda:0", torch.complex64) for o in t.operands])
    with pytest.raises(ValueError):
        p.set("fold_slices", 0)
    assert p.query("fold_slices") == 1


def test_profile_covers_the_folded_call(cases):
    """Per-kind event timing (what bench.py --full reads) runs the call eagerly and records the
    program that ran: a folded call's records are the whole program's launches and flops."""
    t, ref, _ = cases[2]
    ts = [torch.from_numpy(o).to("cuda:0", torch.complex64) for o in t.operands]
    for fold in (1, 0):
        e, p = _expr(t, torch.complex64, fold)
        p.profile(-1)
        out = e(*ts)
        torch.cuda.synchronize()
        rd = p.profile_read(-1)
        print(f"fold {fold}: {rd}")
        assert p.query("graph_builds") == 0 and p.query("folded_executes") == fold
        if fold:
            assert rd["launches"] == p.query("whole_n_launch")
            assert abs(rd["flops"] - p.query("whole_flops")) <= 1
        else:
            assert rd["launches"] >= p.query("n_launch_once") + p.query("n_launch_slice")
            assert abs(rd["flops"] - p.query("flops")) <= 1
        assert float(np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max()) <= 1e-5
        p.profile(None)
        assert p.profile_read(-1)["launches"] == 0


@pytest.mark.parametrize("fold", [1, 0])
def test_group_folds_when_every_member_does(cases, fold):
    """Three plans of one network in lockstep (tq_plan_execute_group), each on its own scaled
    first operand: the members' whole programs when all fold, the slice lanes when one does not."""
    t, ref, _ = cases[2]
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced)
    base = [torch.from_numpy(o).to("cuda:0", torch.complex64) for o in t.operands]
    bound = []
    for m in range(3):
        ops = list(base)
        ops[0] = base[0] * (m + 1)
        bound.append(e.bind(*ops, private_plan=True))
    bound[1].plan.set("fold_slices", fold)
    outs = [b.new_out() for b in bound]
    for _ in range(2):
        run_group(bound, outs)
    torch.cuda.synchronize()
    lead = bound[0].plan
    assert lead.query("graph_builds") == 1 and lead.query("graph_launches") == 2
    for m, b in enumerate(bound):
        assert b.plan.query("folded_executes") == 2 * fold
        assert b.plan.query("resident_arena_bytes") == (0 if fold else b.plan.query("arena_bytes"))
        err = float(np.abs(outs[m].cpu().numpy() - (m + 1) * ref).max() / ((m + 1) * np.abs(ref).max()))
        assert err <= 1e-5, (m, err)
    # a partial range on the same group: the lanes, beside the whole programs
    n = e.n_slices
    run_group(bound, outs, slice_range=(0, n, 2))
    part = [o.clone() for o in outs]
    run_group(bound, outs, slice_range=(1, n, 2))
    torch.cuda.synchronize()
    for m in range(3):
        tot = (part[m] + outs[m]).cpu().numpy()
        assert float(np.abs(tot - (m + 1) * ref).max() / ((m + 1) * np.abs(ref).max())) <= 1e-5
    assert lead.query("graph_builds") == 3
    for b in bound:
        b.plan.release_now()


@pytest.mark.timeout(600)
def test_headline_block_folded_vs_lanes():
    """One C4 block through BlockPipeline(inflight=4) -- the min_chunks-64 plan -- folded and on
    the slice lanes; a pipeline that only ran full ranges never took the sliced program's arena."""
    task = config_task("C4")
    res = {}
    for on in (1, 0):
        pipe = BlockPipeline(task, [3], inflight=4)
        for s in range(pipe.inflight):
            pipe.plan(s).set("fold_slices", on)
        pl = pipe.plan(0)
        assert pl.query("min_chunks") == 64 and pl.query("lanes") == 8
        assert pl.query("fold_slices") == on
        res[on] = pipe.run(1)[0].numpy()
        assert pl.query("folded_executes") == on
        if on:
            assert all(pipe.plan(s).query("resident_arena_bytes") == 0 for s in range(pipe.inflight))
            assert pl.query("whole_resident_arena_bytes") == pl.query("whole_arena_bytes")
        else:
            assert pl.query("resident_arena_bytes") == pl.query("arena_bytes")
            assert pl.query("whole_resident_arena_bytes") == 0
        pipe.close()
    ref = np.abs(res[0]).max()
    assert ref > 0
    d = np.abs(res[1] - res[0]).max() / ref
    print(f"C4 block, folded vs slice lanes: {d:.2e}")
    assert d <= 2e-5
