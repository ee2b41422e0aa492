"""Frozen results on the GPU (tq_plan.h Plan::n_sched_frozen; frozen_begin / frozen_ran in
tq_plan_run.cpp): a plan that was told which operands are volatile contracts the subtrees that
hold none of them in its first execute call only.  Two 12-qubit cut brick-wall networks (closed
qubits 0-3 left of the cut, 8-11 right of it; two sliced legs, so a call over every slice runs the
plan's whole program and a partial range its slice lanes), complex64 and complex128.

Bounds, relative to the largest |amplitude| of the reference: 1e-5 (complex64) / 1e-12
(complex128) against the exact oracle -- the suite's parity bounds; 2e-5 between a declared and an
undeclared plan's complex64 results (the project's bound for regrouped chains: a chain split at
the frozen / live boundary rounds differently), 2e-12 for complex128 (the sum of the two oracle
bounds).  The first (full) and a later (live-only) execute of one plan run the same live kernels
on the same frozen results: bit-equal."""
import numpy as np
import pytest
import torch

from oracle.contract_ref import contract_sliced
from tneq_qc_amd.circuits import BrickWall, amplitude_task, with_batch
from tneq_qc_amd.expression import BoundOperands, HipContractExpression
from tneq_qc_amd.sampling import BlockPipeline

pytestmark = pytest.mark.gpu

REF_TOL = {torch.complex64: 1e-5, torch.complex128: 1e-12}
VAR_TOL = {torch.complex64: 2e-5, torch.complex128: 2e-12}
DTYPES = pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128], ids=["c64", "c128"])
LEFT = list(range(16))              # with_batch indices that flip left-half projectors only
BOTH = [0, 1, 17, 40, 130, 255]     # ... and right-half ones (index bits 4-7)


def _task(k):
    kw = dict(defer=(2, 2)) if k == 0 else {}
    return amplitude_task(BrickWall(12, 6, 2), list(range(4, 8)), cut=6, n_slice=2, **kw)


@pytest.fixture(scope="module")
def nets():
    """Per network: the task and the exact amplitudes of every block the tests use (once)."""
    out = []
    for k in range(2):
        t = _task(k)
        ref = {}
        for b in sorted(set(LEFT + BOTH)):
            tb = with_batch(t, b)
            ref[b] = contract_sliced(tb.eq, tb.operands, tb.sliced, tb.path)
        out.append((t, ref))
    return out


def _err(x, ref):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def _frozen(plan, key):
    """A frozen-part query summed over the plan's two programs (slice lanes + whole program)."""
    return plan.query(key) + max(0, plan.query("whole_" + key))


def _proj(t):
    return {q: i for i, (kind, q) in enumerate(t.kinds) if kind == "proj"}


def _bound(t, dtype, volatile, dev, block=0):
    """One private plan bound to its own copies of block `block`'s operands."""
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced)
    ts = [torch.from_numpy(o).to(dev, dtype) for o in with_batch(t, block).operands]
    return e, e.bind(*ts, private_plan=True, volatile=volatile)


def _set_block(t, bound, block):
    """Write block `block`'s projector vectors into the bound projector operands, in place."""
    tb = with_batch(t, block)
    for i in _proj(t).values():
        bound.tensors[i].copy_(torch.from_numpy(tb.operands[i]).to(bound.tensors[i]))


@DTYPES
@pytest.mark.parametrize("inflight,group", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("k", [0, 1])
def test_blocks_match_oracle_and_undeclared_pipeline(dev, nets, k, inflight, group, dtype):
    t, ref = nets[k]
    pipe = BlockPipeline(t, LEFT, inflight=inflight, group=group, device=dev, dtype=dtype)
    plain = BlockPipeline(t, LEFT, inflight=inflight, group=group, device=dev, dtype=dtype, freeze=False)
    pr = _proj(t)
    assert sorted(pipe.volatile) == sorted(pr[q] for q in range(4)) and plain.volatile is None
    assert _frozen(pipe.plan(), "n_ops_frozen") > 0 and _frozen(plain.plan(), "n_ops_frozen") == 0
    got, got0 = pipe.run(), plain.run()
    worst = [0.0, 0.0, 0.0]
    for b, g, g0 in zip(LEFT, got, got0):
        e = (_err(g, ref[b]), _err(g0, ref[b]), _err(g, g0.numpy()))
        worst = [max(w, x) for w, x in zip(worst, e)]
        assert e[0] <= REF_TOL[dtype] and e[1] <= REF_TOL[dtype], (b, e)
        assert e[2] <= VAR_TOL[dtype], (b, e)
    print(f"net {k} {dtype} {inflight}x{group}: declared {worst[0]:.2e} undeclared {worst[1]:.2e} "
          f"between {worst[2]:.2e}")
    for s in range(inflight):
        for m in range(group):
            assert _frozen(pipe.plan(s, m), "frozen_runs") == 1, (s, m)
            assert _frozen(plain.plan(s, m), "frozen_runs") == 0
    pipe.close()
    plain.close()


@DTYPES
@pytest.mark.parametrize("k", [0, 1])
def test_first_and_later_executes_are_bit_equal(dev, nets, k, dtype):
    t, ref = nets[k]
    pr = _proj(t)
    e, b = _bound(t, dtype, [pr[q] for q in range(4)], dev, block=3)
    first, later = b.new_out(), b.new_out()
    b.run(first)
    assert b.plan.query("whole_frozen_valid") == 1
    b.run(later)
    b.run(later)
    torch.cuda.synchronize()
    assert _frozen(b.plan, "frozen_runs") == 1
    assert torch.equal(first, later)
    assert _err(first, ref[3]) <= REF_TOL[dtype]
    b.plan.release_now()


@DTYPES
def test_right_half_bits_declare_more_and_freeze_less(dev, nets, dtype):
    t, ref = nets[0]
    left = BlockPipeline(t, LEFT, inflight=1, device=dev, dtype=dtype)
    pipe = BlockPipeline(t, BOTH, inflight=2, group=2, device=dev, dtype=dtype)
    pr = _proj(t)
    assert sorted(pipe.volatile) == sorted(pr.values())   # index bits 0-7: all eight closed qubits
    assert 0 < _frozen(pipe.plan(), "n_ops_frozen") < _frozen(left.plan(), "n_ops_frozen")
    for b, g in zip(BOTH, pipe.run()):
        assert _err(g, ref[b]) <= REF_TOL[dtype], b
    for s in range(2):
        for m in range(2):
            assert _frozen(pipe.plan(s, m), "frozen_runs") == 1
    pipe.close()
    left.close()


@DTYPES
def test_invalidate_after_writing_a_steady_operand(dev, nets, dtype):
    """The switch works: a core of the frozen half overwritten in place, invalidate(), and the
    next block is the new core's (frozen results computed a second time)."""
    t, ref = nets[0]
    pipe = BlockPipeline(t, LEFT, inflight=1, device=dev, dtype=dtype)
    first = pipe.run(2)
    assert _err(first[1], ref[1]) <= REF_TOL[dtype]
    bound = pipe.slots[0].bound[0]
    # the last core: right of the cut, so inside the frozen subtree
    i = max(j for j, (kind, _) in enumerate(t.kinds) if kind == "core")
    rng = np.random.default_rng(5)
    new = rng.standard_normal(t.shapes[i]) + 1j * rng.standard_normal(t.shapes[i])
    bound.tensors[i].copy_(torch.from_numpy(new).to(bound.tensors[i]))
    bound.invalidate()
    assert _frozen(bound.plan, "frozen_valid") == 0
    got = pipe.run(1)[0]          # block 2
    tb = with_batch(t, 2)
    ops = list(tb.operands)
    ops[i] = new
    want = contract_sliced(tb.eq, ops, tb.sliced, tb.path)
    assert _err(got, want) <= REF_TOL[dtype]
    assert _err(got, ref[2]) > 1e-3          # (the new core does change the block)
    assert _frozen(bound.plan, "frozen_runs") == 2
    pipe.close()


@DTYPES
def test_another_pointer_for_a_steady_operand_recomputes(dev, nets, dtype):
    t, ref = nets[1]
    pr = _proj(t)
    e, b = _bound(t, dtype, [pr[q] for q in range(4)], dev, block=6)
    out = b.new_out()
    b.run(out)
    b.run(out)
    assert _frozen(b.plan, "frozen_runs") == 1 and _err(out, ref[6]) <= REF_TOL[dtype]
    i = max(j for j, (kind, _) in enumerate(t.kinds) if kind == "core")
    rng = np.random.default_rng(6)
    new = rng.standard_normal(t.shapes[i]) + 1j * rng.standard_normal(t.shapes[i])
    ts = list(b.tensors)
    ts[i] = torch.from_numpy(new).to(dev, dtype)
    b2 = BoundOperands(e, b.plan, b.plan.pointer_array([x.data_ptr() for x in ts]), tuple(ts), dev, dtype)
    b2.run(out)
    assert _frozen(b.plan, "frozen_runs") == 2
    ops = list(with_batch(t, 6).operands)
    ops[i] = new
    assert _err(out, contract_sliced(t.eq, ops, t.sliced, t.path)) <= REF_TOL[dtype]
    b.run(out)                   # back to the first tensor: its pointer differs again
    assert _frozen(b.plan, "frozen_runs") == 3 and _err(out, ref[6]) <= REF_TOL[dtype]
    b.plan.release_now()


@DTYPES
@pytest.mark.parametrize("k", [0, 1])
def test_slice_range_runs_the_lanes_programs_frozen_part(dev, nets, k, dtype):
    t, ref = nets[k]
    pr = _proj(t)
    e, b = _bound(t, dtype, [pr[q] for q in range(4)], dev, block=9)
    e0, b0 = _bound(t, dtype, None, dev, block=9)
    assert b.plan.query("n_ops_frozen") > 0 and b0.plan.query("n_ops_frozen") == 0
    part, part0, rest = b.new_out(), b0.new_out(), b.new_out()
    for _ in range(2):
        b.run(part, slice_range=(0, 1, 1))
    b0.run(part0, slice_range=(0, 1, 1))
    n = e.n_slices
    b.run(rest, slice_range=(1, n, 1))
    torch.cuda.synchronize()
    assert b.plan.query("frozen_runs") == 1 and b.plan.query("whole_frozen_runs") == 0
    assert b.plan.query("folded_executes") == 0
    scale = np.abs(ref[9]).max()
    assert float((part - part0).abs().max()) / scale <= VAR_TOL[dtype]
    assert _err(part + rest, ref[9]) <= REF_TOL[dtype]
    b.plan.release_now()
    b0.plan.release_now()


@DTYPES
def test_live_only_call_on_another_stream(dev, nets, dtype):
    """The second stream's call follows the first with no host synchronization between: its live
    part waits for the event behind the frozen schedule."""
    t, ref = nets[0]
    pr = _proj(t)
    e, b = _bound(t, dtype, [pr[q] for q in range(4)], dev, block=11)
    o1, o2 = b.new_out(), b.new_out()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    b.run(o1, s1)
    b.run(o2, s2)
    torch.cuda.synchronize()
    assert _frozen(b.plan, "frozen_runs") == 1
    assert _err(o1, ref[11]) <= REF_TOL[dtype] and _err(o2, ref[11]) <= REF_TOL[dtype]
    assert torch.equal(o1, o2)
    b.plan.release_now()


@DTYPES
def test_callers_capture_runs_everything_and_keeps_the_state(dev, nets, dtype):
    t, ref = nets[0]
    pr = _proj(t)
    e, b = _bound(t, dtype, [pr[q] for q in range(4)], dev, block=0)
    out, cap = b.new_out(), b.new_out()
    b.run(out)                    # (also takes the plan's device memory, outside the capture)
    torch.cuda.synchronize()
    valid, runs = _frozen(b.plan, "frozen_valid"), _frozen(b.plan, "frozen_runs")
    assert (valid, runs) == (1, 1)
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.run(cap, torch.cuda.current_stream(dev))
    assert (_frozen(b.plan, "frozen_valid"), _frozen(b.plan, "frozen_runs")) == (valid, runs)
    _set_block(t, b, 13)          # other projectors, then the replay
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert _err(cap, ref[13]) <= REF_TOL[dtype]
    b.run(out)                    # the plan's own (live-only) call still agrees
    torch.cuda.synchronize()
    assert _frozen(b.plan, "frozen_runs") == runs and _err(out, ref[13]) <= REF_TOL[dtype]
    del g
    b.plan.release_now()
