"""BlockPipeline (sampling.py): many amplitude blocks of one network, several groups in flight
and several blocks per lockstep group (blocks as lanes: tq_plan_execute_group).  Every block
equals the oracle's contraction of that block (circuits.with_batch: other fixed bits); grouped
and pipelined blocks equal one-at-a-time runs, partial groups included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("inflight,group", [(2, 1), (1, 3), (2, 2)])
def test_blocks_match_the_oracle(dev, inflight, group):
    from oracle.contract_ref import contract_sliced
    from tneq_qc_amd.circuits import BrickWall, amplitude_task, with_batch
    from tneq_qc_amd.sampling import BlockPipeline
    t = amplitude_task(BrickWall(12, 6, 2), list(range(4, 8)), cut=6, n_slice=2, defer=(2, 2))
    blocks = [0, 3, 5, 9, 130]   # 5 blocks: the last group is partial
    pipe = BlockPipeline(t, blocks, inflight=inflight, group=group, device=dev)
    got = pipe.run()
    assert len(got) == len(blocks)
    for b, g in zip(blocks, got):
        tb = with_batch(t, b)
        ref = contract_sliced(tb.eq, tb.operands, tb.sliced, tb.path)
        assert np.abs(g.numpy() - ref).max() <= 1e-5 * np.abs(ref).max(), b


@pytest.mark.parametrize("inflight,group", [(2, 1), (2, 4)])
def test_pipelined_c4_blocks_equal_single_runs(dev, inflight, group):
    """The benchmarked C4 pipeline (bench.py: `--inflight` x `--group`) against single-block
    executes of the plain expression: 2 x group blocks (every slot once), then one block more
    (a partial group through flush())."""
    import torch
    from tneq_qc_amd.circuits import config_task, with_batch
    from tneq_qc_amd.expression import HipContractExpression
    from tneq_qc_amd.sampling import BlockPipeline
    t = config_task("C4")
    n = inflight * group
    blocks = list(range(n + 1))
    pipe = BlockPipeline(t, blocks, inflight=inflight, group=group, device=dev)
    outs = [pipe.step() for _ in range(n)]
    pipe.wait()
    torch.cuda.current_stream().synchronize()
    got = [o.cpu().numpy().copy() for o in outs]
    last = pipe.step()          # block n: member 0 of slot 0 again, launched by synchronize()
    pipe.synchronize()
    got.append(last.cpu().numpy().copy())
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced)
    for b, g in zip(blocks, got):
        tb = with_batch(t, b)
        ops = [torch.from_numpy(x).to(dev, torch.complex64) for x in tb.operands]
        ref = e(*ops).cpu().numpy()
        assert np.abs(g - ref).max() <= 1e-5 * np.abs(ref).max(), b
    assert not np.allclose(got[0], got[1])   # other blocks, other amplitudes


def test_replayed_c4_blocks_one_at_a_time(dev):
    """Graph replays on an idle GPU: one C4 block at a time with a synchronize after each (the plan's
    graph is captured on block 0 and replayed for the rest).  The operand max words of the f16-split
    boundary GEMM were zeroed by a captured memset node that a replay did not keep in order with
    the words' producers: blocks 5-7 came back all zero and 8-11 all NaN.  Every block is finite
    and non-zero, and blocks 5 and 8 equal an eagerly launched plan's result (no graph)."""
    import torch
    from tneq_qc_amd.circuits import config_task, with_batch
    from tneq_qc_amd.expression import HipContractExpression
    from tneq_qc_amd.sampling import BlockPipeline
    t = config_task("C4")
    pipe = BlockPipeline(t, list(range(12)), inflight=1, device=dev)
    got = []
    for _ in range(12):
        o = pipe.step()
        pipe.synchronize()
        got.append(o.cpu().numpy().copy())
    for b, g in enumerate(got):
        assert np.isfinite(g).all() and np.abs(g).max() > 0, b
    # the reference launches eagerly: its plan captures and replays no graph
    e = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced)
    eager = e.plan(torch.complex64, None, dev.index)
    eager.set("graph", 0)
    for b in (5, 8):
        tb = with_batch(t, b)
        ref = e(*[torch.from_numpy(x).to(dev, torch.complex64) for x in tb.operands]).cpu().numpy()
        assert np.abs(got[b] - ref).max() <= 1e-5 * np.abs(ref).max(), b
    assert eager.query("graph_builds") == 0 and eager.query("graph_launches") == 0


def test_run_group_refuses_mismatched_members(dev):
    import torch
    from tneq_qc_amd.expression import HipContractExpression, run_group
    rng = np.random.default_rng(0)

    def ops(shapes):
        return [torch.tensor(rng.standard_normal(s) + 1j * rng.standard_normal(s), dtype=torch.complex64,
                             device=dev) for s in shapes]
    e1 = HipContractExpression("ab,bc->ac", (8, 16), (16, 4))
    e2 = HipContractExpression("ab,bc,cd->ad", (8, 16), (16, 4), (4, 2))
    b1 = e1.bind(*ops([(8, 16), (16, 4)]), private_plan=True)
    b2 = e2.bind(*ops([(8, 16), (16, 4), (4, 2)]), private_plan=True)
    with pytest.raises(ValueError):
        run_group([b1, b2], [b1.new_out(), b2.new_out()])
    # the same plan twice is refused (one arena cannot hold two blocks)
    with pytest.raises(ValueError):
        run_group([b1, b1], [b1.new_out(), b1.new_out()])
    # a matching pair runs and equals the single runs
    x, y = ops([(8, 16), (16, 4)]), ops([(8, 16), (16, 4)])
    m1, m2 = e1.bind(*x, private_plan=True), e1.bind(*y, private_plan=True)
    o1, o2 = m1.new_out(), m2.new_out()
    run_group([m1, m2], [o1, o2])
    torch.cuda.synchronize()
    for o, (a, b) in ((o1, x), (o2, y)):
        ref = (a @ b).cpu().numpy()
        assert np.abs(o.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_group_graph_is_cached_in_the_leader(dev):
    """A group execute is one hipGraph cached in its first plan under every member's buffers: the
    same call again replays it, other output buffers capture a new one, the other members hold no
    graph; the replay equals the eager group run bit for bit."""
    import torch
    from tneq_qc_amd.expression import HipContractExpression, run_group
    rng = np.random.default_rng(1)

    def ops(shapes):
        return [torch.tensor(rng.standard_normal(s) + 1j * rng.standard_normal(s), dtype=torch.complex64,
                             device=dev) for s in shapes]
    e1 = HipContractExpression("ab,bc->ac", (8, 16), (16, 4))
    m1 = e1.bind(*ops([(8, 16), (16, 4)]), private_plan=True)
    m2 = e1.bind(*ops([(8, 16), (16, 4)]), private_plan=True)
    o1, o2 = m1.new_out(), m2.new_out()
    b0, l0 = m1.plan.query("graph_builds"), m1.plan.query("graph_launches")
    run_group([m1, m2], [o1, o2])
    run_group([m1, m2], [o1, o2])
    assert m1.plan.query("graph_builds") == b0 + 1
    assert m1.plan.query("graph_launches") == l0 + 2
    assert m2.plan.query("graph_builds") == 0
    torch.cuda.synchronize()
    g1, g2 = o1.clone(), o2.clone()
    m1.plan.set("graph", 0)                          # the same group run, launched eagerly
    r1, r2 = m1.new_out(), m2.new_out()
    run_group([m1, m2], [r1, r2])
    m1.plan.set("graph", 1)
    torch.cuda.synchronize()
    assert m1.plan.query("graph_builds") == b0 + 1
    assert torch.equal(g1, r1) and torch.equal(g2, r2)
    run_group([m1, m2], [o2, o1])                    # swapped output buffers: another graph
    assert m1.plan.query("graph_builds") == b0 + 2
    assert m2.plan.query("graph_builds") == 0
    torch.cuda.synchronize()
    assert torch.equal(o2, r1) and torch.equal(o1, r2)
