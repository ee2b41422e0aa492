"""Pass programs of the sweep2 block passes (tq_sweep2.hip block_pass<T, B, ID>) on the GPU: for
every program of the set, the smallest network whose single sweep2 op contains that program's pass
-- a tensor of 2^6 (8-element blocks) or 2^13 elements (16-element blocks need a tile of >= 4096:
five gate legs x 128 columns) under two to four 1- / 2-qubit gates -- against the exact oracle,
against the interpreter (s2_programs 0) on the same inputs, and again at rank 15 (8 chunks over 8
workgroups, two chunk-loop forms).  Then one headline block (C4, four in flight: the min_chunks-64
plan) with programs on against the same block with programs off.

A program applies the same gates with the same per-gate arithmetic as the interpreter, so a
program whose steps keep the pass's order is bit-identical to it (measured: every such case
below); where the planner sorted commuting gates into the program's canonical order the products
are the same and the rounding may differ (measured: ~1.5e-7 of max|ref| on two of the three
permuted cases, 1.1e-6 on the C4 block).  The asserted bounds are the project's: 1e-5 of max|ref| for
complex64 against the exact oracle, 1e-12 for complex128, 2e-5 between two complex64 results."""
import numpy as np
import pytest
import torch

from oracle.contract_ref import contract as ref_contract
from tneq_qc_amd.circuits import config_task
from tneq_qc_amd.expression import HipContractExpression
from tneq_qc_amd.sampling import BlockPipeline

pytestmark = pytest.mark.gpu

# (program id, tensor rank, gates as leg tuples in order).  The planner gives leg l of the gate
# legs position (n - 1 - l) and a gate's outputs the positions it frees, so the legs below are
# what yields each block-local sequence (checked through n_s2_prog_passes_<id>).  Every network
# gets a last 1-qubit gate on its last leg, which leaves the chain (the output step).
NETS = [
    (1, 13, [(3, 4), (2, 3), (1, 2), (0,)]),            # 01 12 23
    (2, 13, [(1, 2), (3, 4), (0,)]),                    # 23 01 -> 01 23 (steps permuted)
    (2, 13, [(3, 4), (1, 2), (0,)]),                    # 01 23
    (3, 13, [(3, 2), (3, 0), (5, 1)]),                  # 12 23
    (4, 13, [(1, 4), (4, 3), (2, 3), (0,)]),            # 03 01 12
    (5, 13, [(0,), (2, 3), (1, 4)]),                    # 3 12 (2x2 mixed)
    (6, 13, [(1, 0), (2,), (3, 5)]),                    # 23 1 -> 1 23 (2x2 mixed, permuted)
    (7, 13, [(5, 1), (4, 2), (0, 1)]),                  # 03 12 -> 12 03
    (8, 6, [(1, 2), (0, 1)]),                           # 01 12 on 8-element blocks
    (8, 13, [(1, 2), (0, 1)]),
    (1, 15, [(3, 4), (2, 3), (1, 2), (0,)]),            # 8 chunks
    (3, 13, [(4, 5), (3, 4), (2, 3), (1, 2), (0, 1)]),  # two program passes in one op (1 and 3)
]
_SYMS = [chr(ord("a") + i) for i in range(26)] + [chr(ord("A") + i) for i in range(26)]


def _net(rank, gates, seed):
    rng = np.random.default_rng(seed)

    def rnd(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    cur, nxt = list(range(rank)), rank
    terms = ["".join(_SYMS[i] for i in cur)]
    ops = [rnd((2,) * rank)]
    for g in list(gates) + [(rank - 1,)]:
        ins, outs = [cur[l] for l in g], list(range(nxt, nxt + len(g)))
        nxt += len(g)
        terms.append("".join(_SYMS[i] for i in ins + outs))
        ops.append(rnd((2,) * (2 * len(g))) / 2.0 ** len(g))
        for l, o in zip(g, outs):
            cur[l] = o
    n = len(ops)
    eq = ",".join(terms) + "->" + "".join(_SYMS[i] for i in cur)
    return eq, ops, [(0, 1)] + [(n + k - 1, k + 1) for k in range(1, n - 1)]


@pytest.fixture(scope="module")
def cases():
    """Per network: equation, operands, path and the exact result (computed once)."""
    out = []
    for k, (pid, rank, gates) in enumerate(NETS):
        eq, ops, path = _net(rank, gates, 100 + k)
        out.append((pid, eq, ops, path, ref_contract(eq, *ops)))
    return out


def _run(eq, ops, path, dtype, programs):
    e = HipContractExpression(eq, *[o.shape for o in ops], optimize=path)
    p = e.plan(dtype, None, 0)
    p.set("min_chunks", 1)   # whole 128-column chunks: tiles of >= 4096 elements get 16-element blocks
    p.set("s2_programs", programs)
    got = e(*[torch.from_numpy(o).to("cuda:0", dtype) for o in ops]).cpu().numpy()
    return got, p


@pytest.mark.parametrize("k", range(len(NETS)))
def test_program_pass_c64(cases, k):
    pid, eq, ops, path, ref = cases[k]
    on, p = _run(eq, ops, path, torch.complex64, 1)
    assert p.query("n_sweep2") == 1
    assert p.query(f"n_s2_prog_passes_{pid}") > 0, p.describe()
    off, q = _run(eq, ops, path, torch.complex64, 0)
    assert q.query("n_s2_prog_gate_work") == 0
    scale = np.abs(ref).max()
    e_on, e_off = np.abs(on - ref).max() / scale, np.abs(off - ref).max() / scale
    d = np.abs(on - off).max() / scale
    print(f"program {pid}: on {e_on:.2e} off {e_off:.2e} on-off {d:.2e} bit-identical {np.array_equal(on, off)}")
    assert e_on <= 1e-5
    assert d <= 2e-5


@pytest.mark.parametrize("k", range(len(NETS)))
def test_program_pass_c128(cases, k):
    pid, eq, ops, path, ref = cases[k]
    on, p = _run(eq, ops, path, torch.complex128, 1)
    scale = np.abs(ref).max()
    err = np.abs(on - ref).max() / scale
    print(f"net {k} complex128: {err:.2e}, program work {p.query('n_s2_prog_gate_work')}")
    assert err <= 1e-12


@pytest.mark.timeout(600)
def test_headline_block_programs_on_vs_off():
    """One C4 block through BlockPipeline(inflight=4) -- the min_chunks-64 plan -- with programs
    on and off (the members' plans are switched before their first execute)."""
    task = config_task("C4")
    res = {}
    for on in (1, 0):
        pipe = BlockPipeline(task, [3], inflight=4)
        for s in range(pipe.inflight):
            pipe.plan(s).set("s2_programs", on)
        pl = pipe.plan(0)
        assert pl.query("min_chunks") == 64
        share = pl.query("n_s2_prog_gate_work") / pl.query("n_s2_block_gate_work")
        assert (share > 0.72) if on else (share == 0)
        res[on] = pipe.run(1)[0].numpy()
        del pipe
    ref = np.abs(res[0]).max()
    assert ref > 0
    d = np.abs(res[1] - res[0]).max() / ref
    print(f"C4 block, programs on vs off: {d:.2e}, bit-identical {np.array_equal(res[1], res[0])}")
    assert d <= 2e-5
