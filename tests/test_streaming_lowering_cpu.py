"""The lowering every streaming-kernel case of streaming_cases.py is meant to reach, asserted on
the compiled plan's description (tq_plan_create needs no GPU).  A planner change that routes a
case to another kernel fails here, instead of leaving test_streaming_kernels_gpu.py green on the
wrong kernel."""
import pytest
import torch

import streaming_cases as sc
from tneq_qc_amd.expression import HipContractExpression


def describe_permute(case, dt):
    e = HipContractExpression(sc.perm_equation(case), case.shape)
    strides = None if case.strides is None else [case.strides]
    return e.plan(getattr(torch, dt), strides=strides).describe()


def describe_pair(eq, shapes, path, dt):
    return HipContractExpression(eq, *shapes, optimize=path).plan(getattr(torch, dt)).describe()


@pytest.mark.parametrize("case,dt,env", sc.all_perm_cases(),
                         ids=[f"{c.id}-{dt}" + "".join(f"-{k}" for k in env) for c, dt, env in sc.all_perm_cases()])
def test_permute_lowering(monkeypatch, case, dt, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc.assert_permute_lowering(describe_permute(case, dt), case, dt)


def test_permute_novec_is_read_at_every_plan_build(monkeypatch):
    """TQ_PERM_NOVEC changes the kind of the next plan built, and only while it is set."""
    vec = sc.PERM_KINDS[5]
    assert vec.shape == sc.PERM_NOVEC.shape and vec.perm == sc.PERM_NOVEC.perm
    sc.assert_permute_lowering(describe_permute(vec, "float32"), vec, "float32")
    monkeypatch.setenv("TQ_PERM_NOVEC", "1")
    sc.assert_permute_lowering(describe_permute(sc.PERM_NOVEC, "float32"), sc.PERM_NOVEC, "float32")
    monkeypatch.delenv("TQ_PERM_NOVEC")
    sc.assert_permute_lowering(describe_permute(vec, "float32"), vec, "float32")


def test_second_trip_and_tilemul_shapes():
    """The second-trip premise divides numel by the full tile; TQ_PERM_TILEMUL applies only to a
    power-of-two tile count above one."""
    for case, dt in sc.SECOND_TRIP_RUNS:
        assert sc.numel(case.shape) % sc.perm_tile_elems(dt) == 0
    for case in sc.PERM_TILEMUL:
        for dt in ("float32", "complex64"):
            t = sc.numel(case.shape) // sc.perm_tile_elems(dt)
            assert t > 1 and t & (t - 1) == 0


@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("case", sc.all_apply_cases(), ids=[c.id for c in sc.all_apply_cases()])
def test_apply_lowering(case, dt):
    sc.assert_apply_lowering(describe_pair(case.eq, case.shapes, [(0, 1)], dt), case)


def test_apply_cases_cover_every_instantiation():
    """The (KMAX, NMAX) kernel apply_t picks (first fit in its own order) for each B1 case."""
    inst = [(2, 1), (2, 2), (4, 4), (4, 16), (16, 4), (16, 16), (32, 32)]
    picked = []
    for c in sc.APPLY_INST:
        _, K1, _, K2, _, N = c.lowering
        picked.append(next(kn for kn in inst if K1 * K2 <= kn[0] and N <= kn[1]))
    assert picked == inst
    assert sc.APPLY_INST[-1].lowering[1] * sc.APPLY_INST[-1].lowering[5] == 1024
    for c in sc.APPLY_SECOND_TRIP:
        assert sc.apply_positions(c) > sc.APPLY_GRID_POSITIONS


@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("case", sc.SWEEPS, ids=[c.id for c in sc.SWEEPS])
def test_sweep_lowering(case, dt):
    sc.assert_sweep_lowering(describe_pair(*sc.sweep_network(case), dt), case)


def test_sweep_chunk_counts():
    assert [sc.sweep_chunks(c) for c in sc.SWEEPS] == [384, 512, 274]
    assert [sc.sweep_grid(sc.sweep_chunks(c)) for c in sc.SWEEPS] == [256, 256, 256]
    assert sc.SWEEPS[2].lowering[3] % sc.SWEEP_COLS != 0
