"""The HBM-bound streaming kernels against numpy on the host, per variant and past the first trip
of their persistent / grid-stride loops: permute (tq_permute.hip; bit-exact), APPLY and axpy
(tq_apply.hip) and the table-driven sweep (tq_sweep.hip).  The cases and the lowering each one is
meant to reach live in streaming_cases.py; every test re-asserts that lowering on the plan it runs
(or, for direct tq_permute calls, on the one-op plan of the same shape and strides, which builds
the same permute plan) before it compares values.  float32 / complex64 results are compared with
a float64 / complex128 reference of the same operands under the project's fixed bounds; data
movement and power-of-two betas are compared bit for bit in the operands' own dtype."""
import ctypes

import numpy as np
import pytest

import streaming_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(dev):
    import torch
    return torch


def _to(T, dev, a):
    a = np.asarray(a)
    # (a shared read-only operand is copied: torch wants a writable host array; rank 0 stays rank 0)
    if not (a.flags.c_contiguous and a.flags.writeable):
        a = np.array(a, order="C")
    return T.from_numpy(a).to(dev)


def _expr(eq, *shapes, **kw):
    from tneq_qc_amd.expression import HipContractExpression
    return HipContractExpression(eq, *shapes, **kw)


def _perm_expr(T, case, dt):
    """The one-op expression of a permute case, its lowering asserted."""
    e = _expr(sc.perm_equation(case), case.shape)
    plan = e.plan(getattr(T, dt), strides=None if case.strides is None else [case.strides])
    sc.assert_permute_lowering(plan.describe(), case, dt)
    return e


def _tq_permute(T, src, perm, dst, beta):
    """dst (a contiguous window of numel elements) = permute(src) + beta * dst through the C entry."""
    from tneq_qc_amd import _lib
    from tneq_qc_amd.ops import dtype_code
    shape = [src.shape[d] for d in perm]
    strides = [src.stride(d) for d in perm]
    assert dst.is_contiguous() and dst.numel() == src.numel() and dst.dtype == src.dtype
    rc = _lib.lib().tq_permute(dtype_code(src.dtype), len(shape), _lib.i64(shape), _lib.i64(strides),
                               ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                               float(beta), ctypes.c_void_p(T.cuda.current_stream(src.device).cuda_stream))
    _lib.check(rc, "tq_permute")


# ---- A. permute -------------------------------------------------------------------------------

_A1 = [(c, dt) for c in sc.PERM_KINDS + sc.PERM_EXPANDED for dt in sc.DTYPES]


@pytest.mark.parametrize("case,dt", _A1, ids=[f"{c.id}-{dt}" for c, dt in _A1])
def test_permute_every_kind(T, dev, case, dt):
    rng = np.random.default_rng(31)
    if case.strides is None:
        x = sc.rand(rng, case.shape, dt)
        xd = _to(T, dev, x)
    else:   # stride 0 on the leading leg
        base = sc.rand(rng, (1,) + case.shape[1:], dt)
        x = np.broadcast_to(base, case.shape)
        xd = _to(T, dev, base).expand(*case.shape)
        assert tuple(xd.stride()) == case.strides
    e = _perm_expr(T, case, dt)
    y = e(xd).cpu().numpy()
    assert np.array_equal(y, np.transpose(x, case.perm))


@pytest.mark.parametrize("dt", sc.DTYPES)
def test_permute_edge_operands(T, dev, dt):
    """A 0-d tensor, one element, and zero extents (nothing to launch)."""
    import tneq_qc_amd.ops as ops
    rng = np.random.default_rng(32)
    for shape, perm in [((), ()), ((1,), (0,)), ((1, 1, 1), (2, 0, 1)), ((0,), (0,)), ((3, 0, 5), (2, 0, 1)),
                        ((0, 4), (1, 0))]:
        x = sc.rand(rng, shape, dt)
        y = ops.permute(_to(T, dev, x), perm).cpu().numpy()
        ref = np.transpose(x, perm)
        assert y.shape == ref.shape and y.dtype == ref.dtype and np.array_equal(y, ref), (shape, perm)


_A2 = [(c, dt, how) for c in sc.PERM_MISALIGNED for dt in sc.MISALIGN_DTYPES for how in ("src", "dst", "both")]


@pytest.mark.parametrize("case,dt,how", _A2, ids=[f"{c.id}-{dt}-{how}" for c, dt, how in _A2])
def test_permute_misaligned_falls_back_to_scalar(T, dev, case, dt, how):
    """A source view and / or a destination window one element into its storage: the vector plan
    runs its scalar tables; nothing outside the destination window is written."""
    _perm_expr(T, case, dt)                     # a vector plan ...
    vec = int(case.kind[dt][3:])
    rng = np.random.default_rng(33)
    n = sc.numel(case.shape)
    x = sc.rand(rng, case.shape, dt)
    s_off = 1 if how in ("src", "both") else 0
    d_off = 1 if how in ("dst", "both") else 4  # 4 elements keep 16-byte alignment
    sbuf = T.zeros(n + 1, dtype=getattr(T, dt), device=dev)
    src = sbuf[s_off:s_off + n].view(*case.shape)
    src.copy_(_to(T, dev, x))
    guard = sc.rand(rng, (d_off + n + 4,), dt)
    dbuf = _to(T, dev, guard)
    dst = dbuf[d_off:d_off + n]
    # ... whose launch sees (src | dst) off the vector alignment
    assert ((src.data_ptr() | dst.data_ptr()) % (vec * x.itemsize) != 0)
    assert sbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
    _tq_permute(T, src, case.perm, dst, 0.0)
    got = dbuf.cpu().numpy()
    assert np.array_equal(got[d_off:d_off + n], np.transpose(x, case.perm).reshape(-1))
    assert got[:d_off].tobytes() == guard[:d_off].tobytes()
    assert got[d_off + n:].tobytes() == guard[d_off + n:].tobytes()


_A3 = [(c, dt) for c in sc.PERM_BETA for dt in sc.DTYPES]


@pytest.mark.parametrize("case,dt", _A3, ids=[f"{c.id}-{dt}" for c, dt in _A3])
def test_permute_beta(T, dev, case, dt):
    """dst = permute(src) + beta * dst: bit-exact for power-of-two betas (exact product, one
    rounding of the sum), the fixed bounds against float64 / complex128 for beta = 0.3."""
    _perm_expr(T, case, dt)
    rng = np.random.default_rng(34)
    x = sc.rand(rng, case.shape, dt)
    xd = _to(T, dev, x)
    xt = np.ascontiguousarray(np.transpose(x, case.perm))
    y0 = sc.rand(rng, xt.shape, dt)
    for beta in sc.BETAS_EXACT:
        yd = _to(T, dev, y0)
        _tq_permute(T, xd, case.perm, yd, beta)
        assert np.array_equal(yd.cpu().numpy(), sc.scaled_add(xt, y0, beta)), beta
    yd = _to(T, dev, y0)
    _tq_permute(T, xd, case.perm, yd, sc.BETA_INEXACT)
    err = sc.rel_err(yd.cpu().numpy(), sc.scaled_add_exact(xt, y0, sc.BETA_INEXACT))
    print(f"permute beta=0.3 {case.id} {dt}: rel err {err:.3e}")
    assert err < sc.TOL[dt]


@pytest.fixture(scope="module")
def big(T, dev):
    """Per dtype: one flat operand of the largest second-trip size on the host and on the device,
    generated once and never written (the cases view prefixes of it)."""
    cache = {}

    def get(dt):
        if dt not in cache:
            n = max(sc.numel(c.shape) for c, d in sc.SECOND_TRIP_RUNS if d == dt)
            x = sc.rand_flat(np.random.default_rng([35, len(cache)]), n, dt)
            x.setflags(write=False)
            cache[dt] = (x, _to(T, dev, x))
        return cache[dt]
    return get


def _second_trip_premise(T, dev, case, dt):
    """More tiles than the persistent grid can hold workgroups: some workgroup takes a second tile."""
    cus = T.cuda.get_device_properties(dev).multi_processor_count
    tiles = sc.numel(case.shape) / sc.perm_tile_elems(dt)
    assert tiles > 8 * cus, (tiles, cus)


@pytest.mark.parametrize("case,dt", sc.SECOND_TRIP_RUNS, ids=[f"{c.id}-{dt}" for c, dt in sc.SECOND_TRIP_RUNS])
def test_permute_second_trip(T, dev, big, case, dt):
    _second_trip_premise(T, dev, case, dt)
    e = _perm_expr(T, case, dt)
    n = sc.numel(case.shape)
    x, xd = big(dt)
    y = e(xd[:n].view(*case.shape)).cpu().numpy()
    assert np.array_equal(y, np.transpose(x[:n].reshape(case.shape), case.perm))


def test_permute_second_trip_accumulates(T, dev, big):
    """beta = 1 on a three-trip shape: the read-modify-write of dst uses each trip's own base."""
    case, dt = sc.PERM_SECOND_TRIP[1], "float32"
    _second_trip_premise(T, dev, case, dt)
    _perm_expr(T, case, dt)
    n = sc.numel(case.shape)
    x, xd = big(dt)
    xt = np.ascontiguousarray(np.transpose(x[:n].reshape(case.shape), case.perm))
    y0 = np.ascontiguousarray(x[:n][::-1]).reshape(xt.shape)
    yd = _to(T, dev, y0)
    _tq_permute(T, xd[:n].view(*case.shape), case.perm, yd, 1.0)
    assert np.array_equal(yd.cpu().numpy(), sc.scaled_add(xt, y0, 1.0))


_A5 = [(c, dt) for c in sc.PERM_TILEMUL for dt in ("float32", "complex64")]


@pytest.mark.parametrize("case,dt", _A5, ids=[f"{c.id}-{dt}" for c, dt in _A5])
def test_permute_tile_order_knob(T, dev, big, monkeypatch, case, dt):
    """TQ_PERM_TILEMUL=5 (read when the plan is built): tiles are visited as (t * 5) mod n_tiles."""
    monkeypatch.setenv("TQ_PERM_TILEMUL", "5")
    n = sc.numel(case.shape)
    tiles = n // sc.perm_tile_elems(dt)
    assert tiles > 1 and tiles & (tiles - 1) == 0     # the knob applies to power-of-two tile counts
    e = _perm_expr(T, case, dt)
    x, xd = big(dt)
    y = e(xd[:n].view(*case.shape)).cpu().numpy()
    assert np.array_equal(y, np.transpose(x[:n].reshape(case.shape), case.perm))


def test_permute_novec_knob(T, dev, monkeypatch):
    """TQ_PERM_NOVEC: the scalar tables of a shape that otherwise lowers to vec4."""
    monkeypatch.setenv("TQ_PERM_NOVEC", "1")
    case, dt = sc.PERM_NOVEC, "float32"
    e = _perm_expr(T, case, dt)
    x = sc.rand(np.random.default_rng(36), case.shape, dt)
    assert np.array_equal(e(_to(T, dev, x)).cpu().numpy(), np.transpose(x, case.perm))


# ---- B. APPLY ---------------------------------------------------------------------------------

def _run_apply(T, dev, case, dt, operands, out=None):
    e = _expr(case.eq, *case.shapes, optimize=[(0, 1)])
    sc.assert_apply_lowering(e.plan(getattr(T, dt)).describe(), case)
    ts = [_to(T, dev, o) for o in operands]
    if out is None:
        return e(*ts).cpu().numpy()
    return e(*ts, out=out, accumulate=True).cpu().numpy()


_B12 = sc.APPLY_INST + sc.APPLY_EDGES


@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("case", _B12, ids=[c.id for c in _B12])
def test_apply_variants(T, dev, case, dt):
    operands = sc.apply_operands(case, dt)
    ref = sc.apply_reference(case, operands)
    err = sc.rel_err(_run_apply(T, dev, case, dt, operands), ref)
    print(f"apply {case.id} {dt}: rel err {err:.3e}")
    assert err < sc.TOL[dt]


@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("case", sc.APPLY_EDGES, ids=[c.id for c in sc.APPLY_EDGES])
def test_apply_accumulates(T, dev, case, dt):
    operands = sc.apply_operands(case, dt)
    prod = sc.apply_reference(case, operands)
    out0 = sc.rand(np.random.default_rng(41), prod.shape, dt)
    ref = prod + out0.astype(sc.EXACT[dt])
    err = sc.rel_err(_run_apply(T, dev, case, dt, operands, out=_to(T, dev, out0)), ref)
    print(f"apply accumulate {case.id} {dt}: rel err {err:.3e}")
    assert err < sc.TOL[dt]


@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("case", sc.APPLY_SECOND_TRIP, ids=[c.id for c in sc.APPLY_SECOND_TRIP])
def test_apply_second_trip(T, dev, case, dt):
    assert sc.apply_positions(case) > sc.APPLY_GRID_POSITIONS   # the grid-stride loop goes round again
    operands = sc.apply_operands(case, dt)
    ref = sc.apply_reference(case, operands)
    err = sc.rel_err(_run_apply(T, dev, case, dt, operands), ref)
    print(f"apply {case.id} {dt}: rel err {err:.3e}")
    assert err < sc.TOL[dt]


# ---- C. axpy ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("n", sc.AXPY_SIZES)
def test_axpy(T, dev, dt, n):
    """y = x + beta * y in place: bit-exact for beta 0, 1, -0.5, the fixed bounds for 0.3; x is
    left alone.  The largest size takes more than three ragged trips of the 4096 x 256 grid."""
    import tneq_qc_amd.ops as ops
    if n == max(sc.AXPY_SIZES):
        assert n > 3 * sc.AXPY_GRID_POSITIONS and n % 256 != 0
    rng = np.random.default_rng(51)
    x = sc.rand(rng, (n,), dt)
    y0 = sc.rand(rng, (n,), dt)
    xd = _to(T, dev, x)
    for beta in sc.AXPY_BETAS_EXACT:
        yd = _to(T, dev, y0)
        assert ops.axpy(xd, yd, beta) is yd
        assert np.array_equal(yd.cpu().numpy(), sc.scaled_add(x, y0, beta)), beta
    yd = _to(T, dev, y0)
    ops.axpy(xd, yd, sc.BETA_INEXACT)
    err = sc.rel_err(yd.cpu().numpy(), sc.scaled_add_exact(x, y0, sc.BETA_INEXACT))
    print(f"axpy beta=0.3 n={n} {dt}: rel err {err:.3e}")
    assert err < sc.TOL[dt]
    assert xd.cpu().numpy().tobytes() == x.tobytes()


# ---- D. table-driven sweep ----------------------------------------------------------------------

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("case", sc.SWEEPS, ids=[c.id for c in sc.SWEEPS])
def test_sweep_tables(T, dev, case, dt, accumulate):
    eq, shapes, path = sc.sweep_network(case)
    e = _expr(eq, *shapes, optimize=path)
    sc.assert_sweep_lowering(e.plan(getattr(T, dt)).describe(), case)
    operands, ref = sc.sweep_operands_and_reference(case, dt)
    ts = [_to(T, dev, o) for o in operands]
    if accumulate:
        out0 = sc.rand(np.random.default_rng(61), ref.shape, dt)
        got = e(*ts, out=_to(T, dev, out0), accumulate=True).cpu().numpy()
        ref = ref + out0.astype(sc.EXACT[dt])
    else:
        got = e(*ts).cpu().numpy()
    err = sc.rel_err(got, ref)
    print(f"sweep {case.id} {dt} accumulate={accumulate}: rel err {err:.3e}")
    assert err < sc.TOL[dt]
