"""Case tables and numpy references of the HBM-bound streaming kernels (tq_permute.hip, the APPLY
and axpy kernels of tq_apply.hip, the table-driven tq_sweep.hip), shared by
test_streaming_lowering_cpu.py and test_streaming_kernels_gpu.py.  Every case carries the lowering
it is meant to reach: the CPU file asserts it on the compiled plan's description, the GPU file
re-asserts it before it compares values.  Helper module: no tests here."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

DTYPES = ["float32", "float64", "complex64", "complex128"]
EXACT = {"float32": "float64", "float64": "float64", "complex64": "complex128", "complex128": "complex128"}
# the project's fixed bounds (test_kernels_gpu.py): max error / max |exact reference|
TOL = {"float32": 2e-5, "complex64": 2e-5, "float64": 1e-12, "complex128": 1e-12}
SYMS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def rand(rng, shape, dt):
    x = rng.standard_normal(shape)
    if dt.startswith("complex"):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dt)


def rand_flat(rng, n, dt):
    """n distinct-looking values in [0, 1) drawn in the dtype's own precision (cheap for the
    20 M element operands of the second-trip cases, whose checks are bit-exact data movement)."""
    real = np.float32 if dt in ("float32", "complex64") else np.float64
    if dt.startswith("complex"):
        return rng.random(2 * n, dtype=real).view(dt)
    return rng.random(n, dtype=real)


def scaled_add(w, y, beta):
    """w + beta * y in the operands' own dtype, the real and imaginary parts scaled separately (what
    add_scaled in tq_permute.hip and axpy_kernel compute); beta is rounded to that precision."""
    w = np.ascontiguousarray(w)
    y = np.ascontiguousarray(y)
    assert w.dtype == y.dtype and w.shape == y.shape
    real = np.float32 if w.dtype in (np.float32, np.complex64) else np.float64
    out = w.view(real) + real(beta) * y.view(real)
    assert out.dtype == real
    return out.view(w.dtype)


def scaled_add_exact(w, y, beta):
    """w + beta * y in float64 / complex128."""
    ex = EXACT[str(w.dtype)]
    return w.astype(ex) + beta * y.astype(ex)


def numel(shape):
    n = 1
    for e in shape:
        n *= e
    return n


def op_lines(desc):
    """The op lines of a plan description (NativePlan.describe())."""
    return [ln for ln in desc.splitlines() if " step " in ln]


def rel_err(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / max(1e-300, np.abs(ref).max()))


# ---- permute --------------------------------------------------------------------------------

class PermCase(NamedTuple):
    id: str
    shape: Tuple[int, ...]
    perm: Tuple[int, ...]
    kind: dict                                  # dtype -> plan kind in describe()'s brackets
    strides: Optional[Tuple[int, ...]] = None   # element strides of the source view (None: contiguous)


def _kinds(f32, f64_c64, c128="tiled"):
    return {"float32": f32, "float64": f64_c64, "complex64": f64_c64, "complex128": c128}


def _rev(n):
    return tuple(range(n))[::-1]


_ALL = lambda k: _kinds(k, k, k)  # noqa: E731

# A1: one case per plan kind; complex128 moves one element per 16-byte access, so it is never vector
PERM_KINDS = [
    PermCase("generic-257x263", (257, 263), (1, 0), _ALL("generic")),
    PermCase("tiled-3x5x7", (3, 5, 7), (2, 1, 0), _ALL("tiled")),
    PermCase("tiled-64x33", (64, 33), (1, 0), _ALL("tiled")),
    PermCase("vec2-128x2x2x130", (128, 2, 2, 130), (3, 1, 2, 0), _kinds("vec2", "vec2")),
    PermCase("vec2-npow2-6x10x12x6", (6, 10, 12, 6), _rev(4), _kinds("vec2", "vec2")),
    PermCase("vec-96x96", (96, 96), (1, 0), _kinds("vec4", "vec2")),
    PermCase("vec-4x3x4x3x4x3x4", (4, 3, 4, 3, 4, 3, 4), _rev(7), _kinds("vec4", "vec2")),
    PermCase("swizzle-2p16-rotl", (2,) * 16, tuple(range(1, 16)) + (0,), _kinds("vec4", "vec2")),
    PermCase("swizzle-2p16-rotr", (2,) * 16, (15,) + tuple(range(15)), _kinds("vec4", "vec2")),
]
# a (1, 64, 33) operand expanded to (7, 64, 33): stride 0 on the leading leg
PERM_EXPANDED = [
    PermCase("expand-012", (7, 64, 33), (0, 1, 2), _kinds("vec4", "vec2"), (0, 33, 1)),
    PermCase("expand-210", (7, 64, 33), (2, 1, 0), _ALL("tiled"), (0, 33, 1)),
    PermCase("expand-120", (7, 64, 33), (1, 2, 0), _ALL("tiled"), (0, 33, 1)),
]
# A2: source and / or destination one element off their allocation: the vector plans fall back to
# the scalar tables (EPT = 16 for a 4096-element tile of a 4- or 8-byte type) at launch
PERM_MISALIGNED = [
    PermCase("misalign-2p14", (2,) * 14, _rev(14), _kinds("vec4", "vec2")),
    PermCase("misalign-96x96", (96, 96), (1, 0), _kinds("vec4", "vec2")),
]
MISALIGN_DTYPES = ["float32", "complex64"]
# A3: beta on a generic, a tiled and a vector case
PERM_BETA = [PERM_KINDS[0], PERM_KINDS[2], PERM_KINDS[5]]
BETAS_EXACT = [1.0, -1.0, 0.5, 2.0]   # powers of two: the product is exact, the sum rounds once
BETA_INEXACT = 0.3
# A4: more tiles than the persistent grid has workgroups (8 x CUs at the most)
PERM_SECOND_TRIP = [
    PermCase("trip-5x2048x2048-210", (5, 2048, 2048), (2, 1, 0), _kinds("vec4", "vec2")),
    PermCase("trip-5x2048x2048-120", (5, 2048, 2048), (1, 2, 0), _kinds("vec4", "vec2")),
    PermCase("trip-5x1024x2048-210", (5, 1024, 2048), (2, 1, 0), _kinds("vec4", "vec2")),
    PermCase("trip-5x1024x2048-120", (5, 1024, 2048), (1, 2, 0), _kinds("vec4", "vec2")),
    PermCase("trip-4096x4096", (4096, 4096), (1, 0), _kinds("vec4", "vec2")),
]
SECOND_TRIP_RUNS = ([(c, dt) for c in PERM_SECOND_TRIP[:2] for dt in ("float32", "float64", "complex64")]
                    + [(c, "complex128") for c in PERM_SECOND_TRIP[2:4]]
                    + [(PERM_SECOND_TRIP[4], dt) for dt in ("float32", "complex64")])
# A5: the plan-build knobs
PERM_TILEMUL = [PERM_SECOND_TRIP[4], PermCase("tilemul-2p16", (2,) * 16, _rev(16), _kinds("vec4", "vec2"))]
PERM_NOVEC = PermCase("novec-96x96", (96, 96), (1, 0), _ALL("tiled"))


def perm_tile_elems(dt):
    """Elements of a full permute tile (kMaxTile; halved for 16-byte elements)."""
    return 2048 if dt == "complex128" else 4096


def perm_equation(case):
    s = SYMS[:len(case.shape)]
    return s + "->" + "".join(s[i] for i in case.perm)


def perm_expected(case, dt):
    return f"[{case.kind[dt]}]"


def assert_permute_lowering(desc, case, dt):
    """The plan is one PERMUTE of the kind the case is meant to reach, written to the output."""
    ops = op_lines(desc)
    assert len(ops) == 1 and " PERMUTE " in ops[0] and ops[0].endswith(perm_expected(case, dt) + " ->OUT"), desc


def all_perm_cases():
    """(case, dtype, env) of every permute lowering the two test files rely on."""
    out = []
    for c in PERM_KINDS + PERM_EXPANDED:
        out += [(c, dt, {}) for dt in DTYPES]
    for c in PERM_MISALIGNED:
        out += [(c, dt, {}) for dt in MISALIGN_DTYPES]
    out += [(c, dt, {}) for c, dt in SECOND_TRIP_RUNS]
    out += [(c, dt, {"TQ_PERM_TILEMUL": "5"}) for c in PERM_TILEMUL for dt in ("float32", "complex64")]
    out.append((PERM_NOVEC, "float32", {"TQ_PERM_NOVEC": "1"}))
    return out


# ---- APPLY ----------------------------------------------------------------------------------

class ApplyCase(NamedTuple):
    id: str
    eq: str
    shapes: Tuple[Tuple[int, ...], ...]
    lowering: Tuple[int, int, int, int, int, int]   # O K1 M K2 I N


def apply_expected(case):
    O, K1, M, K2, I, N = case.lowering
    return f" APPLY O={O} K1={K1} M={M} K2={K2} I={I} N={N} ->OUT"


def assert_apply_lowering(desc, case):
    """The plan is one APPLY with the case's layout numbers, written straight to the output."""
    ops = op_lines(desc)
    assert len(ops) == 1 and ops[0].endswith(apply_expected(case)), desc


_S10 = (2,) * 10
# B1: the seven (KMAX, NMAX) instantiations, a small operand on a (2,)*10 state
APPLY_INST = [
    ApplyCase("K2N1", "abcdefghij,e->abcdfghij", (_S10, (2,)), (16, 2, 1, 1, 32, 1)),
    ApplyCase("K2N2", "abcdefghij,ex->abcdxfghij", (_S10, (2, 2)), (16, 2, 1, 1, 32, 2)),
    ApplyCase("K4N4", "abcdefghij,efxy->abcdxyghij", (_S10, (2,) * 4), (16, 4, 1, 1, 16, 4)),
    ApplyCase("K4N16", "abcdefghij,efwxyz->abcdwxyzghij", (_S10, (2,) * 6), (16, 4, 1, 1, 16, 16)),
    ApplyCase("K16N4", "abcdefghij,defgxy->abcxyhij", (_S10, (2,) * 6), (8, 16, 1, 1, 8, 4)),
    ApplyCase("K16N16", "abcdefghij,defgwxyz->abcwxyzhij", (_S10, (2,) * 8), (8, 16, 1, 1, 8, 16)),
    ApplyCase("K32N32", "abcdefghij,cdefgvwxyz->abvwxyzhij", (_S10, (2,) * 10), (4, 32, 1, 1, 8, 32)),
]
_NP2 = (5, 3, 7, 3, 4)
# B2: layout edges
APPLY_EDGES = [
    ApplyCase("two-runs", "abcdefghij,cgxy->abxydefhij", (_S10, (2,) * 4), (4, 2, 8, 2, 8, 4)),
    ApplyCase("npow2", "abcde,bx->axcde", (_NP2, (3, 5)), (5, 3, 1, 1, 84, 5)),
    ApplyCase("npow2-two-runs", "abcde,bdx->axce", (_NP2, (3, 3, 2)), (5, 3, 7, 3, 4, 2)),
    ApplyCase("O1", "abcdefghij,abxy->xycdefghij", (_S10, (2,) * 4), (1, 4, 1, 1, 256, 4)),
    ApplyCase("I1", "abcdefghij,ijxy->abcdefghxy", (_S10, (2,) * 4), (256, 4, 1, 1, 1, 4)),
    ApplyCase("gather", "abcdefghij,xyfe->abcdxyghij", (_S10, (2,) * 4), (16, 4, 1, 1, 16, 4)),
    ApplyCase("gather-npow2", "abcde,xb->axcde", (_NP2, (5, 3)), (5, 3, 1, 1, 84, 5)),
    ApplyCase("vector", "abcde,c->abde", (_NP2, (7,)), (15, 7, 1, 1, 12, 1)),
]
# B4: more positions (O * M * I) than the grid covers in one trip (8192 x 256)
APPLY_SECOND_TRIP = [
    ApplyCase("trip-one-run", "abcd,bcxy->axyd", ((5, 2, 2, 524288), (2,) * 4), (5, 4, 1, 1, 524288, 4)),
    ApplyCase("trip-two-runs", "abcde,bdxy->axyce", ((5, 2, 1024, 2, 512), (2,) * 4), (5, 2, 1024, 2, 512, 4)),
]
APPLY_GRID_POSITIONS = 8192 * 256


def apply_positions(case):
    O, _, M, _, I, _ = case.lowering
    return O * M * I


def all_apply_cases():
    return APPLY_INST + APPLY_EDGES + APPLY_SECOND_TRIP


def apply_operands(case, dt, seed=0):
    rng = np.random.default_rng([17, seed, len(case.eq)])
    return [rand(rng, s, dt) for s in case.shapes]


def apply_reference(case, operands):
    ex = EXACT[str(operands[0].dtype)]
    return np.einsum(case.eq, *[o.astype(ex) for o in operands])


# ---- axpy -----------------------------------------------------------------------------------

AXPY_SIZES = [1, 255, 257, 3 * 2 ** 20 + 17]
AXPY_GRID_POSITIONS = 4096 * 256
AXPY_BETAS_EXACT = [0.0, 1.0, -0.5]


# ---- table-driven sweep -----------------------------------------------------------------------

class SweepCase(NamedTuple):
    id: str
    state: Tuple[int, ...]
    chain: Tuple[Tuple[int, int, int], ...]   # (position, legs contracted, new legs), left to right
    lowering: Tuple[int, int, int, int]       # gates tin tout cols of the SWEEP op


_CHAIN4 = lambda p: ((p, 2, 2), (p + 2, 2, 2), (p + 1, 2, 2), (p, 2, 2))  # noqa: E731

SWEEPS = [
    # extent-3 outer leg: the mixed-radix column offsets; 384 chunks of 64 columns
    SweepCase("D1-outer3", (3,) + (2,) * 17, _CHAIN4(14), (3, 16, 16, 24576)),
    # extent-3 tile leg: a 24-element tile; 512 chunks (the chain's last gate is an APPLY to the output)
    SweepCase("D2-tile3", (2,) * 14 + (3, 2, 2, 2, 2), _CHAIN4(14)[:3], (2, 24, 24, 32768)),
    # 17496 columns: 274 chunks, the last one ragged
    SweepCase("D3-ragged", (3,) * 7 + (2,) * 3 + (2,) * 4, _CHAIN4(10), (3, 16, 16, 17496)),
]
SWEEP_COLS = 64


def sweep_expected(case):
    g, tin, tout, cols = case.lowering
    return f" SWEEP gates={g} tin={tin} tout={tout} cols={cols} "


def assert_sweep_lowering(desc, case):
    """Exactly one table-driven SWEEP op with the case's numbers, and no sweep2 op."""
    assert sum(sweep_expected(case) in ln + " " for ln in op_lines(desc)) == 1, desc
    assert " SWEEP2 " not in desc, desc
    # some workgroups take a second chunk, so the register prefetch inside the loop runs
    assert sweep_chunks(case) > sweep_grid(sweep_chunks(case))


def sweep_chunks(case):
    return -(-case.lowering[3] // SWEEP_COLS)


def sweep_grid(nchunks):
    """Workgroups sweep_t launches for one lane."""
    cap = 512
    return max(1, min(nchunks, cap if nchunks >= 2 * cap else max(256, (nchunks + 1) // 2)))


def sweep_network(case):
    """(equation, shapes, SSA path) of the chain: a new leg takes the extent of the contracted leg
    it replaces (2 when the gate adds more legs than it contracts)."""
    syms = iter(SYMS)
    ext = {}
    cur = []
    for e in case.state:
        s = next(syms)
        ext[s] = e
        cur.append(s)
    terms = ["".join(cur)]
    for pos, kc, kn in case.chain:
        contracted = cur[pos:pos + kc]
        new = []
        for q in range(kn):
            s = next(syms)
            ext[s] = ext[contracted[q]] if q < kc else 2
            new.append(s)
        terms.append("".join(contracted) + "".join(new))
        cur[pos:pos + kc] = new
    eq = ",".join(terms) + "->" + "".join(cur)
    shapes = [tuple(ext[c] for c in t) for t in terms]
    path = [(0, 1)] + [(len(terms) + i, i + 2) for i in range(len(terms) - 2)]
    return eq, shapes, path


@functools.lru_cache(maxsize=None)
def sweep_operands_and_reference(case, dt):
    """Operands in `dt` and the oracle's exact contraction of those very operands (read-only)."""
    from oracle.contract_ref import contract
    eq, shapes, path = sweep_network(case)
    rng = np.random.default_rng([23, len(eq)])
    ops = [rand(rng, shapes[0], dt)]
    for s in shapes[1:]:
        k = len(s) // 2
        ops.append((rand(rng, s, EXACT[dt]) / np.sqrt(np.prod(s[:k]))).astype(dt))
    ref = np.ascontiguousarray(contract(eq, *ops, path=path))
    for a in ops + [ref]:
        a.setflags(write=False)
    return ops, ref
