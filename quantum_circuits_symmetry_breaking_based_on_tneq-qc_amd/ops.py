"""torch-tensor entry points over the C ABI (device memory and streams come from torch).

These are the device primitives the backend and the contraction plans are built from:
``permute`` (reference: BackendPyTorch.permute, tneq_qc/backends/backend_pytorch.py:619-621),
``gemm`` (the GEMM under every tensordot), ``contract_pair`` (one pairwise einsum,
BackendPyTorch.einsum with two operands, backend_pytorch.py:623-625), and the measurement-data
kernels of EngineSiamese: ``hermite_features`` (generate_data, engine_siamese.py:133-254) and
``inverse_cdf_sample`` (the CDF block of sample, engine_siamese.py:854-905).  ``born_sample`` has
no counterpart in the reference: bitstring indices drawn from an amplitude block by the Born rule;
nor has ``born_topk``, the k most probable bitstrings of a block (post-selection), nor
``born_pool_sample`` / ``born_pool_merge``, the weighted reservoir that samples across blocks.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, i32, i64

_DT = {
    torch.float32: _lib.TQ_F32,
    torch.float64: _lib.TQ_F64,
    torch.complex64: _lib.TQ_C64,
    torch.complex128: _lib.TQ_C128,
}


def dtype_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {dtype}; supported: float32, float64, complex64, complex128")


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_device(*ts: torch.Tensor) -> torch.device:
    dev = ts[0].device
    if dev.type != "cuda":
        raise ValueError(f"tensors must be on a HIP device (got {dev}); use BackendHIP.convert_to_tensor")
    for t in ts[1:]:
        if t.device != dev:
            raise ValueError("all operands must live on the same device")
        if t.dtype != ts[0].dtype:
            raise ValueError("all operands must have the same dtype")
    return dev


def permute(x: torch.Tensor, dims: Sequence[int]) -> torch.Tensor:
    """Materialised ``x.permute(dims).contiguous()`` through the LDS-tiled HIP kernel."""
    dev = _require_device(x)
    dims = [int(d) % max(1, x.ndim) for d in dims]
    if sorted(dims) != list(range(x.ndim)):
        raise ValueError(f"invalid permutation {dims} for rank {x.ndim}")
    shape = [x.shape[d] for d in dims]
    strides = [x.stride(d) for d in dims]
    out = torch.empty(shape, dtype=x.dtype, device=dev)
    if out.numel() == 0:
        return out
    rc = _lib.lib().tq_permute(dtype_code(x.dtype), len(shape), i64(shape), i64(strides),
                               ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                               0.0, ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_permute")
    return out


def gemm(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False,
         out: torch.Tensor | None = None, beta: float = 0.0) -> torch.Tensor:
    """Batched ``C = op(A) @ op(B) (+ beta*C)`` on MFMA; a, b are 2-D or 3-D (batch first), contiguous."""
    dev = _require_device(a, b)
    a3 = a if a.ndim == 3 else a.unsqueeze(0)
    b3 = b if b.ndim == 3 else b.unsqueeze(0)
    if not (a3.is_contiguous() and b3.is_contiguous()):
        raise ValueError("gemm operands must be contiguous")
    batch = a3.shape[0]
    if b3.shape[0] != batch:
        raise ValueError("batch mismatch")
    M, K = (a3.shape[2], a3.shape[1]) if trans_a else (a3.shape[1], a3.shape[2])
    Kb, N = (b3.shape[2], b3.shape[1]) if trans_b else (b3.shape[1], b3.shape[2])
    if K != Kb:
        raise ValueError(f"inner dimension mismatch {K} vs {Kb}")
    if out is None:
        out = torch.empty((batch, M, N), dtype=a.dtype, device=dev)
        beta = 0.0
    out3 = out if out.ndim == 3 else out.unsqueeze(0)
    code = dtype_code(a.dtype)
    L = _lib.lib()
    wsb = L.tq_gemm_workspace_size(code, M, N, K, batch)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=dev) if wsb else None
    rc = L.tq_gemm_batched(code, int(trans_a), int(trans_b), M, N, K, batch,
                           ctypes.c_void_p(a3.data_ptr()), a3.shape[2], a3.shape[1] * a3.shape[2],
                           ctypes.c_void_p(b3.data_ptr()), b3.shape[2], b3.shape[1] * b3.shape[2],
                           float(beta), ctypes.c_void_p(out3.data_ptr()), N, M * N,
                           ctypes.c_void_p(ws.data_ptr() if ws is not None else 0), wsb,
                           ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_gemm_batched")
    if a.ndim == 2 and b.ndim == 2 and out.ndim == 3:
        return out3[0]
    return out


def contract_pair(modes_a: Sequence[int], a: torch.Tensor, modes_b: Sequence[int], b: torch.Tensor,
                  modes_c: Sequence[int]) -> torch.Tensor:
    """einsum("A,B->C") with integer mode labels, on the HIP engine."""
    dev = _require_device(a, b)
    a = a.contiguous()
    b = b.contiguous()
    ext = {}
    for m, e in list(zip(modes_a, a.shape)) + list(zip(modes_b, b.shape)):
        if ext.setdefault(int(m), int(e)) != int(e):
            raise ValueError(f"mode {m} has inconsistent extents")
    try:
        shape_c = [ext[int(m)] for m in modes_c]
    except KeyError as e:
        raise ValueError(f"output mode {e} not present in inputs")
    out = torch.empty(shape_c, dtype=a.dtype, device=dev)
    code = dtype_code(a.dtype)
    L = _lib.lib()
    args = (code, len(modes_a), i64(a.shape), i32(modes_a), len(modes_b), i64(b.shape), i32(modes_b),
            len(modes_c), i32(modes_c))
    wsb = L.tq_contract_pair_workspace(*args)
    if wsb == 0:
        raise ValueError(f"contract_pair: {_lib.last_error()}")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = L.tq_contract_pair(code, len(modes_a), i64(a.shape), i32(modes_a), ctypes.c_void_p(a.data_ptr()),
                            len(modes_b), i64(b.shape), i32(modes_b), ctypes.c_void_p(b.data_ptr()),
                            len(modes_c), i32(modes_c), ctypes.c_void_p(out.data_ptr()),
                            ctypes.c_void_p(ws.data_ptr()), wsb, ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_contract_pair")
    return out


def axpy(x: torch.Tensor, y: torch.Tensor, beta: float = 1.0) -> torch.Tensor:
    """y = x + beta*y in place (partial-amplitude accumulation)."""
    dev = _require_device(x, y)
    if x.numel() != y.numel() or not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("axpy needs equal-size contiguous tensors")
    rc = _lib.lib().tq_axpy(dtype_code(x.dtype), x.numel(), ctypes.c_void_p(x.data_ptr()),
                            ctypes.c_void_p(y.data_ptr()), float(beta), ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_axpy")
    return y


def hermite_features(x: torch.Tensor, K: int, weights, dtype: torch.dtype, want_phi: bool = True):
    """Hermite measurement data of every entry of ``x`` (any shape; the real part is used):
    ``phi[..., k] = (w_k * sqrt(exp(-x^2/2))) * He_k(x)`` and ``mx[..., k, l] = conj(phi_k) phi_l``
    in ``dtype``; complex dtypes compute in float64, real dtypes in their own precision
    (engine_siamese.py:133-254).  ``weights``: host array of at least K float64 w_k.
    Returns (phi or None, mx)."""
    dev = _require_device(x)
    K = int(K)
    if not 1 <= K <= _lib.TQ_HERMITE_MAX_K:
        raise ValueError(f"K must be in [1, {_lib.TQ_HERMITE_MAX_K}], got {K}")
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1)[:K])
    if w.shape[0] < K:
        raise ValueError(f"need {K} Hermite weights, got {w.shape[0]}")
    xd = (x.real if x.is_complex() else x).to(torch.float64).contiguous()
    phi = torch.empty(tuple(x.shape) + (K,), dtype=dtype, device=dev) if want_phi else None
    mx = torch.empty(tuple(x.shape) + (K, K), dtype=dtype, device=dev)
    rc = _lib.lib().tq_hermite_features(dtype_code(dtype), xd.numel(), K, ctypes.c_void_p(xd.data_ptr()),
                                        w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        ctypes.c_void_p(phi.data_ptr() if phi is not None else None),
                                        ctypes.c_void_p(mx.data_ptr()), ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_hermite_features")
    return phi, mx


def inverse_cdf_sample(density: torch.Tensor, grid: torch.Tensor, u: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One inverse-CDF draw per row of a real (S, G) density on a (G,) grid with S float32
    uniforms ``u`` (engine_siamese.py:857-905): clamp >= 0, cumsum, / (total + 1e-10),
    idx = min(#(cdf < u), G - 2), linear interpolation.  Returns (S,) in the density's dtype."""
    if density.ndim != 2 or grid.ndim != 1 or grid.shape[0] != density.shape[1]:
        raise ValueError(f"density must be (S, G) and grid (G,), got {tuple(density.shape)} and {tuple(grid.shape)}")
    if density.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"density must be real float32/float64, got {density.dtype}")
    dev = _require_device(density, grid)
    S, G = density.shape
    d = density.contiguous()
    gr = grid.contiguous()
    uu = u.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    if uu.numel() != S:
        raise ValueError(f"need {S} uniforms, got {uu.numel()}")
    if out is None:
        out = torch.empty(S, dtype=density.dtype, device=dev)
    elif out.shape != (S,) or out.dtype != density.dtype or out.device != dev:
        raise ValueError("out must be an (S,) tensor of the density's dtype on its device")
    rc = _lib.lib().tq_inverse_cdf_sample(dtype_code(density.dtype), S, G, ctypes.c_void_p(d.data_ptr()), G,
                                          ctypes.c_void_p(gr.data_ptr()), ctypes.c_void_p(uu.data_ptr()),
                                          ctypes.c_void_p(out.data_ptr()), out.stride(0),
                                          ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_inverse_cdf_sample")
    return out


def born_workspace_size(dtype: torch.dtype, n: int, n_draws: int) -> int:
    """Bytes of device workspace one ``born_sample`` call of these sizes needs (host only)."""
    wsb = _lib.lib().tq_born_sample_workspace(dtype_code(dtype), int(n), int(n_draws))
    if wsb == 0:
        raise ValueError(f"born_sample: {_lib.last_error()}")
    return int(wsb)


def born_sample(amps: torch.Tensor, u: torch.Tensor, *, prob=True,
                axis_qubit: Optional[Sequence[int]] = None, base: int = 0,
                out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None):
    """Draw ``len(u)`` indices of the amplitude block ``amps`` (complex64 / complex128, contiguous,
    any shape, on the HIP device) with probability |a_i|^2 / S1, one per float64 uniform in ``u``:
    ``index_j = min{i : C_i > u_j S1}`` with C the float64 inclusive prefix sum of
    ``p_i = re^2 + im^2`` (include/tneqhip.h, tq_born_sample).  Runs on the current stream of
    ``amps``' device; no host copy, no synchronisation.

    ``axis_qubit`` (one qubit per axis of a 2 x 2 x ... block, axis 0 slowest) and ``base`` turn
    every index into a bitstring word (bit q = qubit q).  ``prob``: True (allocate), False (no
    probabilities) or a float64 buffer.  ``out`` (int64) and a ``prob`` buffer are 1-D with at
    least len(u) elements (the first len(u) are written and returned); ``stats`` (float64, (2,))
    and ``workspace`` (at least ``born_workspace_size`` bytes) likewise are allocated when not
    given.  Returns ``(index_or_words, prob or None, stats)``; stats = (S1, sum p^2)."""
    if not isinstance(amps, torch.Tensor) or not isinstance(u, torch.Tensor):
        raise ValueError("born_sample: amps and u must be tensors")
    dev = _require_device(amps)
    if u.device != dev:
        raise ValueError("born_sample: u must live on the amplitudes' device")
    if amps.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"born_sample: amplitudes must be complex64 / complex128, got {amps.dtype}")
    if u.dtype != torch.float64:
        raise ValueError(f"born_sample: uniforms must be float64, got {u.dtype}")
    if not amps.is_contiguous():
        raise ValueError("born_sample: amplitudes must be contiguous")
    if u.ndim != 1 or not u.is_contiguous():
        raise ValueError("born_sample: u must be a contiguous 1-D tensor")
    n, nd = amps.numel(), u.numel()
    code = dtype_code(amps.dtype)
    wsb = born_workspace_size(amps.dtype, n, nd)

    def _buf(t, size, dtype, what, exact=False):
        if t is None:
            return torch.empty(size, dtype=dtype, device=dev)
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or t.ndim != 1
                or not t.is_contiguous() or t.numel() < size or (exact and t.numel() != size)):
            raise ValueError(f"born_sample: {what} must be a contiguous 1-D {dtype} tensor of "
                             f"{'' if exact else 'at least '}{size} elements on {dev}")
        return t[:size]

    out = _buf(out, nd, torch.int64, "out")
    stats = _buf(stats, 2, torch.float64, "stats", exact=True)
    if prob is False or prob is None:
        pr = None
    else:
        pr = _buf(None if prob is True else prob, nd, torch.float64, "prob")
    if workspace is None:
        workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
    elif workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("born_sample: workspace must be a contiguous tensor on the amplitudes' device")
    base = int(base)
    if not 0 <= base < (1 << 64):
        raise ValueError("born_sample: base must fit 64 bits")
    if axis_qubit is not None:
        axes = [int(q) for q in axis_qubit]
        if any(not -(1 << 31) <= q < (1 << 31) for q in axes):
            raise ValueError("born_sample: axis qubit out of range")
        n_axes, table = len(axes), i32(axes)
    else:
        n_axes, table = 0, None
    rc = _lib.lib().tq_born_sample(code, n, ctypes.c_void_p(amps.data_ptr()), nd,
                                   ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                   ctypes.c_void_p(pr.data_ptr() if pr is not None else None),
                                   ctypes.c_void_p(stats.data_ptr()), n_axes, table, base,
                                   ctypes.c_void_p(workspace.data_ptr()),
                                   workspace.numel() * workspace.element_size(),
                                   ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_born_sample")
    return out, pr, stats


def born_pool_workspace_size(dtype: torch.dtype, n: int, n_draws: int) -> int:
    """Bytes of device workspace one ``born_pool_sample`` call of these sizes needs (host only)."""
    wsb = _lib.lib().tq_born_pool_workspace(dtype_code(dtype), int(n), int(n_draws))
    if wsb == 0:
        raise ValueError(f"born_pool_sample: {_lib.last_error()}")
    return int(wsb)


def _pool_buf(who, t, size, dtype, what, dev):
    if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or t.ndim != 1
            or not t.is_contiguous() or t.numel() != size):
        raise ValueError(f"{who}: {what} must be a contiguous 1-D {dtype} tensor of {size} elements on {dev}")
    return t


def born_pool_sample(amps: torch.Tensor, u: torch.Tensor, v: torch.Tensor, index: torch.Tensor,
                     prob: Optional[torch.Tensor], pool: torch.Tensor, *,
                     axis_qubit: Optional[Sequence[int]] = None, base: int = 0,
                     stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Fold the amplitude block ``amps`` into the weighted reservoir ``(index, prob, pool)`` of
    ``len(u)`` slots (include/tneqhip.h, tq_born_pool_sample): the block's candidate for slot j is
    what ``born_sample`` draws for ``u[j]``, and it replaces the slot iff the pool is empty or
    ``v[j] * (W + S1) < S1``, so that after any number of blocks every slot is a Born-rule draw
    over all of them.  ``pool`` (float64, (4,)) = W, sum S2, blocks that contributed, slots the
    last call replaced; zero it to start a pool.  A block whose mass is not a finite number > 0
    changes nothing but ``pool[3] = 0``.  Runs on the current stream of ``amps``' device; no host
    copy, no synchronisation.

    ``u``, ``v``: float64 uniforms, 1-D, the same length >= 1; ``index`` (int64) and ``prob``
    (float64, or None: no probabilities) have exactly that length and are updated in place.
    ``axis_qubit`` and ``base`` turn every index into a bitstring word as in ``born_sample``.
    ``stats`` (float64, (2,)) and ``workspace`` (at least ``born_pool_workspace_size`` bytes) are
    allocated when not given.  Returns ``(index, prob, pool, stats)``; stats = this block's
    (S1, sum p^2)."""
    who = "born_pool_sample"
    if not all(isinstance(t, torch.Tensor) for t in (amps, u, v)):
        raise ValueError(f"{who}: amps, u and v must be tensors")
    dev = _require_device(amps)
    if amps.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"{who}: amplitudes must be complex64 / complex128, got {amps.dtype}")
    if not amps.is_contiguous():
        raise ValueError(f"{who}: amplitudes must be contiguous")
    if not isinstance(u, torch.Tensor) or u.ndim != 1 or u.numel() < 1:
        raise ValueError(f"{who}: u must be a 1-D tensor of at least one uniform")
    n, nd = amps.numel(), u.numel()
    code = dtype_code(amps.dtype)
    wsb = born_pool_workspace_size(amps.dtype, n, nd)
    _pool_buf(who, u, nd, torch.float64, "u", dev)
    _pool_buf(who, v, nd, torch.float64, "v", dev)
    _pool_buf(who, index, nd, torch.int64, "index", dev)
    if prob is not None:
        _pool_buf(who, prob, nd, torch.float64, "prob", dev)
    _pool_buf(who, pool, 4, torch.float64, "pool", dev)
    if stats is None:
        stats = torch.empty(2, dtype=torch.float64, device=dev)
    else:
        _pool_buf(who, stats, 2, torch.float64, "stats", dev)
    if workspace is None:
        workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"{who}: workspace must be a contiguous tensor on the amplitudes' device")
    base = int(base)
    if not 0 <= base < (1 << 64):
        raise ValueError(f"{who}: base must fit 64 bits")
    if axis_qubit is not None:
        axes = [int(q) for q in axis_qubit]
        if any(not -(1 << 31) <= q < (1 << 31) for q in axes):
            raise ValueError(f"{who}: axis qubit out of range")
        n_axes, table = len(axes), i32(axes)
    else:
        n_axes, table = 0, None
    vp = ctypes.c_void_p
    rc = _lib.lib().tq_born_pool_sample(code, n, vp(amps.data_ptr()), nd, vp(u.data_ptr()), vp(v.data_ptr()),
                                        vp(index.data_ptr()), vp(prob.data_ptr() if prob is not None else None),
                                        vp(pool.data_ptr()), vp(stats.data_ptr()), n_axes, table, base,
                                        vp(workspace.data_ptr()), workspace.numel() * workspace.element_size(),
                                        vp(_stream_ptr(dev)))
    check(rc, "tq_born_pool_sample")
    return index, prob, pool, stats


def born_pool_merge(index_a: torch.Tensor, prob_a: Optional[torch.Tensor], pool_a: torch.Tensor,
                    index_b: torch.Tensor, prob_b: Optional[torch.Tensor], pool_b: torch.Tensor,
                    v: torch.Tensor, *, workspace: Optional[torch.Tensor] = None):
    """Fold reservoir B into reservoir A in place (include/tneqhip.h, tq_born_pool_merge): slot j is
    taken from B iff A is empty or ``v[j] * (W_a + W_b) < W_b``; ``pool_a`` becomes the sums and the
    number of slots taken.  An empty B (``pool_b[0]`` not a finite number > 0) changes nothing but
    ``pool_a[3] = 0``; B is never modified.  ``prob_a`` and ``prob_b`` are both None or neither.
    ``workspace``: at least ``TQ_BORN_POOL_MERGE_WORKSPACE`` (64) bytes, allocated when not given.
    Runs on the current stream of A's device.  Returns ``(index_a, prob_a, pool_a)``."""
    who = "born_pool_merge"
    if not isinstance(index_a, torch.Tensor):
        raise ValueError(f"{who}: index_a must be a tensor")
    dev = _require_device(index_a)
    nd = index_a.numel()
    if index_a.ndim != 1 or nd < 1:
        raise ValueError(f"{who}: index_a must be a 1-D tensor of at least one slot")
    if (prob_a is None) != (prob_b is None):
        raise ValueError(f"{who}: prob_a and prob_b are both None or neither")
    _pool_buf(who, index_a, nd, torch.int64, "index_a", dev)
    _pool_buf(who, index_b, nd, torch.int64, "index_b", dev)
    if prob_a is not None:
        _pool_buf(who, prob_a, nd, torch.float64, "prob_a", dev)
        _pool_buf(who, prob_b, nd, torch.float64, "prob_b", dev)
    _pool_buf(who, pool_a, 4, torch.float64, "pool_a", dev)
    _pool_buf(who, pool_b, 4, torch.float64, "pool_b", dev)
    _pool_buf(who, v, nd, torch.float64, "v", dev)
    if workspace is None:
        workspace = torch.empty(_lib.TQ_BORN_POOL_MERGE_WORKSPACE, dtype=torch.uint8, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"{who}: workspace must be a contiguous tensor on the reservoirs' device")
    vp = ctypes.c_void_p
    rc = _lib.lib().tq_born_pool_merge(nd, vp(v.data_ptr()), vp(index_a.data_ptr()),
                                       vp(prob_a.data_ptr() if prob_a is not None else None), vp(pool_a.data_ptr()),
                                       vp(index_b.data_ptr()), vp(prob_b.data_ptr() if prob_b is not None else None),
                                       vp(pool_b.data_ptr()), vp(workspace.data_ptr()),
                                       workspace.numel() * workspace.element_size(), vp(_stream_ptr(dev)))
    check(rc, "tq_born_pool_merge")
    return index_a, prob_a, pool_a


def born_topk_workspace_size(dtype: torch.dtype, n: int, k: int) -> int:
    """Bytes of device workspace one ``born_topk`` call of these sizes needs (host only)."""
    wsb = _lib.lib().tq_born_topk_workspace(dtype_code(dtype), int(n), int(k))
    if wsb == 0:
        raise ValueError(f"born_topk: {_lib.last_error()}")
    return int(wsb)


def born_topk(amps: torch.Tensor, k: int, *, axis_qubit: Optional[Sequence[int]] = None, base: int = 0,
              out: Optional[torch.Tensor] = None, prob: Optional[torch.Tensor] = None,
              count: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """The ``k`` most probable elements of the amplitude block ``amps`` (complex64 / complex128,
    contiguous, any shape, on the HIP device): the elements with ``p_i = re^2 + im^2 > 0``
    (float64; +inf counts, NaN and 0 never) ordered by p descending and by index ascending among
    equal p (include/tneqhip.h, tq_born_topk).  Exact and bitwise reproducible.  Runs on the
    current stream of ``amps``' device; no host copy, no synchronisation.

    ``axis_qubit`` and ``base`` turn every index into a bitstring word as in ``born_sample``.
    ``out`` (int64), ``prob`` (float64), both 1-D of exactly ``k`` elements, ``count`` (int64,
    (1,)) and ``workspace`` (at least ``born_topk_workspace_size`` bytes) are allocated when not
    given.  Returns ``(index_or_words, prob, count)``: with m = min(k, number of candidates) the
    first m entries are the selection, the rest is -1 / 0, and ``count[0] = m``."""
    if not isinstance(amps, torch.Tensor):
        raise ValueError("born_topk: amps must be a tensor")
    dev = _require_device(amps)
    if amps.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"born_topk: amplitudes must be complex64 / complex128, got {amps.dtype}")
    if not amps.is_contiguous():
        raise ValueError("born_topk: amplitudes must be contiguous")
    n, k = amps.numel(), int(k)
    code = dtype_code(amps.dtype)
    wsb = born_topk_workspace_size(amps.dtype, n, k)

    def _buf(t, size, dtype, what):
        if t is None:
            return torch.empty(size, dtype=dtype, device=dev)
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or t.ndim != 1
                or not t.is_contiguous() or t.numel() != size):
            raise ValueError(f"born_topk: {what} must be a contiguous 1-D {dtype} tensor of {size} elements on {dev}")
        return t

    out = _buf(out, k, torch.int64, "out")
    prob = _buf(prob, k, torch.float64, "prob")
    count = _buf(count, 1, torch.int64, "count")
    if workspace is None:
        workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("born_topk: workspace must be a contiguous tensor on the amplitudes' device")
    base = int(base)
    if not 0 <= base < (1 << 64):
        raise ValueError("born_topk: base must fit 64 bits")
    if axis_qubit is not None:
        axes = [int(q) for q in axis_qubit]
        if any(not -(1 << 31) <= q < (1 << 31) for q in axes):
            raise ValueError("born_topk: axis qubit out of range")
        n_axes, table = len(axes), i32(axes)
    else:
        n_axes, table = 0, None
    rc = _lib.lib().tq_born_topk(code, n, ctypes.c_void_p(amps.data_ptr()), k,
                                 ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(prob.data_ptr()),
                                 ctypes.c_void_p(count.data_ptr()), n_axes, table, base,
                                 ctypes.c_void_p(workspace.data_ptr()),
                                 workspace.numel() * workspace.element_size(),
                                 ctypes.c_void_p(_stream_ptr(dev)))
    check(rc, "tq_born_topk")
    return out, prob, count


class _FidelityLoss(torch.autograd.Function):
    """L = 1 - |<t, o>|^2 / max(<t, t> <o, o>, 1e-12) (symmetry_breaking_quantum.py:220-229):
    one launch forward (tq_fidelity_forward), one backward (tq_fidelity_backward); the target
    gets no gradient (it is a constant of the fit)."""

    @staticmethod
    def forward(ctx, out_f, tgt_f):
        dev = _require_device(out_f, tgt_f)
        o = out_f.contiguous()
        t = tgt_f.contiguous()
        stats = torch.empty(4, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=o.real.dtype, device=dev)
        check(_lib.lib().tq_fidelity_forward(dtype_code(o.dtype), o.numel(), ctypes.c_void_p(t.data_ptr()),
                                             ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                                             ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(_stream_ptr(dev))),
              "tq_fidelity_forward")
        ctx.save_for_backward(o, t, stats)
        return loss

    @staticmethod
    def backward(ctx, g):
        o, t, stats = ctx.saved_tensors
        dev = o.device
        gg = g.to(dtype=o.real.dtype).contiguous()
        grad = torch.empty_like(o)
        check(_lib.lib().tq_fidelity_backward(dtype_code(o.dtype), o.numel(), ctypes.c_void_p(t.data_ptr()),
                                              ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                                              ctypes.c_void_p(gg.data_ptr()), ctypes.c_void_p(grad.data_ptr()),
                                              ctypes.c_void_p(_stream_ptr(dev))), "tq_fidelity_backward")
        return grad, None


def fidelity_loss(out: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The symmetry-breaking fit's loss 1 - |<target, out>|^2 / max(<target, target> <out, out>,
    1e-12) over the flattened tensors (symmetry_breaking_quantum.py:220-229: vdot, abs()**2,
    clamp_min, 1 - num/den), differentiable w.r.t. ``out``; complex64 / complex128 on the HIP
    device.  Returns a 0-d real tensor."""
    if out.dtype not in (torch.complex64, torch.complex128) or target.dtype != out.dtype:
        raise ValueError(f"fidelity_loss: complex64 / complex128 operands of one dtype (got {out.dtype}, {target.dtype})")
    if out.numel() != target.numel():
        raise ValueError(f"fidelity_loss: {out.numel()} vs {target.numel()} elements")
    if target.requires_grad:
        raise ValueError("fidelity_loss: the target is a constant (no gradient)")
    return _FidelityLoss.apply(out.reshape(-1), target.reshape(-1))
