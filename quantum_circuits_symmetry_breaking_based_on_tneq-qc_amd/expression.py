"""HipContractExpression: the drop-in for ``opt_einsum.contract_expression(eq, *shapes)``.

The reference builds one einsum equation per network and evaluates it with
``opt_einsum.contract_expression(eq, *shapes, optimize=...)`` followed by ``expr(*tensors)``
(tneq_qc/contractor/einsum_strategy.py:622-643; symmetry_breaking_quantum.py:142-144, 213-221;
executed through ComputeBackend.execute_expression, backend_interface.py:102-114).  Here the same
call shape returns an object whose ``__call__`` runs the whole pairwise tree on the MI355X through
one native plan (libtneqhip ``tq_plan_*``): intermediates live in a preallocated HBM arena, every
pairwise step is lowered to APPLY / permute+MFMA-GEMM kernels on the current torch stream.
Index slicing is a first-class option: ``slices=[symbols]`` removes those
contracted symbols from the inputs and sums the sub-contractions.
"""
from __future__ import annotations

import ctypes
import math
import operator
import threading
import weakref
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, graphs
from ._lib import check, i32, i64
from .einsum import (Network, _State, greedy_path, linear_path, parse_equation, path_info,
                     validate_path)
from .ops import dtype_code

PathSpec = Union[str, Sequence[Tuple[int, int]]]


class NativePlan:
    """Owner of one ``tq_plan`` (compiled for a dtype + input strides; arena allocated lazily)."""

    def __init__(self, net: Network, path: Sequence[Tuple[int, int]], dtype: torch.dtype,
                 strides: Optional[Sequence[Sequence[int]]], sliced: Sequence[int]):
        L = _lib.lib()
        graphs.drain_deferred()
        ranks = [len(t) for t in net.terms]
        modes = [m for t in net.terms for m in t]
        exts = [net.extents[m] for t in net.terms for m in t]
        st = None
        if strides is not None:
            st = i64([s for ss in strides for s in ss])
        flat_path = [x for p in path for x in p]
        h = ctypes.c_void_p()
        rc = L.tq_plan_create(ctypes.byref(h), dtype_code(dtype), len(net.terms), i32(ranks),
                              i32(modes), i64(exts), st, len(net.out), i32(net.out), len(path),
                              i32(flat_path), len(sliced), i32(sliced))
        check(rc, "tq_plan_create")
        self._h = h
        self.dtype = dtype
        self.n_slices = self.query("n_slices")

    def query(self, key: str) -> int:
        return int(_lib.lib().tq_plan_query(self._h, key.encode()))

    def clone(self) -> "NativePlan":
        """A copy of this compiled plan with its own device state (arena, tables, graphs): one per
        stream or block in flight, without compiling the network again (tq_plan_clone)."""
        graphs.drain_deferred()
        h = ctypes.c_void_p()
        check(_lib.lib().tq_plan_clone(self._h, ctypes.byref(h)), "tq_plan_clone")
        p = NativePlan.__new__(NativePlan)
        p._h = h
        p.dtype = self.dtype
        p.n_slices = self.n_slices
        return p

    def set(self, key: str, value: int) -> None:
        """Plan option (tq_plan_set): "graph" (replay a captured hipGraph, default 1),
        "sweep_chain" (chain launches of small dependent sweep2 ops, default 1), "sweep_coop"
        (cooperative launches of dependent multi-chunk sweep2 levels, default 0 = TQ_S2_COOP;
        diagnostic, measured slower), "s2_programs" (sweep2 block passes as compile-time pass
        programs, default 1 = TQ_S2_PROG; before the first execute), "fold_slices" (a call over
        every slice runs the plan's whole program instead of the slice lanes when that costs no
        more, default 1 = TQ_FOLD_SLICES; before the first execute)."""
        check(_lib.lib().tq_plan_set(self._h, key.encode(), int(value)), "tq_plan_set")

    def set_volatile(self, input_ids: Optional[Sequence[int]]) -> None:
        """Declare the inputs whose contents may change between two execute calls
        (tq_plan_set_volatile; None: every input, the default); before the first execute.  What
        the other inputs' subtrees hold is then computed by the first call only and kept."""
        if input_ids is None:
            rc = _lib.lib().tq_plan_set_volatile(self._h, -1, None)
        else:
            ids = [int(i) for i in input_ids]
            rc = _lib.lib().tq_plan_set_volatile(self._h, len(ids), i32(ids))
        check(rc, "tq_plan_set_volatile")

    def describe(self) -> str:
        L = _lib.lib()
        n = L.tq_plan_describe(self._h, None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        L.tq_plan_describe(self._h, buf, n + 1)
        return buf.value.decode()

    @staticmethod
    def pointer_array(ptrs: Sequence[int]):
        return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)

    def execute(self, ptrs, out_ptr: int, stream: int, begin: int = 0,
                end: Optional[int] = None, step: int = 1, accumulate: bool = False) -> None:
        """`ptrs`: the input base pointers (a sequence of ints, or an array from pointer_array)."""
        end = self.n_slices if end is None else end
        if graphs._DEFERRED:
            graphs.drain_deferred()
        arr = ptrs if isinstance(ptrs, ctypes.Array) else self.pointer_array(ptrs)
        rc = _lib.lib().tq_plan_execute(self._h, arr, ctypes.c_void_p(out_ptr), begin, end, step,
                                        int(accumulate), ctypes.c_void_p(stream))
        check(rc, "tq_plan_execute")

    @staticmethod
    def execute_group(plans: Sequence["NativePlan"], ptr_arrays, out_ptrs: Sequence[int], stream: int,
                      begin: int = 0, end: Optional[int] = None, step: int = 1, accumulate: bool = False) -> None:
        """Run plans compiled from the same network in lockstep on one stream (blocks as lanes:
        tq_plan_execute_group); ptr_arrays[k] / out_ptrs[k] are member k's inputs / output."""
        n = len(plans)
        if n == 0:
            return
        end = plans[0].n_slices if end is None else end
        if graphs._DEFERRED:
            graphs.drain_deferred()
        hs = (ctypes.c_void_p * n)(*[p._h for p in plans])
        arrs = [a if isinstance(a, ctypes.Array) else NativePlan.pointer_array(a) for a in ptr_arrays]
        ins = (ctypes.POINTER(ctypes.c_void_p) * n)(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) for a in arrs])
        outs = (ctypes.c_void_p * n)(*[int(o) for o in out_ptrs])
        rc = _lib.lib().tq_plan_execute_group(n, hs, ins, outs, begin, end, step, int(accumulate),
                                              ctypes.c_void_p(stream))
        check(rc, "tq_plan_execute_group")

    def profile(self, kinds=-1) -> None:
        """Reset the records and time (HIP events on the execution stream) the op kinds in
        `kinds` (one _lib.TQ_OP_* or an iterable of them; -1 = all; None / [] = off)."""
        if kinds is None:
            mask = 0
        elif isinstance(kinds, int):
            mask = -1 if kinds == -1 else (1 << kinds)
        else:
            mask = 0
            for k in kinds:
                mask |= 1 << int(k)
        check(_lib.lib().tq_plan_profile(self._h, int(mask)), "tq_plan_profile")

    def profile_read(self, op_kind: int = -1) -> dict:
        """Summed event time / launches / algorithmic flops and bytes of one op kind
        (_lib.TQ_OP_GEMM, TQ_OP_APPLY, TQ_OP_PERMUTE; -1 = all) since the last reset."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        fl, by = ctypes.c_double(), ctypes.c_double()
        check(_lib.lib().tq_plan_profile_read(self._h, op_kind, ctypes.byref(ms), ctypes.byref(n),
                                              ctypes.byref(fl), ctypes.byref(by)), "tq_plan_profile_read")
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}

    def release_now(self) -> None:
        """Destroy the native plan; inside a stream capture (HIP refuses graph / memory releases
        then) or when HIP refuses, the handle is parked and released after the capture
        (graphs.drain_deferred)."""
        h = getattr(self, "_h", None)
        if h is None or _lib._lib is None:
            return
        if graphs.capturing() or _lib._lib.tq_plan_destroy(h) != 0:
            graphs.defer_release(_PlanHandle(h))
        self._h = None

    def __del__(self):
        # a finalizer may run while ANOTHER thread holds a global-mode capture (which a destroy's
        # hipEventSynchronize / hipGraphExecDestroy / hipFree would invalidate, and the current
        # stream's capture state does not show): the handle is always parked and released at the
        # next drain point (plan creation / execution, the end of our own captures) -- ADVICE r5
        try:
            h = getattr(self, "_h", None)
            if h is not None and _lib._lib is not None:
                graphs.defer_release(_PlanHandle(h))
            self._h = None
        except Exception:  # interpreter shutdown: modules may already be gone
            pass


class _PlanHandle:
    """A native plan handle whose destroy was deferred (NativePlan.release_now)."""

    def __init__(self, h):
        self._h = h

    release_now = NativePlan.release_now


class HipContractExpression:
    """Callable contraction of a fixed einsum equation over fixed shapes on the HIP engine.

    ``optimize``: 'greedy' / 'auto' (opt_einsum's greedy rule), 'linear' (sweep with `order`
    hint), or an explicit SSA path [(i, j), ...].  ``slices``: symbols (or mode ids) to slice.
    """

    def __init__(self, eq: str, *shapes, optimize: PathSpec = "greedy",
                 order: Optional[Sequence[int]] = None, slices: Sequence = ()):
        self.eq = eq
        self.shapes = [tuple(int(x) for x in s) for s in shapes]
        self.net = parse_equation(eq, self.shapes)
        n = len(self.net.terms)
        if isinstance(optimize, str):
            if optimize in ("greedy", "auto", "optimal", "dp", "branch-2", "random-greedy"):
                self.path = greedy_path(self.net) if n > 1 else []
            elif optimize == "linear":
                self.path = linear_path(self.net, order)[0] if n > 1 else []
            else:
                raise ValueError(f"unknown optimize={optimize!r}")
        else:
            self.path = [tuple(int(x) for x in p) for p in optimize]
        validate_path(n, self.path)
        sym2id = {s: i for i, s in enumerate(self.net.symbols)}
        self.sliced = [sym2id[s] if isinstance(s, str) else int(s) for s in slices]
        for m in self.sliced:
            if m in self.net.out:
                raise ValueError("cannot slice an output symbol")
        self.n_slices = 1
        for m in self.sliced:
            self.n_slices *= self.net.extents[m]
        self._plans: Dict[tuple, NativePlan] = {}
        self._lock = threading.Lock()
        self._bound = None   # operands of the last call (see _forward's fast path)

    # -- introspection ---------------------------------------------------------------------
    @property
    def out_shape(self) -> Tuple[int, ...]:
        return tuple(self.net.extents[m] for m in self.net.out)

    def info(self):
        return path_info(self.net, self.path, self.sliced)

    def plan(self, dtype: torch.dtype, strides=None, device: Optional[int] = None) -> NativePlan:
        """The native plan for (dtype, input strides, device).  A plan's arena, tables and graphs
        live on the device that was current at its first execute; the library refuses to run it
        with another device current, so plans are keyed by device.  One plan serves one stream
        at a time (its arena is shared by its launches)."""
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else -1
        key = (dtype, None if strides is None else tuple(tuple(s) for s in strides), int(device))
        p = self._plans.get(key)
        if p is None:
            with self._lock:
                p = self._plans.get(key)
                if p is None:
                    p = NativePlan(self.net, self.path, dtype, strides, self.sliced)
                    self._plans[key] = p
        return p

    # -- execution ---------------------------------------------------------------------------
    def bind(self, *tensors, private_plan: bool = False, volatile: Optional[Sequence[int]] = None) -> "BoundOperands":
        """Validate `tensors` once (shapes, device, dtype, strides) and return the plan bound to
        their storage.  The binding reads whatever values those tensors hold when it runs, so an
        owner that updates operand VALUES in place (a sampler's projector vectors) runs it again
        without re-validation; the tensors themselves must stay alive and keep their storage,
        shapes and strides (the binding holds references to them).  `private_plan`: a clone of
        the expression's plan owned by this binding (one per stream / block in flight).
        `volatile` (private plans only): the operands whose values the owner changes between
        runs (NativePlan.set_volatile); it must not write the others without `invalidate()`."""
        if volatile is not None and not private_plan:
            raise ValueError("bind(volatile=...) needs private_plan=True (the shared plan serves other callers)")
        if len(tensors) != len(self.net.terms):
            raise ValueError(f"expression takes {len(self.net.terms)} operands, got {len(tensors)}")
        ts = list(tensors)
        for t, s in zip(ts, self.shapes):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
                raise ValueError("bind() takes device tensors")
            if tuple(t.shape) != s:
                raise ValueError(f"operand shape {tuple(t.shape)} does not match expression shape {s}")
            if t.is_conj() or t.is_neg() or any(st < 0 for st in t.stride()):
                raise ValueError("bind() takes plain (non-conjugated, non-negative-stride) tensors")
        dt = ts[0].dtype
        dev = ts[0].device
        for t in ts:
            if t.dtype != dt or t.device != dev:
                raise ValueError("bind() takes operands of one dtype on one device")
        dtype_code(dt)
        contiguous = all(t.is_contiguous() for t in ts)
        plan = self.plan(dt, None if contiguous else [t.stride() for t in ts], dev.index)
        if private_plan:
            plan = plan.clone()
            if volatile is not None:
                plan.set_volatile(volatile)
        return BoundOperands(self, plan, plan.pointer_array([t.data_ptr() for t in ts]), tuple(ts), dev, dt)

    def __call__(self, *tensors, out: Optional[torch.Tensor] = None, slice_range=None,
                 accumulate: bool = False, backend=None) -> torch.Tensor:
        if (torch.is_grad_enabled() and out is None
                and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)):
            if slice_range is None or not self.sliced:
                return _HipContractFn.apply(self, *tensors)
            return self._sliced_autograd(tensors, slice_range)
        return self._forward(*tensors, out=out, slice_range=slice_range, accumulate=accumulate)

    # -- differentiable slice ranges ---------------------------------------------------------
    def slice_expression(self) -> "HipContractExpression":
        """The network of ONE slice: every sliced mode removed from the terms, same SSA path."""
        hit = self._plans.get("slice_expr")
        if hit is None:
            sym = self.net.symbols
            sl = set(self.sliced)
            terms = ["".join(sym[m] for m in t if m not in sl) for t in self.net.terms]
            shapes = [tuple(self.net.extents[m] for m in t if m not in sl) for t in self.net.terms]
            eq = ",".join(terms) + "->" + "".join(sym[m] for m in self.net.out)
            hit = HipContractExpression(eq, *shapes, optimize=self.path if self.path else "greedy")
            self._plans["slice_expr"] = hit
        return hit

    def slice_values(self, s: int) -> Dict[int, int]:
        """Mode values of slice `s`: row-major over the sliced modes, last fastest (the
        enumeration of tq_plan_execute)."""
        vals, rem = {}, int(s)
        for m in reversed(self.sliced):
            vals[m] = rem % self.net.extents[m]
            rem //= self.net.extents[m]
        if rem:
            raise ValueError("slice id out of range")
        return vals

    def _sliced_autograd(self, tensors, slice_range) -> torch.Tensor:
        """Differentiable sum of the slices `slice_range` = (begin, end, step): each slice is the
        one-slice expression (autograd through its reverse tree) applied to `select` views of the
        operands, so the gradient of an operand that carries a sliced mode lands in exactly the
        entries its slices read (the reference differentiates its K-sharded partial contraction the
        same way, distributed_engine.py:1474-1497)."""
        begin, end, step = slice_range
        end = self.n_slices if end is None else end
        sub = self.slice_expression()
        total = None
        for s in range(begin, end, step):
            vals = self.slice_values(s)
            views = []
            for t, term in zip(tensors, self.net.terms):
                v = t
                for ax in reversed(range(len(term))):
                    if term[ax] in vals:
                        v = v.select(ax, vals[term[ax]])
                views.append(v)
            r = sub(*views)
            total = r if total is None else total + r
        if total is None:
            dt = tensors[0].dtype
            for t in tensors[1:]:
                dt = torch.promote_types(dt, t.dtype)
            dev = next((t.device for t in tensors if t.device.type == "cuda"), tensors[0].device)
            total = torch.zeros(self.out_shape, dtype=dt, device=dev)
        return total

    def reverse_tree(self, dtype: torch.dtype = torch.complex64) -> "_ReverseTree":
        """The per-step forward / gradient expressions used by autograd (built once per dtype:
        the in-place mode orders are chosen from that dtype's step plans)."""
        key = ("reverse", dtype)
        rev = self._plans.get(key)
        if rev is None:
            with self._lock:
                rev = self._plans.get(key)
                if rev is None:
                    rev = _ReverseTree(self, dtype)
                    self._plans[key] = rev
        return rev

    def grad_expression(self, i: int) -> Tuple["HipContractExpression", List[int]]:
        """Expression for d(out)/d(operand i) contracted with grad_out:
        operands = the other inputs (conjugated by the caller) + grad_out -> operand i's modes.
        Modes only present in operand i are broadcast afterwards (returned as positions)."""
        key = ("grad", i)
        hit = self._plans.get(key)
        if hit is not None:
            return hit
        sym = self.net.symbols
        others = [j for j in range(len(self.net.terms)) if j != i]
        present = set(self.net.out)
        for j in others:
            present |= set(self.net.terms[j])
        term_i = self.net.terms[i]
        kept = [m for m in term_i if m in present]
        bcast = [k for k, m in enumerate(term_i) if m not in present]
        eq = ",".join("".join(sym[m] for m in self.net.terms[j]) for j in others)
        eq += ("," if others else "") + "".join(sym[m] for m in self.net.out)
        eq += "->" + "".join(sym[m] for m in kept)
        shapes = [self.shapes[j] for j in others] + [self.out_shape]
        g = HipContractExpression(eq, *shapes, optimize="greedy")
        self._plans[key] = (g, bcast)
        return g, bcast

    def _bound_call(self, tensors):
        """(plan, pointer array, device, dtype) when `tensors` are the very objects of the last
        validated call, unmodified since: same data pointers, strides, shapes and version
        counters (every in-place op, the metadata ones included, bumps them; a lazy conj / neg
        bit cannot appear on an existing tensor object except through ``.data`` reassignment,
        which -- as for autograd's version checks -- is not tracked).  A network of hundreds of
        cores (C4: 606 operands) is then re-bound in ~0.3 ms instead of the ~2 ms per-operand
        conversion + validation pass."""
        b = self._bound
        if b is None or len(tensors) != len(b[0]):
            return None
        objs, vers, ptrs, strides, shapes, hit = b
        if not all(r() is t for r, t in zip(objs, tensors)):
            return None
        if ([t._version for t in tensors] != vers or [t.data_ptr() for t in tensors] != ptrs
                or [t.stride() for t in tensors] != strides or [t.shape for t in tensors] != shapes):
            return None
        return hit

    def _forward(self, *tensors, out: Optional[torch.Tensor] = None, slice_range=None,
                 accumulate: bool = False) -> torch.Tensor:
        hit = self._bound_call(tensors)
        if hit is not None:
            plan, arr, dev, dt = hit
            return self._run(plan, arr, dev, dt, out, slice_range, accumulate)
        if len(tensors) != len(self.net.terms):
            raise ValueError(f"expression takes {len(self.net.terms)} operands, got {len(tensors)}")
        ts = [t if isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in tensors]
        for t, s in zip(ts, self.shapes):
            if tuple(t.shape) != s:
                raise ValueError(f"operand shape {tuple(t.shape)} does not match expression shape {s}")
        dev = next((t.device for t in ts if t.device.type == "cuda"), None)
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        dt = ts[0].dtype
        for t in ts[1:]:
            dt = torch.promote_types(dt, t.dtype)
        dtype_code(dt)
        # torch's lazy conj/neg bits are not visible through data_ptr(): materialise them
        ts = [t.to(device=dev, dtype=dt).resolve_conj().resolve_neg() for t in ts]
        # views with odd strides are fine (the plan reads through strides); negative/overlap not
        ts = [t if all(s >= 0 for s in t.stride()) else t.contiguous() for t in ts]
        strides = [t.stride() for t in ts]
        contiguous = all(t.is_contiguous() for t in ts)
        plan = self.plan(dt, None if contiguous else strides, dev.index)
        ptrs = [t.data_ptr() for t in ts]
        arr = plan.pointer_array(ptrs)
        # remembered only when the plan reads the caller's own tensors (no converted copies)
        if all(map(operator.is_, ts, tensors)):
            # weak references: the binding does not keep the caller's operands alive
            self._bound = (tuple(map(weakref.ref, ts)), [t._version for t in ts], ptrs, strides,
                           [t.shape for t in ts], (plan, arr, dev, dt))
        else:
            self._bound = None
        return self._run(plan, arr, dev, dt, out, slice_range, accumulate)

    def _run(self, plan: NativePlan, arr, dev, dt, out, slice_range, accumulate) -> torch.Tensor:
        if out is None:
            out = torch.empty(self.out_shape, dtype=dt, device=dev)
            accumulate = False
        elif (tuple(out.shape) != self.out_shape or out.dtype != dt or not out.is_contiguous()
              or out.device != dev):
            raise ValueError("out tensor has the wrong shape/dtype/device or is not contiguous")
        begin, end, step = (0, plan.n_slices, 1) if slice_range is None else slice_range
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            plan.execute(arr, out.data_ptr(), stream, begin, end, step, accumulate)
        return out


class BoundOperands:
    """An expression's native plan bound to fixed operand storage (HipContractExpression.bind)."""

    __slots__ = ("expr", "plan", "arr", "tensors", "device", "dtype")

    def __init__(self, expr, plan, arr, tensors, device, dtype):
        self.expr, self.plan, self.arr, self.tensors, self.device, self.dtype = expr, plan, arr, tensors, device, dtype

    def new_out(self) -> torch.Tensor:
        return torch.empty(self.expr.out_shape, dtype=self.dtype, device=self.device)

    def invalidate(self) -> None:
        """Forget what the plan keeps of its non-volatile operands (bind(volatile=...)): call it
        after writing into one of them in place; the next run computes those results again."""
        self.plan.set("frozen_valid", 0)

    def _check_out(self, out: torch.Tensor) -> None:
        if (tuple(out.shape) != self.expr.out_shape or out.dtype != self.dtype or not out.is_contiguous()
                or out.device != self.device):
            raise ValueError("out tensor has the wrong shape/dtype/device or is not contiguous")

    def run(self, out: torch.Tensor, stream: Optional[torch.cuda.Stream] = None, slice_range=None) -> torch.Tensor:
        """Contract into `out` on `stream` (default: the current stream)."""
        self._check_out(out)
        begin, end, step = (0, self.plan.n_slices, 1) if slice_range is None else slice_range
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        with torch.cuda.device(self.device):
            self.plan.execute(self.arr, out.data_ptr(), s, begin, end, step, False)
        return out


def run_group(bound: Sequence[BoundOperands], outs: Sequence[torch.Tensor],
              stream: Optional[torch.cuda.Stream] = None, slice_range=None) -> None:
    """Contract every member of `bound` (one network, distinct plans: e.g. the same expression
    compiled once per block) into its own output in ONE lockstep schedule (tq_plan_execute_group:
    blocks as lanes)."""
    if len(bound) != len(outs):
        raise ValueError("one output per bound member")
    if not bound:
        return
    for b, o in zip(bound, outs):
        b._check_out(o)
    plans = [b.plan for b in bound]
    if len({id(p) for p in plans}) != len(plans):
        raise ValueError("run_group members need distinct plans (one expression per member)")
    dev = bound[0].device
    begin, end, step = (0, plans[0].n_slices, 1) if slice_range is None else slice_range
    s = (stream or torch.cuda.current_stream(dev)).cuda_stream
    with torch.cuda.device(dev):
        NativePlan.execute_group(plans, [b.arr for b in bound], [o.data_ptr() for o in outs], s, begin, end, step)


def _in_place_order(mi, mj, res, ext):
    """Mode order of a pairwise result written in place into the larger operand's layout: its
    kept modes where they are, the smaller operand's new modes at the first contracted one."""
    size = lambda ms: math.prod(ext[m] for m in ms)
    big, small = (mi, mj) if size(mi) >= size(mj) else (mj, mi)
    keep = set(res)
    new = [m for m in small if m in keep and m not in big]
    out, put = [], False
    for m in big:
        if m in keep:
            out.append(m)
        elif not put:
            out.extend(new)
            put = True
    if not put:
        out.extend(new)
    return tuple(out) if set(out) == keep and len(out) == len(keep) else None


def _writes_through_permute(e: "HipContractExpression", dtype: torch.dtype) -> bool:
    """True when the step's plan for `dtype` ends with a permute of its result into the
    requested order (the plan is kept: the runtime of that dtype reuses it)."""
    return "result->out" in e.plan(dtype).describe()


class _ReverseTree:
    """Reverse-mode differentiation through the expression's pairwise path.

    The reference differentiates ``oe.contract_expression(...)(*params)`` with torch autograd
    (symmetry_breaking_quantum.py:210-224; engine_siamese.py:351-554): the forward keeps every
    pairwise intermediate and the backward runs two contractions per pairwise step.  Same here,
    on the HIP engine.  Step s contracts T_i, T_j -> T_k (one small native plan).  The backward
    propagates conjugated gradients h = conj(dL/dT) (torch's complex convention
    dT_i = dT_k . conj(T_j) becomes a plain contraction h_i = h_k . T_j), so every backward step
    is one plain contraction: modes of T_i that neither T_k nor T_j carry (summed inside the step)
    come back through a ones vector operand.  Cost: two pairwise steps per step instead of one
    full-network contraction per operand.

    Runtime (_TreeRuntime): intermediates and gradients live in static buffers per (dtype,
    device, stream) -- two streams running one expression concurrently do not share them; the
    step plans launch eagerly and, once an input-pointer set repeats (a training loop updating
    its parameters in place), the whole forward / backward launch sequence is captured once into
    a hipGraph (torch.cuda.CUDAGraph) and replayed."""

    _MAX_RUNTIMES = 4   # per tree: (device, stream) pairs kept, least recently used dropped

    def __init__(self, expr: "HipContractExpression", dtype: torch.dtype = torch.complex64):
        self.dtype = dtype
        net = expr.net
        sym = net.symbols
        st = _State(net)
        ext = net.extents
        self.ext = ext
        self.n_in = len(net.terms)
        self.modes: Dict[int, Tuple[int, ...]] = {i: tuple(t) for i, t in enumerate(net.terms)}
        self.steps = []
        last = len(expr.path) - 1
        s2 = lambda ms: "".join(sym[m] for m in ms)
        shp = lambda ms: tuple(ext[m] for m in ms)
        fsteps = []
        for s, (i, j) in enumerate(expr.path):
            res = st.result(i, j)
            if s == last:
                res = tuple(net.out)      # the final step writes the output's mode order
            k = st.contract(i, j)
            mi, mj = self.modes[i], self.modes[j]
            fwd = None
            if s != last:
                # an intermediate's mode order is free: prefer the one the step's kernel writes in
                # place (a small operand absorbed into a large one: its new modes where the
                # contracted ones were), which saves the step's output permute
                nat = _in_place_order(mi, mj, res, ext)
                if nat is not None and nat != tuple(res):
                    cand = HipContractExpression(f"{s2(mi)},{s2(mj)}->{s2(nat)}", shp(mi), shp(mj),
                                                 optimize=[(0, 1)])
                    if not _writes_through_permute(cand, dtype):
                        fwd, res = cand, nat
            self.modes[k] = tuple(res)
            if fwd is None:
                fwd = HipContractExpression(f"{s2(mi)},{s2(mj)}->{s2(res)}", shp(mi), shp(mj), optimize=[(0, 1)])
            fsteps.append((i, j, k, fwd))
        # gradient (conjugated) of every node: the inputs' in their own order, an intermediate's in
        # the order its gradient step writes in place (chosen in reverse, consumers first)
        self.hmodes: Dict[int, Tuple[int, ...]] = {i: self.modes[i] for i in range(self.n_in)}
        if fsteps:
            self.hmodes[fsteps[-1][2]] = self.modes[fsteps[-1][2]]
        bwds = {}
        for (i, j, k, fwd) in reversed(fsteps):
            hk = self.hmodes[k]
            bwd = []
            for a, other in ((i, j), (j, i)):
                m_a, m_o = self.modes[a], self.modes[other]
                avail = set(hk) | set(m_o)
                extra = [m for m in m_a if m not in avail]          # broadcast back via ones
                terms = [s2(hk), s2(m_o)] + [sym[m] for m in extra]
                shapes = [shp(hk), shp(m_o)] + [(ext[m],) for m in extra]
                nt = 2 + len(extra)          # SSA path: (0, 1), then each ones vector joins
                path = [(0, 1)] + [(1 + t, nt + t - 1) for t in range(1, 1 + len(extra))]
                g = None
                h_a = m_a
                if a >= self.n_in and not extra:
                    nat = _in_place_order(hk, m_o, m_a, ext)
                    if nat is not None and nat != tuple(m_a):
                        cand = HipContractExpression(",".join(terms) + "->" + s2(nat), *shapes, optimize=path)
                        if not _writes_through_permute(cand, dtype):
                            g, h_a = cand, nat
                if g is None:
                    g = HipContractExpression(",".join(terms) + "->" + s2(m_a), *shapes, optimize=path)
                self.hmodes[a] = tuple(h_a)
                bwd.append((a, other, g, [ext[m] for m in extra]))
            bwds[k] = bwd
        for (i, j, k, fwd) in fsteps:
            self.steps.append((i, j, k, fwd, bwds[k]))
        self.final = self.n_in + len(expr.path) - 1 if expr.path else 0
        self.single = None
        if not expr.path:   # one operand: a transpose / single-side sum of it
            self.single = expr.grad_expression(0)
        self._rt: Dict[tuple, "_TreeRuntime"] = {}

    def runtime(self, dtype, device) -> "_TreeRuntime":
        """The static buffers / graphs of (dtype, device, current stream), a bounded LRU: each
        graphs.capture_step call brings a new stream, so older runtimes are dropped (a backward
        still holding one keeps it alive through its autograd context)."""
        key = (dtype, device.index, torch.cuda.current_stream(device).cuda_stream)
        rt = self._rt.pop(key, None)
        if rt is None:
            rt = _TreeRuntime(self, dtype, device)
            while len(self._rt) >= self._MAX_RUNTIMES:
                self._rt.pop(next(iter(self._rt)))
        self._rt[key] = rt
        return rt


class _TreeRuntime:
    _MAX_GRAPHS = 4
    _MAX_SEEN = 64     # pointer sets remembered for the capture-on-repeat rule

    def __init__(self, tree: _ReverseTree, dtype, device):
        self.tree, self.dtype, self.dev = tree, dtype, device
        self.stream = torch.cuda.current_stream(device).cuda_stream   # the stream it is keyed on
        t = tree
        shape = lambda n: tuple(t.ext[m] for m in t.modes[n])
        hshape = lambda n: tuple(t.ext[m] for m in t.hmodes[n])
        with torch.cuda.device(device):
            self.vals = {k: torch.empty(shape(k), dtype=dtype, device=device) for (_, _, k, _, _) in t.steps}
            # conjugated gradients: the inputs' in one flat buffer (one conj at the end), the
            # intermediates' separately
            sizes = [int(torch.Size(shape(i)).numel()) for i in range(t.n_in)]
            self.flat = torch.empty(sum(sizes), dtype=dtype, device=device)
            self.h: Dict[int, torch.Tensor] = {}
            off = 0
            for i, n in enumerate(sizes):
                self.h[i] = self.flat[off:off + n].view(shape(i))
                off += n
            for (_, _, k, _, _) in t.steps:
                self.h[k] = torch.empty(hshape(k), dtype=dtype, device=device)
            self.ones = {}
            for (_, _, _, _, bwd) in t.steps:
                for (_, _, _, exts) in bwd:
                    for e in exts:
                        if e not in self.ones:
                            self.ones[e] = torch.ones((e,), dtype=dtype, device=device)
            # step plans: eager launches (the sequence is captured as a whole)
            self.fplans = []
            self.bplans = []
            for (i, j, k, fwd, bwd) in t.steps:
                fp = fwd.plan(dtype, None, device.index)
                _lib.check(_lib.lib().tq_plan_set(fp._h, b"graph", 0), "tq_plan_set")
                self.fplans.append(fp)
                bp = []
                for (a, other, g, exts) in bwd:
                    pl = g.plan(dtype, None, device.index)
                    _lib.check(_lib.lib().tq_plan_set(pl._h, b"graph", 0), "tq_plan_set")
                    bp.append(pl)
                self.bplans.append(bp)
        self.gen = 0
        self.seen: Dict[tuple, int] = {}
        self.graphs: Dict[tuple, "torch.cuda.CUDAGraph"] = {}

    def __del__(self):
        # a finalizer may run inside a capture (this thread's or another's): HIP would refuse the
        # CUDAGraphs' destruction (hipGraphExecDestroy), so they are always parked until the next
        # drain point (the step plans park themselves, NativePlan.__del__)
        try:
            if getattr(self, "graphs", None):
                graphs.defer_release(self.graphs)
                self.graphs = {}
        except Exception:  # interpreter shutdown
            pass

    def _val(self, n, ins):
        return ins[n] if n < self.tree.n_in else self.vals[n]

    def _fwd_eager(self, ins):
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        for (i, j, k, _, _), pl in zip(self.tree.steps, self.fplans):
            pl.execute([self._val(i, ins).data_ptr(), self._val(j, ins).data_ptr()],
                       self.vals[k].data_ptr(), stream)

    def _bwd_eager(self, ins, need):
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        for (i, j, k, _, bwd), bps in zip(reversed(self.tree.steps), reversed(self.bplans)):
            if not need[k]:
                continue
            for (a, other, _, exts), pl in zip(bwd, bps):
                if not need[a]:
                    continue
                ptrs = [self.h[k].data_ptr(), self._val(other, ins).data_ptr()]
                ptrs += [self.ones[e].data_ptr() for e in exts]
                pl.execute(ptrs, self.h[a].data_ptr(), stream)

    def _run(self, kind, key, fn):
        """fn() eagerly; captured into a graph the second time `key` is seen, replayed after.
        Inside a caller's capture (a whole training step being captured, graphs.capture_step)
        the launches go straight into that capture."""
        if torch.cuda.is_current_stream_capturing():
            fn()
            return
        g = self.graphs.get(key)
        if g is not None:
            g.replay()
            return
        n = self.seen.get(key, 0) + 1
        if n == 1 and len(self.seen) >= self._MAX_SEEN:   # bounded: forget the oldest pointer set
            self.seen.pop(next(iter(self.seen)))
        self.seen[key] = n
        if n < 2 or _graphs_off():
            fn()
            return
        if len(self.graphs) >= self._MAX_GRAPHS:
            self.graphs.pop(next(iter(self.graphs)))
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.dev)
        from .graphs import gc_paused   # (no collection inside the capture: graphs.gc_paused)
        with gc_paused(), torch.cuda.graph(g):
            fn()
        self.graphs[key] = g
        graphs.drain_deferred()
        g.replay()

    def forward(self, ins):
        key = ("f",) + tuple(t.data_ptr() for t in ins)
        self._run("f", key, lambda: self._fwd_eager(ins))
        self.gen += 1
        return self.vals[self.tree.final]

    def backward(self, ins, grad_out, needs):
        t = self.tree
        need = {i: bool(needs[i]) for i in range(t.n_in)}
        for i, j, k, _, _ in t.steps:
            need[k] = need[i] or need[j]
        hf = self.h[t.final]
        g = grad_out.to(device=self.dev, dtype=self.dtype)
        if self.dtype.is_complex:
            torch.conj_physical(g.contiguous(), out=hf)
        else:
            hf.copy_(g)
        key = ("b",) + tuple(x.data_ptr() for x in ins) + tuple(need[i] for i in range(t.n_in))
        self._run("b", key, lambda: self._bwd_eager(ins, need))
        res = self.flat.conj_physical() if self.dtype.is_complex else self.flat.clone()
        out, off = [], 0
        for i in range(t.n_in):
            n = self.h[i].numel()
            out.append(res[off:off + n].view(self.h[i].shape) if need[i] else None)
            off += n
        return out


def _graphs_off() -> bool:
    import os
    return os.environ.get("TQ_GRAPH", "1") == "0"


class _HipContractFn(torch.autograd.Function):
    """Autograd for a HIP expression: reverse mode through the pairwise path (_ReverseTree),
    every step and its two gradient contractions on the HIP engine."""

    @staticmethod
    def forward(ctx, expr, *tensors):
        ts = [t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in tensors]
        ctx.expr = expr
        ctx.in_meta = [(t.dtype, t.device, tuple(t.shape)) for t in ts]
        dt = ts[0].dtype
        for t in ts[1:]:
            dt = torch.promote_types(dt, t.dtype)
        ctx.dt = dt
        rev = expr.reverse_tree(dt)
        with torch.no_grad():
            if rev.single is not None:
                ctx.save_for_backward(*ts)
                return expr._forward(*ts)
            dev = next((t.device for t in ts if t.device.type == "cuda"),
                       torch.device("cuda", torch.cuda.current_device()))
            dtype_code(dt)
            ins = [t.to(device=dev, dtype=dt).resolve_conj().resolve_neg().contiguous() for t in ts]
            for t, shp in zip(ins, expr.shapes):
                if tuple(t.shape) != shp:
                    raise ValueError(f"operand shape {tuple(t.shape)} does not match expression shape {shp}")
            rt = rev.runtime(dt, dev)
            with torch.cuda.device(dev):
                out = rt.forward(ins).clone()
        # saved through autograd: a second backward (retain_graph=True) finds them again, and an
        # in-place change of an input between forward and backward raises (version counter)
        ctx.save_for_backward(*ins)
        ctx.rt, ctx.gen = rt, rt.gen
        return out

    @staticmethod
    def backward(ctx, grad_out):
        expr = ctx.expr
        rev = expr.reverse_tree(ctx.dt)
        needs = list(ctx.needs_input_grad[1:])
        if rev.single is not None:
            (t,) = ctx.saved_tensors
            g_expr, bcast = rev.single
            g = g_expr._forward(grad_out.to(dtype=torch.promote_types(grad_out.dtype, t.dtype)))
            for k in bcast:
                g = g.unsqueeze(k)
            return (None, g.expand(t.shape).to(device=t.device, dtype=t.dtype))
        rt, ins = ctx.rt, list(ctx.saved_tensors)
        # (autograd runs this on the forward's stream: the runtime's own)
        with torch.cuda.device(rt.dev):
            if rt.gen != ctx.gen:        # another forward reused the static buffers: recompute
                rt.forward(ins)
                ctx.gen = rt.gen
            g = rt.backward(ins, grad_out, needs)
        out = [None]
        for gi, (dt, dev, shape), nd in zip(g, ctx.in_meta, needs):
            if not nd:
                out.append(None)
                continue
            if not dt.is_complex and gi.is_complex():
                gi = gi.real
            out.append(gi.to(device=dev, dtype=dt))
        return tuple(out)


def contract_expression(eq: str, *shapes, optimize: PathSpec = "greedy", **kw) -> HipContractExpression:
    """Same call shape as ``opt_einsum.contract_expression`` (einsum_strategy.py:639-643)."""
    return HipContractExpression(eq, *shapes, optimize=optimize, **kw)


def contract(eq: str, *tensors, optimize: PathSpec = "greedy", **kw) -> torch.Tensor:
    """One-shot einsum on the HIP engine (``opt_einsum.contract`` / ``torch.einsum`` drop-in)."""
    expr = HipContractExpression(eq, *[tuple(t.shape) for t in tensors], optimize=optimize, **kw)
    return expr(*tensors)
