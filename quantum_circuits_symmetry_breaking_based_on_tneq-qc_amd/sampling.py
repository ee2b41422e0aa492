"""Many amplitude blocks of one network: several in flight on one GPU, and several per launch.

An amplitude workload that samples more than one block of bitstrings ("shard
bitstrings instead of slices") contracts the same network again and again with other fixed bits:
only the closed qubits' projector operands change (circuits.with_batch), so one compiled plan
serves every block.  The sweeps of one block are latency-bound: a 2^19-element
level is one workgroup lifetime of dependent passes.  `BlockPipeline` fills the GPU two ways:

* **blocks as lanes** (`group`): G blocks contract in ONE lockstep schedule
  (`expression.run_group` -> `tq_plan_execute_group`): every sweep level of the G blocks is one
  kernel launch over G x the ops, so G blocks cost the launches, prologues and pass latencies of
  about one;
* **groups in flight** (`inflight`): consecutive groups run on their own HIP streams, each with
  its own plans (arenas), so one group's GEMM / permute / latency tails overlap another's sweeps.

Block k goes to member k mod G of slot (k div G) mod inflight; a slot's group is launched when
its last member is enqueued (or by `flush()`).  Block b's projector vectors come from a device
table built once (`blocks` given up front); a group launch first copies its members' rows into
the members' projector buffers on the slot's stream (one copy when the rows are consecutive).

Between two blocks only the projectors that differ somewhere in the block table change: the
pipeline declares exactly those volatile (`NativePlan.set_volatile`), so every member's plan
contracts the subtrees that hold none of them -- for consecutive `with_batch` indices below 2^17
on C4 the whole right half, its GEMM-operand producer included -- in its first launch only.

Operand contract: the pipeline OWNS its operands and binds every member's plan to them once
(`HipContractExpression.bind`, private plans): the projector buffers are updated IN PLACE between
launches (ordinary stream-ordered copies) and the bound plans read the new values at run time --
no re-validation of the 606 operands per block, and no `.data` rebinding trick.  Outputs are
written on the slot's stream: `wait()` (current stream waits) or `synchronize()` before reading.

`BlockSampler` is the consumer: a `BlockPipeline` whose every block is followed, on the slot's
stream, by one Born-rule sampling call (`ops.born_sample`, csrc/tq_born.hip), so `step()` hands
back bitstring words, their probabilities and the block's mass instead of 8 MB of amplitudes --
nothing is copied to the host.  `BlockTopK` is the other consumer (post-selection): the same
pipeline with one top-k call (`tq_born_topk`, csrc/tq_topk.hip) behind every block, handing back the
k most probable bitstrings of each.  `PoolSampler` samples ACROSS the blocks: one weighted
reservoir per slot that every block of the slot is folded into (`tq_born_pool_sample`), merged by
`result()` (`tq_born_pool_merge`) into draws from the distribution over everything contracted.

The product path is the native plan only (no CPU fallback): the plans raise when the HIP library
is missing.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .circuits import AmplitudeTask, with_batch
from .expression import HipContractExpression, run_group

__all__ = ["BlockPipeline", "BlockSampler", "BlockTopK", "PoolSampler"]


class _Slot:
    __slots__ = ("stream", "pbuf", "bound", "outs", "event", "pending")

    def __init__(self, stream, pbuf, bound, outs):
        self.stream, self.pbuf, self.bound, self.outs = stream, pbuf, bound, outs
        self.event = torch.cuda.Event()
        self.pending: List[int] = []   # table rows of the members enqueued since the last launch


class BlockPipeline:
    """`inflight` slots x `group` members contracting blocks `blocks[k]` (with_batch indices) in
    order; `step()` enqueues the next block and returns its output tensor (written when its
    group is launched and has run: `wait()` / `synchronize()`)."""

    def __init__(self, task: AmplitudeTask, blocks: Sequence[int], inflight: int = 2, group: int = 1,
                 device: Optional[torch.device] = None, dtype: torch.dtype = torch.complex64,
                 min_chunks: Optional[int] = None, freeze: bool = True):
        if inflight < 1 or group < 1:
            raise ValueError("inflight and group must be >= 1")
        if len(blocks) == 0:
            raise ValueError("no blocks")
        self.task = task
        self.blocks = [int(b) for b in blocks]
        self.inflight = int(inflight)
        self.group = int(group)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dtype = dtype
        self.proj = [i for i, (kind, _) in enumerate(task.kinds) if kind == "proj"]
        # device table: block k's projector vectors (n_proj x 2), built once
        tab = np.zeros((len(self.blocks), len(self.proj), 2), dtype=np.complex128)
        for k, b in enumerate(self.blocks):
            tb = with_batch(task, b)
            for j, i in enumerate(self.proj):
                tab[k, j] = tb.operands[i]
        self.table = torch.from_numpy(tab).to(self.device, dtype)
        # the cores and input vectors are read-only: every member reads the same device copies
        base_ops = [torch.from_numpy(o).to(self.device, dtype) for o in task.operands]
        self.expr = HipContractExpression(task.eq, *task.shapes, optimize=task.path, slices=task.sliced)
        plan = self.expr.plan(dtype, None, self.device.index)
        if min_chunks is None and self.inflight >= 4:
            # deep pipelines: fewer, wider chunks per sweep op -- the other streams fill the CUs
            # one launch leaves idle (r06, same box: 4 in flight 0.389 -> 0.375 ms per block at
            # 64 instead of 128 chunks; one block at a time it is slower, 0.646 -> 0.714)
            min_chunks = 64
        if min_chunks:
            plan.set("min_chunks", int(min_chunks))
        if self.group > 1:
            # compiled for lockstep groups: wider sweep chunks (G ops share every launch)
            plan.set("group_hint", self.group)
        # volatile operands: exactly the projectors whose rows differ anywhere in the block table
        # (the pipeline owns every other operand and never writes them), so what the rest of the
        # network contracts to is computed by each member's first launch only
        # (`freeze=False`: nothing is declared, every launch contracts the whole network)
        self.volatile = ([i for j, i in enumerate(self.proj) if bool((tab[:, j] != tab[0, j]).any())]
                         if freeze else None)
        plan.set_volatile(self.volatile)
        self.slots: List[_Slot] = []
        for s in range(self.inflight):
            stream = torch.cuda.current_stream(self.device) if s == 0 else torch.cuda.Stream(self.device)
            pbuf = torch.zeros((self.group, len(self.proj), 2), dtype=dtype, device=self.device)
            bound, outs = [], []
            for m in range(self.group):
                ops = list(base_ops)
                for j, i in enumerate(self.proj):
                    ops[i] = pbuf[m, j]
                bound.append(self.expr.bind(*ops, private_plan=True, volatile=self.volatile))
                outs.append(torch.empty(self.expr.out_shape, dtype=dtype, device=self.device))
            self.slots.append(_Slot(stream, pbuf, bound, outs))
        self.k = 0
        self._closed = False
        torch.cuda.synchronize(self.device)   # the table and operands exist before any slot stream reads them

    def plan(self, slot: int = 0, member: int = 0):
        """The native plan of one member (queries / profiling)."""
        return self.slots[slot].bound[member].plan

    def _launch(self, slot: _Slot) -> None:
        rows = slot.pending
        n = len(rows)
        if n == 0:
            return
        with torch.cuda.stream(slot.stream):
            r0 = rows[0]
            if rows == list(range(r0, r0 + n)):
                slot.pbuf[:n].copy_(self.table[r0:r0 + n])
            else:
                for m, r in enumerate(rows):
                    slot.pbuf[m].copy_(self.table[r])
            if n == 1:
                slot.bound[0].run(slot.outs[0], slot.stream)
            else:
                run_group(slot.bound[:n], slot.outs[:n], slot.stream)
            slot.event.record(slot.stream)
        slot.pending = []

    def step(self) -> torch.Tensor:
        """Enqueue block blocks[k mod len(blocks)] as member k mod group of slot
        (k div group) mod inflight; launches the slot's group once it is full.  Returns that
        member's output tensor (overwritten when the slot runs again)."""
        if self._closed:
            raise RuntimeError("the pipeline is closed")
        k = self.k
        slot = self.slots[(k // self.group) % self.inflight]
        m = k % self.group
        if m == 0 and slot.pending:   # (after a reset: a partial group left behind)
            self._launch(slot)
        slot.pending.append(k % len(self.blocks))
        self.k += 1
        if m == self.group - 1:
            self._launch(slot)
        return slot.outs[m]

    def flush(self) -> None:
        """Launch every partially filled group."""
        for slot in self.slots:
            self._launch(slot)

    def wait(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Flush, then make `stream` (default: the current one) wait for every launched group:
        the outputs may then be read on it."""
        self.flush()
        st = stream or torch.cuda.current_stream(self.device)
        for slot in self.slots:
            if slot.stream is not st:
                st.wait_event(slot.event)

    def reset(self) -> None:
        """Flush and start again at block 0 (slot 0, member 0)."""
        self.flush()
        self.k = 0

    def run(self, n: Optional[int] = None) -> List[torch.Tensor]:
        """Contract the next `n` blocks (default: every block once); returns host copies of their
        amplitudes in order (a checking helper: `step()` is the pipelined form)."""
        n = len(self.blocks) if n is None else n
        res = []
        pend = []
        for _ in range(n):
            pend.append(self.step())
            if self.k % self.group == 0:
                self.synchronize()
                res.extend(o.cpu() for o in pend)
                pend = []
        if pend:
            self.synchronize()
            res.extend(o.cpu() for o in pend)
        return res

    def synchronize(self) -> None:
        self.flush()
        torch.cuda.synchronize(self.device)

    def close(self) -> None:
        """Wait for the launched groups and release every member's private plan now
        (`NativePlan.release_now`: inside a stream capture the handle is parked and released after
        it), not whenever the garbage collector gets to them.  `step()` then raises."""
        if self._closed:
            return
        self._closed = True
        for slot in self.slots:
            slot.pending = []
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(self.device)
        for slot in self.slots:
            for b in slot.bound:
                b.plan.release_now()


def _word_of(bits) -> int:
    w = 0
    for q, v in bits.items():
        if v:
            w |= 1 << int(q)
    return w


def _word_axes(task, who: str) -> List[int]:
    """The open qubits (one per axis of a block, axis 0 slowest) of a task whose bitstrings fit an
    int64 word (bit q = qubit q); refuses the others before a device is touched."""
    qubits = [int(q) for q in task.open_qubits] + [int(q) for q in task.fixed_bits]
    if len(qubits) > 63 or (qubits and max(qubits) > 62):
        raise ValueError(f"{who}: {len(qubits)} qubits do not fit a 63-bit bitstring word")
    return [int(q) for q in task.open_qubits]


def _block_bases(task, blocks) -> List[int]:
    """The closed qubits' bits of every block, as a word: once, not per step."""
    return [_word_of(with_batch(task, b).fixed_bits) for b in blocks]


def _run_consumer(pipe, n: Optional[int]):
    """`run()` of a pipeline whose `step()` returns a tuple of device tensors: host copies in block
    order, copied before a slot is reused."""
    n = len(pipe.blocks) if n is None else n
    res, pend = [], []

    def drain():
        pipe.synchronize()
        res.extend(tuple(t.cpu() for t in o) for o in pend)
        pend.clear()

    for _ in range(n):
        pend.append(pipe.step())
        if pipe.k % pipe.group == 0:
            drain()
    if pend:
        drain()
    return res


class BlockSampler(BlockPipeline):
    """A `BlockPipeline` that samples every block it contracts: `draws` bitstrings per block with
    probability |amplitude|^2 / (block mass), on the device.

    When a slot's group is launched, one Born-rule sampling call (`tq_born_sample`, the call
    under `ops.born_sample`) per member is enqueued on the slot's stream right behind the
    contraction; it writes into buffers the sampler owns per (slot,
    member).  `step()` enqueues the next block and returns that member's `(words, prob, stats)`
    device tensors -- `draws` int64 bitstring words (bit q = qubit q: the open qubits from the
    drawn index, the closed ones from the block's fixed bits), `draws` float64 probabilities
    |amplitude|^2 of the drawn strings (the XEB statistic) and `stats = (S1, S2)` = (the block's
    probability mass, sum of |amplitude|^4).  Like `BlockPipeline.step()`'s outputs they are
    written when the group has run (`wait()` / `synchronize()`) and overwritten when the slot runs
    again.  A block whose mass is not a finite number > 0 yields words of -1 and probabilities 0.

    Uniforms: row k of `uniforms` (a `(len(blocks), draws)` float64 device tensor) serves block k;
    without it they are drawn at launch time from a `torch.Generator` of the device seeded with
    `seed` (the same seed and the same call sequence give the same words).

    Every block gets the same number of draws: `PoolSampler` is the sampler that chooses WHICH
    block a draw comes from, in proportion to the blocks' masses (`stats[0]` here).
    Circuits of more than 63 qubits do not fit the int64 words and are refused."""

    def __init__(self, task: AmplitudeTask, blocks: Sequence[int], draws: int, inflight: int = 2,
                 group: int = 1, device: Optional[torch.device] = None, dtype: torch.dtype = torch.complex64,
                 seed: int = 0, uniforms: Optional[torch.Tensor] = None, min_chunks: Optional[int] = None):
        axes = _word_axes(task, "BlockSampler")
        draws = int(draws)
        if draws < 1:
            raise ValueError("draws must be >= 1")
        if dtype not in (torch.complex64, torch.complex128):
            raise ValueError(f"BlockSampler: complex64 / complex128 amplitudes, got {dtype}")
        super().__init__(task, blocks, inflight=inflight, group=group, device=device, dtype=dtype,
                         min_chunks=min_chunks)
        self.draws = draws
        self.axis_qubit = axes
        self.base = _block_bases(task, self.blocks)
        if uniforms is not None:
            if (uniforms.dtype != torch.float64 or uniforms.device != self.device
                    or tuple(uniforms.shape) != (len(self.blocks), draws) or not uniforms.is_contiguous()):
                raise ValueError(f"uniforms must be a contiguous ({len(self.blocks)}, {draws}) float64 tensor on {self.device}")
            self.gen = None
        else:
            self.gen = torch.Generator(self.device)
            self.gen.manual_seed(int(seed))
        self.uniforms = uniforms
        n = 2 ** len(self.axis_qubit)
        wsb = ops.born_workspace_size(dtype, n, draws)
        f64 = dict(dtype=torch.float64, device=self.device)
        # generated uniforms: one refill of `_refill` launches' worth per slot, on the slot's stream
        self._refill = 16
        self.sbuf = []    # [slot][member] -> (words, prob, stats, workspace)
        self.ubuf = []    # [slot] -> (_refill, group, draws) uniforms, or None
        self._ucur = []   # [slot] -> launches served from the slot's current refill
        self._call = []   # [slot][member] -> the constant arguments of tq_born_sample
        vp = ctypes.c_void_p
        self._axes = _lib.i32(self.axis_qubit)
        self._fn = _lib.lib().tq_born_sample
        for slot in self.slots:
            bufs = [(torch.empty(draws, dtype=torch.int64, device=self.device), torch.empty(draws, **f64),
                     torch.empty(2, **f64), torch.empty(wsb, dtype=torch.uint8, device=self.device))
                    for _ in range(self.group)]
            self.sbuf.append(bufs)
            self.ubuf.append(torch.empty((self._refill, self.group, draws), **f64) if self.gen is not None else None)
            self._ucur.append(self._refill)
            self._call.append([((ops.dtype_code(dtype), n, vp(slot.outs[m].data_ptr()), draws),
                                (vp(b[0].data_ptr()), vp(b[1].data_ptr()), vp(b[2].data_ptr()),
                                 len(self.axis_qubit), self._axes),
                                (vp(b[3].data_ptr()), wsb, vp(slot.stream.cuda_stream)))
                               for m, b in enumerate(bufs)])
        # one validated call per member (arguments, buffers, the kernels' code objects): the launches
        # behind the contractions then pass the same arguments straight to the C ABI
        for s, slot in enumerate(self.slots):
            with torch.cuda.stream(slot.stream):
                for m, b in enumerate(self.sbuf[s]):
                    slot.outs[m].zero_()
                    ops.born_sample(slot.outs[m], torch.zeros(draws, **f64), prob=b[1], axis_qubit=self.axis_qubit,
                                    base=self.base[0], out=b[0], stats=b[2], workspace=b[3])
        torch.cuda.synchronize(self.device)

    def _launch(self, slot: _Slot) -> None:
        rows = list(slot.pending)
        if not rows:
            return
        super()._launch(slot)
        s = self.slots.index(slot)
        if self.gen is not None:
            if self._ucur[s] == self._refill:
                with torch.cuda.stream(slot.stream):
                    self.ubuf[s].uniform_(0.0, 1.0, generator=self.gen)
                self._ucur[s] = 0
            u0 = self.ubuf[s].data_ptr() + self._ucur[s] * self.group * self.draws * 8
            self._ucur[s] += 1
        else:
            u0 = self.uniforms.data_ptr()
        for m, r in enumerate(rows):
            head, outs, tail = self._call[s][m]
            up = u0 + (m if self.gen is not None else r) * self.draws * 8
            check(self._fn(*head, ctypes.c_void_p(up), *outs, self.base[r], *tail), "tq_born_sample")
        slot.event.record(slot.stream)

    def step(self):
        """Enqueue the next block (as `BlockPipeline.step()`); returns the `(words, prob, stats)`
        device tensors of its (slot, member)."""
        if self._closed:
            raise RuntimeError("the sampler is closed")
        k = self.k
        s, m = (k // self.group) % self.inflight, k % self.group
        super().step()
        return self.sbuf[s][m][:3]

    def run(self, n: Optional[int] = None):
        """Sample the next `n` blocks (default: every block once); returns host copies
        `[(words, prob, stats), ...]` in block order, copied before a slot is reused."""
        return _run_consumer(self, n)

    def close(self) -> None:
        """Release the pipeline's private plans and the sampler's buffers now."""
        super().close()
        self.sbuf, self.ubuf, self._call = [], [], []
        self.uniforms = None


class BlockTopK(BlockPipeline):
    """A `BlockPipeline` that post-selects every block it contracts: the `k` most probable
    bitstrings of each block, on the device.

    When a slot's group is launched, one top-k call (`tq_born_topk`, the call under
    `ops.born_topk`) per member is enqueued on the slot's stream right behind the contraction; it
    writes into buffers the pipeline owns per (slot, member).  `step()` enqueues the next block
    and returns that member's `(words, prob, count)` device tensors -- `k` int64 bitstring words
    (bit q = qubit q: the open qubits from the selected index, the closed ones from the block's
    fixed bits) in the order |amplitude|^2 descending, index ascending among equal ones; their `k`
    float64 probabilities; and `count[0]` = how many were selected (a block with fewer than `k`
    non-zero amplitudes: the rest is words of -1 and probabilities 0).  Like
    `BlockPipeline.step()`'s outputs they are written when the group has run (`wait()` /
    `synchronize()`) and overwritten when the slot runs again.  The selection is exact and the
    same amplitudes give the same bits.  Circuits of more than 63 qubits do not fit the int64
    words and are refused."""

    def __init__(self, task: AmplitudeTask, blocks: Sequence[int], k: int, inflight: int = 2,
                 group: int = 1, device: Optional[torch.device] = None, dtype: torch.dtype = torch.complex64,
                 min_chunks: Optional[int] = None):
        axes = _word_axes(task, "BlockTopK")
        k = int(k)
        if not 1 <= k <= _lib.TQ_BORN_TOPK_MAX_K:
            raise ValueError(f"BlockTopK: k must be in [1, {_lib.TQ_BORN_TOPK_MAX_K}]")
        if dtype not in (torch.complex64, torch.complex128):
            raise ValueError(f"BlockTopK: complex64 / complex128 amplitudes, got {dtype}")
        super().__init__(task, blocks, inflight=inflight, group=group, device=device, dtype=dtype,
                         min_chunks=min_chunks)
        self.topk = k
        self.axis_qubit = axes
        self.base = _block_bases(task, self.blocks)
        n = 2 ** len(self.axis_qubit)
        wsb = ops.born_topk_workspace_size(dtype, n, k)
        self.sbuf = []    # [slot][member] -> (words, prob, count, workspace)
        self._call = []   # [slot][member] -> the constant arguments of tq_born_topk
        vp = ctypes.c_void_p
        self._axes = _lib.i32(self.axis_qubit)
        self._fn = _lib.lib().tq_born_topk
        for slot in self.slots:
            bufs = [(torch.empty(k, dtype=torch.int64, device=self.device),
                     torch.empty(k, dtype=torch.float64, device=self.device),
                     torch.empty(1, dtype=torch.int64, device=self.device),
                     torch.empty(wsb, dtype=torch.uint8, device=self.device))
                    for _ in range(self.group)]
            self.sbuf.append(bufs)
            self._call.append([((ops.dtype_code(dtype), n, vp(slot.outs[m].data_ptr()), k,
                                 vp(b[0].data_ptr()), vp(b[1].data_ptr()), vp(b[2].data_ptr()),
                                 len(self.axis_qubit), self._axes),
                                (vp(b[3].data_ptr()), wsb, vp(slot.stream.cuda_stream)))
                               for m, b in enumerate(bufs)])
        # one validated call per member (arguments, buffers, the kernels' code objects): the launches
        # behind the contractions then pass the same arguments straight to the C ABI
        for s, slot in enumerate(self.slots):
            with torch.cuda.stream(slot.stream):
                for m, b in enumerate(self.sbuf[s]):
                    slot.outs[m].zero_()
                    ops.born_topk(slot.outs[m], k, axis_qubit=self.axis_qubit, base=self.base[0],
                                  out=b[0], prob=b[1], count=b[2], workspace=b[3])
        torch.cuda.synchronize(self.device)

    def _launch(self, slot: _Slot) -> None:
        rows = list(slot.pending)
        if not rows:
            return
        super()._launch(slot)
        s = self.slots.index(slot)
        for m, r in enumerate(rows):
            head, tail = self._call[s][m]
            check(self._fn(*head, self.base[r], *tail), "tq_born_topk")
        slot.event.record(slot.stream)

    def step(self):
        """Enqueue the next block (as `BlockPipeline.step()`); returns the `(words, prob, count)`
        device tensors of its (slot, member)."""
        if self._closed:
            raise RuntimeError("the pipeline is closed")
        k = self.k
        s, m = (k // self.group) % self.inflight, k % self.group
        super().step()
        return self.sbuf[s][m][:3]

    def run(self, n: Optional[int] = None):
        """Select from the next `n` blocks (default: every block once); returns host copies
        `[(words, prob, count), ...]` in block order, copied before a slot is reused."""
        return _run_consumer(self, n)

    def close(self) -> None:
        """Release the pipeline's private plans and the selection buffers now."""
        super().close()
        self.sbuf, self._call = [], []


class PoolSampler(BlockPipeline):
    """A `BlockPipeline` that samples across the blocks it contracts: `draws` bitstrings from the
    Born distribution over EVERY block stepped so far, |amplitude|^2 / (sum of the blocks'
    masses), on the device.  The block boundary does not reach the caller.

    Every slot holds a weighted reservoir `(words, prob, pool)` of `draws` slots.  When a slot's
    group is launched, one `tq_born_pool_sample` call per member (in member order) is enqueued on
    the slot's stream right behind the contraction: block b of mass S1_b replaces reservoir slot j
    by its own Born-rule draw j with probability S1_b / (W + S1_b), W the mass the reservoir has
    seen (include/tneqhip.h).  After any number of blocks slot j holds a draw from block b with
    probability S1_b / sum S1 and, inside it, bitstring i with p_i / S1_b: p_i / sum, the Born rule
    over the pool.  Only the accepted draws (about draws / k of the k-th block) are resolved.

    `step()` enqueues the next block and returns None: there is no per-block result.  `result()`
    merges the slots' reservoirs (`tq_born_pool_merge`) and returns `(words, prob, pool)`.

    Uniforms: `uniforms` is a contiguous `(len(blocks), 2, draws)` float64 device tensor; row
    `[k, 0]` is `u` (the draw inside block k) and `[k, 1]` is `v` (the acceptance) of block k.
    Without it both come from a `torch.Generator` of the device seeded with `seed` (the same seed
    and the same call sequence give the same words).  Circuits of more than 63 qubits do not fit
    the int64 words and are refused."""

    def __init__(self, task: AmplitudeTask, blocks: Sequence[int], draws: int, inflight: int = 2,
                 group: int = 1, device: Optional[torch.device] = None, dtype: torch.dtype = torch.complex64,
                 seed: int = 0, uniforms: Optional[torch.Tensor] = None, min_chunks: Optional[int] = None):
        axes = _word_axes(task, "PoolSampler")
        draws = int(draws)
        if draws < 1:
            raise ValueError("draws must be >= 1")
        if dtype not in (torch.complex64, torch.complex128):
            raise ValueError(f"PoolSampler: complex64 / complex128 amplitudes, got {dtype}")
        super().__init__(task, blocks, inflight=inflight, group=group, device=device, dtype=dtype,
                         min_chunks=min_chunks)
        self.draws = draws
        self.axis_qubit = axes
        self.base = _block_bases(task, self.blocks)
        if uniforms is not None:
            if (uniforms.dtype != torch.float64 or uniforms.device != self.device
                    or tuple(uniforms.shape) != (len(self.blocks), 2, draws) or not uniforms.is_contiguous()):
                raise ValueError(f"uniforms must be a contiguous ({len(self.blocks)}, 2, {draws}) float64 tensor on {self.device}")
            self.gen = None
        else:
            self.gen = torch.Generator(self.device)
            self.gen.manual_seed(int(seed))
        self._seed, self._mgen = int(seed), None
        self.uniforms = uniforms
        n = 2 ** len(self.axis_qubit)
        wsb = ops.born_pool_workspace_size(dtype, n, draws)
        f64 = dict(dtype=torch.float64, device=self.device)
        # generated uniforms: one refill of `_refill` launches' worth per slot, on the slot's stream
        self._refill = 16
        self.rbuf = []    # [slot] -> (words, prob, pool, workspace): the slot's reservoir
        self.sstat = []   # [slot][member] -> the member's last block's (S1, S2)
        self.ubuf = []    # [slot] -> (_refill, group, 2, draws) uniforms, or None
        self._ucur = []   # [slot] -> launches served from the slot's current refill
        self._call = []   # [slot][member] -> the constant arguments of tq_born_pool_sample
        vp = ctypes.c_void_p
        self._axes = _lib.i32(self.axis_qubit)
        self._fn = _lib.lib().tq_born_pool_sample
        for slot in self.slots:
            r = (torch.full((draws,), -1, dtype=torch.int64, device=self.device), torch.zeros(draws, **f64),
                 torch.zeros(4, **f64), torch.empty(wsb, dtype=torch.uint8, device=self.device))
            st = [torch.empty(2, **f64) for _ in range(self.group)]
            self.rbuf.append(r)
            self.sstat.append(st)
            self.ubuf.append(torch.empty((self._refill, self.group, 2, draws), **f64) if self.gen is not None else None)
            self._ucur.append(self._refill)
            self._call.append([((ops.dtype_code(dtype), n, vp(slot.outs[m].data_ptr()), draws),
                                (vp(r[0].data_ptr()), vp(r[1].data_ptr()), vp(r[2].data_ptr()),
                                 vp(st[m].data_ptr()), len(self.axis_qubit), self._axes),
                                (vp(r[3].data_ptr()), wsb, vp(slot.stream.cuda_stream)))
                               for m in range(self.group)])
        self._mws = torch.empty(_lib.TQ_BORN_POOL_MERGE_WORKSPACE, dtype=torch.uint8, device=self.device)
        self._merged = torch.cuda.Event()
        # one validated call per member (arguments, buffers, the kernels' code objects) on a block of
        # zeros, which contributes nothing: the pools stay empty
        zu = torch.zeros(draws, **f64)
        for s, slot in enumerate(self.slots):
            with torch.cuda.stream(slot.stream):
                r = self.rbuf[s]
                for m in range(self.group):
                    slot.outs[m].zero_()
                    ops.born_pool_sample(slot.outs[m], zu, zu, r[0], r[1], r[2], axis_qubit=self.axis_qubit,
                                         base=self.base[0], stats=self.sstat[s][m], workspace=r[3])
        torch.cuda.synchronize(self.device)

    def _launch(self, slot: _Slot) -> None:
        rows = list(slot.pending)
        if not rows:
            return
        super()._launch(slot)
        s = self.slots.index(slot)
        row = 2 * self.draws * 8
        if self.gen is not None:
            if self._ucur[s] == self._refill:
                with torch.cuda.stream(slot.stream):
                    self.ubuf[s].uniform_(0.0, 1.0, generator=self.gen)
                self._ucur[s] = 0
            u0 = self.ubuf[s].data_ptr() + self._ucur[s] * self.group * row
            self._ucur[s] += 1
        else:
            u0 = self.uniforms.data_ptr()
        for m, r in enumerate(rows):
            head, outs, tail = self._call[s][m]
            up = u0 + (m if self.gen is not None else r) * row
            check(self._fn(*head, ctypes.c_void_p(up), ctypes.c_void_p(up + self.draws * 8), *outs,
                           self.base[r], *tail), "tq_born_pool_sample")
        slot.event.record(slot.stream)

    def step(self) -> None:
        """Enqueue the next block (as `BlockPipeline.step()`).  Returns None: a block leaves no
        result of its own, only its share of the slot's reservoir; see `result()`."""
        if self._closed:
            raise RuntimeError("the sampler is closed")
        super().step()

    def result(self, merge_uniforms: Optional[torch.Tensor] = None):
        """Flush, make the current stream wait for every slot, and merge the slots' reservoirs in
        slot order 0, 1, ... into a fresh output: device tensors `(words, prob, pool)` -- `draws`
        int64 bitstring words (bit q = qubit q), their float64 probabilities |amplitude|^2, and
        `pool` = (the mass of every block stepped so far, the sum of |amplitude|^4, the number of
        blocks that contributed, the slots taken from the last slot merged).  With no mass at all
        the words are -1 and the probabilities 0.  Row s of `merge_uniforms` (`(inflight, draws)`
        float64, device) decides what is taken from slot s; without it the rows come from the
        generator (one seeded with `seed` when the blocks' uniforms were given).  The slot reservoirs stay intact: stepping may go on, and a later `result()`
        reflects more blocks."""
        if self._closed:
            raise RuntimeError("the sampler is closed")
        f64 = dict(dtype=torch.float64, device=self.device)
        if merge_uniforms is None:
            if self.gen is None and self._mgen is None:   # the blocks' uniforms were given: `seed` serves the merges
                self._mgen = torch.Generator(self.device)
                self._mgen.manual_seed(self._seed)
            mv = torch.rand((self.inflight, self.draws), generator=self.gen or self._mgen, **f64)
        else:
            mv = merge_uniforms
            if (not isinstance(mv, torch.Tensor) or mv.dtype != torch.float64 or mv.device != self.device
                    or tuple(mv.shape) != (self.inflight, self.draws) or not mv.is_contiguous()):
                raise ValueError(f"merge_uniforms must be a contiguous ({self.inflight}, {self.draws}) float64 tensor on {self.device}")
        self.wait()
        cur = torch.cuda.current_stream(self.device)
        words = torch.full((self.draws,), -1, dtype=torch.int64, device=self.device)
        prob = torch.zeros(self.draws, **f64)
        pool = torch.zeros(4, **f64)
        for s in range(self.inflight):
            r = self.rbuf[s]
            ops.born_pool_merge(words, prob, pool, r[0], r[1], r[2], mv[s], workspace=self._mws)
        # the slots' next launches overwrite what these merges read
        self._merged.record(cur)
        for slot in self.slots:
            if slot.stream is not cur:
                slot.stream.wait_event(self._merged)
        return words, prob, pool

    def reset(self) -> None:
        """Flush, start again at block 0 and empty every slot's reservoir."""
        super().reset()
        for s, slot in enumerate(self.slots):
            with torch.cuda.stream(slot.stream):
                self.rbuf[s][2].zero_()

    def run(self, n: Optional[int] = None, merge_uniforms: Optional[torch.Tensor] = None):
        """Step through the next `n` blocks (default: every block once) and return host copies of
        `result(merge_uniforms)`."""
        n = len(self.blocks) if n is None else n
        for _ in range(n):
            self.step()
        return tuple(t.cpu() for t in self.result(merge_uniforms))

    def close(self) -> None:
        """Release the pipeline's private plans and the sampler's buffers now."""
        super().close()
        self.rbuf, self.sstat, self.ubuf, self._call = [], [], [], []
        self.uniforms = None
