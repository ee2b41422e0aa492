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
k most probable bitstrings of each.

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

__all__ = ["BlockPipeline", "BlockSampler", "BlockTopK"]


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

    Every block gets the same number of draws: choosing WHICH block to sample, in proportion to
    the blocks' masses, is the caller's business -- `stats[0]` is the mass they need for it.
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
