#!/usr/bin/env python
"""What sampling ACROSS blocks costs the headline pipeline.

One process, C4, complex64, a 64-block window, `--inflight` x `--group` as bench.py's headline:
  1. `BlockPipeline.step()`, `BlockSampler.step()` and `PoolSampler.step()`, timed exactly as
     bench.py's headline loop does (warm-up steps, synchronize, K steps + flush, synchronize),
     ALTERNATING the three, three runs each: ms per block and the range of the runs;
  2. on an otherwise idle stream, on one finished block with preallocated buffers, three rounds
     alternating `ops.born_sample`, `ops.born_pool_sample` into an empty pool (the pool is zeroed
     before every call: every draw accepted) and `ops.born_pool_sample` into a pool preloaded to
     W = 63 S1 (reset before every call: about 1/64 of the draws accepted); the resets are one
     8-byte-aligned 32-byte device copy per call and are timed with the call;
  3. the preloaded call replayed from a graph (20 calls and resets per replay), and born_sample
     likewise;
  4. `PoolSampler.result()` for the `--inflight` slots.
Prints one JSON object (profiles/born_pool.json is this output on an MI355X)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--group", type=int, default=1)
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--idle-calls", type=int, default=200)
    args = ap.parse_args()

    import torch
    from tneq_qc_amd import ops
    from tneq_qc_amd.circuits import config_task
    from tneq_qc_amd.sampling import BlockPipeline, BlockSampler, PoolSampler

    dev = torch.device("cuda:0")
    task = config_task(args.config)
    blocks = list(range(max(64, args.inflight * args.group)))
    f64 = dict(dtype=torch.float64, device=dev)

    def timed(pipe):
        for _ in range(args.warmup):
            pipe.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pipe.step()
        pipe.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    kw = dict(inflight=args.inflight, group=args.group, device=dev)
    pipes = {"plain": BlockPipeline(task, blocks, **kw),
             "sampler": BlockSampler(task, blocks, args.draws, seed=1, **kw),
             "pool": PoolSampler(task, blocks, args.draws, seed=1, **kw)}
    runs = {k: [] for k in pipes}
    for _ in range(3):
        for k, p in pipes.items():
            runs[k].append(timed(p))
    out = pipes["plain"].slots[0].outs[0].clone()   # one finished block for the idle-stream timings
    pool_pipe = pipes["pool"]
    pool_pipe.reset()
    for _ in blocks:
        pool_pipe.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            words, prob, pool = pool_pipe.result()
        e1.record()
        torch.cuda.synchronize()
        res_ms.append(e0.elapsed_time(e1) / 20)
    pool_final = pool.tolist()
    valid = bool((words >= 0).all()) and bool((prob > 0).all())
    for p in pipes.values():
        p.close()

    # the sampling launches alone
    n = out.numel()
    u, v = torch.rand(args.draws, **f64), torch.rand(args.draws, **f64)
    wsb = ops.born_workspace_size(out.dtype, n, args.draws)
    pwsb = ops.born_pool_workspace_size(out.dtype, n, args.draws)
    skw = dict(out=torch.empty(args.draws, dtype=torch.int64, device=dev), prob=torch.empty(args.draws, **f64),
               stats=torch.empty(2, **f64), workspace=torch.empty(wsb, dtype=torch.uint8, device=dev))
    index, prob = torch.empty(args.draws, dtype=torch.int64, device=dev), torch.empty(args.draws, **f64)
    pool = torch.zeros(4, **f64)
    pkw = dict(stats=torch.empty(2, **f64), workspace=torch.empty(pwsb, dtype=torch.uint8, device=dev))
    ops.born_sample(out, u, **skw)
    torch.cuda.synchronize()
    S1 = float(skw["stats"][0])
    empty = torch.zeros(4, **f64)
    loaded = torch.tensor([63.0 * S1, 0.0, 63.0, 0.0], **f64)

    def call_sample():
        ops.born_sample(out, u, **skw)

    def call_pool(start):
        pool.copy_(start)
        ops.born_pool_sample(out, u, v, index, prob, pool, **pkw)

    calls = {"born_sample": call_sample, "pool_empty": lambda: call_pool(empty),
             "pool_preloaded": lambda: call_pool(loaded), "pool_reset_copy_alone": lambda: pool.copy_(loaded)}
    idle = {k: [] for k in calls}
    accepted = {}
    for f in calls.values():
        for _ in range(10):
            f()
    for _ in range(3):
        for k, f in calls.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.idle_calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            idle[k].append(e0.elapsed_time(e1) / args.idle_calls)
            accepted[k] = float(pool[3])
    # ... and replayed from a graph (no host issue between the launches): 20 calls per replay
    side = torch.cuda.Stream(dev)
    graph_ms = {}
    for k in ("born_sample", "pool_preloaded", "pool_reset_copy_alone"):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(20):
                calls[k]()
        graph.replay()
        torch.cuda.synchronize()
        graph_ms[k] = []
        for _ in range(3):
            e0.record()
            for _ in range(10):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            graph_ms[k].append(e0.elapsed_time(e1) / 200)

    def rng(x):
        return {"min": min(x), "max": max(x), "runs": x}

    res = {
        "config": args.config, "device": torch.cuda.get_device_name(0), "dtype": "complex64",
        "inflight": args.inflight, "group": args.group, "blocks": len(blocks), "draws": args.draws,
        "steps": args.steps, "warmup": args.warmup, "idle_calls": args.idle_calls,
        "step_ms_per_block": {k: rng(x) for k, x in runs.items()},
        "idle_stream_ms_per_call": {k: rng(x) for k, x in idle.items()},
        "graph_replay_ms_per_call": {k: rng(x) for k, x in graph_ms.items()},
        "accepted_last_call": {k: accepted[k] for k in ("pool_empty", "pool_preloaded")},
        "result_ms": rng(res_ms), "result_slots": args.inflight,
        "sample_launches_per_block": 3, "pool_launches_per_block": 4, "merge_launches": 3,
        "block_bytes": n * out.element_size(), "sample_workspace_bytes": wsb, "pool_workspace_bytes": pwsb,
        "block_mass": S1, "pool_after_window": pool_final, "all_words_valid": valid,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
