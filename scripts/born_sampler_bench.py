#!/usr/bin/env python
"""What Born-rule sampling costs the headline pipeline.

One process, C4, complex64, a 64-block window, `--inflight` x `--group` as bench.py's headline:
  1. a plain `BlockPipeline`, `step()` timed exactly as bench.py's headline loop does (warm-up
     steps, synchronize, K steps + flush, synchronize);
  2. a `BlockSampler(draws=N)`, timed the same way;
  3. the sampling launches alone (`ops.born_sample` on one finished block, preallocated buffers)
     on an otherwise idle stream, issued eagerly and replayed from a graph: ms per call, and the
     achieved bytes/s (the faster of the two) against the algorithmic bytes (one read of the
     block + the uniforms + the slab + the outputs).
Prints one JSON object (profiles/born_sampler.json is this output on an MI355X)."""
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
    from tneq_qc_amd.sampling import BlockPipeline, BlockSampler

    dev = torch.device("cuda:0")
    task = config_task(args.config)
    blocks = list(range(max(64, args.inflight * args.group)))

    def timed(pipe):
        for _ in range(args.warmup):
            pipe.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pipe.step()
        pipe.flush()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, (t1 - t0) / args.steps * 1e3

    plain = BlockPipeline(task, blocks, inflight=args.inflight, group=args.group, device=dev)
    ms_plain = [timed(plain) for _ in range(3)]
    out = plain.slots[0].outs[0].clone()   # one finished block for the idle-stream timing
    plain.close()
    samp = BlockSampler(task, blocks, args.draws, inflight=args.inflight, group=args.group, device=dev, seed=1)
    ms_samp = [timed(samp) for _ in range(3)]
    words, prob, stats = samp.step()
    samp.synchronize()
    mass, valid = float(stats[0]), bool((words >= 0).all())
    samp.close()

    # the sampling launches alone
    n = out.numel()
    u = torch.rand(args.draws, dtype=torch.float64, device=dev)
    wsb = ops.born_workspace_size(out.dtype, n, args.draws)
    kw = dict(out=torch.empty(args.draws, dtype=torch.int64, device=dev),
              prob=torch.empty(args.draws, dtype=torch.float64, device=dev),
              stats=torch.empty(2, dtype=torch.float64, device=dev),
              workspace=torch.empty(wsb, dtype=torch.uint8, device=dev))
    for _ in range(10):
        ops.born_sample(out, u, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.idle_calls):
        ops.born_sample(out, u, **kw)
    e1.record()
    t_issue = (time.perf_counter() - t0) / args.idle_calls * 1e3
    torch.cuda.synchronize()
    ms_idle = e0.elapsed_time(e1) / args.idle_calls
    # ... and replayed from a graph (no host issue between the launches): 20 calls per replay
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(20):
            ops.born_sample(out, u, **kw)
    graph.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    ms_graph = e0.elapsed_time(e1) / 200
    block_bytes = n * out.element_size()
    alg_bytes = block_bytes + args.draws * (8 + 8 + 8) + wsb + 16
    res = {
        "config": args.config, "device": torch.cuda.get_device_name(0), "dtype": "complex64",
        "inflight": args.inflight, "group": args.group, "blocks": len(blocks), "draws": args.draws,
        "steps": args.steps, "warmup": args.warmup,
        "plain_ms_per_block": min(ms_plain)[0], "plain_ms_per_block_runs": [m[0] for m in ms_plain],
        "plain_host_issue_ms_per_block": min(m[1] for m in ms_plain),
        "sampler_ms_per_block": min(ms_samp)[0], "sampler_ms_per_block_runs": [m[0] for m in ms_samp],
        "sampler_host_issue_ms_per_block": min(m[1] for m in ms_samp),
        "sampler_minus_plain_ms": min(ms_samp)[0] - min(ms_plain)[0],
        "sampling_idle_stream_ms_per_block": ms_idle,
        "sampling_host_issue_ms_per_block": t_issue,
        "sampling_graph_replay_ms_per_block": ms_graph,
        "sampling_launches_per_block": 3,
        "block_bytes": block_bytes, "workspace_bytes": wsb, "algorithmic_bytes": alg_bytes,
        "achieved_bytes_per_s": alg_bytes / (min(ms_idle, ms_graph) * 1e-3),
        "block_mass": mass, "all_words_valid": valid,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
