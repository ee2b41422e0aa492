#!/usr/bin/env python
"""What post-selection (the k most probable bitstrings of every block) costs the headline
pipeline, and what it replaces.

One process, C4, complex64, a 64-block window, `--inflight` x `--group` as bench.py's headline,
k = 4096 and k = 1:
  a. a plain `BlockPipeline`, `step()` timed exactly as bench.py's headline loop does (warm-up
     steps, synchronize, K steps + flush, synchronize), three runs;
  b. a `BlockTopK(k)`, timed the same way, the runs alternating with (a)'s;
  c. the top-k launches alone (`ops.born_topk` on one finished block, preallocated buffers) on an
     otherwise idle stream, issued eagerly and replayed from a graph, three runs each;
  d. the torch composition a user would otherwise write, on the same block and stream, timed the
     same way and alternating with (c): float64 re^2 + im^2, `torch.topk`, gather;
  e. the mean of 2^qubits x prob over the selected words of a few blocks (the linear XEB of the
     emitted set + 1), beside the same quantity over `BlockSampler`'s draws.
Prints one JSON object (profiles/born_topk.json is this output on an MI355X)."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--idle-calls", type=int, default=200)
    ap.add_argument("--xeb-blocks", type=int, default=8)
    args = ap.parse_args()

    import torch
    from tneq_qc_amd import ops
    from tneq_qc_amd.circuits import config_task
    from tneq_qc_amd.sampling import BlockPipeline, BlockSampler, BlockTopK

    dev = torch.device("cuda:0")
    task = config_task(args.config)
    blocks = list(range(max(64, args.inflight * args.group)))
    qubits = len(task.open_qubits) + len(task.fixed_bits)
    ks = (4096, 1)

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
    plain = BlockPipeline(task, blocks, **kw)
    sel = {k: BlockTopK(task, blocks, k, **kw) for k in ks}
    ms_plain, ms_sel = [], {k: [] for k in ks}
    for _ in range(3):
        ms_plain.append(timed(plain))
        for k in ks:
            ms_sel[k].append(timed(sel[k]))
    out = plain.slots[0].outs[0].clone()   # one finished block for the idle-stream timings
    plain.close()

    # (e) the emitted sets of a few blocks
    xeb = {}
    for k in ks:
        sel[k].reset()
        vals = []
        for words, prob, count in sel[k].run(args.xeb_blocks):
            vals.append(prob[:int(count[0])])
        xeb[k] = float(torch.cat(vals).mean() * 2.0 ** qubits)
        sel[k].close()
    samp = BlockSampler(task, blocks, 4096, **kw, seed=1)
    vals = [prob for words, prob, stats in samp.run(args.xeb_blocks)]
    xeb_born = float(torch.cat(vals).mean() * 2.0 ** qubits)
    samp.close()

    # (c), (d): the launches alone
    n = out.numel()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def eager(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.idle_calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.idle_calls

    def graphed(fn):
        """20 calls per replay (no host issue between the launches); None if not capturable."""
        side = torch.cuda.Stream(dev)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, stream=side):
                for _ in range(20):
                    fn()
        except Exception:
            return None
        graph.replay()
        torch.cuda.synchronize()

        def run():
            e0.record()
            for _ in range(10):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 200
        return run

    def torch_path(k):
        flat = out.reshape(-1)

        def fn():
            re, im = flat.real.to(torch.float64), flat.imag.to(torch.float64)
            p = re * re + im * im
            _, idx = torch.topk(p, k)
            return idx, torch.gather(p, 0, idx)
        return fn

    alone = {}
    for k in ks:
        wsb = ops.born_topk_workspace_size(out.dtype, n, k)
        bufs = dict(out=torch.empty(k, dtype=torch.int64, device=dev),
                    prob=torch.empty(k, dtype=torch.float64, device=dev),
                    count=torch.empty(1, dtype=torch.int64, device=dev),
                    workspace=torch.empty(wsb, dtype=torch.uint8, device=dev))
        ours = lambda: ops.born_topk(out, k, **bufs)   # noqa: E731
        theirs = torch_path(k)
        # the two paths agree on this block (indices may differ only among equal p)
        gi, gp, gc = ours()
        ti, tp = theirs()
        torch.cuda.synchronize()
        same = bool(torch.equal(gp[:int(gc[0])], tp[:int(gc[0])]))
        g_ours, g_theirs = graphed(ours), graphed(theirs)
        r = {"eager_ms": [], "graph_ms": [], "torch_eager_ms": [], "torch_graph_ms": []}
        for _ in range(3):
            r["eager_ms"].append(eager(ours))
            r["torch_eager_ms"].append(eager(theirs))
            r["graph_ms"].append(g_ours() if g_ours else None)
            r["torch_graph_ms"].append(g_theirs() if g_theirs else None)
        r["workspace_bytes"] = wsb
        r["probabilities_equal_torch"] = same
        alone[k] = r

    res = {
        "config": args.config, "device": torch.cuda.get_device_name(0), "dtype": "complex64",
        "inflight": args.inflight, "group": args.group, "blocks": len(blocks), "steps": args.steps,
        "warmup": args.warmup, "idle_calls": args.idle_calls, "block_elements": n, "qubits": qubits,
        "plain_ms_per_block_runs": ms_plain, "plain_ms_per_block": min(ms_plain),
        "topk_launches_per_block": 9,
        "xeb_blocks": args.xeb_blocks, "born_sampler_mean_2q_prob": xeb_born,
    }
    for k in ks:
        res[f"k{k}"] = {
            "topk_ms_per_block_runs": ms_sel[k], "topk_ms_per_block": min(ms_sel[k]),
            "topk_minus_plain_ms": min(ms_sel[k]) - min(ms_plain),
            "mean_2q_prob": xeb[k], **alone[k],
        }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
