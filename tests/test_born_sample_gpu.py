"""Born-rule sampling of amplitude blocks on the device: ops.born_sample (csrc/tq_born.hip) against
the numpy reference (born_ref.py), and sampling.BlockSampler end to end.  The kernel works in
chunks of 4096 elements (256 lanes x 16) and groups of 16 chunks, so the sizes sit on either side
of a wave, a chunk and a group, plus the production block (2^20), non-powers-of-two needing many
chunks, and one size with more than 256 groups (the base scan's tile)."""
import functools

import numpy as np
import pytest

from born_ref import born_p, born_reference, check_draws, index_of_word, words_reference

pytestmark = pytest.mark.gpu

DRAWS = 4096
SENT = -7


@functools.lru_cache(maxsize=None)
def _exact_case(n, dtype):
    """Amplitudes from {0, 1, 1+1j, 2} (p in {0, 1, 2, 4}: every sum is an exact integer in any
    order) and uniforms (m + 0.5) / S1 that cannot cross an integer, plus u = 1.0 (fallback)."""
    rng = np.random.default_rng(1000 + n)
    a = rng.choice(np.array([0, 1, 1 + 1j, 2], dtype=dtype), size=n)
    if n == 1:
        a[:] = 2
    if n >= 4:
        a[0] = a[-1] = 0
    if n > (1 << 20):
        a[:5000] = 0
        a[-5000:] = 0
        a[300000:320000] = 0
    if not np.any(a != 0):
        a[n // 2] = 1 + 1j
    S1 = int(born_p(a).sum())
    m = rng.integers(0, S1, size=DRAWS - 1)
    m[0], m[1] = 0, S1 - 1
    u = np.concatenate([(m + 0.5) / S1, [1.0]])
    assert np.array_equal(np.floor(u[:-1] * float(S1)), m)   # t_j cannot cross an integer
    ref = born_reference(a, u)
    for x in (a, u) + tuple(r for r in ref if isinstance(r, np.ndarray)):
        x.setflags(write=False)
    return a, u, ref


@functools.lru_cache(maxsize=None)
def _random_case(n, dtype):
    rng = np.random.default_rng(2000 + n)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)
    a[rng.random(n) < 0.3] = 0
    a[:2] = 0
    a[-2:] = 0
    u = rng.random(DRAWS)
    u[0], u[1] = 0.0, 1.0
    ref = born_reference(a, u)
    for x in (a, u) + tuple(r for r in ref if isinstance(r, np.ndarray)):
        x.setflags(write=False)
    return a, u, ref


def _run(dev, a, u, **kw):
    import torch
    from tneq_qc_amd import ops
    idx, prob, stats = ops.born_sample(torch.from_numpy(np.array(a)).to(dev), torch.from_numpy(np.array(u)).to(dev), **kw)
    torch.cuda.synchronize(dev)
    return idx.cpu().numpy(), (None if prob is None else prob.cpu().numpy()), stats.cpu().numpy()


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) + 77])
def test_exact(dev, n, dtype):
    _check_exact(dev, *_exact_case(n, dtype))


def _check_exact(dev, a, u, ref):
    index, prob, C, S1, S2 = ref
    gi, gp, gs = _run(dev, a, u)
    p = born_p(a)
    assert np.array_equal(gi, index)
    assert np.array_equal(gp, p[index])
    assert gs[0] == S1 and gs[1] == S2
    assert np.all(gp > 0)


def test_exact_more_than_256_groups(dev):
    """Beyond 2^24 elements the base scan walks the groups in tiles of 256: 257 groups and a bit."""
    _check_exact(dev, *_exact_case.__wrapped__((1 << 24) + 70001, "complex64"))   # 134 MB: not cached


@pytest.mark.parametrize("n,dtype", [(4097, "complex64"), (1 << 20, "complex64"), ((1 << 22) + 3, "complex64"),
                                     (1 << 20, "complex128")])
def test_random(dev, n, dtype):
    a, u, (index, prob, C, S1, S2) = _random_case(n, dtype)
    gi, gp, gs = _run(dev, a, u)
    bad = check_draws(a, u, gi, C, S1)
    assert bad.size == 0, (bad[:8], gi[bad[:8]], index[bad[:8]])
    p = born_p(a)
    if dtype == "complex64":
        assert np.array_equal(gp, p[gi])
    else:
        assert np.all(np.abs(gp - p[gi]) <= 2 * np.spacing(p[gi]))
    assert np.all(gp > 0)
    print(f"n={n} {dtype}: S1 rel {abs(gs[0] - S1) / S1:.3e} S2 rel {abs(gs[1] - S2) / S2:.3e} "
          f"differs from searchsorted in {int((gi != index).sum())} draws")
    assert abs(gs[0] - S1) <= n * 2.0 ** -52 * S1
    assert abs(gs[1] - S2) <= n * 2.0 ** -52 * S2


def test_deterministic(dev):
    import torch
    from tneq_qc_amd import ops
    a, u, _ = _random_case(1 << 20, "complex64")
    ta, tu = torch.from_numpy(np.array(a)).to(dev), torch.from_numpy(np.array(u)).to(dev)
    r1 = ops.born_sample(ta, tu)
    r2 = ops.born_sample(ta, tu)
    torch.cuda.synchronize(dev)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def test_degenerate(dev):
    import torch
    from tneq_qc_amd import ops
    n = 5000
    u = np.linspace(0.0, 1.0, 64)
    gi, gp, gs = _run(dev, np.zeros(n, dtype=np.complex64), u)
    assert np.all(gi == -1) and np.all(gp == 0) and gs.tolist() == [0.0, 0.0]
    a = np.ones(n, dtype=np.complex64)
    a[4500] = np.nan
    gi, gp, gs = _run(dev, a, u)
    assert np.all(gi == -1) and np.all(gp == 0) and np.isnan(gs[0])
    # no draws: the index buffer is left alone, stats are still written
    out = torch.full((8,), SENT, dtype=torch.int64, device=dev)
    idx, prob, stats = ops.born_sample(torch.ones(n, dtype=torch.complex64, device=dev),
                                       torch.empty(0, dtype=torch.float64, device=dev), out=out)
    torch.cuda.synchronize(dev)
    assert idx.numel() == 0 and prob.numel() == 0
    assert torch.all(out == SENT)
    assert stats.tolist() == [float(n), float(n)]


def test_bit_scatter(dev):
    import torch
    from tneq_qc_amd import ops
    axes = [9, 3, 40, 0, 62, 17]
    base = (1 << 5) | (1 << 61) | (1 << 20) | (1 << 1)
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype(np.complex64)
    u = (np.arange(256) + 0.5) / 256
    gi, _, _ = _run(dev, a, u)
    gw, gp, _ = _run(dev, a, u, axis_qubit=axes, base=base)
    assert len(set(gi.tolist())) > 20
    assert np.array_equal(gw, words_reference(gi, axes, base))
    assert np.array_equal(gp, born_p(a)[gi])
    # -1 stays -1
    gw, _, _ = _run(dev, np.zeros(64, dtype=np.complex64), u, axis_qubit=axes, base=base)
    assert np.all(gw == -1)
    ta, tu = torch.from_numpy(a).to(dev), torch.from_numpy(u).to(dev)
    out = torch.full((256,), SENT, dtype=torch.int64, device=dev)
    for bad_axes, bad_base in ((axes[:5], base), ([9, 3, 40, 0, 62, 9], base), ([9, 3, 40, 0, 63, 17], base),
                               (axes, base | (1 << 40))):
        with pytest.raises(ValueError):
            ops.born_sample(ta, tu, axis_qubit=bad_axes, base=bad_base, out=out)
    torch.cuda.synchronize(dev)
    assert torch.all(out == SENT)


def test_arguments(dev):
    import torch
    from tneq_qc_amd import ops
    n = 4097
    ta = torch.ones(n, dtype=torch.complex64, device=dev)
    tu = torch.rand(16, dtype=torch.float64, device=dev)
    out = torch.full((16,), SENT, dtype=torch.int64, device=dev)
    prob = torch.full((16,), float(SENT), dtype=torch.float64, device=dev)
    stats = torch.full((2,), float(SENT), dtype=torch.float64, device=dev)
    kw = dict(out=out, prob=prob, stats=stats)
    with pytest.raises(ValueError):
        ops.born_sample(ta.real.contiguous(), tu, **kw)                  # a real dtype
    with pytest.raises(ValueError):
        ops.born_sample(ta, tu.float(), **kw)                            # float32 uniforms
    with pytest.raises(ValueError):
        ops.born_sample(torch.ones(2 * n, dtype=torch.complex64, device=dev)[::2], tu, **kw)   # strided
    with pytest.raises(ValueError):
        ops.born_sample(ta, tu, workspace=torch.empty(8, dtype=torch.uint8, device=dev), **kw)  # short
    torch.cuda.synchronize(dev)
    assert torch.all(out == SENT) and torch.all(prob == SENT) and torch.all(stats == SENT)
    # ... and the same buffers are written by a good call
    ops.born_sample(ta, tu, **kw)
    torch.cuda.synchronize(dev)
    assert torch.all(out >= 0) and torch.all(prob == 1.0) and stats.tolist() == [float(n), float(n)]


def test_capture(dev):
    """One born_sample call with preallocated outputs and workspace captured into a graph on a
    side stream (a linear chain of three launches); replayed on new data it equals an eager call."""
    import torch
    from tneq_qc_amd import ops
    n = (1 << 14) + 5
    a0, u0, _ = _random_case(n, "complex64")
    rng = np.random.default_rng(77)
    a1 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    u1 = rng.random(DRAWS)
    ta, tu = torch.from_numpy(np.array(a0)).to(dev), torch.from_numpy(np.array(u0)).to(dev)
    out = torch.empty(DRAWS, dtype=torch.int64, device=dev)
    prob = torch.empty(DRAWS, dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.born_workspace_size(torch.complex64, n, DRAWS), dtype=torch.uint8, device=dev)
    kw = dict(out=out, prob=prob, stats=stats, workspace=ws)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.born_sample(ta, tu, **kw)   # warm: the code object is loaded before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.born_sample(ta, tu, **kw)
    ta.copy_(torch.from_numpy(a1))
    tu.copy_(torch.from_numpy(u1))
    torch.cuda.synchronize(dev)
    g.replay()
    torch.cuda.synchronize(dev)
    got = (out.clone(), prob.clone(), stats.clone())
    want = ops.born_sample(ta, tu)
    torch.cuda.synchronize(dev)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert check_draws(a1, u1, got[0].cpu().numpy()).size == 0


# ---- BlockSampler ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _task(which):
    from tneq_qc_amd.circuits import BrickWall, amplitude_task
    if which == 16:
        return amplitude_task(BrickWall(12, 6, 2), list(range(4, 8)), cut=6, n_slice=2, defer=(2, 2))
    return amplitude_task(BrickWall(16, 6, 2), list(range(2, 14)), cut=8, n_slice=2, defer=(2, 2))


def _closed_bits_ok(task, b, words):
    from tneq_qc_amd.circuits import with_batch
    w = np.asarray(words).astype(np.int64)
    return all(np.all(((w >> q) & 1) == v) for q, v in with_batch(task, b).fixed_bits.items())


@pytest.mark.parametrize("which", [16, 4096])
@pytest.mark.parametrize("inflight,group", [(2, 1), (2, 2)])
def test_block_sampler_end_to_end(dev, which, inflight, group):
    import torch
    from tneq_qc_amd.sampling import BlockSampler
    task = _task(which)
    blocks = [0, 3, 5, 9][:inflight * group]     # every slot runs once: its amplitudes survive
    draws = 512
    u = np.random.default_rng(11).random((len(blocks), draws))
    u[0, 0], u[0, 1] = 0.0, 1.0
    samp = BlockSampler(task, blocks, draws, inflight=inflight, group=group, device=dev,
                        uniforms=torch.from_numpy(u).to(dev))
    res = [samp.step() for _ in blocks]
    samp.synchronize()
    for k, b in enumerate(blocks):
        words, prob, stats = (t.cpu().numpy() for t in res[k])
        # the truth is the pipeline's own amplitude output of this block
        amps = samp.slots[(k // group) % inflight].outs[k % group].cpu().numpy().reshape(-1)
        assert amps.size == which
        assert _closed_bits_ok(task, b, words), b
        idx = np.array([index_of_word(w, task.open_qubits) for w in words.tolist()])
        assert check_draws(amps, u[k], idx).size == 0, b
        p = born_p(amps)
        assert np.array_equal(prob, p[idx]) and np.all(prob > 0)
        S1 = np.cumsum(p)[-1]
        assert abs(stats[0] - S1) <= which * 2.0 ** -52 * S1
    samp.close()


def test_block_sampler_run_seed_close(dev):
    import torch
    from tneq_qc_amd.sampling import BlockSampler
    task = _task(16)
    blocks = [0, 3, 5, 9, 14]                    # (2, 2): the last group is partial
    samp = BlockSampler(task, blocks, 512, inflight=2, group=2, device=dev, seed=3)
    res = samp.run()
    assert len(res) == 5
    for b, (words, prob, stats) in zip(blocks, res):
        assert words.device.type == "cpu" and words.shape == (512,) and prob.shape == (512,) and stats.shape == (2,)
        assert _closed_bits_ok(task, b, words.numpy()), b
        assert torch.all(prob > 0) and stats[0] > 0
    keep = [tuple(t.clone() for t in r) for r in res]
    samp.step()
    samp.synchronize()
    for r, k in zip(res, keep):
        assert all(torch.equal(x, y) for x, y in zip(r, k))
    again = BlockSampler(task, blocks, 512, inflight=2, group=2, device=dev, seed=3).run()
    other = BlockSampler(task, blocks, 512, inflight=2, group=2, device=dev, seed=4).run()
    assert all(torch.equal(x[0], y[0]) for x, y in zip(res, again))
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(res, other))
    samp.close()
    with pytest.raises(RuntimeError):
        samp.step()
    samp.close()                                 # idempotent
