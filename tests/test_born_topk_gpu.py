"""The k most probable elements of amplitude blocks on the device: ops.born_topk (csrc/tq_topk.hip)
against the numpy reference (born_topk_ref.py), and sampling.BlockTopK end to end.  Everything is
exact: index, prob and count are compared with np.array_equal.  The kernels walk the block in
tiles of 4096 elements (256 lanes x 16) grouped into at most 1024 spans, select the threshold key
digit by digit (11 exponent bits, then 4 x 13 mantissa bits) and sort at most 4096 survivors, so
the sizes sit on either side of a wave and a tile, reach more than one tile per span, and the key
sets differ in one digit at a time."""
import functools

import numpy as np
import pytest

from born_ref import born_p, index_of_word, words_reference
from born_topk_ref import topk_reference
from test_born_sample_gpu import _closed_bits_ok, _exact_case, _random_case, _task

pytestmark = pytest.mark.gpu

SENT = -7
KS = (1, 64, 65, 4096)


def _run(dev, a, k, **kw):
    import torch
    from tneq_qc_amd import ops
    ta = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(dev)
    idx, prob, count = ops.born_topk(ta, k, **kw)
    torch.cuda.synchronize(dev)
    return idx.cpu().numpy(), prob.cpu().numpy(), count.cpu().numpy()


def _check(dev, a, ks, what=""):
    import torch
    ta = torch.from_numpy(np.array(a)).to(dev)
    for k in ks:
        got = _run(dev, ta, k)
        want = topk_reference(a, k)
        for g, w, name in zip(got, want, ("index", "prob", "count")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, name, g[:8], w[:8])
    return want


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 65537, (1 << 20) + 77])
def test_mass_ties(dev, n, dtype):
    """p in {0, 1, 2, 4}: whenever fewer than k elements lie above it, the cut falls inside a tie
    class and the lowest indices of the class win."""
    a = _exact_case(n, dtype)[0]
    _check(dev, a, KS, (n, dtype))


def test_all_equal(dev):
    n = 3 * 4096 + 5
    a = np.ones(n, dtype=np.complex64)
    for k in KS:
        gi, gp, gc = _run(dev, a, k)
        m = min(k, n)
        assert np.array_equal(gi, np.arange(k)) and np.all(gp == 1.0) and gc.tolist() == [m]
    a[:n - 1] = 0
    for k in KS:
        gi, gp, gc = _run(dev, a, k)
        assert gi.tolist() == [n - 1] + [-1] * (k - 1) and gp.tolist() == [1.0] + [0.0] * (k - 1)
        assert gc.tolist() == [1]


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_ties_across_unit_boundaries(dev, dtype):
    n = (1 << 17) + 9
    top = [4095, 4096, 8191, 8192, 65535, 65536, n - 1]
    rng = np.random.default_rng(31)
    a = np.zeros(n, dtype=dtype)
    nchunks = (n + 4095) // 4096
    pos = set()
    i = 0
    while len(pos) < 300:                         # p = 2 in every chunk of 4096, the last short one too
        c = i % nchunks
        x = c * 4096 + int(rng.integers(0, min(4096, n - c * 4096)))
        i += 1
        if x not in top:
            pos.add(x)
    a[sorted(pos)] = 1 + 1j
    a[top] = 2
    assert set((np.array(sorted(pos)) // 4096).tolist()) == set(range(nchunks))
    _check(dev, a, (3, 7, 8, 150), dtype)


def _digit_sets():
    m = np.arange(2048)
    sets = {
        "low22_c64": (1 + 1j * (m * 2.0 ** -26)).astype(np.complex64),       # p = 1 + j^2 2^-52
        "middle_c64": (1 + m * 2.0 ** -23).astype(np.complex64),
        "low12_c128": (1 + m * 2.0 ** -52).astype(np.complex128),
        "exponent_c64": (2.0 ** np.arange(-60, 61)).astype(np.complex64),
        "exponent_c128": (2.0 ** np.arange(-60, 61)).astype(np.complex128),
    }
    return sets


@pytest.mark.parametrize("which", ["low22_c64", "middle_c64", "low12_c128", "exponent_c64", "exponent_c128"])
def test_digit_coverage(dev, which):
    vals = _digit_sets()[which]
    keys = born_p(vals).view(np.uint64)
    assert np.unique(keys).size == vals.size      # all distinct: no tie rule can hide a wrong digit
    if which == "low22_c64":
        assert np.all((keys >> np.uint64(22)) == (keys[0] >> np.uint64(22)))
    if which == "low12_c128":
        assert np.all((keys >> np.uint64(12)) == (keys[0] >> np.uint64(12))) and np.all(np.diff(keys.astype(np.int64)) > 0)
    if which.startswith("exponent"):
        assert np.all((keys & np.uint64((1 << 52) - 1)) == 0)
    n = 8192
    rng = np.random.default_rng(41)
    a = np.zeros(n, dtype=vals.dtype)
    a[rng.permutation(n)[:vals.size]] = vals
    _check(dev, a, (1, 100, 2048), which)


@pytest.mark.parametrize("n,dtype", [(1 << 20, "complex64"), (1 << 20, "complex128"), ((1 << 22) + 3, "complex64")])
def test_random(dev, n, dtype):
    a = _random_case(n, dtype)[0]
    _check(dev, a, (4096,), (n, dtype))


def test_short_and_special(dev):
    n = 5000
    # fewer than k positives
    a = np.zeros(n, dtype=np.complex64)
    a[[7, 4096, 4999]] = [0.5, 2, 1j]
    gi, gp, gc = _run(dev, a, 64)
    assert gi.tolist() == [4096, 4999, 7] + [-1] * 61 and gp.tolist() == [4.0, 1.0, 0.25] + [0.0] * 61 and gc.tolist() == [3]
    # all zeros
    gi, gp, gc = _run(dev, np.zeros(n, dtype=np.complex128), 64)
    assert np.all(gi == -1) and np.all(gp == 0) and gc.tolist() == [0]
    # k > n
    a = np.array([0.5, 0, 2j], dtype=np.complex64)
    _check(dev, a, (8, 4096))
    # NaN never, +inf first and in index order
    a = np.ones(n, dtype=np.complex64)
    a[[3, 4500]] = np.nan
    a[[4097, 12, 4998]] = np.inf
    a[100] = complex(0, -np.inf)
    want = _check(dev, a, (1, 3, 4, 64, 4096))
    assert want[0][:6].tolist() == [12, 100, 4097, 4998, 0, 1] and 3 not in want[0] and 4500 not in want[0]
    assert want[2].tolist() == [4096]
    # the issue's hand-written cases, on the device
    _check(dev, np.array([1, np.inf, np.nan, 0, 2, 3e30], dtype=np.complex64), (4, 6))
    _check(dev, np.array([1e-160, 2e-160, 1e-170, 0], dtype=np.complex128), (2, 4))


def test_deterministic(dev):
    import torch
    from tneq_qc_amd import ops
    a = _random_case(1 << 20, "complex64")[0]
    ta = torch.from_numpy(np.array(a)).to(dev)
    r1 = ops.born_topk(ta, 4096)
    r2 = ops.born_topk(ta, 4096)
    torch.cuda.synchronize(dev)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    assert torch.equal(r1[1].view(torch.int64), r2[1].view(torch.int64))


def test_capture(dev):
    """One born_topk call with preallocated buffers captured into a graph on a side stream (the
    launch sequence depends on (dtype, n, k) only); replayed on new data it equals an eager call
    and the reference."""
    import torch
    from tneq_qc_amd import ops
    n, k = (1 << 14) + 5, 300
    a0 = _random_case(1 << 20, "complex64")[0][:n]
    rng = np.random.default_rng(78)
    a1 = rng.choice(np.array([0, 1, 1 + 1j, 2, 0.5], dtype=np.complex64), size=n)   # ties at the cut
    ta = torch.from_numpy(np.array(a0)).to(dev)
    out = torch.empty(k, dtype=torch.int64, device=dev)
    prob = torch.empty(k, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(ops.born_topk_workspace_size(torch.complex64, n, k), dtype=torch.uint8, device=dev)
    kw = dict(out=out, prob=prob, count=count, workspace=ws)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.born_topk(ta, k, **kw)      # warm: the code object is loaded before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.born_topk(ta, k, **kw)
    ta.copy_(torch.from_numpy(a1))
    ws.fill_(0xA5)                      # the call zeroes what it counts in
    torch.cuda.synchronize(dev)
    g.replay()
    torch.cuda.synchronize(dev)
    got = (out.clone(), prob.clone(), count.clone())
    want = ops.born_topk(ta, k)
    torch.cuda.synchronize(dev)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    for x, y in zip(got, topk_reference(a1, k)):
        assert np.array_equal(x.cpu().numpy(), y)


def test_arguments(dev):
    import torch
    from tneq_qc_amd import ops
    n, k = 4097, 16
    ta = torch.ones(n, dtype=torch.complex64, device=dev)
    out = torch.full((k,), SENT, dtype=torch.int64, device=dev)
    prob = torch.full((k,), float(SENT), dtype=torch.float64, device=dev)
    count = torch.full((1,), SENT, dtype=torch.int64, device=dev)
    kw = dict(out=out, prob=prob, count=count)
    with pytest.raises(ValueError):
        ops.born_topk(ta.real.contiguous(), k, **kw)                                      # a real dtype
    with pytest.raises(ValueError):
        ops.born_topk(torch.ones(2 * n, dtype=torch.complex64, device=dev)[::2], k, **kw)  # strided
    with pytest.raises(ValueError):
        ops.born_topk(ta, k, workspace=torch.empty(8, dtype=torch.uint8, device=dev), **kw)  # short
    with pytest.raises(ValueError):
        ops.born_topk(ta, 0, **kw)
    with pytest.raises(ValueError):
        ops.born_topk(ta, 4097, **kw)
    with pytest.raises(ValueError):
        ops.born_topk(ta, k + 1, **kw)                                                    # wrong-sized out
    with pytest.raises(ValueError):
        ops.born_topk(ta, k, out=out, prob=prob[:8], count=count)
    torch.cuda.synchronize(dev)
    assert torch.all(out == SENT) and torch.all(prob == SENT) and torch.all(count == SENT)
    # ... and the same buffers are written by a good call
    ops.born_topk(ta, k, **kw)
    torch.cuda.synchronize(dev)
    assert out.tolist() == list(range(k)) and torch.all(prob == 1.0) and count.tolist() == [k]


def test_bit_scatter(dev):
    import torch
    from tneq_qc_amd import ops
    axes = [9, 3, 40, 0, 62, 17]
    base = (1 << 5) | (1 << 61) | (1 << 20) | (1 << 1)
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype(np.complex64)
    a[[4, 9]] = 0
    gi, gp, gc = _run(dev, a, 64)
    gw, gq, gd = _run(dev, a, 64, axis_qubit=axes, base=base)
    want = topk_reference(a, 64)
    assert np.array_equal(gi, want[0]) and gc.tolist() == [62] and gd.tolist() == [62]
    assert np.array_equal(gw, words_reference(gi, axes, base))     # -1 stays -1
    assert gw[-2:].tolist() == [-1, -1]
    assert np.array_equal(gq, gp) and np.array_equal(gp, want[1])
    ta = torch.from_numpy(a).to(dev)
    out = torch.full((64,), SENT, dtype=torch.int64, device=dev)
    for bad_axes, bad_base in ((axes[:5], base), ([9, 3, 40, 0, 62, 9], base), ([9, 3, 40, 0, 63, 17], base),
                               (axes, base | (1 << 40))):
        with pytest.raises(ValueError):
            ops.born_topk(ta, 64, axis_qubit=bad_axes, base=bad_base, out=out)
    torch.cuda.synchronize(dev)
    assert torch.all(out == SENT)


# ---- BlockTopK ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [16, 4096])
@pytest.mark.parametrize("inflight,group", [(2, 1), (2, 2)])
def test_block_topk_end_to_end(dev, which, inflight, group):
    from tneq_qc_amd.sampling import BlockTopK
    task = _task(which)
    blocks = [0, 3, 5, 9][:inflight * group]     # every slot runs once: its amplitudes survive
    k = 64
    sel = BlockTopK(task, blocks, k, inflight=inflight, group=group, device=dev)
    res = [sel.step() for _ in blocks]
    sel.synchronize()
    for j, b in enumerate(blocks):
        words, prob, count = (t.cpu().numpy() for t in res[j])
        # the truth is the pipeline's own amplitude output of this block
        amps = sel.slots[(j // group) % inflight].outs[j % group].cpu().numpy().reshape(-1)
        assert amps.size == which
        m = int(count[0])
        assert 0 < m <= min(k, which)
        assert _closed_bits_ok(task, b, words[:m]), b
        idx = np.array([index_of_word(w, task.open_qubits) for w in words[:m].tolist()], dtype=np.int64)
        want = topk_reference(amps, k)
        assert want[2].tolist() == [m]
        assert np.array_equal(idx, want[0][:m]) and np.array_equal(prob, want[1])
        assert np.all(words[m:] == -1) and np.all(prob[m:] == 0)
        if which == 16:
            assert m <= 16 and np.all(words[16:] == -1) and np.all(prob[16:] == 0)
    sel.close()


def test_block_topk_run_close(dev):
    import torch
    from tneq_qc_amd.sampling import BlockTopK
    task = _task(16)
    blocks = [0, 3, 5, 9, 14]                    # (2, 2): the last group is partial
    sel = BlockTopK(task, blocks, 8, inflight=2, group=2, device=dev)
    res = sel.run()
    assert len(res) == 5
    for b, (words, prob, count) in zip(blocks, res):
        assert words.device.type == "cpu" and words.shape == (8,) and prob.shape == (8,) and count.shape == (1,)
        m = int(count[0])
        assert m > 0 and _closed_bits_ok(task, b, words[:m].numpy()), b
        assert torch.all(prob[:m] > 0) and torch.all(prob[:m - 1] >= prob[1:m])
    assert len({tuple(r[0].tolist()) for r in res}) == 5      # other closed bits: other words
    keep = [tuple(t.clone() for t in r) for r in res]
    sel.step()
    sel.synchronize()
    for r, q in zip(res, keep):
        assert all(torch.equal(x, y) for x, y in zip(r, q))
    sel.close()
    with pytest.raises(RuntimeError):
        sel.step()
    sel.close()                                  # idempotent
