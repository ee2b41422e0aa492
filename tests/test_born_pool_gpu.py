"""Sampling across amplitude blocks on the device: ops.born_pool_sample / ops.born_pool_merge
(csrc/tq_born.hip) against the numpy reference of the weighted reservoir (born_pool_ref.py), and
sampling.PoolSampler end to end.  The candidates come from the kernels of born_sample (chunks of
4096 elements, groups of 16 chunks); the accepted draws are resolved in tiles of 1024, so the draw
counts sit on either side of a tile."""
import ctypes
import functools

import numpy as np
import pytest

from born_pool_ref import merge_reference, pool_reference, pool_step, window_count
from born_ref import born_p, check_draws, index_of_word, words_reference

pytestmark = pytest.mark.gpu

SENT = -7
Q = 2.0 ** -20


def _exact_block(rng, n, dtype):
    a = rng.choice(np.array([0, 1, 1 + 1j, 2], dtype=dtype), size=n)
    if n == 1:
        a[:] = 2
    if n >= 4:
        a[0] = a[-1] = 0
    if not np.any(a != 0):
        a[n // 2] = 1 + 1j
    return a


@functools.lru_cache(maxsize=None)
def _exact_case(n, dtype, draws, nblocks=5, seed=0):
    """Blocks of amplitudes from {0, 1, 1+1j, 2} (every sum an exact integer in any order), block 3
    all zero and block 4 with one NaN amplitude; u = (m + 0.5) / S1 cannot cross an integer and v is
    a multiple of 2^-20, so v W' is exact (W' < 2^33)."""
    rng = np.random.default_rng(3000 + n + 7 * draws + seed)
    blocks, U, V = [], [], []
    for b in range(nblocks):
        a = _exact_block(rng, n, dtype)
        if b == 3:
            a[:] = 0
        if b == 4:
            a[n // 3] = np.nan
        S1 = born_p(a).sum()
        if np.isfinite(S1) and S1 > 0:
            m = rng.integers(0, int(S1), size=draws)
            m[0] = 0
            m[-1] = int(S1) - 1
            u = (m + 0.5) / S1
            assert np.array_equal(np.floor(u * S1), m)
        else:
            u = rng.random(draws)
        v = rng.integers(0, 1 << 20, size=draws) * Q
        v[0] = 0.0
        if draws > 3:
            v[1], v[2], v[3] = 1.0, np.nan, 1.0 - Q
        blocks.append(a)
        U.append(u)
        V.append(v)
    U, V = np.array(U), np.array(V)
    for x in blocks + [U, V]:
        x.setflags(write=False)
    return blocks, U, V


def _dev(x, dev):
    import torch
    return torch.from_numpy(np.array(x)).to(dev)


def _fresh(dev, draws):
    import torch
    return (torch.full((draws,), SENT, dtype=torch.int64, device=dev),
            torch.full((draws,), float(SENT), dtype=torch.float64, device=dev),
            torch.zeros(4, dtype=torch.float64, device=dev))


def _fold(dev, blocks, U, V, state=None, axis_qubit=None, bases=None):
    """One born_pool_sample call per block into one reservoir; host copies of (index, prob, pool,
    stats) after every call, and the device reservoir."""
    import torch
    from tneq_qc_amd import ops
    draws = U.shape[1]
    index, prob, pool = state if state is not None else _fresh(dev, draws)
    snaps = []
    for k, a in enumerate(blocks):
        kw = {} if axis_qubit is None else dict(axis_qubit=axis_qubit, base=bases[k])
        _, _, _, stats = ops.born_pool_sample(_dev(a, dev), _dev(U[k], dev), _dev(V[k], dev), index, prob, pool, **kw)
        snaps.append((index.clone(), prob.clone(), pool.clone(), stats))
    torch.cuda.synchronize(dev)
    return [tuple(t.cpu().numpy() for t in s) for s in snaps], (index, prob, pool)


def _ref_fold(blocks, U, V):
    """The reference, call by call, from the same sentinel-filled reservoir."""
    draws = U.shape[1]
    index = np.full(draws, SENT, dtype=np.int64)
    prob = np.full(draws, float(SENT))
    source = np.full(draws, -1, dtype=np.int64)
    pool = np.zeros(4)
    out = []
    for k, a in enumerate(blocks):
        stats, _ = pool_step(a, U[k], V[k], index, prob, source, pool, k)
        out.append((index.copy(), prob.copy(), pool.copy(), stats, source.copy()))
    return out


def _check_exact(dev, blocks, U, V):
    got, _ = _fold(dev, blocks, U, V)
    want = _ref_fold(blocks, U, V)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), k
        assert np.array_equal(g[1], w[1]), k
        assert np.array_equal(g[2], w[2]), (k, g[2], w[2])
        assert np.array_equal(g[3], w[3], equal_nan=True), (k, g[3], w[3])
    assert want[-1][2][2] == 3.0 and want[3][2][3] == 0.0 and want[4][2][3] == 0.0
    assert np.all(got[-1][0] >= 0) and np.all(got[-1][1] > 0)


@pytest.mark.parametrize("draws", [1, 1023, 1025, 4096])
@pytest.mark.parametrize("n", [1, 65, 4097, 65537, (1 << 20) + 77])
def test_exact(dev, n, draws):
    _check_exact(dev, *_exact_case(n, "complex64", draws))


@pytest.mark.parametrize("draws", [1, 1023, 1025, 4096])
@pytest.mark.parametrize("n", [4097, 65537])
def test_exact_complex128(dev, n, draws):
    _check_exact(dev, *_exact_case(n, "complex128", draws))


def test_first_block_contributes_nothing(dev):
    """A zero block first: the pool stays empty and the reservoir untouched; the next block then
    takes every slot whatever v is (1.0 and NaN among them)."""
    n, draws = 4097, 1025
    blocks, U, V = _exact_case(n, "complex64", draws)
    blocks = [blocks[3], blocks[0], blocks[1]]
    U, V = U[[3, 0, 1]], V[[3, 0, 1]].copy()
    V[1, :] = 1.0
    V[1, ::2] = np.nan
    got, _ = _fold(dev, blocks, U, V)
    assert np.all(got[0][0] == SENT) and np.all(got[0][1] == SENT) and np.all(got[0][2] == 0)
    assert got[0][3].tolist() == [0.0, 0.0]
    want = _ref_fold(blocks, U, V)
    assert np.all(want[1][4] == 1)
    for g, w in zip(got, want):
        assert all(np.array_equal(x, y) for x, y in zip(g, w[:4]))
    assert got[1][2][3] == draws and got[1][2][2] == 1.0


@functools.lru_cache(maxsize=None)
def _random_case(n, seed, draws=4096, nblocks=5):
    rng = np.random.default_rng(seed)
    blocks = []
    for b in range(nblocks):
        a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        a[rng.random(n) < 0.3] = 0
        a[:2] = 0
        a[-2:] = 0
        a *= 0.5 + b          # unequal masses
        blocks.append(a)
    U, V = rng.random((nblocks, draws)), rng.random((nblocks, draws))
    U[0, 0], U[0, 1] = 0.0, 1.0
    return blocks, U, V


@pytest.mark.parametrize("n,seed", [(4097, 41), (1 << 20, 42)])
def test_random(dev, n, seed):
    blocks, U, V = _random_case(n, seed)
    draws = U.shape[1]
    # no acceptance decision of the reference lies where the last bits of a sum decide it
    assert window_count(blocks, U, V) == 0
    rindex, rprob, rsource, rpool, raccepted = pool_reference(blocks, U, V)
    got, _ = _fold(dev, blocks, U, V)
    # a replaced slot changes (index, prob): the blocks' amplitudes are all different
    source = np.full(draws, -1)
    prev = (np.full(draws, SENT), np.full(draws, float(SENT)))
    for k, g in enumerate(got):
        changed = (g[0] != prev[0]) | (g[1] != prev[1])
        assert changed.sum() == g[2][3], k        # ... which pool[3] confirms
        source[changed] = k
        prev = g
    print(f"n={n}: accepted per block {[int(g[2][3]) for g in got]} reference {raccepted.tolist()}")
    assert np.array_equal(source, rsource)
    index, prob, pool, _ = got[-1]
    for b, a in enumerate(blocks):
        sel = np.flatnonzero(source == b)
        if sel.size:
            bad = check_draws(a, U[b][sel], index[sel])
            assert bad.size == 0, (b, sel[bad[:8]])
            assert np.array_equal(prob[sel], born_p(a)[index[sel]])
    assert np.all(prob > 0)
    print(f"n={n}: W rel {abs(pool[0] - rpool[0]) / rpool[0]:.3e}")
    assert abs(pool[0] - rpool[0]) <= 5 * n * 2.0 ** -52 * rpool[0]
    assert pool[2] == 5.0


def test_deterministic(dev):
    import torch
    blocks, U, V = _random_case(1 << 20, 42)
    _, r1 = _fold(dev, blocks, U, V)
    _, r2 = _fold(dev, blocks, U, V)
    torch.cuda.synchronize(dev)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def test_bit_scatter(dev):
    axes = [9, 3, 40, 0, 62, 17]
    bases = [(1 << 5) | (1 << 61), (1 << 20) | (1 << 1), 0, 1 << 33, (1 << 5) | (1 << 2)]
    blocks, U, V = _exact_case(64, "complex64", 1025)
    want = _ref_fold(blocks, U, V)[-1]
    got, _ = _fold(dev, blocks, U, V, axis_qubit=axes, bases=bases)
    index, source = want[0], want[4]
    assert len(set(source.tolist())) == 3 and len(set(index.tolist())) > 20
    expect = np.empty_like(index)
    for b in range(5):
        sel = source == b
        expect[sel] = words_reference(index[sel], axes, bases[b])
    assert np.array_equal(got[-1][0], expect)
    assert np.array_equal(got[-1][1], want[1])


def test_capture(dev):
    """One born_pool_sample call captured into a graph on a side stream with a dirty workspace;
    the pool is zeroed, then three replays on new amplitudes, u and v continue one pool."""
    import torch
    from tneq_qc_amd import ops
    n, draws = (1 << 14) + 5, 1025
    blocks, U, V = _exact_case(n, "complex64", draws, nblocks=3, seed=1)
    ta, tu, tv = _dev(blocks[0], dev), _dev(U[0], dev), _dev(V[0], dev)
    index, prob, pool = _fresh(dev, draws)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.full((ops.born_pool_workspace_size(torch.complex64, n, draws),), 0xFF, dtype=torch.uint8, device=dev)
    kw = dict(stats=stats, workspace=ws)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.born_pool_sample(ta, tu, tv, index, prob, pool, **kw)   # warm: the code object is loaded
    side.synchronize()
    ws.fill_(0xFF)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.born_pool_sample(ta, tu, tv, index, prob, pool, **kw)
    pool.zero_()
    index.fill_(SENT)
    prob.fill_(float(SENT))
    want = _ref_fold(blocks, U, V)
    for k in range(3):
        ta.copy_(_dev(blocks[k], dev))
        tu.copy_(_dev(U[k], dev))
        tv.copy_(_dev(V[k], dev))
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        for x, y in zip((index, prob, pool, stats), want[k][:4]):
            assert np.array_equal(x.cpu().numpy(), y), k
    assert pool[2].item() == 3.0


def test_merge(dev):
    import torch
    from tneq_qc_amd import ops
    n, draws = 4097, 1025
    blocks, U, V = _exact_case(n, "complex64", draws, nblocks=3, seed=2)
    blocks2, U2, V2 = _exact_case(n, "complex64", draws, nblocks=2, seed=3)
    _, A = _fold(dev, blocks, U, V)
    _, B = _fold(dev, blocks2, U2, V2)
    ra, rb = _ref_fold(blocks, U, V)[-1], _ref_fold(blocks2, U2, V2)[-1]
    rng = np.random.default_rng(9)
    v = rng.integers(0, 1 << 20, size=draws) * Q
    v[0], v[1], v[2] = 0.0, np.nan, 1.0
    tv = _dev(v, dev)
    keepB = tuple(t.clone() for t in B)
    # into an empty pool: B is copied whatever v is
    E = _fresh(dev, draws)
    ops.born_pool_merge(E[0], E[1], E[2], B[0], B[1], B[2], tv)
    torch.cuda.synchronize(dev)
    assert torch.equal(E[0], B[0]) and torch.equal(E[1], B[1])
    assert E[2].tolist() == B[2].tolist()[:3] + [float(draws)]
    # an empty B changes nothing but pool_a[3]
    Z = _fresh(dev, draws)
    keepA = tuple(t.clone() for t in A)
    ops.born_pool_merge(A[0], A[1], A[2], Z[0], Z[1], Z[2], tv)
    torch.cuda.synchronize(dev)
    assert torch.equal(A[0], keepA[0]) and torch.equal(A[1], keepA[1])
    assert A[2].tolist() == keepA[2].tolist()[:3] + [0.0]
    # B into A, exactly the reference (indices only: prob NULL on both sides, then with prob)
    wi, wp, ws_, wpool = merge_reference(ra[0], ra[1], ra[4], ra[2], rb[0], rb[1], rb[4], rb[2], v)
    assert 0 < wpool[3] < draws
    I2, P2 = A[0].clone(), A[2].clone()
    ops.born_pool_merge(I2, None, P2, B[0], None, B[2], tv)
    ops.born_pool_merge(A[0], A[1], A[2], B[0], B[1], B[2], tv)
    torch.cuda.synchronize(dev)
    assert np.array_equal(A[0].cpu().numpy(), wi) and np.array_equal(A[1].cpu().numpy(), wp)
    assert np.array_equal(A[2].cpu().numpy(), wpool)
    assert torch.equal(I2, A[0]) and torch.equal(P2, A[2])
    for x, y in zip(B, keepB):
        assert torch.equal(x, y)


def test_arguments(dev):
    import torch
    from tneq_qc_amd import _lib, ops
    n, draws = 4096, 16
    f64 = dict(dtype=torch.float64, device=dev)
    ta = torch.ones(n, dtype=torch.complex64, device=dev)
    tu, tv = torch.rand(draws, **f64), torch.rand(draws, **f64)
    index, prob, pool = _fresh(dev, draws)
    pool.fill_(float(SENT))
    stats = torch.full((2,), float(SENT), **f64)
    wsb = ops.born_pool_workspace_size(torch.complex64, n, draws)
    ws = torch.empty(wsb + 8, dtype=torch.uint8, device=dev)
    axes = list(range(12))
    bad = [
        lambda: ops.born_pool_sample(ta.real.contiguous(), tu, tv, index, prob, pool, stats=stats),      # a real dtype
        lambda: ops.born_pool_sample(ta, tu.float(), tv, index, prob, pool, stats=stats),                # float32 u
        lambda: ops.born_pool_sample(ta, tu, tv.float(), index, prob, pool, stats=stats),                # float32 v
        lambda: ops.born_pool_sample(ta, tu, tv[:-1], index, prob, pool, stats=stats),                   # short v
        lambda: ops.born_pool_sample(ta, tu, tv, index[:-1], prob, pool, stats=stats),                   # short index
        lambda: ops.born_pool_sample(ta, tu, tv, index, prob[:-1], pool, stats=stats),                   # short prob
        lambda: ops.born_pool_sample(ta, tu, tv, index, prob, pool[:3], stats=stats),                    # short pool
        lambda: ops.born_pool_sample(ta, tu[:0], tv[:0], index[:0], prob[:0], pool, stats=stats),        # n_draws = 0
        lambda: ops.born_pool_sample(ta, tu, tv, index, prob, pool, stats=stats, workspace=ws[:wsb - 8]),   # too small
        lambda: ops.born_pool_sample(ta, tu, tv, index, prob, pool, stats=stats, workspace=ws[4:]),      # misaligned
        lambda: ops.born_pool_sample(ta, tu, tv, index, prob, pool, stats=stats, axis_qubit=axes, base=1 << 5),
        lambda: ops.born_pool_sample(ta, tu, tv, index, prob, pool, stats=stats, axis_qubit=axes[:11]),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    # null pointers and n_draws = 0 at the C ABI
    L = _lib.lib()
    vp = ctypes.c_void_p
    good = [vp(ta.data_ptr()), draws, vp(tu.data_ptr()), vp(tv.data_ptr()), vp(index.data_ptr()), vp(prob.data_ptr()),
            vp(pool.data_ptr()), vp(stats.data_ptr()), 0, None, 0, vp(ws.data_ptr()), wsb, vp(0)]
    for at in (0, 2, 3, 4, 6, 7, 11):
        args = list(good)
        args[at] = vp(None)
        assert L.tq_born_pool_sample(_lib.TQ_C64, n, *args) == _lib.TQ_ERR_INVALID, at
        assert "born_pool" in _lib.last_error()
    args = list(good)
    args[1] = 0
    assert L.tq_born_pool_sample(_lib.TQ_C64, n, *args) == _lib.TQ_ERR_INVALID
    # the merge
    B = _fresh(dev, draws)
    mws = torch.empty(_lib.TQ_BORN_POOL_MERGE_WORKSPACE + 8, dtype=torch.uint8, device=dev)
    for f in (lambda: ops.born_pool_merge(index, prob, pool, B[0], None, B[2], tv),
              lambda: ops.born_pool_merge(index, prob, pool, B[0], B[1], B[2], tv[:-1]),
              lambda: ops.born_pool_merge(index, prob, pool, B[0][:-1], B[1], B[2], tv),
              lambda: ops.born_pool_merge(index, prob, pool, B[0], B[1], B[2], tv, workspace=mws[:32]),
              lambda: ops.born_pool_merge(index, prob, pool, B[0], B[1], B[2], tv, workspace=mws[4:]),
              lambda: ops.born_pool_merge(index, prob, pool, index, prob, pool, tv)):
        with pytest.raises(ValueError):
            f()
    mgood = [draws, vp(tv.data_ptr()), vp(index.data_ptr()), vp(prob.data_ptr()), vp(pool.data_ptr()),
             vp(B[0].data_ptr()), vp(B[1].data_ptr()), vp(B[2].data_ptr()), vp(mws.data_ptr()), 64, vp(0)]
    for at in (1, 2, 4, 5, 7, 8):
        args = list(mgood)
        args[at] = vp(None)
        assert L.tq_born_pool_merge(*args) == _lib.TQ_ERR_INVALID, at
    torch.cuda.synchronize(dev)
    assert torch.all(index == SENT) and torch.all(prob == SENT) and torch.all(pool == SENT) and torch.all(stats == SENT)
    # ... and the same buffers are written by a good call
    pool.zero_()
    ops.born_pool_sample(ta, tu, tv, index, prob, pool, stats=stats, workspace=ws[:wsb])
    torch.cuda.synchronize(dev)
    assert torch.all(index >= 0) and torch.all(prob == 1.0) and stats.tolist() == [float(n), float(n)]
    assert pool.tolist() == [float(n), float(n), 1.0, float(draws)]


# ---- PoolSampler -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _task():
    from tneq_qc_amd.circuits import BrickWall, amplitude_task
    return amplitude_task(BrickWall(12, 6, 2), list(range(4, 8)), cut=6, n_slice=2, defer=(2, 2))


def _merge_window(Wa, Wb, v, n):
    W1 = Wa + Wb
    return 0 if Wa == 0 else int((np.abs(v * W1 - Wb) <= 8 * n * 2.0 ** -52 * W1).sum())


@pytest.mark.parametrize("inflight,group", [(2, 1), (2, 2)])
def test_pool_sampler_end_to_end(dev, inflight, group):
    """The whole 12-qubit circuit as 256 blocks of 16 amplitudes.  The truth is the plain
    pipeline's amplitudes; the reference restates the sampler's bookkeeping: block k folds into
    the reservoir of slot (k div group) mod inflight, and the slots merge in slot order.  (The
    uniforms' seed needs no choosing: at n = 16 the window 8 n 2^-52 W' around an acceptance
    boundary is 3e-14 W' wide, and the test asserts that no decision falls into it.)"""
    import torch
    from tneq_qc_amd.circuits import with_batch
    from tneq_qc_amd.sampling import BlockPipeline, PoolSampler, _word_of
    task = _task()
    blocks = list(range(256))
    draws = 512
    pipe = BlockPipeline(task, blocks, inflight=inflight, group=group, device=dev)
    truth = [t.numpy().reshape(-1) for t in pipe.run()]
    pipe.close()
    rng = np.random.default_rng(23)
    UV = rng.random((256, 2, draws))
    MV = rng.random((inflight, draws))
    samp = PoolSampler(task, blocks, draws, inflight=inflight, group=group, device=dev,
                       uniforms=torch.from_numpy(UV).to(dev))
    tmv = torch.from_numpy(MV).to(dev)
    for _ in blocks:
        assert samp.step() is None
    words, prob, pool = (t.cpu().numpy() for t in samp.result(tmv))
    again = samp.result(tmv)
    assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip((words, prob, pool), again))

    # the reference: slot reservoirs, then the slot-order merge
    windows = 0
    out = (np.full(draws, -1, dtype=np.int64), np.zeros(draws), np.full(draws, -1, dtype=np.int64), np.zeros(4))
    for s in range(inflight):
        ks = [k for k in blocks if (k // group) % inflight == s]
        windows += window_count([truth[k] for k in ks], UV[ks, 0], UV[ks, 1])
        ri, rp, rs, rpool, _ = pool_reference([truth[k] for k in ks], UV[ks, 0], UV[ks, 1])
        rs = np.array(ks)[rs]
        windows += _merge_window(out[3][0], rpool[0], MV[s], 16)
        out = merge_reference(*out, ri, rp, rs, rpool, MV[s])
    assert windows == 0
    rindex, rprob, rsource, rpool = out

    # every word's closed bits name its source block, the open bits a draw of that block
    closed = {_word_of(with_batch(task, b).fixed_bits): b for b in blocks}
    open_mask = sum(1 << int(q) for q in task.open_qubits)
    source = np.array([closed[int(w) & ~open_mask] for w in words.tolist()])
    index = np.array([index_of_word(w, task.open_qubits) for w in words.tolist()])
    assert np.array_equal(source, rsource)
    for b in np.unique(source):
        sel = np.flatnonzero(source == b)
        assert check_draws(truth[b], UV[b, 0][sel], index[sel]).size == 0, b
        assert np.array_equal(prob[sel], born_p(truth[b])[index[sel]])
    assert np.all(prob > 0)
    print(f"({inflight}, {group}): W = {pool[0]!r}, {len(np.unique(source))} source blocks")
    assert abs(pool[0] - 1.0) <= 1e-5
    assert pool[2] == 256.0
    assert abs(pool[0] - rpool[0]) <= 5 * 16 * 2.0 ** -52 * rpool[0] and pool[3] == rpool[3]

    # sampling goes on: the reservoirs were left intact
    for _ in blocks:
        samp.step()
    assert samp.result(tmv)[2][2].item() == 512.0
    w2, p2, pool2 = samp.result()                # merge uniforms from the sampler's own generator
    assert pool2[2].item() == 512.0 and bool((w2 >= 0).all()) and bool((p2 > 0).all())
    samp.reset()
    for _ in blocks[:5]:
        samp.step()
    assert samp.result(tmv)[2][2].item() == 5.0
    samp.close()
    with pytest.raises(RuntimeError):
        samp.step()
    samp.close()                                 # idempotent


def test_pool_sampler_seed(dev):
    from tneq_qc_amd.sampling import PoolSampler
    task = _task()
    blocks = list(range(256))
    res = []
    for seed in (3, 3, 4):
        samp = PoolSampler(task, blocks, 512, inflight=2, group=2, device=dev, seed=seed)
        words, prob, pool = samp.run()
        assert words.device.type == "cpu" and words.shape == (512,) and prob.shape == (512,) and pool.shape == (4,)
        assert pool[2] == 256.0 and bool((prob > 0).all())
        res.append(words)
        samp.close()
    import torch
    assert torch.equal(res[0], res[1])
    assert not torch.equal(res[0], res[2])
