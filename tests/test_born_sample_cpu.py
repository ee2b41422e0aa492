"""Born-rule block sampling, the parts that need no GPU: the numpy reference the GPU tests compare
against, the host-only workspace query, and the argument checks that fire before a device is
touched."""
import types

import numpy as np
import pytest

from born_ref import born_reference, words_reference, index_of_word


def test_reference_counts_follow_the_distribution():
    """u_j = (j + 0.5) / 65536: the thresholds are a uniform lattice of spacing S1 / 65536, so an
    interval of length p_i holds 65536 p_i / S1 lattice points give or take one."""
    a = np.array([0.5, 0, 1 + 1j, 0.25j, 0, 2, 0.125, 0], dtype=np.complex128)
    m = 65536
    u = (np.arange(m) + 0.5) / m
    index, prob, C, S1, S2 = born_reference(a, u)
    p = a.real ** 2 + a.imag ** 2
    assert S1 == p.sum() and S2 == (p * p).sum()
    counts = np.bincount(index, minlength=a.size)
    assert np.all(np.abs(counts - m * p / S1) <= 1.0)
    assert np.all(counts[p == 0] == 0)
    assert np.array_equal(prob, p[index])


def test_reference_fallback_and_degenerate():
    a = np.array([0, 1, 0, 1j, 0], dtype=np.complex64)
    index, prob, _, S1, _ = born_reference(a, [0.0, 0.49, 0.5, 1.0, 2.0, np.nan])
    assert S1 == 2.0
    assert index.tolist() == [1, 1, 3, 3, 3, 3] and np.all(prob == 1.0)
    index, prob, _, S1, _ = born_reference(np.zeros(4, dtype=np.complex64), [0.3])
    assert index.tolist() == [-1] and prob.tolist() == [0.0] and S1 == 0.0
    index, _, _, S1, _ = born_reference(np.array([1, np.nan], dtype=np.complex64), [0.3])
    assert index.tolist() == [-1] and np.isnan(S1)


def test_words_reference_round_trip():
    axes = [9, 3, 40, 0, 62, 17]
    base = (1 << 5) | (1 << 61) | (1 << 20)
    idx = np.array([0, 1, 32, 63, 21, -1])
    w = words_reference(idx, axes, base)
    assert w[0] == base and w[1] == base | (1 << 17) and w[2] == base | (1 << 9) and w[5] == -1
    assert [index_of_word(x, axes) for x in w[:5]] == idx[:5].tolist()


def test_workspace_query_needs_no_gpu():
    from tneq_qc_amd import _lib
    L = _lib.lib()
    q = L.tq_born_sample_workspace
    assert q(_lib.TQ_C64, 1 << 20, 4096) > 0
    sizes = [q(_lib.TQ_C64, n, 4096) for n in (1, 2, 4095, 4096, 4097, 65536, 65537, 1 << 20, (1 << 22) + 3, 1 << 31)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for args in ((_lib.TQ_F32, 1 << 20, 4096), (_lib.TQ_F64, 16, 1), (_lib.TQ_C64, 0, 4096),
                 (_lib.TQ_C64, (1 << 31) + 1, 1), (_lib.TQ_C128, 16, -1), (_lib.TQ_C128, 16, 1 << 31)):
        assert q(*args) == 0
        assert "born_sample" in _lib.last_error()


def test_born_sample_refuses_cpu_tensors():
    import torch
    from tneq_qc_amd import ops
    with pytest.raises(ValueError):
        ops.born_sample(torch.ones(8, dtype=torch.complex64), torch.rand(4, dtype=torch.float64))


def test_block_sampler_refuses_64_qubits_before_touching_a_device():
    from tneq_qc_amd.sampling import BlockSampler
    task = types.SimpleNamespace(open_qubits=list(range(20, 40)),
                                 fixed_bits={q: 0 for q in range(64) if not 20 <= q < 40})
    with pytest.raises(ValueError, match="qubits"):
        BlockSampler(task, [0], draws=16)
