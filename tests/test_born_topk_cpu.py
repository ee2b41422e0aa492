"""Block top-k select, the parts that need no GPU: the numpy reference the GPU tests compare
against, the host-only workspace query, and the argument checks that fire before a device is
touched."""
import types

import numpy as np
import pytest

from born_topk_ref import topk_reference


def test_reference_ties_by_index():
    a = np.array([1, 2, 1, 2, 0, 1, 2], dtype=np.complex64)
    index, prob, count = topk_reference(a, 5)
    assert index.tolist() == [1, 3, 6, 0, 2] and prob.tolist() == [4, 4, 4, 1, 1] and count.tolist() == [5]
    index, prob, count = topk_reference(a, 2)
    assert index.tolist() == [1, 3] and count.tolist() == [2]
    a = np.array([1j, 1, -1, -1j], dtype=np.complex128)
    assert topk_reference(a, 3)[0].tolist() == [0, 1, 2]


def test_reference_special_values():
    a = np.array([1, np.inf, np.nan, 0, 2, 3e30], dtype=np.complex64)
    index, prob, count = topk_reference(a, 4)
    assert index.tolist() == [1, 5, 4, 0] and count.tolist() == [4]
    assert prob[0] == np.inf and prob[2] == 4.0 and prob[3] == 1.0
    index, prob, count = topk_reference(a, 6)
    assert index.tolist() == [1, 5, 4, 0, -1, -1] and count.tolist() == [4] and prob[4:].tolist() == [0, 0]


def test_reference_denormal_and_underflow():
    a = np.array([1e-160, 2e-160, 1e-170, 0], dtype=np.complex128)
    index, prob, count = topk_reference(a, 4)
    assert index.tolist() == [1, 0, -1, -1] and count.tolist() == [2]
    assert 0 < prob[1] < prob[0] < np.finfo(np.float64).tiny       # denormal p; 1e-340 underflows to 0


def test_reference_k_larger_than_n():
    a = np.array([0.5, 0, 2j], dtype=np.complex64)
    index, prob, count = topk_reference(a, 8)
    assert index.tolist() == [2, 0] + [-1] * 6 and prob.tolist() == [4.0, 0.25] + [0.0] * 6 and count.tolist() == [2]


def test_workspace_query_needs_no_gpu():
    from tneq_qc_amd import _lib
    L = _lib.lib()
    q = L.tq_born_topk_workspace
    assert q(_lib.TQ_C64, 1 << 20, 4096) > 0 and q(_lib.TQ_C128, 1, 1) > 0
    sizes = [q(_lib.TQ_C64, n, 4096) for n in (1, 2, 4095, 4096, 4097, 65536, 65537, 1 << 20, (1 << 22) + 3, 1 << 31)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for args in ((_lib.TQ_F32, 1 << 20, 4096), (_lib.TQ_F64, 16, 1), (_lib.TQ_C64, 0, 4096),
                 (_lib.TQ_C64, (1 << 31) + 1, 1), (_lib.TQ_C128, 16, 0), (_lib.TQ_C128, 16, 4097)):
        assert q(*args) == 0
        assert "born_topk" in _lib.last_error()
    assert _lib.TQ_BORN_TOPK_MAX_K == 4096


def test_born_topk_refuses_cpu_tensors():
    import torch
    from tneq_qc_amd import ops
    with pytest.raises(ValueError):
        ops.born_topk(torch.ones(8, dtype=torch.complex64), 4)


def test_block_topk_refuses_64_qubits_before_touching_a_device():
    from tneq_qc_amd.sampling import BlockTopK
    task = types.SimpleNamespace(open_qubits=list(range(20, 40)),
                                 fixed_bits={q: 0 for q in range(64) if not 20 <= q < 40})
    with pytest.raises(ValueError, match="qubits"):
        BlockTopK(task, [0], k=16)
