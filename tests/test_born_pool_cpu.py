"""Sampling across amplitude blocks, the parts that need no GPU: the numpy reference of the
weighted reservoir the GPU tests compare against (born_pool_ref.py), the host-only workspace
query, the argument checks that fire before a device is touched, and the C ABI's declarations."""
import re
import types
from pathlib import Path

import numpy as np
import pytest

from born_pool_ref import merge_reference, pool_reference

ROOT = Path(__file__).resolve().parents[1]
DRAWS = 4096


def _mass_blocks():
    """Blocks of integer masses 64 : 128 : 192 : 256, a zero block and a second 256 block."""
    blocks = []
    for mass in (64, 128, 192, 256, 0, 256):
        a = np.zeros(300, dtype=np.complex64)
        a[7:7 + mass] = 1
        blocks.append(a)
    return blocks


def _within_five_sigma(counts, masses, draws):
    total = float(sum(masses))
    z = []
    for c, m in zip(counts, masses):
        q = m / total
        sd = np.sqrt(draws * q * (1 - q))
        if m == 0:
            assert c == 0
        else:
            z.append(abs(c - draws * q) / sd)
    print("z scores", np.round(z, 2))
    return max(z) <= 5.0


def test_reference_sources_follow_the_masses():
    blocks = _mass_blocks()
    masses = [64, 128, 192, 256, 0, 256]
    rng = np.random.default_rng(7)
    U, V = rng.random((6, DRAWS)), rng.random((6, DRAWS))
    index, prob, source, pool, accepted = pool_reference(blocks, U, V)
    counts = np.bincount(source, minlength=6)
    assert counts.sum() == DRAWS and counts[4] == 0
    assert _within_five_sigma(counts, masses, DRAWS)
    assert pool[0] == float(sum(masses)) and pool[1] == float(sum(masses)) and pool[2] == 5.0
    assert accepted[0] == DRAWS and accepted[4] == 0 and pool[3] == accepted[5]
    # every slot holds an element of its source block with p = 1
    assert np.all((index >= 7) & (index < 7 + np.array(masses)[source])) and np.all(prob == 1.0)


def test_reference_merge_is_one_pool_over_the_concatenation():
    blocks = _mass_blocks()
    masses = [64, 128, 192, 256, 0, 256]
    rng = np.random.default_rng(7)
    U, V = rng.random((6, DRAWS)), rng.random((6, DRAWS))
    whole = pool_reference(blocks, U, V)
    a = pool_reference(blocks[:3], U[:3], V[:3])
    b = pool_reference(blocks[3:], U[3:], V[3:], first=3)
    index, prob, source, pool = merge_reference(*a[:4], *b[:4], rng.random(DRAWS))
    assert np.array_equal(pool[:3], whole[3][:3])
    counts = np.bincount(source, minlength=6)
    assert counts.sum() == DRAWS and counts[4] == 0
    assert _within_five_sigma(counts, masses, DRAWS)
    assert pool[3] == (np.isin(source, [3, 4, 5])).sum()
    # an empty A takes everything, an empty B nothing
    empty = (np.full(DRAWS, -1), np.zeros(DRAWS), np.full(DRAWS, -1), np.zeros(4))
    v = np.full(DRAWS, np.nan)
    got = merge_reference(*empty, *b[:4], v)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], b[:3]))
    assert np.array_equal(got[3], [b[3][0], b[3][1], b[3][2], DRAWS])
    got = merge_reference(*a[:4], *empty, np.zeros(DRAWS))
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], a[:3]))
    assert np.array_equal(got[3], [a[3][0], a[3][1], a[3][2], 0.0])


def test_pool_workspace_query_needs_no_gpu():
    from tneq_qc_amd import _lib
    L = _lib.lib()
    q = L.tq_born_pool_workspace
    assert q(_lib.TQ_C64, 1 << 20, 4096) >= L.tq_born_sample_workspace(_lib.TQ_C64, 1 << 20, 4096) + 4 * 4096 + 4
    sizes = [q(_lib.TQ_C64, n, 4096) for n in (1, 2, 4095, 4096, 4097, 65536, 65537, 1 << 20, (1 << 22) + 3, 1 << 31)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    sizes = [q(_lib.TQ_C128, 4097, d) for d in (1, 2, 1023, 1024, 1025, 4096, 65537, (1 << 31) - 1)]
    assert all(s >= _lib.TQ_BORN_POOL_MERGE_WORKSPACE for s in sizes) and sizes == sorted(sizes)
    for args in ((_lib.TQ_F32, 1 << 20, 4096), (_lib.TQ_F64, 16, 1), (_lib.TQ_C64, 0, 4096),
                 (_lib.TQ_C64, (1 << 31) + 1, 1), (_lib.TQ_C128, 16, -1), (_lib.TQ_C128, 16, 0),
                 (_lib.TQ_C128, 16, 1 << 31)):
        assert q(*args) == 0
        assert "born_pool" in _lib.last_error()


def test_born_pool_refuses_cpu_tensors():
    import torch
    from tneq_qc_amd import ops
    f64 = torch.float64
    with pytest.raises(ValueError):
        ops.born_pool_sample(torch.ones(8, dtype=torch.complex64), torch.rand(4, dtype=f64), torch.rand(4, dtype=f64),
                             torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=f64), torch.zeros(4, dtype=f64))
    with pytest.raises(ValueError):
        ops.born_pool_merge(torch.zeros(4, dtype=torch.int64), None, torch.zeros(4, dtype=f64),
                            torch.zeros(4, dtype=torch.int64), None, torch.zeros(4, dtype=f64),
                            torch.rand(4, dtype=f64))


def test_pool_sampler_refuses_64_qubits_before_touching_a_device():
    from tneq_qc_amd import sampling
    assert "PoolSampler" in sampling.__all__
    task = types.SimpleNamespace(open_qubits=list(range(20, 40)),
                                 fixed_bits={q: 0 for q in range(64) if not 20 <= q < 40})
    with pytest.raises(ValueError, match="qubits"):
        sampling.PoolSampler(task, [0], draws=16)


def test_pool_symbols_declared_and_exported():
    from tneq_qc_amd import _lib
    header = (ROOT / "include" / "tneqhip.h").read_text()
    declared = set(re.findall(r"\b(tq_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in ("tq_born_pool_workspace", "tq_born_pool_sample", "tq_born_pool_merge"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    m = re.search(r"#define\s+TQ_BORN_POOL_MERGE_WORKSPACE\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.TQ_BORN_POOL_MERGE_WORKSPACE
