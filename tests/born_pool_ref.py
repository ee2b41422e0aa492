"""numpy reference of the pool sampler (include/tneqhip.h, tq_born_pool_sample and
tq_born_pool_merge): a weighted reservoir over amplitude blocks, every block's candidates taken
from born_ref.born_reference.  Helper module: no tests here."""
import numpy as np

from born_ref import born_reference


def _mass(x):
    return bool(np.isfinite(x) and x > 0)


def pool_step(a, u, v, index, prob, source, pool, b):
    """One tq_born_pool_sample call on block number `b`, in place; returns (stats, accepted mask)."""
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    ci, cp, _, S1, S2 = born_reference(a, u)
    stats = np.array([S1, S2])
    if not _mass(S1):
        pool[3] = 0.0
        return stats, np.zeros(u.shape, dtype=bool)
    W = pool[0]
    W1 = W + S1
    with np.errstate(invalid="ignore"):
        take = np.ones(u.shape, dtype=bool) if W == 0 else v * W1 < S1
    index[take] = ci[take]
    prob[take] = cp[take]
    source[take] = b
    pool[0] = W1
    pool[1] = pool[1] + S2
    pool[2] = pool[2] + 1.0
    pool[3] = float(take.sum())
    return stats, take


def pool_reference(blocks, U, V, index=None, prob=None, source=None, pool=None, first=0):
    """Blocks folded in order into one reservoir (a fresh one unless index / prob / source / pool
    are given); row k of U and V serves block k.  Returns index, prob, source_block, pool,
    accepted_per_block; a slot no block has touched keeps index -1 / prob 0 / source -1."""
    draws = np.asarray(U).shape[1]
    index = np.full(draws, -1, dtype=np.int64) if index is None else index
    prob = np.zeros(draws) if prob is None else prob
    source = np.full(draws, -1, dtype=np.int64) if source is None else source
    pool = np.zeros(4) if pool is None else pool
    accepted = []
    for k, a in enumerate(blocks):
        _, take = pool_step(a, U[k], V[k], index, prob, source, pool, first + k)
        accepted.append(int(take.sum()))
    return index, prob, source, pool, np.array(accepted, dtype=np.int64)


def merge_reference(index_a, prob_a, source_a, pool_a, index_b, prob_b, source_b, pool_b, v):
    """tq_born_pool_merge: B folded into copies of A; returns index, prob, source, pool."""
    index, prob, source, pool = (np.array(x) for x in (index_a, prob_a, source_a, pool_a))
    v = np.asarray(v, dtype=np.float64)
    Wa, Wb = pool[0], pool_b[0]
    if not _mass(Wb):
        pool[3] = 0.0
        return index, prob, source, pool
    W1 = Wa + Wb
    with np.errstate(invalid="ignore"):
        take = np.ones(v.shape, dtype=bool) if Wa == 0 else v * W1 < Wb
    index[take] = np.asarray(index_b)[take]
    prob[take] = np.asarray(prob_b)[take]
    source[take] = np.asarray(source_b)[take]
    pool[:] = [W1, pool[1] + pool_b[1], pool[2] + pool_b[2], float(take.sum())]
    return index, prob, source, pool


def window_count(blocks, U, V, scale=8.0):
    """How many acceptance decisions of pool_reference over `blocks` lie within
    scale * n * 2^-52 * W' of the boundary v W' = S1 (reference values): the draws a device sum
    that differs in the last bits could decide the other way."""
    W = 0.0
    count = 0
    for k, a in enumerate(blocks):
        _, _, _, S1, _ = born_reference(a, U[k])
        if not _mass(S1):
            continue
        W1 = W + S1
        if W != 0:
            n = np.asarray(a).size
            count += int((np.abs(np.asarray(V[k]) * W1 - S1) <= scale * n * 2.0 ** -52 * W1).sum())
        W = W1
    return count
