"""numpy reference of the block top-k select (include/tneqhip.h, tq_born_topk).  Helper module: no
tests here."""
import numpy as np

from born_ref import born_p


def topk_reference(a, k):
    """(index, prob, count): the elements with p > 0 (+inf counts, NaN and 0 never) ordered by p
    descending and index ascending among equal p, the first k of them; padded with -1 / 0."""
    with np.errstate(all="ignore"):
        p = born_p(a)
        cand = np.flatnonzero(p > 0)
        o = cand[np.lexsort((cand, -p[cand]))][:k]
    m = o.size
    index = np.full(k, -1, dtype=np.int64)
    prob = np.zeros(k, dtype=np.float64)
    index[:m] = o
    prob[:m] = p[o]
    return index, prob, np.array([m], dtype=np.int64)
