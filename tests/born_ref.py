"""numpy reference of the Born-rule block sampler (include/tneqhip.h, tq_born_sample) and the
acceptance rule the GPU tests apply to random data.  Helper module: no tests here."""
import numpy as np


def born_p(a):
    """p_i = re^2 + im^2 in float64 (complex64 widened first)."""
    a = np.asarray(a).reshape(-1)
    re = a.real.astype(np.float64)
    im = a.imag.astype(np.float64)
    return re * re + im * im


def born_reference(a, u):
    """(index, prob, C, S1, S2): index_j = min{i : C_i > u_j S1}; when none qualifies the largest i
    with p_i > 0; all -1 (prob 0) when S1 is not a finite number > 0."""
    p = born_p(a)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        C = np.cumsum(p)
        S1 = C[-1]
        S2 = np.sum(p * p)
        if not (np.isfinite(S1) and S1 > 0):
            return np.full(u.shape, -1, dtype=np.int64), np.zeros(u.shape), C, S1, S2
        t = u * S1
        index = np.searchsorted(C, t, side="right").astype(np.int64)
        # searchsorted sorts NaN thresholds past the end, like every t >= S1
        none = (index >= p.size) | np.isnan(t)
    index[none] = np.flatnonzero(p > 0)[-1]
    return index, p[index], C, S1, S2


def words_reference(index, axis_qubit, base):
    """Bitstring words, one plain loop per bit: axis a of the row-major block is qubit
    axis_qubit[a] (axis 0 slowest); -1 stays -1."""
    n_axes = len(axis_qubit)
    out = []
    for i in np.asarray(index).reshape(-1).tolist():
        if i < 0:
            out.append(-1)
            continue
        w = int(base)
        for a in range(n_axes):
            if (i >> (n_axes - 1 - a)) & 1:
                w |= 1 << int(axis_qubit[a])
        out.append(w)
    return np.array(out, dtype=np.int64)


def index_of_word(word, axis_qubit):
    """Inverse of words_reference on the open bits."""
    n_axes = len(axis_qubit)
    i = 0
    for a in range(n_axes):
        i |= ((int(word) >> int(axis_qubit[a])) & 1) << (n_axes - 1 - a)
    return i


def check_draws(a, u, index, C=None, S1=None):
    """Rule 2 of the GPU tests, for EVERY draw: index_j = i is accepted iff
    C[i-1] - eps <= t_j and (t_j < C[i] + eps or i is the last positive element), with
    eps = 4 n 2^-52 S1: twice the n 2^-53 S1 worst-case error of a float64 sum of n non-negative
    terms, for each of the two sides (the kernel's C and the reference's C are both within that
    of the exact sums; the threshold product adds one rounding).  Returns the offending draws."""
    p = born_p(a)
    if C is None:
        C = np.cumsum(p)
        S1 = C[-1]
    n = p.size
    eps = 4.0 * n * 2.0 ** -52 * S1
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    index = np.asarray(index).reshape(-1)
    t = u * S1
    assert index.min() >= 0 and index.max() < n
    lastpos = np.flatnonzero(p > 0)[-1]
    below = np.where(index > 0, C[np.maximum(index - 1, 0)], 0.0)
    ok = (below - eps <= t) & ((t < C[index] + eps) | (index == lastpos))
    return np.flatnonzero(~ok)
