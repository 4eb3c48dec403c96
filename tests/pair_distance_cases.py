"""Inputs of the pair-distance tests (CPU and GPU): planted graphs whose node rows carry the communities, so that every
metric ranks edges above non-edges but not perfectly.  Known-answer cases have distances that are exact in float32 in any
order, so the expected AUC is a rational in Python integers; accuracy cases are generic float32 rows."""
from fractions import Fraction

import numpy as np

from tests import pair_distance_truth as T

U = 2.0 ** -24      # unit roundoff of float32


def planted(n, seed, groups=4, p_in=0.36, p_out=0.04):
    """(labels n x n float32 symmetric 0 / 1 with a zero diagonal, group of every node): about 12 % edges."""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, groups, n)
    prob = np.where(g[:, None] == g[None, :], p_in, p_out)
    up = np.triu(rng.rand(n, n) < prob, 1)
    return (up | up.T).astype(np.float32), g


# ---- accuracy cases: name -> (labels, Z)
def _randn_case(n, d, seed, offset=0.0):
    """offset: the standard deviation of a shift of each whole row, without which the mean of a wide row is so close to 0
    that correlation ranks as cosine does."""
    lab, g = planted(n, seed)
    rng = np.random.RandomState(seed + 1)
    centres = rng.randn(4, d)
    return lab, ((rng.randn(n, d) + centres[g] + offset * rng.randn(n, 1)) * 0.8).astype(np.float32)


def _softmax_case(n, d, seed):
    lab, g = planted(n, seed)
    rng = np.random.RandomState(seed + 1)
    logits = rng.randn(n, d) * 1.5
    logits[np.arange(n), g % d] += 2.5
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return lab, (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


ACCURACY = {"randn_257x16": lambda: _randn_case(257, 16, 11), "randn_300x80": lambda: _randn_case(300, 80, 12, 0.7),
            "softmax_515x7": lambda: _softmax_case(515, 7, 13), "softmax_400x4": lambda: _softmax_case(400, 4, 14)}
SOFTMAX = ("softmax_515x7", "softmax_400x4")
_cache = {}


def accuracy_case(name):
    """(labels, Z, {metric: float64 scores}) of an accuracy case, computed once."""
    if name not in _cache:
        lab, Z = ACCURACY[name]()
        _cache[name] = (lab, Z, {m: T.scores64(Z, m) for m in T.METRICS})
    return _cache[name]


def kappa(Z):
    """max over rows of |z|_2 / |z - mean(z)|_2: how much of a row the centring of `correlation` cancels."""
    Z = np.asarray(Z, np.float64)
    C = Z - Z.mean(axis=1, keepdims=True)
    return float((np.sqrt((Z * Z).sum(axis=1)) / np.sqrt((C * C).sum(axis=1))).max())


def score_bound(metric, d, kap=0.0):
    """The a-priori float32 error bound of a materialised score against float64 (DESIGN.md "Pair distances"): ("rel", b) means
    |s32 - s64| <= b |s64|, ("abs", b) means |s32 - s64| <= b.  gamma(k) = k u / (1 - k u) bounds k roundings in a row."""
    gamma = lambda k: k * U / (1.0 - k * U)
    if metric == "chebyshev":
        return "rel", gamma(1)                       # one rounded difference
    if metric == "cityblock":
        return "rel", gamma(d)                       # a rounded term, d - 1 additions of non-negative terms
    if metric == "sqeuclidean":
        return "rel", gamma(d + 2)                   # the difference enters squared (2), one fma per k
    if metric == "euclidean":
        return "rel", gamma(d + 4)                   # at most half of sqeuclidean's + a square root within 2 ulp
    if metric == "canberra":
        return "rel", gamma(d + 5)                   # difference, denominator, a division within 2 ulp (4 u), d - 1 additions
    if metric == "braycurtis":
        return "rel", gamma(2 * d + 4)               # two cityblock-like sums and a division within 2 ulp
    # cosine: both rows carry ((d + 1) / 2 + 3) u from their norm and division, the d fmas d u |zn_i| |zn_j|, 1 - s two more
    b = gamma(2 * d + 10)
    if metric == "correlation":                      # a mean that is off by u sqrt(d) |z| shifts a centred row by (d + 1) u |z|
        b += 2 * (d + 1) * kap * U
    return "abs", b * 1.01                           # (first-order terms; 1 % for the second order)


# ---- known-answer cases: (labels, Z, exact distances as an n x n object array of Python ints / Fractions)
def _flip_rows(proto, g, rng, flips, values):
    Z = proto[g].copy()
    for i in range(len(Z)):
        for k in rng.choice(Z.shape[1], flips, replace=False):
            Z[i, k] = values[rng.randint(len(values))]
    return Z


def known_case(metric, n, seed=5):
    lab, g = planted(n, seed)
    rng = np.random.RandomState(seed + 7)
    if metric in ("cityblock", "sqeuclidean", "euclidean", "chebyshev"):
        Z = _flip_rows(rng.randint(-2, 3, (4, 6)), g, rng, 3, (-2, -1, 0, 1, 2))
        D = Z[:, None, :].astype(np.int64) - Z[None, :, :]
        exact = {"cityblock": np.abs(D).sum(2), "chebyshev": np.abs(D).max(2)}.get(metric, (D * D).sum(2))   # euclidean ranks as sqeuclidean
    elif metric == "canberra":
        Z = _flip_rows(rng.randint(0, 2, (4, 12)), g, rng, 4, (0, 1))
        exact = (Z[:, None, :] != Z[None, :, :]).sum(2)                     # a Hamming count: 0 / 0 -> 0, 0 / 2 -> 0, 1 / 1 -> 1
    elif metric == "braycurtis":
        Z = _flip_rows(rng.randint(0, 4, (4, 5)), g, rng, 2, (0, 1, 2, 3))
        num = np.abs(Z[:, None, :] - Z[None, :, :]).sum(2)
        den = np.abs(Z[:, None, :] + Z[None, :, :]).sum(2)
        exact = np.array([[Fraction(int(a), int(b)) if b else Fraction(0) for a, b in zip(ra, rb)] for ra, rb in zip(num, den)],
                         dtype=object)
    elif metric == "cosine":
        Z = _flip_rows(rng.choice((-1, 1), (4, 16)), g, rng, 5, (-1, 1))       # every norm is exactly 4
        exact = 16 - Z.astype(np.int64) @ Z.T                                    # 16 (1 - <zn_i, zn_j>)
    else:                                                                        # correlation: eight +1 and eight -1, mean exactly 0
        proto = np.array([rng.permutation([1] * 8 + [-1] * 8) for _ in range(4)])
        Z = proto[g].copy()
        for i in range(n):
            for _ in range(3):                                                   # swap a +1 with a -1: the balance stays
                p, q = rng.choice(np.flatnonzero(Z[i] == 1)), rng.choice(np.flatnonzero(Z[i] == -1))
                Z[i, p], Z[i, q] = -1, 1
        exact = 16 - Z.astype(np.int64) @ Z.T
    return lab, Z.astype(np.float32), exact


def known_auc(metric, n, idx=None):
    """(labels, Z, the exact rational AUC of the scores 0 - dist, the integers) of a known-answer case."""
    lab, Z, exact = known_case(metric, n)
    neg = np.array([[-v for v in row] for row in exact], dtype=object)
    frac, ints = T.exact_auc(neg, lab, idx)
    return lab, Z, frac, ints
