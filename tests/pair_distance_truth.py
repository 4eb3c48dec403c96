"""Truth of the link-stealing pair distances (mcgra_pair_distance_scores / mcgra_pair_distance_rank_metrics), in two forms:
float64 scipy.spatial.distance.cdist with the exact-rational AUC of the selected lower triangle, and a numpy float32
restatement of the kernels' k-ascending chains (one rounding per operation, every operation a numpy float32 one)."""
from fractions import Fraction

import numpy as np
from scipy.spatial.distance import cdist

METRICS = ("cosine", "euclidean", "correlation", "chebyshev", "braycurtis", "canberra", "cityblock", "sqeuclidean")


def dist64(Z, metric):
    """float64 cdist of the float32 rows of Z with the header's degenerate rules in place of scipy's NaN / warnings: cosine and
    correlation of a zero (constant) row are 1, clipped at 0 from below; a zero braycurtis denominator gives 0."""
    Z = np.asarray(Z, np.float32).astype(np.float64)
    if metric in ("cosine", "correlation"):
        C = Z - Z.mean(axis=1, keepdims=True) if metric == "correlation" else Z
        flat = (Z.max(axis=1) == Z.min(axis=1)) if metric == "correlation" else np.zeros(len(Z), bool)
        C = np.where(flat[:, None], 0.0, C)
        nrm = np.sqrt((C * C).sum(axis=1))
        Zn = C / np.maximum(nrm, 1e-12)[:, None]
        return np.maximum(0.0, 1.0 - Zn @ Zn.T)
    if metric == "braycurtis":
        num = cdist(Z, Z, "cityblock")
        den = np.zeros_like(num)
        for k in range(Z.shape[1]):
            den += np.abs(Z[:, k][:, None] + Z[:, k][None, :])
        return np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))
    return cdist(Z, Z, metric)


def scores64(Z, metric):
    return 0.0 - dist64(Z, metric)


def _normalised32(Z, centre):
    """k_pd_rows in float32: (z - mean) / max(|.|_2, 1e-12), the mean taken from a float32 sum (its order is the kernel's own
    business: the accuracy bound covers any order), a row of equal entries centred to exact zeros."""
    Z = np.asarray(Z, np.float32)
    C = Z
    if centre:
        mean = (Z.sum(axis=1, dtype=np.float32) / np.float32(Z.shape[1])).astype(np.float32)
        flat = Z.max(axis=1) == Z.min(axis=1)
        C = np.where(flat[:, None], np.float32(0), Z - mean[:, None]).astype(np.float32)
    ss = np.zeros(len(Z), np.float32)
    for k in range(Z.shape[1]):
        ss = (ss + C[:, k] * C[:, k]).astype(np.float32)
    den = np.maximum(np.sqrt(ss).astype(np.float32), np.float32(1e-12))
    return (C / den[:, None]).astype(np.float32)


def dist32(Z, metric, fma=True):
    """The kernels' chains in numpy float32, k ascending.  fma: the products of sqeuclidean / euclidean / cosine / correlation
    are formed exactly (in float64: a product of two float32 values is exact there) and rounded once with the sum, as fmaf does
    up to double rounding; fma=False rounds the product first (a plain float32 sum over k)."""
    Z = np.asarray(Z, np.float32)
    n, d = Z.shape
    f32 = np.float32
    if metric in ("cosine", "correlation"):
        Z = _normalised32(Z, metric == "correlation")
    s = np.zeros((n, n), f32)
    t = np.zeros((n, n), f32)
    for k in range(d):
        a, b = Z[:, k][:, None], Z[:, k][None, :]
        if metric in ("cosine", "correlation"):
            s = (s.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(f32) if fma else (s + (a * b).astype(f32)).astype(f32)
        elif metric in ("euclidean", "sqeuclidean"):
            e = (a - b).astype(f32)
            s = (s.astype(np.float64) + e.astype(np.float64) ** 2).astype(f32) if fma else (s + (e * e).astype(f32)).astype(f32)
        elif metric == "chebyshev":
            s = np.maximum(s, np.abs(a - b).astype(f32))
        elif metric == "braycurtis":
            s = (s + np.abs(a - b).astype(f32)).astype(f32)
            t = (t + np.abs(a + b).astype(f32)).astype(f32)
        elif metric == "canberra":
            den = (np.abs(a) + np.abs(b)).astype(f32)
            term = np.where(den == 0, f32(0), np.abs(a - b).astype(f32) / np.where(den == 0, f32(1), den)).astype(f32)
            s = (s + term).astype(f32)
        else:
            s = (s + np.abs(a - b).astype(f32)).astype(f32)
    if metric in ("cosine", "correlation"):
        return np.maximum(f32(0), f32(1) - s).astype(f32)
    if metric == "euclidean":
        return np.sqrt(s).astype(f32)
    if metric == "braycurtis":
        return np.where(t == 0, f32(0), s / np.where(t == 0, f32(1), t)).astype(f32)
    return s


def loop_dist(Z, metric):
    """A literal double loop of each definition in Python floats (float64), n small."""
    Z = np.asarray(Z, np.float32).astype(np.float64)
    n, d = Z.shape
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            x, y = Z[i], Z[j]
            if metric in ("cosine", "correlation"):
                if metric == "correlation":
                    x, y = x - sum(x) / d, y - sum(y) / d
                nx, ny = sum(v * v for v in x) ** 0.5, sum(v * v for v in y) ** 0.5
                dot = sum(p * q for p, q in zip(x, y)) / (max(nx, 1e-12) * max(ny, 1e-12))
                out[i, j] = max(0.0, 1.0 - dot)
            elif metric == "cityblock":
                out[i, j] = sum(abs(p - q) for p, q in zip(x, y))
            elif metric == "sqeuclidean":
                out[i, j] = sum((p - q) ** 2 for p, q in zip(x, y))
            elif metric == "euclidean":
                out[i, j] = sum((p - q) ** 2 for p, q in zip(x, y)) ** 0.5
            elif metric == "chebyshev":
                out[i, j] = max(abs(p - q) for p, q in zip(x, y))
            elif metric == "braycurtis":
                den = sum(abs(p + q) for p, q in zip(x, y))
                out[i, j] = 0.0 if den == 0 else sum(abs(p - q) for p, q in zip(x, y)) / den
            else:
                out[i, j] = sum(0.0 if abs(p) + abs(q) == 0 else abs(p - q) / (abs(p) + abs(q)) for p, q in zip(x, y))
    return out


def lower_pairs(values, real, idx=None):
    """(values, labels) of the unordered pairs of positions a > b of idx (None: all nodes): entry [idx[a], idx[b]]."""
    ix = np.arange(len(real)) if idx is None else np.asarray(idx, np.int64).reshape(-1)
    a, b = np.tril_indices(len(ix), -1)
    return np.asarray(values)[ix[a], ix[b]], np.asarray(real)[ix[a], ix[b]]


def rank_ints(values, labels):
    """{m, P, N, T} of mcgra_auc_delong's header in Python integers: T = sum over positives of 2 #{neg < s} + #{neg == s}.
    `values`: any totally ordered numbers (float, int or Fraction)."""
    values, lab = list(values), np.asarray(labels) == 1
    levels = sorted(set(values))
    rank = {v: r for r, v in enumerate(levels)}
    p, q = [0] * len(levels), [0] * len(levels)
    for v, l in zip(values, lab):
        (p if l else q)[rank[v]] += 1
    T, below = 0, 0
    for pv, qv in zip(p, q):
        T += pv * (2 * below + qv)
        below += qv
    return {"pairs": len(values), "positives": sum(p), "negatives": sum(q), "T": T}


def exact_auc(values, real, idx=None):
    """The exact rational AUC T / (2 P N) of the selected lower triangle (None when a class is absent) and the integers."""
    v, l = lower_pairs(values, real, idx)
    ints = rank_ints(v.tolist(), l)
    P, N = ints["positives"], ints["negatives"]
    return (Fraction(ints["T"], 2 * P * N) if P and N else None), ints
