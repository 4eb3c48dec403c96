"""The truth the 2-means tests compare against (numpy and Python integers only, no GPU, no project code).

The candidates are those of tests/topk_truth.py: the m = r (r - 1) / 2 pairs of positions a > b of idx (None: all nodes) in
packed order p = a (a - 1) / 2 + b, pair (a, b) with score pred[idx[a], idx[b]] and label real[idx[a], idx[b]].

q = rint(s 2^28), round half to even: the product is exact in float64 (a float32 times a power of two), np.rint rounds half to
even, and the result becomes a Python integer.  Lloyd's iteration on the q, every sum and division in Python integers:
    lo = min q, hi = max q; lo == hi: degenerate (iterations 0, converged, no edges, t = lo + 1, c0 = c1 = lo)
    t_0 = (lo + hi) // 2 + 1
    round k: low = {q < t_k}, high = {q >= t_k}; c0 = sum_low // n_low, c1 = sum_high // n_high; t_{k+1} = (c0 + c1) // 2 + 1
    iterations = k + 1; stop when t_{k+1} == t_k (converged) or iterations == max_iter (not converged)
    reported: the partition that was counted, that of t_k
The sums run over the distinct values times their multiplicities (object dtype: Python integers, no float, no overflow).

`variant` selects one of five deliberately WRONG readings; tests/test_two_means_cases_cpu.py shows that the shared case list
tells each of them from the truth:
    "ties_high"    a value equidistant from the two centres goes to the high cluster
    "ceil_means"   ceiling instead of floor means
    "truncate"     q = floor(s 2^28) instead of round-half-even
    "t0_no_plus1"  t_0 = (lo + hi) // 2
    "report_next"  at the cap (not converged) t_{k+1} is reported in place of t_k"""
import numpy as np

from tests import topk_truth as K

VARIANTS = ("ties_high", "ceil_means", "truncate", "t0_no_plus1", "report_next")
SCALE = 2.0 ** 28
INTS = ("pairs", "iterations", "converged", "t", "edges", "c0", "c1", "degenerate")


def quantise(s, variant=None):
    """q of float32 scores 0 <= s < 16 as a uint64 array."""
    s = np.asarray(s, np.float32)
    assert np.isfinite(s).all() and (s >= 0).all() and (s < 16).all()
    x = s.astype(np.float64) * SCALE                      # exact
    return (np.floor(x) if variant == "truncate" else np.rint(x)).astype(np.uint64)


def lloyd(q, max_iter=256, variant=None):
    """The iteration on quantised values q: {"iterations", "converged", "t", "edges" (n_high), "c0", "c1", "degenerate"}."""
    vals, cnts = np.unique(np.asarray(q, np.uint64), return_counts=True)
    vals = np.array([int(v) for v in vals], dtype=object)
    cnts = np.array([int(c) for c in cnts], dtype=object)
    lo, hi = int(vals[0]), int(vals[-1])
    if lo == hi:
        return {"iterations": 0, "converged": 1, "t": lo + 1, "edges": 0, "c0": lo, "c1": lo, "degenerate": 1}
    assert max_iter >= 1
    total_n, total_s = int(cnts.sum()), int((vals * cnts).sum())
    t = (lo + hi) // 2 + (0 if variant == "t0_no_plus1" else 1)
    it = 0
    while True:
        low = vals < t
        n_low, s_low = int(cnts[low].sum()), int((vals[low] * cnts[low]).sum())
        n_high, s_high = total_n - n_low, total_s - s_low
        if n_low == 0 or n_high == 0:                      # (a wrong reading only: the definition never gets here)
            return {"iterations": it + 1, "converged": 0, "t": t, "edges": n_high, "c0": -1, "c1": -1, "degenerate": 0}
        if variant == "ceil_means":
            c0, c1 = -(-s_low // n_low), -(-s_high // n_high)
        else:
            c0, c1 = s_low // n_low, s_high // n_high
        tn = (c0 + c1 + 1) // 2 if variant == "ties_high" else (c0 + c1) // 2 + 1
        it += 1
        if tn == t or it == max_iter:
            conv = int(tn == t)
            rep = tn if (variant == "report_next" and not conv) else t
            return {"iterations": it, "converged": conv, "t": rep, "edges": n_high, "c0": c0, "c1": c1, "degenerate": 0}
        t = tn


def split(real, pred, idx=None, max_iter=256, variant=None):
    """Everything engine.two_means_split returns (thresholds as np.float32 or None), plus "high": the bool mask of the high
    cluster over the candidates in packed order."""
    s, lab, _, _ = K.packed(real, pred, idx)
    q = quantise(s, variant)
    r = lloyd(q, max_iter, variant)
    high = np.zeros(len(q), bool) if r["degenerate"] else q >= np.uint64(r["t"])
    r.update({"pairs": len(s), "high": high, "center_low": r["c0"] * 2.0 ** -28, "center_high": r["c1"] * 2.0 ** -28})
    if r["degenerate"]:
        r.update({"threshold": None, "threshold_low": None})
    else:
        r.update({"threshold": plus_zero(s[high].min()), "threshold_low": plus_zero(s[~high].max())})
    if lab is not None:
        P, tp = int(lab.sum()), int(lab[high].sum())
        r.update({"positives": P, "hits": tp, "precision": K.ratio(tp, r["edges"]), "recall": K.ratio(tp, P),
                  "f1": K.ratio(2 * tp, r["edges"] + P)})
    return r


def plus_zero(x):
    """-0.0 as +0.0, anything else as it is."""
    x = np.float32(x)
    return np.float32(0.0) if x == 0 else x


def threshold_pairs(real, pred, thr, idx=None):
    """(pairs [k, 2] int64, scores [k] float32, hits [k] bool or None): np.nonzero(packed_scores >= thr), float32 comparison."""
    s, lab, u, v = K.packed(real, pred, idx)
    with np.errstate(invalid="ignore"):
        at = np.nonzero(s >= np.float32(thr))[0]
    return np.stack([u[at], v[at]], 1).astype(np.int64).reshape(len(at), 2), s[at], None if lab is None else lab[at]
