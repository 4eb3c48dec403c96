"""The truth the curve tests compare against (no GPU, no project code): a numpy restatement of sklearn 1.7's
_binary_clf_curve, roc_curve and precision_recall_curve on real[idx][:, idx] against pred[idx][:, idx].

A LEVEL is a distinct float32 score (np.unique: -0.0 == +0.0, reported as +0.0); levels are numbered by descending score.
tps[l] / fps[l] = selected positives / negatives with a score >= level l's (reversed cumulative counts).  The two keep rules:

    roc_curve, drop_intermediate and levels > 2:   first, last, interior l with fps[l-1] - 2 fps[l] + fps[l+1] != 0 or the
                                                   same expression in tps != 0
    precision_recall_curve, the same condition:    first, last, interior l with tps[l] != tps[l-1] or tps[l+1] != tps[l]

Rates are one float64 division of exact integers each, as sklearn's.  tests/test_curves_cases_cpu.py holds all of this to
sklearn, arrays equal element for element, on the inputs the GPU tests use."""
from fractions import Fraction

import numpy as np


def select(real, pred, idx=None):
    real, pred = np.asarray(real), np.asarray(pred)
    if idx is not None:
        idx = np.asarray(idx).reshape(-1)
        real, pred = real[idx][:, idx], pred[idx][:, idx]
    return real.reshape(-1) == 1, pred.reshape(-1).astype(np.float32)


def levels(real, pred, idx=None, elements=False):
    """(tps, fps, thresholds): int64, int64, float32, thresholds descending.  elements: every selected ENTRY is a level of
    its own (ties not merged, positives first inside a tie) -- NOT sklearn's curve; the tests use it to show that their
    tied inputs tell the two apart."""
    lab, s = select(real, pred, idx)
    if elements:
        order = np.lexsort((~lab, -s.astype(np.float64)))
        return np.cumsum(lab[order]).astype(np.int64), np.cumsum(~lab[order]).astype(np.int64), s[order] + np.float32(0)
    vals, inv = np.unique(s, return_inverse=True)
    inv = inv.reshape(-1)
    p = np.bincount(inv[lab], minlength=len(vals)).astype(np.int64)
    q = np.bincount(inv[~lab], minlength=len(vals)).astype(np.int64)
    thr = (vals + np.float32(0))[::-1].astype(np.float32)          # -0.0 + 0.0 = +0.0
    return np.cumsum(p[::-1]), np.cumsum(q[::-1]), thr


def keep_roc(tps, fps, drop_intermediate):
    L = len(tps)
    if not drop_intermediate or L <= 2:
        return np.ones(L, bool)
    return np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0), True]


def keep_pr(tps, drop_intermediate):
    L = len(tps)
    if not drop_intermediate or L <= 2:
        return np.ones(L, bool)
    return np.r_[True, (np.diff(tps[:-1]) != 0) | (np.diff(tps[1:]) != 0), True]


def _f1_candidates(tps, fps):
    """The levels whose float64 F1 is within 1e-12 of the largest, ascending: the exact maximum is among them (a float64
    quotient of integers below 2^53 is off by 2^-53 relative at most); the exact comparison then runs on these alone."""
    f = 2.0 * tps / (tps + fps + float(tps[-1]))
    return np.flatnonzero(f >= f.max() * (1 - 1e-12)).tolist()


def best_f1(tps, fps):
    """(tp, fp, level) maximising 2 tp / (tp + fp + P) over all levels, in Python integers; ties to the lowest level.  None
    when P == 0."""
    P = int(tps[-1])
    if P == 0:
        return None
    best, at = None, None
    for l in _f1_candidates(tps, fps):
        v = Fraction(2 * int(tps[l]), int(tps[l]) + int(fps[l]) + P)
        if best is None or v > best:
            best, at = v, l
    return int(tps[at]), int(fps[at]), at


def f1_ties(tps, fps):
    """How many levels share the maximal F1."""
    P = int(tps[-1])
    vals = [Fraction(2 * int(tps[l]), int(tps[l]) + int(fps[l]) + P) for l in _f1_candidates(tps, fps)]
    return vals.count(max(vals))


def curves(real, pred, idx=None, drop_intermediate=True, elements=False):
    """Everything mcgra_rank_curves and its wrapper return, as a dict: "counts" = (P, N, levels, ROC points, PR points),
    "roc" = (tps, fps, thresholds) with the origin (0, 0, +inf) in front, "pr" = the same in descending-threshold order
    without an origin, "best" = best_f1, and the rates "fpr", "tpr", "precision", "recall", "pr_thresholds" as sklearn
    returns them."""
    tps, fps, thr = levels(real, pred, idx, elements)
    P, N, L = int(tps[-1]), int(fps[-1]), len(tps)
    kr, kp = keep_roc(tps, fps, drop_intermediate), keep_pr(tps, drop_intermediate)
    roc = (np.r_[0, tps[kr]].astype(np.int64), np.r_[0, fps[kr]].astype(np.int64),
           np.r_[np.float32(np.inf), thr[kr]].astype(np.float32))
    pr = (tps[kp], fps[kp], thr[kp])
    nan = np.full(len(roc[0]), np.nan)
    fpr = roc[1] / roc[1][-1] if N > 0 else nan
    tpr = roc[0] / roc[0][-1] if P > 0 else nan.copy()
    ps = (pr[0] + pr[1]).astype(np.float64)
    precision = np.zeros(len(ps))
    np.divide(pr[0].astype(np.float64), ps, out=precision, where=ps != 0)
    recall = pr[0] / pr[0][-1] if P > 0 else np.ones(len(ps))
    return {"counts": (P, N, L, len(roc[0]), len(pr[0])), "roc": roc, "pr": pr, "best": best_f1(tps, fps),
            "keep_roc": kr, "keep_pr": kp, "fpr": fpr, "tpr": tpr, "precision": np.r_[precision[::-1], 1.0],
            "recall": np.r_[recall[::-1], 0.0], "pr_thresholds": pr[2][::-1]}


def sklearn_curves(real, pred, idx=None, drop_intermediate=True):
    """(roc_curve, precision_recall_curve) of sklearn on the same selection, warnings silenced."""
    import warnings

    from sklearn.metrics import precision_recall_curve, roc_curve
    lab, s = select(real, pred, idx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (roc_curve(lab, s, drop_intermediate=drop_intermediate),
                precision_recall_curve(lab, s, drop_intermediate=drop_intermediate))
