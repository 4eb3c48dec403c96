"""The truth the average-precision tests compare against (no GPU, no project code): the closed form of
sklearn.metrics.average_precision_score on real[idx][:, idx] against pred[idx][:, idx],

    AP = (1 / P) * sum over selected positives i of TP(s_i) / (TP(s_i) + FP(s_i)),
    TP(s) = #selected positives with score >= s,  FP(s) = #selected negatives with score >= s,

ties being float32 equality (-0.0 == +0.0).  TP + FP < 2^53, so each term is one correctly rounded float64 division; the
terms are summed with math.fsum (exactly, one rounding) and divided by P.  tests/test_average_precision_cpu.py holds this
to sklearn within 1e-15 on the inputs the GPU tests use."""
import math
from fractions import Fraction

import numpy as np


def level_counts(real, pred, idx=None):
    """(p, q): positives and negatives of real[idx][:, idx] at each distinct float32 score of pred[idx][:, idx], ascending."""
    real, pred = np.asarray(real), np.asarray(pred)
    if idx is not None:
        idx = np.asarray(idx).reshape(-1)
        real, pred = real[idx][:, idx], pred[idx][:, idx]
    lab = real.reshape(-1) == 1
    vals, inv = np.unique(pred.reshape(-1).astype(np.float32), return_inverse=True)       # -0.0 == +0.0: one value
    inv = inv.reshape(-1)
    p = np.bincount(inv[lab], minlength=len(vals)).astype(np.int64)
    q = np.bincount(inv[~lab], minlength=len(vals)).astype(np.int64)
    return p, q


def from_counts(p, q, strict=False):
    """AP from per-level counts, levels ascending.  strict: a tie does not count (score > s in place of >= s, a term with
    TP + FP = 0 dropped) -- NOT average precision; the tests use it to show that their inputs tell the two apart."""
    p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
    P = int(p.sum())
    if P == 0:
        return float("nan")
    tp, fp = np.cumsum(p[::-1])[::-1], np.cumsum(q[::-1])[::-1]
    if strict:
        tp, fp = tp - p, fp - q
    den = tp + fp
    terms = np.where(den > 0, tp.astype(np.float64) / np.maximum(den, 1).astype(np.float64), 0.0)
    return math.fsum(np.repeat(terms, p).tolist()) / P


def average_precision(real, pred, idx=None, strict=False):
    return from_counts(*level_counts(real, pred, idx), strict=strict)


def from_counts_exact(p, q):
    """The same AP as the nearest double of the exact rational (Python integers; for a handful of levels)."""
    P = sum(int(x) for x in p)
    if P == 0:
        return float("nan")
    tot, tp, fp = Fraction(0), 0, 0
    for pv, qv in zip(reversed(list(p)), reversed(list(q))):
        tp += int(pv); fp += int(qv)
        if pv:
            tot += Fraction(int(pv) * tp, tp + fp)
    return float(tot / P)


def sklearn_average_precision(real, pred, idx=None):
    from sklearn.metrics import average_precision_score
    real, pred = np.asarray(real), np.asarray(pred)
    if idx is not None:
        idx = np.asarray(idx).reshape(-1)
        real, pred = real[idx][:, idx], pred[idx][:, idx]
    return float(average_precision_score(real.reshape(-1), pred.reshape(-1)))
