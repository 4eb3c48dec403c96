"""The truth of mcgra_auc_delong / mcgra_auc_delong_paired (include/mcgra.h): the placement sums from np.sort + np.searchsorted
and Python integers, the rates from fractions.Fraction, each rounded to a double once.  No device, nothing of the package.

Candidates: the pairs of positions a > b of idx (None: all nodes) in packed order, score pred[idx[a], idx[b]], label
real[idx[a], idx[b]].  Scores compare as float32 values (numpy's comparison: -0.0 == +0.0, subnormals are ordinary values)."""
import math
import statistics
from fractions import Fraction

import numpy as np

SINGLE = ("pairs", "positives", "negatives", "T", "A2", "B2")
PAIRED = ("pairs", "positives", "negatives", "T_a", "T_b", "A2_a", "B2_a", "A2_b", "B2_b", "A_ab", "B_ab")
RATES = ("auc", "var", "se", "ci_low", "ci_high")
PAIRED_RATES = ("cov", "delta", "se_delta", "ci_low", "ci_high", "z", "p_value")


def candidates(real, pred, idx=None):
    """(labels bool [m], scores float32 [m]) of the selected strict lower triangle, in packed order."""
    real, pred = np.asarray(real), np.asarray(pred)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx, np.int64)
    a, b = np.tril_indices(len(ix), -1)
    lab = real[ix[a], ix[b]]
    assert np.all((lab == 0) | (lab == 1))
    s = pred[ix[a], ix[b]].astype(np.float32)
    assert np.all(np.isfinite(s))
    return lab == 1, s


def placements(lab, s):
    """(a [P], b [N]) int64: a_i = 2 #{neg < s_i} + #{neg == s_i} per positive, b_j = 2 #{pos > s_j} + #{pos == s_j} per
    negative, each in the candidates' own order."""
    pos, neg = s[lab], s[~lab]
    sp, sn = np.sort(pos), np.sort(neg)
    a = np.searchsorted(sn, pos, "left").astype(np.int64) + np.searchsorted(sn, pos, "right").astype(np.int64)
    b = 2 * len(pos) - np.searchsorted(sp, neg, "left").astype(np.int64) - np.searchsorted(sp, neg, "right").astype(np.int64)
    return a, b


def dot(x, y):
    """sum x_i y_i as a Python int, exactly; 0 <= x_i, y_i < 2^32 and fewer than 2^31 terms (four int64 sums of 16-bit halves)."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    xh, xl, yh, yl = x >> 16, x & 0xffff, y >> 16, y & 0xffff
    return ((int((xh * yh).sum()) << 32) + ((int((xh * yl).sum()) + int((xl * yh).sum())) << 16) + int((xl * yl).sum()))


def ints(real, pred, idx=None):
    lab, s = candidates(real, pred, idx)
    a, b = placements(lab, s)
    assert int(a.sum()) == int(b.sum())
    return {"pairs": len(lab), "positives": int(lab.sum()), "negatives": int((~lab).sum()), "T": int(a.sum()),
            "A2": dot(a, a), "B2": dot(b, b)}


def paired_ints(real, pred_a, pred_b, idx=None):
    lab, sa = candidates(real, pred_a, idx)
    _, sb = candidates(real, pred_b, idx)
    aa, ba = placements(lab, sa)
    ab, bb = placements(lab, sb)
    return {"pairs": len(lab), "positives": int(lab.sum()), "negatives": int((~lab).sum()), "T_a": int(aa.sum()),
            "T_b": int(ab.sum()), "A2_a": dot(aa, aa), "B2_a": dot(ba, ba), "A2_b": dot(ab, ab), "B2_b": dot(bb, bb),
            "A_ab": dot(aa, ab), "B_ab": dot(ba, bb)}


def variance(P, N, T_a, T_b, A, B):
    """DeLong's variance (T_a == T_b, A = A2, B = B2) or covariance (A = A_ab, B = B_ab) as an exact rational; P, N >= 2."""
    return Fraction(P * A - T_a * T_b, 4 * N ** 2 * P ** 2 * (P - 1)) + Fraction(N * B - T_a * T_b, 4 * P ** 2 * N ** 2 * (N - 1))


def quantile(level):
    return statistics.NormalDist().inv_cdf((1 + level) / 2)


def stats(g, level=0.95):
    """The doubles of engine.auc_delong from the integers g (SINGLE)."""
    nan = float("nan")
    P, N, T = g["positives"], g["negatives"], g["T"]
    out = dict.fromkeys(RATES, nan)
    if P == 0 or N == 0:
        return out
    out["auc"] = float(Fraction(T, 2 * P * N))
    if P == 1 or N == 1:
        return out
    out["var"] = float(variance(P, N, T, T, g["A2"], g["B2"]))
    out["se"] = math.sqrt(out["var"])
    z = quantile(level)
    out["ci_low"], out["ci_high"] = max(0.0, out["auc"] - z * out["se"]), min(1.0, out["auc"] + z * out["se"])
    return out


def paired_stats(g, level=0.95):
    """The doubles of engine.auc_delong_paired from the integers g (PAIRED): {"a", "b": stats, and PAIRED_RATES}."""
    nan = float("nan")
    P, N = g["positives"], g["negatives"]
    one = lambda s: {"pairs": g["pairs"], "positives": P, "negatives": N, "T": g["T_" + s], "A2": g["A2_" + s], "B2": g["B2_" + s]}
    out = dict.fromkeys(PAIRED_RATES, nan)
    out["a"], out["b"] = stats(one("a"), level), stats(one("b"), level)
    if P == 0 or N == 0:
        return out
    delta = Fraction(g["T_a"] - g["T_b"], 2 * P * N)
    out["delta"] = float(delta)
    if P == 1 or N == 1:
        return out
    cov = variance(P, N, g["T_a"], g["T_b"], g["A_ab"], g["B_ab"])
    var_d = (variance(P, N, g["T_a"], g["T_a"], g["A2_a"], g["B2_a"]) + variance(P, N, g["T_b"], g["T_b"], g["A2_b"], g["B2_b"])
             - 2 * cov)                                                  # ONE rational: the cancellation is exact
    assert var_d >= 0
    out["cov"] = float(cov)
    out["se_delta"] = math.sqrt(float(var_d))
    z = quantile(level)
    out["ci_low"] = max(-1.0, out["delta"] - z * out["se_delta"])
    out["ci_high"] = min(1.0, out["delta"] + z * out["se_delta"])
    if var_d == 0:
        out["z"] = 0.0 if delta == 0 else (math.inf if delta > 0 else -math.inf)
    else:
        out["z"] = out["delta"] / out["se_delta"]
    out["p_value"] = math.erfc(abs(out["z"]) / math.sqrt(2))
    return out
