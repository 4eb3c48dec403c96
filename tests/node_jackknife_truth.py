"""The truth of mcgra_auc_node_jackknife (include/mcgra.h) and of engine.node_jackknife_stats / node_jackknife_paired_stats: the
five per-node integers from numpy sorts and Python integers, the doubles from fractions.Fraction and math.fsum.  No device,
nothing of the package.

Candidates: those of tests/delong_truth.py -- the pairs of positions a > b of idx (None: all nodes), score pred[idx[a], idx[b]],
label real[idx[a], idx[b]], float32 comparison, a tie counts 1/2.  Row v of the answer belongs to POSITION v of idx."""
import math
import statistics
from fractions import Fraction

import numpy as np

from tests import delong_truth as DT

COLUMNS = ("P_v", "N_v", "A_v", "B_v", "C_v")
RATES = ("auc", "auc_jackknife", "var", "se", "ci_low", "ci_high")
PAIRED_RATES = ("delta", "delta_jackknife", "var_delta", "se_delta", "ci_low", "ci_high", "z", "p_value")


def doubled_wins(pos, neg, tie=1):
    """sum over (p, q) of 2 [p > q] + tie [p == q] as a Python int (float32 arrays)."""
    sn = np.sort(neg)
    below, upto = np.searchsorted(sn, pos, "left").astype(np.int64), np.searchsorted(sn, pos, "right").astype(np.int64)
    return int((2 * below + tie * (upto - below)).sum())


def ints(real, pred, idx=None, tie=1, drop_c=False):
    """{"pairs", "positives", "negatives", "T", "P_v", "N_v", "A_v", "B_v", "C_v"}: Python ints and lists of them."""
    lab, s = DT.candidates(real, pred, idx)
    rows = np.asarray(real).shape[0] if idx is None else len(idx)
    a, b = np.tril_indices(rows, -1)
    pos, neg = s[lab], s[~lab]
    sp, sn = np.sort(pos), np.sort(neg)
    lo, hi = np.searchsorted(sn, pos, "left").astype(np.int64), np.searchsorted(sn, pos, "right").astype(np.int64)
    ap = 2 * lo + tie * (hi - lo)
    lo, hi = np.searchsorted(sp, neg, "left").astype(np.int64), np.searchsorted(sp, neg, "right").astype(np.int64)
    bq = 2 * (len(pos) - hi) + tie * (hi - lo)
    assert int(ap.sum()) == int(bq.sum())
    cols = {k: np.zeros(rows, np.int64) for k in COLUMNS}              # every sum is below 2^61
    for end in (a, b):
        np.add.at(cols["P_v"], end[lab], 1)
        np.add.at(cols["N_v"], end[~lab], 1)
        np.add.at(cols["A_v"], end[lab], ap)
        np.add.at(cols["B_v"], end[~lab], bq)
    if not drop_c:
        sym, lsym = np.zeros((rows, rows), np.float32), np.zeros((rows, rows), bool)      # the pairs of v: row v, v left out
        sym[a, b], sym[b, a], lsym[a, b], lsym[b, a] = s, s, lab, lab
        for v in range(rows):
            other = np.arange(rows) != v
            cols["C_v"][v] = doubled_wins(sym[v][other & lsym[v]], sym[v][other & ~lsym[v]], tie)
    out = {"pairs": len(lab), "positives": int(lab.sum()), "negatives": int((~lab).sum()), "T": int(ap.sum())}
    out.update({k: [int(x) for x in v] for k, v in cols.items()})
    return out


def recount(real, pred, idx=None):
    """The literal reading: delete position v, count again.  [(T_-v, P_-v, N_-v)] per position."""
    real = np.asarray(real)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx, np.int64)
    out = []
    for v in range(len(ix)):
        rest = np.delete(ix, v)
        if len(rest) < 2:
            out.append((0, 0, 0))
            continue
        lab, s = DT.candidates(real, pred, rest)
        t = 0
        for p in s[lab]:
            for q in s[~lab]:
                t += 2 if p > q else (1 if p == q else 0)
        out.append((t, int(lab.sum()), int((~lab).sum())))
    return out


def influences(g):
    """(auc, [d_v]) as Fractions; None where undefined."""
    P, N, T = g["positives"], g["negatives"], g["T"]
    m = len(g["P_v"])
    if P == 0 or N == 0:
        return None, [None] * m
    auc = Fraction(T, 2 * P * N)
    d = []
    for pv, nv, av, bv, cv in zip(*(g[k] for k in COLUMNS)):
        d.append(None if pv == P or nv == N else auc - Fraction(T - av - bv + cv, 2 * (P - pv) * (N - nv)))
    return auc, d


def jackknife(d):
    """(mean, var) of the doubles of the exact influences d."""
    m = len(d)
    x = [float(v) for v in d]
    mean = math.fsum(x) / m
    return mean, (m - 1) / m * math.fsum((v - mean) ** 2 for v in x)


def exact_variance(d):
    """The same formula with nothing rounded: a Fraction."""
    m = len(d)
    mean = sum(d, Fraction(0)) / m
    return Fraction(m - 1, m) * sum(((v - mean) ** 2 for v in d), Fraction(0))


def influence_doubles(d):
    return [float("nan") if v is None else float(v) for v in d]


def stats(g, level=0.95):
    """The doubles of engine.auc_node_jackknife from the integers g, "undefined_nodes" and "influence" (a list)."""
    nan = float("nan")
    auc, d = influences(g)
    out = dict.fromkeys(RATES, nan)
    out["undefined_nodes"] = sum(v is None for v in d)
    out["influence"] = influence_doubles(d)
    if auc is None:
        return out
    out["auc"] = float(auc)
    if out["undefined_nodes"] or len(d) < 3:
        return out
    mean, var = jackknife(d)
    out["auc_jackknife"] = out["auc"] + (len(d) - 1) * mean
    out["var"], out["se"] = var, math.sqrt(var)
    z = statistics.NormalDist().inv_cdf((1 + level) / 2)
    out["ci_low"], out["ci_high"] = max(0.0, out["auc"] - z * out["se"]), min(1.0, out["auc"] + z * out["se"])
    return out


def paired_stats(ga, gb, level=0.95):
    nan = float("nan")
    auc_a, da = influences(ga)
    auc_b, db = influences(gb)
    d = [None if x is None else x - y for x, y in zip(da, db)]
    out = dict.fromkeys(PAIRED_RATES, nan)
    out["a"], out["b"] = stats(ga, level), stats(gb, level)
    out["undefined_nodes"] = sum(v is None for v in d)
    out["influence"] = influence_doubles(d)
    if auc_a is None:
        return out
    delta = auc_a - auc_b
    out["delta"] = float(delta)
    if out["undefined_nodes"] or len(d) < 3:
        return out
    mean, var = jackknife(d)
    out["delta_jackknife"] = out["delta"] + (len(d) - 1) * mean
    out["var_delta"], out["se_delta"] = var, math.sqrt(var)
    z = statistics.NormalDist().inv_cdf((1 + level) / 2)
    out["ci_low"] = max(-1.0, out["delta"] - z * out["se_delta"])
    out["ci_high"] = min(1.0, out["delta"] + z * out["se_delta"])
    if var == 0:
        out["z"] = 0.0 if delta == 0 else (math.inf if delta > 0 else -math.inf)
    else:
        out["z"] = out["delta"] / out["se_delta"]
    out["p_value"] = math.erfc(abs(out["z"]) / math.sqrt(2))
    return out
