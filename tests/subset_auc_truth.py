"""The truth of mcgra_subset_auc, engine.ablation_masks and engine.shapley_shares (include/mcgra.h, mc-gra_amd/engine.py): a
numpy float32 sequential sum of the selected components in ascending k, then tests/delong_truth.py's T on the materialised
sum; the mask table from its four rules; the Shapley values from the permutation definition.  No device, nothing of the package.

Candidates: the pairs of positions a > b of idx (None: all nodes), label real[idx[a], idx[b]], component k read at
comps[k][idx[a], idx[b]]; bit k of a mask selects component k."""
import itertools
import math
from fractions import Fraction

import numpy as np

from tests import delong_truth as DT

NAMES = ("learned", "feature", "H_A1", "H_A2", "Y_A2", "ori_HA", "ori_YA", "label")
BASE = 0x1f


def subset_sum(comps, mask, order=1, dtype=np.float32):
    """s = c_first; s = s + c_next; ... over the components of the mask in ascending k (order = -1: descending), every add
    rounded to dtype."""
    ks = [k for k in range(len(comps)) if mask >> k & 1][::order]
    s = np.asarray(comps[ks[0]], dtype=dtype).copy()
    for k in ks[1:]:
        s = (s + np.asarray(comps[k], dtype=dtype)).astype(dtype)
    return s


def T_of(lab, s):
    """mcgra_auc_delong's T of the candidates (labels, scores): twice the Mann-Whitney count, ties once."""
    a, b = DT.placements(lab, s)
    assert int(a.sum()) == int(b.sum())
    return int(b.sum())


def T_with_ties(lab, s, tie):
    """2 #{edge > non-edge} + tie #{edge == non-edge}: T for tie = 1, the wrong readings for 0 and 2."""
    sn = np.sort(s[~lab])
    lt, le = np.searchsorted(sn, s[lab], "left").astype(np.int64), np.searchsorted(sn, s[lab], "right").astype(np.int64)
    return 2 * int(lt.sum()) + tie * int((le - lt).sum())


def brute_T(lab, s, tie=1):
    """The literal double loop over positives x negatives (tie: what a tie counts, 1 in the definition)."""
    t = 0
    for p in s[lab].tolist():
        for q in s[~lab].tolist():
            t += 2 if p > q else (tie if p == q else 0)
    return t


def ints(real, comps, masks, idx=None, order=1, dtype=np.float32):
    """{"pairs", "positives", "negatives", "T": [T_s]} of the entry."""
    real = np.asarray(real)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx, np.int64)
    a, b = np.tril_indices(len(ix), -1)
    lab = real[ix[a], ix[b]]
    assert np.all((lab == 0) | (lab == 1))
    lab = lab == 1
    sel = [np.asarray(c)[ix[a], ix[b]] for c in comps]                 # the selected entries alone are looked at
    assert all(np.all(np.isfinite(c)) for c in sel)
    cache, T = {}, []
    for q in masks:
        if q not in cache:
            s = subset_sum(sel, q, order, dtype)
            assert np.all(np.isfinite(s))
            cache[q] = T_of(lab, s)
        T.append(cache[q])
    return {"pairs": len(lab), "positives": int(lab.sum()), "negatives": int((~lab).sum()), "T": T}


def stats(g, masks):
    """engine.subset_auc's dict from the integers."""
    P, N = g["positives"], g["negatives"]
    return {"pairs": g["pairs"], "positives": P, "negatives": N, "masks": list(masks), "T": list(g["T"]),
            "auc": [float(Fraction(t, 2 * P * N)) if P and N else float("nan") for t in g["T"]]}


def same(got, want):
    """Every integer equal, every double the same bits (NaN where NaN)."""
    if sorted(got) != sorted(want):
        return False
    for k in ("pairs", "positives", "negatives", "masks", "T"):
        if got[k] != want[k] or any(type(v) is not int for v in (got[k] if isinstance(got[k], list) else [got[k]])):
            return False
    return np.array_equal(np.asarray(got["auc"], np.float64).view(np.int64), np.asarray(want["auc"], np.float64).view(np.int64))


def ablation_masks(present, used):
    """used; each present component alone; used minus each of its components; the base five plus each subset of {5, 6, 7}
    that is present, in the binary order of (useH_A, useY_A, useY); first occurrences, in that order."""
    bits = [k for k in range(8) if present >> k & 1]
    out = [used]
    out += [1 << k for k in bits]
    out += [used ^ (1 << k) for k in bits if used >> k & 1 and used ^ (1 << k)]
    for y in (0, 1):
        for ya in (0, 1):
            for h in (0, 1):
                q = BASE | h << 5 | ya << 6 | y << 7
                if q & ~present == 0:
                    out.append(q)
    seen, table = set(), []
    for q in out:
        if q not in seen:
            seen.add(q)
            table.append(q)
    return table


def shapley_by_permutations(K, value):
    """The definition: a player's marginal contribution v(before + i) - v(before), averaged over all K! orders; v(0) = 1/2."""
    v = dict(value)
    v[0] = Fraction(1, 2)
    tot = [Fraction(0)] * K
    for perm in itertools.permutations(range(K)):
        S = 0
        for i in perm:
            tot[i] += v[S | 1 << i] - v[S]
            S |= 1 << i
    return [t / math.factorial(K) for t in tot]
