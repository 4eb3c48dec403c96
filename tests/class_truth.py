"""The truth of mcgra_class_auc (include/mcgra.h): per stratum every non-edge compared with every edge of ITS stratum, the counts
as Python integers, the rates as Python int / int and fractions.Fraction.  No device, nothing of the package.

Candidates: the pairs of positions a > b of idx (None: all nodes) in packed order, score pred[idx[a], idx[b]], label
real[idx[a], idx[b]]; the class of position a is classes[idx[a]] (by node id), the stratum of a candidate table[c_a][c_b].
Scores compare as float32 values (numpy's comparison: -0.0 == +0.0, subnormals are ordinary values)."""
import math
from fractions import Fraction

import numpy as np

from tests.delong_truth import candidates

CLASS_MAX = 16
STRATA_MAX = 136
BRUTE = 1 << 24          # (edge, non-edge) pairs compared at a time
HOWS = ("one", "same", "own", "blocks")


def strata(C, how):
    """(table as a list of C lists, names) of engine.class_strata, written as loops."""
    table = [[0] * C for _ in range(C)]
    if how == "one":
        names = ["all"]
    elif how == "same":
        names = ["same", "different"]
        for i in range(C):
            for j in range(C):
                table[i][j] = 0 if i == j else 1
    elif how == "own":
        names = [str(c) for c in range(C)] + ["different"]
        for i in range(C):
            for j in range(C):
                table[i][j] = i if i == j else C
    else:
        assert how == "blocks"
        names, g = [], 0
        for i in range(C):
            for j in range(i, C):
                table[i][j] = table[j][i] = g
                names.append(f"{i}-{j}")
                g += 1
    return table, tuple(names)


def prepare(real, pred, classes, idx=None):
    """(labels bool [m], scores float32 [m], c_a [m], c_b [m]) of the candidates in packed order."""
    lab, s = candidates(real, pred, idx)
    ix = np.arange(np.asarray(real).shape[0]) if idx is None else np.asarray(idx, np.int64)
    a, b = np.tril_indices(len(ix), -1)
    cl = np.asarray(classes, np.int64)[ix]
    return lab, s, cl[a], cl[b]


def rows_of(prep, table, G, threshold=None, brute=True):
    """The G rows [pairs_g, P_g, T_g, above_g, hits_g] of the entry (threshold None: +inf, as the engine passes).  brute False
    (inputs too large to compare every pair): T_g from a sort and two searches inside the stratum, which
    tests/test_class_cases_cpu.py holds to the comparison of every pair."""
    lab, s, ca, cb = prep
    table = np.asarray(table, np.int64)
    thr = np.float32(np.inf if threshold is None else threshold)
    assert not np.isnan(thr) and np.array_equal(table, table.T) and table.max() < G
    g_of = table[ca, cb] if len(ca) else np.zeros(0, np.int64)
    rows = []
    for g in range(G):
        sel = g_of == g
        pos, neg = s[sel & lab], s[sel & ~lab]
        if brute:
            t = 0
            step = max(1, BRUTE // max(1, len(pos)))
            for k in range(0, len(neg), step):
                q = neg[k:k + step][None, :]
                t += 2 * int((pos[:, None] > q).sum()) + int((pos[:, None] == q).sum())
        else:
            sp = np.sort(pos)
            t = int((2 * len(pos) - np.searchsorted(sp, neg, "left").astype(np.int64)
                     - np.searchsorted(sp, neg, "right").astype(np.int64)).sum())
        rows.append([int(sel.sum()), len(pos), t, int((s[sel] >= thr).sum()), int((pos >= thr).sum())])
    return rows


def ints(real, pred, classes, idx, table, G, threshold=None, brute=True):
    return rows_of(prepare(real, pred, classes, idx), table, G, threshold, brute)


def loop_ints(real, pred, classes, idx, table, G, threshold=None):
    """The definition, literally (small inputs): a double loop over the candidates, then per stratum over its edges and
    non-edges."""
    ix = list(range(len(pred))) if idx is None else [int(v) for v in idx]
    thr = np.float32(np.inf if threshold is None else threshold)
    edges, rest = [[] for _ in range(G)], [[] for _ in range(G)]
    for a in range(len(ix)):
        for b in range(a):
            g = table[classes[ix[a]]][classes[ix[b]]]
            (edges if real[ix[a]][ix[b]] == 1 else rest)[g].append(np.float32(pred[ix[a]][ix[b]]))
    rows = []
    for g in range(G):
        t = 0
        for q in rest[g]:
            for p in edges[g]:
                t += 2 if p > q else 1 if p == q else 0
        rows.append([len(edges[g]) + len(rest[g]), len(edges[g]), t, sum(1 for x in edges[g] + rest[g] if x >= thr),
                     sum(1 for x in edges[g] if x >= thr)])
    return rows


def stats(rows, names, threshold=None):
    """The dict of engine.class_auc_stats from the rows."""
    nan = float("nan")
    q = lambda a, b: a / b if b else nan
    count, pos, T, above, hits = ([r[k] for r in rows] for k in range(5))
    neg = [c - p for c, p in zip(count, pos)]
    m, P = sum(count), sum(pos)
    num, den = Fraction(0), 0
    for g in range(len(rows)):
        if pos[g] * neg[g] > 0:
            num += pos[g] * Fraction(T[g], 2 * pos[g] * neg[g])
            den += pos[g]
    out = {"names": tuple(names), "threshold": None if threshold is None else float(threshold), "pairs": m,
           "count": tuple(count), "positives": tuple(pos), "negatives": tuple(neg), "T": tuple(T),
           "auc": tuple(q(t, 2 * p * n) for t, p, n in zip(T, pos, neg)),
           "pair_share": tuple(q(c, m) for c in count), "edge_share": tuple(q(p, P) for p in pos),
           "auc_within": q(sum(T), sum(2 * p * n for p, n in zip(pos, neg))),
           "auc_adjusted": float(num / den) if den else nan, "ints": [tuple(r) for r in rows]}
    if threshold is not None:
        out.update({"above": tuple(above), "hits": tuple(hits), "precision": tuple(q(h, a) for h, a in zip(hits, above)),
                    "recall": tuple(q(h, p) for h, p in zip(hits, pos))})
    return out


def same(a, b):
    """Two stats dicts hold the same keys, the same integers and the same bits."""
    eq = lambda x, y: (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y)) or \
        (type(x) is type(y) and x == y)
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], (tuple, list)):
            assert len(a[k]) == len(b[k]) and all(eq(x, y) for x, y in zip(a[k], b[k])), (k, a[k], b[k])
        else:
            assert eq(a[k], b[k]), (k, a[k], b[k])
    return True


def circulant_rows(n, C=16):
    """The rows of the `blocks` of C classes v % C on graph_structure_cases.circulant(n) -- the edges {v, v +- 1}, {v, v +- 2}
    mod n -- as scores and labels at once, threshold 0.5, in O(n): every edge scores 1 and every non-edge 0, so T_g = 2 P_g N_g,
    above_g = hits_g = P_g.  n >= 5."""
    size = [len(range(c, n, C)) for c in range(C)]
    table, names = strata(C, "blocks")
    pairs, P = [0] * len(names), [0] * len(names)
    for i in range(C):
        for j in range(i, C):
            pairs[table[i][j]] = size[i] * (size[i] - 1) // 2 if i == j else size[i] * size[j]
    for v in range(n):
        for d in (1, 2):                                                 # each edge once: from v to v + d
            P[table[v % C][(v + d) % n % C]] += 1
    return [[c, p, 2 * p * (c - p), p, p] for c, p in zip(pairs, P)]
