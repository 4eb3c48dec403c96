"""The truth of mcgra_hop_auc (include/mcgra.h): distances by a breadth-first search on the induced subgraph, the class sums
by brute force over every (positive, negative) pair, the rates as Python int / int.  No device, nothing of the package.

Candidates: the pairs of positions a > b of idx (None: all nodes) in packed order, score pred[idx[a], idx[b]], label
real[idx[a], idx[b]].  G has the edge {a, b} iff that label is 1: nothing but the selected strict lower triangle is read.
Scores compare as float32 values (numpy's comparison: -0.0 == +0.0, subnormals are ordinary values)."""
import math

import numpy as np

from tests.delong_truth import candidates
from tests.delong_truth import placements as sorted_placements

HOP_MAX = 8
BRUTE = 1 << 24          # (positive, negative) pairs compared at a time


def adjacency(real, idx=None):
    """G as a symmetric bool matrix over the positions, from the selected strict lower triangle of real alone."""
    real = np.asarray(real)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx, np.int64)
    m = len(ix)
    A = np.zeros((m, m), bool)
    a, b = np.tril_indices(m, -1)
    A[a, b] = real[ix[a], ix[b]] == 1
    return A | A.T


def distances(A, limit=None):
    """Shortest-path lengths of the graph A over its positions (int64 [m, m]): breadth-first, one level of every source at a
    time; 0 on the diagonal, -1 where there is no path (or none of at most `limit` edges)."""
    m = len(A)
    dist = np.full((m, m), -1, np.int64)
    np.fill_diagonal(dist, 0)
    adj = A.astype(np.float32)
    frontier = np.eye(m, dtype=bool)
    d = 0
    while frontier.any() and (limit is None or d < limit):
        d += 1
        frontier = ((frontier.astype(np.float32) @ adj) > 0) & (dist < 0)      # reached now, and never before
        dist[frontier] = d
    return dist


def placements(pos, neg):
    """b_q = 2 #{positives above it} + #{positives equal to it} of every negative, by comparing it with every positive."""
    b = np.zeros(len(neg), np.int64)
    step = max(1, BRUTE // max(1, len(pos)))
    for k in range(0, len(neg), step):
        q = neg[k:k + step][None, :]
        b[k:k + step] = 2 * (pos[:, None] > q).sum(0) + (pos[:, None] == q).sum(0)
    return b


def prepare(real, pred, idx=None, brute=True):
    """What every (hops, threshold) of one input shares, computed once: (labels, scores, distances up to HOP_MAX, b) of the
    candidates in packed order; b is 0 at the positives.  brute False (inputs too large to compare every pair): b from
    tests/delong_truth.py's sort and searchsorted, which tests/test_hop_cases_cpu.py holds to the comparison of every pair."""
    lab, s = candidates(real, pred, idx)
    A = adjacency(real, idx)
    a, b = np.tril_indices(len(A), -1)
    d = distances(A, HOP_MAX)[a, b]
    assert np.array_equal(d == 1, lab)
    place = np.zeros(len(lab), np.int64)
    place[~lab] = placements(s[lab], s[~lab]) if brute else sorted_placements(lab, s)[1]
    return lab, s, d, place


def rows_of(prep, hops, threshold=None):
    """The hops + 1 rows [pairs_c, T_c, above_c] of the entry (threshold None: +inf, as the engine passes)."""
    assert 1 <= hops <= HOP_MAX
    lab, s, d, place = prep
    thr = np.float32(np.inf if threshold is None else threshold)
    assert not np.isnan(thr)
    cls = np.where((d < 1) | (d > hops), hops, d - 1)          # dist - 1; hops for dist > hops or no path
    rows = []
    for c in range(hops + 1):
        sel = cls == c
        rows.append([int(sel.sum()), int(place[sel].sum()), int((s[sel] >= thr).sum())])
    assert rows[0][1] == 0
    rows[0][1] = sum(r[1] for r in rows[1:])
    return rows


def ints(real, pred, idx=None, hops=3, threshold=None):
    return rows_of(prepare(real, pred, idx), hops, threshold)


def loop_ints(real, pred, idx=None, hops=3, threshold=None):
    """The definition, literally (small inputs): a queue per source, a double loop over the positives and a class's negatives."""
    ix = list(range(len(pred))) if idx is None else [int(v) for v in idx]
    m = len(ix)
    nb = [[] for _ in range(m)]
    for a in range(m):
        for b in range(a):
            if real[ix[a]][ix[b]] == 1:
                nb[a].append(b)
                nb[b].append(a)
    thr = np.float32(np.inf if threshold is None else threshold)
    by_class = [[] for _ in range(hops + 1)]
    for a in range(m):
        dist = {a: 0}
        queue = [a]
        for u in queue:
            for w in nb[u]:
                if w not in dist:
                    dist[w] = dist[u] + 1
                    queue.append(w)
        for b in range(a):
            d = dist.get(b, hops + 1)
            by_class[min(d, hops + 1) - 1].append(np.float32(pred[ix[a]][ix[b]]))
    rows = []
    for c, scores in enumerate(by_class):
        t = 0
        if c:
            for p in by_class[0]:
                for q in scores:
                    t += 2 if p > q else 1 if p == q else 0
        rows.append([len(scores), t, sum(1 for q in scores if q >= thr)])
    rows[0][1] = sum(r[1] for r in rows[1:])
    return rows


def stats(rows, hops, threshold=None):
    """The dict of engine.hop_auc_stats from the rows."""
    nan = float("nan")
    count, T, above = ([r[q] for r in rows] for q in range(3))
    P, N, fp = count[0], sum(count[1:]), sum(above[1:])
    out = {"hops": hops, "threshold": None if threshold is None else float(threshold), "pairs": P + N, "positives": P,
           "negatives": N, "distance": tuple(range(1, hops + 1)) + ("beyond",), "count": tuple(count), "T": tuple(T),
           "auc": tuple(nan if c == 0 or P == 0 or count[c] == 0 else T[c] / (2 * P * count[c]) for c in range(hops + 1)),
           "share": tuple(nan if c == 0 or N == 0 else count[c] / N for c in range(hops + 1)),
           "auc_pooled": T[0] / (2 * P * N) if P and N else nan, "ints": [tuple(r) for r in rows]}
    if threshold is not None:
        out["above"] = tuple(above)
        out["fp_share"] = tuple(nan if c == 0 or fp == 0 else above[c] / fp for c in range(hops + 1))
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


def circulant_rows(n, hops, threshold=0.5):
    """The rows of graph_structure_cases.circulant(n) as scores and labels at once, n >= 4 hops + 3: the distance of two nodes
    r apart on the ring is ceil(r / 2), so 2 n pairs at each distance; every edge scores 1 and every non-edge 0."""
    assert n >= 4 * hops + 3 and 0 < threshold <= 1
    P, m = 2 * n, n * (n - 1) // 2
    rows = [[2 * n, 2 * P * 2 * n, 0] for _ in range(hops)] + [[m - 2 * n * hops, 2 * P * (m - 2 * n * hops), 0]]
    rows[0] = [P, 2 * P * (m - P), P]
    return rows
