"""The truth of mcgra_knn_graph (include/mcgra.h) and of engine.knn_graph_stats: numpy and Python integers only, no GPU, no
project code.

The selection is that of tests/node_rank_truth.py: positions 0 .. m - 1 of idx (None: all nodes); for position a the candidates
are the positions b != a with score pred[idx[a], idx[b]].  Scores compare through the order-preserving key of their float32 bits
(-0.0 == +0.0, subnormals distinct); the best-first ranking of a row is key descending, ties by ascending position b.
    L_k(a)  the first k positions of row a's ranking                D  the arc a -> b iff b in L_k(a)
    U       {a, b} iff a -> b or b -> a                             Mu {a, b} iff both
    G       {a, b}, a > b, iff real[idx[a], idx[b]] == 1 (the strict lower triangle)
    header  pairs m (m - 1) / 2, k, E_U, E_M, E_G, H_D (arcs of D whose pair is in G), H_U, H_M (edges of U / Mu in G)
    row a   in = |{b : b -> a}|, d_U, d_M, d_G, h_D = |L_k(a) & N_G(a)|, h_U, h_M (U- / Mu-neighbours that are G-neighbours)
    edges   U's edges in ascending packed position a (a - 1) / 2 + b, a > b: (idx[a], idx[b]), the stored score
            pred[idx[a], idx[b]], kind (bit 0: a -> b, bit 1: b -> a), hit ({a, b} in G)
The last four header entries and columns are -1 without real.

`variant` selects one of the deliberately WRONG readings; tests/test_knn_cases_cpu.py shows that the shared case list tells each
of them from the truth:
    "ties_desc"  ties by descending position             "node_id"   ties by ascending node id idx[b]
    "columns"    column a is ranked (pred transposed)    "diagonal"  b == a is a candidate like any other
    "k_plus"     k + 1 partners                          "k_minus"   k - 1 partners
    "swapped"    union and mutual change places          "global"    D is the symmetric graph of the m k / 2 best pairs a > b
    "neg_zero"   -0.0 orders below +0.0"""
import math
from fractions import Fraction

import numpy as np

VARIANTS = ("ties_desc", "node_id", "columns", "diagonal", "k_plus", "k_minus", "swapped", "global", "neg_zero")
HEADER = ("pairs", "k", "E_U", "E_M", "E_G", "H_D", "H_U", "H_M")
COLUMNS = ("in", "d_U", "d_M", "d_G", "h_D", "h_U", "h_M")
IN_BINS = ((0, 0), (1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, None))
GRAPH_DOUBLES = ("precision", "recall", "f1")


def key(s, merge_zeros=True):
    """float32 -> int64 with the same order; -0.0 and +0.0 are one value (unless told otherwise), subnormals stay distinct."""
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.int64)
    if merge_zeros:
        u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _ids(pred, idx):
    ix = np.arange(np.asarray(pred).shape[0]) if idx is None else np.asarray(idx, np.int64).reshape(-1)
    assert len(ix) >= 2 and len(set(ix.tolist())) == len(ix)
    return ix


def lists(pred, k, idx=None, variant=None):
    """int64 [m, k]: L_k(a) as positions, in ranking order (one stable sort of a composite per row)."""
    pred = np.asarray(pred, np.float32)
    ix = _ids(pred, idx)
    m = len(ix)
    k = k + (variant == "k_plus") - (variant == "k_minus")
    assert 0 <= k <= m - 1 + (variant == "diagonal")
    s = pred[np.ix_(ix, ix)]
    if variant == "columns":
        s = s.T
    K = key(s, merge_zeros=variant != "neg_zero")
    pos = np.arange(m, dtype=np.int64)
    tie = {"ties_desc": pos, "node_id": int(ix.max()) - ix}.get(variant, m - 1 - pos)       # larger = earlier among equals
    comp = K * (1 << 20) + tie[None, :]
    if variant != "diagonal":
        comp[pos, pos] = -1
    neg = -comp                                                   # distinct within a row: the order is total
    if not 0 < k < m - 1:
        return np.argsort(neg, axis=1, kind="stable")[:, :k]
    part = np.argpartition(neg, k - 1, axis=1)[:, :k]             # select the k, then sort only them
    return np.take_along_axis(part, np.argsort(np.take_along_axis(neg, part, 1), axis=1, kind="stable"), 1)


def row_by_definition(pred, k, a, idx=None):
    """L_k(a) by the definition, literally: candidate b is ahead of candidate c when its float32 score is larger, or equal with
    b < c; the list is the candidates with fewer than k others ahead, by the number ahead."""
    pred = np.asarray(pred, np.float32)
    ix = _ids(pred, idx)
    cand = [b for b in range(len(ix)) if b != a]
    s = {b: pred[ix[a], ix[b]] for b in cand}
    ahead = {b: sum(1 for c in cand if s[c] > s[b] or (s[c] == s[b] and c < b)) for b in cand}
    return [b for b in sorted(cand, key=lambda b: ahead[b]) if ahead[b] < k]


def directed(pred, k, idx=None, variant=None, L=None):
    """D as a bool m x m matrix, D[a, b] = (a -> b).  L: lists() of the same arguments, when at hand."""
    pred = np.asarray(pred, np.float32)
    ix = _ids(pred, idx)
    m = len(ix)
    D = np.zeros((m, m), bool)
    if variant == "global":
        a, b = np.nonzero(np.tril(np.ones((m, m), bool), -1))                 # packed order
        order = np.lexsort((np.arange(len(a)), -key(pred[ix[a], ix[b]])))[:m * k // 2]
        D[a[order], b[order]] = True
        return D | D.T
    L = lists(pred, k, idx, variant) if L is None else L
    D[np.repeat(np.arange(m), L.shape[1]), L.reshape(-1)] = True
    return D


def true_graph(real, idx, m):
    ix = np.arange(m) if idx is None else np.asarray(idx, np.int64).reshape(-1)
    low = np.tril(np.asarray(real, np.float32)[np.ix_(ix, ix)] == 1, -1)
    return low | low.T


def ints(real, pred, k, idx=None, variant=None):
    """The eight header integers by name, the seven columns as lists, "lists" (int64 [m, k]) and the edge list "edges" =
    (pairs int64 [E_U, 2], scores float32 [E_U], kind uint8 [E_U], hits bool [E_U] or None)."""
    pred = np.asarray(pred, np.float32)
    ix = _ids(pred, idx)
    m = len(ix)
    L = None if variant == "global" else lists(pred, k, idx, variant)
    D = directed(pred, k, idx, variant, L)
    U, Mu = D | D.T, D & D.T
    if variant == "swapped":
        U, Mu = Mu, U
    G = None if real is None else true_graph(real, idx, m)
    out = {"pairs": m * (m - 1) // 2, "k": k}
    cols = {"in": D.sum(0), "d_U": U.sum(1), "d_M": Mu.sum(1)}
    minus = np.full(m, -1, np.int64)
    cols.update({"d_G": minus, "h_D": minus, "h_U": minus, "h_M": minus} if G is None else
                {"d_G": G.sum(1), "h_D": (D & G).sum(1), "h_U": (U & G).sum(1), "h_M": (Mu & G).sum(1)})
    out.update({q: np.asarray(cols[q], np.int64).tolist() for q in COLUMNS})
    out["E_U"], out["E_M"] = int(U.sum()) // 2, int(Mu.sum()) // 2
    out["E_G"], out["H_D"], out["H_U"], out["H_M"] = (-1, -1, -1, -1) if G is None else (
        int(G.sum()) // 2, int((D & G).sum()), int((U & G).sum()) // 2, int((Mu & G).sum()) // 2)
    if L is not None:
        out["lists"] = L
    a, b = np.nonzero(np.tril(U, -1))                                         # row-major: ascending a, then b = packed order
    out["edges"] = (np.stack([ix[a], ix[b]], 1).astype(np.int64).reshape(-1, 2), pred[ix[a], ix[b]],
                    (D[a, b].astype(np.uint8) | (D[b, a].astype(np.uint8) << 1)), None if G is None else G[a, b])
    return out


def ints_from_lists(L, m):
    """The label-free integers from the lists alone, without an m x m matrix (the capacity case): header E_U, E_M and the
    columns in, d_U, d_M."""
    L = np.asarray(L, np.int64)
    k = L.shape[1]
    a = np.repeat(np.arange(m, dtype=np.int64), k)
    b = L.reshape(-1)
    arcs = a * m + b
    both = np.isin(b * m + a, arcs)                                            # the arc a -> b whose reverse exists too
    ind = np.bincount(b, minlength=m)
    dM = np.bincount(a[both], minlength=m)
    return {"E_M": int(both.sum()) // 2, "E_U": m * k - int(both.sum()) // 2, "in": ind.tolist(), "d_M": dM.tolist(),
            "d_U": (k + ind - dM).tolist()}


def check_identities(g):
    """The identities of the definition on the integers of ints() (variant None)."""
    m, k = len(g["in"]), g["k"]
    assert sum(g["in"]) == m * k and g["E_U"] + g["E_M"] == m * k
    assert all(dm == k + i - du for i, du, dm in zip(g["in"], g["d_U"], g["d_M"]))
    assert sum(g["d_U"]) == 2 * g["E_U"] and sum(g["d_M"]) == 2 * g["E_M"]
    if g["E_G"] >= 0:
        assert g["H_D"] == g["H_U"] + g["H_M"] and sum(g["d_G"]) == 2 * g["E_G"]
        assert sum(g["h_D"]) == g["H_D"] and sum(g["h_U"]) == 2 * g["H_U"] and sum(g["h_M"]) == 2 * g["H_M"]


def _graph(edges, positives, hits, have):
    nan = float("nan")
    if not have:
        return {"edges": edges, "positives": None, "hits": None, "precision": nan, "recall": nan, "f1": nan}
    ratio = lambda a, b: float(Fraction(a, b)) if b else nan
    return {"edges": edges, "positives": positives, "hits": hits, "precision": ratio(hits, edges),
            "recall": ratio(hits, positives), "f1": ratio(2 * hits, edges + positives)}


def stats(g):
    """The dict of engine.knn_graph_stats from the integers g of ints(): every double one rounding of an exact rational."""
    ind, m, k = g["in"], len(g["in"]), g["k"]
    have = g["E_G"] >= 0
    res = {"nodes": m, "k": k, "directed": _graph(m * k, 2 * g["E_G"], g["H_D"], have),
           "union": _graph(g["E_U"], g["E_G"], g["H_U"], have), "mutual": _graph(g["E_M"], g["E_G"], g["H_M"], have)}
    res["union"]["isolated"] = sum(1 for d in g["d_U"] if d == 0)
    res["mutual"]["isolated"] = sum(1 for d in g["d_M"] if d == 0)
    S2, S3 = sum((x - k) ** 2 for x in ind), sum((x - k) ** 3 for x in ind)
    res["hubness"] = {"max_in": max(ind), "orphans": ind.count(0),
                      "skewness": math.copysign(math.sqrt(float(Fraction(S3 * S3 * m, S2 ** 3))), S3) if S2 else float("nan"),
                      "in_hist": [(lo, hi, sum(1 for x in ind if x >= lo and (hi is None or x <= hi))) for lo, hi in IN_BINS]}
    return res


def k_of_mean_degree(m, P):
    """--knn 0: the mean true degree 2 P / m rounded half up (Fraction arithmetic), at least 1."""
    q = Fraction(2 * P, m)
    return max(1, math.floor(q + Fraction(1, 2)))
