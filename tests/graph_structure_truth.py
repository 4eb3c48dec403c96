"""The truth of mcgra_graph_structure (include/mcgra.h) and of engine.graph_structure_stats: numpy and Python integers only, no
GPU, no project code.

The selection is that of tests/topk_truth.py: positions 0 .. m - 1 of idx (None: all nodes); the pair of positions a > b has
score pred[idx[a], idx[b]] and label real[idx[a], idx[b]].  R has the edge {a, b} iff score >= threshold as float32 values, G
iff the label is 1, C = R & G.  For each graph X (a symmetric 0 / 1 matrix with a zero diagonal), in int64:
    d = rowsum(X),  t = rowsum((X @ X) * X) / 2,  E = sum d / 2,  T = sum t / 3,  W = sum d (d - 1) / 2.
Beyond DENSE_MAX positions the same product runs on scipy's int64 sparse matrices (the large cases are sparse graphs).

`variant` selects one of the deliberately WRONG readings; tests/test_graph_structure_cases_cpu.py shows that the shared case
list tells each of them from the truth:
    "transposed"   pred[idx[b], idx[a]] and real[idx[b], idx[a]] are read
    "strict"       score > threshold
    "node_id"      the row of `out` is the node id idx[v] instead of the position v (rows of unselected nodes are dropped)
    "ordered2"     every triangle through v is counted from both of its other corners: t is doubled
    "ordered6"     T counts ordered triangles: sum t * 2 instead of sum t / 3
    "diagonal"     a node whose own entry pred[idx[a], idx[a]] passes the threshold (label: is 1) is its own neighbour
    "union"        C = R | G
    "pad_bits"     the positions m .. 64 ceil(m / 64) - 1 exist and are joined to every position below m"""
import math
from fractions import Fraction

import numpy as np

VARIANTS = ("transposed", "strict", "node_id", "ordered2", "ordered6", "diagonal", "union", "pad_bits")
HEADER = ("pairs", "E_R", "T_R", "W_R", "E_G", "T_G", "W_G", "E_C", "T_C")
COLUMNS = ("d_R", "t_R", "d_G", "t_G", "d_C", "t_C")
GRAPH_DOUBLES = ("density", "mean_degree", "transitivity", "avg_clustering")
GRAPH_INTS = ("edges", "max_degree", "triangles", "wedges", "degree_hist")
VERSUS_DOUBLES = ("precision", "recall", "f1", "triangle_recall", "triangle_precision", "degree_l1", "degree_ks", "degree_corr",
                  "clustering_l1")
DENSE_MAX = 600


def graphs(real, pred, thr, idx=None, variant=None):
    """(R, G, C) as symmetric bool m x m matrices (G, C None without real)."""
    pred = np.asarray(pred, np.float32)
    ix = np.arange(pred.shape[0]) if idx is None else np.asarray(idx, np.int64)
    m = len(ix)
    assert m >= 2 and len(set(ix.tolist())) == m and not math.isnan(float(thr))
    low = np.tril(np.ones((m, m), bool), 0 if variant == "diagonal" else -1)

    def sym(hit):
        if variant == "transposed":
            hit = hit.T
        hit = hit & low
        return hit | hit.T

    s = pred[np.ix_(ix, ix)]
    with np.errstate(invalid="ignore"):
        R = sym(s > np.float32(thr) if variant == "strict" else s >= np.float32(thr))
    if real is None:
        return R, None, None
    G = sym(np.asarray(real, np.float32)[np.ix_(ix, ix)] == 1)
    return R, G, (R | G) if variant == "union" else (R & G)


def degrees_triangles(X):
    """(d, t) of a symmetric bool matrix as int64 arrays; the diagonal, when set, counts as the definition's product counts it."""
    m = X.shape[0]
    if m <= DENSE_MAX:
        A = X.astype(np.int64)
        return A.sum(1), ((A @ A) * A).sum(1) // 2
    import scipy.sparse as sp
    A = sp.csr_matrix(X.astype(np.int64))
    return np.asarray(A.sum(1)).reshape(-1).astype(np.int64), np.asarray((A @ A).multiply(A).sum(1)).reshape(-1).astype(np.int64) // 2


def ints(real, pred, thr, idx=None, variant=None):
    """The nine header integers by name and the six columns as lists (G and C: -1 without real)."""
    R, G, C = graphs(real, pred, thr, idx, variant)
    m = R.shape[0]
    if variant == "pad_bits":
        full = -(-m // 64) * 64

        def padded(X):
            Y = np.zeros((full, full), bool)
            Y[:m, :m] = X
            Y[:m, m:] = True
            Y[m:, :m] = True
            return Y
        R, G, C = (None if X is None else padded(X) for X in (R, G, C))
    out = {"pairs": m * (m - 1) // 2}
    for name, X in (("R", R), ("G", G), ("C", C)):
        if X is None:
            d = t = np.full(m, -1, np.int64)
            E = T = W = -1
        else:
            d, t = (v[:m] for v in degrees_triangles(X))
            if variant == "ordered2":
                t = t * 2
            E, W = int(d.sum()) // 2, int((d * (d - 1) // 2).sum())
            T = int(t.sum()) * 2 if variant == "ordered6" else int(t.sum()) // 3
        out[f"d_{name}"], out[f"t_{name}"] = d.tolist(), t.tolist()
        out[f"E_{name}"], out[f"T_{name}"] = E, T
        if name != "C":
            out[f"W_{name}"] = W
    if variant == "node_id" and idx is not None:
        ix = np.asarray(idx, np.int64)
        for k in COLUMNS:
            col = [-7] * (int(ix.max()) + 1)
            for v, node in enumerate(ix.tolist()):
                col[node] = out[k][v]
            out[k] = col[:m] + [-7] * max(0, m - len(col))
    return out


def _c(d, t):
    return [Fraction(2 * tv, dv * (dv - 1)) if dv >= 2 else Fraction(0) for dv, tv in zip(d, t)]


def _graph(pairs, E, T, W, d, t):
    m = len(d)
    return {"edges": E, "density": float(Fraction(E, pairs)), "mean_degree": float(Fraction(2 * E, m)), "max_degree": max(d),
            "triangles": T, "wedges": W, "transitivity": float(Fraction(3 * T, W)) if W else 0.0,
            "avg_clustering": math.fsum(float(x) for x in _c(d, t)) / m,
            "degree_hist": np.bincount(np.asarray(d, np.int64)).tolist()}


def stats(g):
    """The dict of engine.graph_structure_stats from the integers g of ints(): every double one rounding of an exact rational,
    or a math.fsum of such."""
    nan = float("nan")
    dR, tR = g["d_R"], g["t_R"]
    m = len(dR)
    res = {"nodes": m, "recovered": _graph(g["pairs"], g["E_R"], g["T_R"], g["W_R"], dR, tR), "true": None}
    if g["E_G"] < 0:
        return res
    dG, tG = g["d_G"], g["t_G"]
    res["true"] = _graph(g["pairs"], g["E_G"], g["T_G"], g["W_G"], dG, tG)
    ratio = lambda a, b: float(Fraction(a, b)) if b else nan
    res["precision"], res["recall"] = ratio(g["E_C"], g["E_R"]), ratio(g["E_C"], g["E_G"])
    res["f1"] = ratio(2 * g["E_C"], g["E_R"] + g["E_G"])
    res["triangle_hits"] = g["T_C"]
    res["triangle_recall"], res["triangle_precision"] = ratio(g["T_C"], g["T_G"]), ratio(g["T_C"], g["T_R"])
    res["degree_l1"] = float(Fraction(sum(abs(a - b) for a, b in zip(dR, dG)), m))
    top = max(max(dR), max(dG))
    below = lambda d: np.cumsum(np.bincount(np.asarray(d, np.int64), minlength=top + 1))
    res["degree_ks"] = float(Fraction(int(np.abs(below(dR) - below(dG)).max()), m))
    sr, sg = sum(dR), sum(dG)
    cov = m * sum(a * b for a, b in zip(dR, dG)) - sr * sg
    vr, vg = m * sum(a * a for a in dR) - sr * sr, m * sum(b * b for b in dG) - sg * sg
    res["degree_corr"] = math.copysign(math.sqrt(float(Fraction(cov * cov, vr * vg))), cov) if vr and vg else nan
    res["clustering_l1"] = math.fsum(float(abs(a - b)) for a, b in zip(_c(dR, tR), _c(dG, tG))) / m
    return res
