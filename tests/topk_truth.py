"""The truth the top-k tests compare against (numpy only, no GPU, no project code).

The candidates are the m = r (r - 1) / 2 unordered pairs of positions a > b of idx (None: all nodes in order), in packed order
p = a (a - 1) / 2 + b -- the order of np.tril_indices(r, -1).  Pair (a, b) is nodes u = idx[a], v = idx[b] with score
pred[u, v] and label real[u, v].  The ranking is np.argsort(-s, kind="stable"): score descending as float32 values
(-0.0 == +0.0), ties by ascending packed position.  P = candidates with label 1, TP = those among the first k; k = 0 / None
means k = P.  precision = TP / k, recall = TP / P, F1 = 2 TP / (k + P), each one float64 division, NaN for a zero denominator.

`variant` selects one of three deliberately WRONG readings; tests/test_topk_cases_cpu.py shows that the test inputs tell each
of them from the truth:
    "ties_last"   ties taken last-in-packed-order first
    "upper"       the upper-triangle entry [v, u] read in place of [u, v]
    "ordered"     all ordered pairs of positions, diagonal included, row-major"""
import numpy as np

VARIANTS = ("ties_last", "upper", "ordered")


def packed(real, pred, idx=None, variant=None):
    """(s, lab, u, v) of every candidate in packed order: float32 scores, bool labels (None without real), node ids."""
    pred = np.asarray(pred)
    ids = np.arange(pred.shape[0]) if idx is None else np.asarray(idx).reshape(-1)
    if variant == "ordered":
        a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(len(ids)), np.arange(len(ids)), indexing="ij"))
    else:
        a, b = np.tril_indices(len(ids), -1)
    u, v = ids[a], ids[b]
    if variant == "upper":
        u, v = v, u
    s = pred[u, v].astype(np.float32)
    lab = None if real is None else np.asarray(real)[u, v] == 1
    return s, lab, u, v


def ranking(s, variant=None):
    """Candidate positions, best first."""
    if variant == "ties_last":
        return len(s) - 1 - np.argsort(-s[::-1], kind="stable")
    return np.argsort(-s, kind="stable")


def ratio(num, den):
    return num / den if den else float("nan")


def top_k(real, pred, k=None, idx=None, variant=None):
    """Everything the entries return for one k: the dict of engine.topk_metrics (threshold as np.float32, NaN when k = 0)
    plus "order" (packed positions), "edges" [k, 2] (u, v), "scores" [k] float32 and "edge_hits" [k] bool in ranking order."""
    s, lab, u, v = packed(real, pred, idx, variant)
    P = int(lab.sum())
    k = int(k) if k else P
    assert 0 <= k <= len(s), (k, len(s))
    order = ranking(s, variant)[:k]
    tp = int(lab[order].sum())
    return {"k": k, "positives": P, "hits": tp, "pairs": len(s), "precision": ratio(tp, k), "recall": ratio(tp, P),
            "f1": ratio(2 * tp, k + P), "threshold": s[order[-1]] if k else np.float32("nan"),
            "order": order, "edges": np.stack([u[order], v[order]], 1).astype(np.int64).reshape(k, 2), "scores": s[order],
            "edge_hits": lab[order]}


def bits(x):
    """The float32 bit patterns of x (scalar or array)."""
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def tie_group(real, pred, k, idx=None):
    """(members, taken): the packed positions whose score equals the k-th pair's, and how many of them the k best hold."""
    s, _, _, _ = packed(real, pred, idx)
    order = ranking(s)[:k]
    members = np.flatnonzero(s == s[order[-1]])
    return members, int((s[order] == s[order[-1]]).sum())
