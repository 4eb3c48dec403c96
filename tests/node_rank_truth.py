"""The truth the per-node ranking tests compare against (numpy only, no GPU, no project code).

For position a of idx (None: all nodes in order) the candidates are the positions b != a of idx; candidate b has score
pred[idx[a], idx[b]] and label real[idx[a], idx[b]] == 1: row a of the gathered submatrix without its diagonal.  Scores
compare through the order-preserving key of their float32 bits (-0.0 == +0.0, subnormals distinct); the best-first ranking is
np.lexsort((position, -key)): key descending, ties by ascending position b.  Per row:
    P           positive candidates                        N = candidates - P
    wins        (positive, negative) pairs with key(pos) > key(neg)
    ties        (positive, negative) pairs with equal keys
    hits        positives among the first P of the ranking
    first_rank  1 + candidates with a key strictly above the best positive's; 0 when P = 0
    auc = (2 wins + ties) / (2 P N), r_precision = hits / P, reciprocal_rank = 1 / first_rank,
    mean_rank = (P N - wins - ties + P) / (P N): one float64 division each, NaN for a zero denominator.

`by` selects what breaks ties in the ranking: "position" (the truth) or "node" (the node id -- a deliberately WRONG reading
that tests/test_node_rank_cases_cpu.py uses to show that the permuted-idx case can tell the two apart)."""
import numpy as np

COLUMNS = ("positives", "wins", "ties", "hits", "first_rank")
RATES = ("auc", "r_precision", "reciprocal_rank", "mean_rank")
DEGREE_BINS = ((1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, None))


def key(s):
    """float32 -> int64 with the same order; -0.0 and +0.0 are one value, subnormals stay distinct (bit tests only)."""
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.int64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def candidates(real, pred, a, idx=None):
    """(keys, labels, positions b) of row a's candidates, in position order."""
    pred = np.asarray(pred)
    ids = np.arange(pred.shape[0]) if idx is None else np.asarray(idx).reshape(-1)
    b = np.delete(np.arange(len(ids)), a)
    return key(pred[ids[a], ids[b]]), np.asarray(real)[ids[a], ids[b]] == 1, b


def ratio(num, den):
    return np.float64(num) / np.float64(den) if den else float("nan")


def counts(k, lab, tiebreak):
    """The five counts of one row from its candidates' keys, labels and what orders equal keys (ascending)."""
    order = np.lexsort((tiebreak, -k))
    ls = lab[order]
    P = int(ls.sum())
    negs = np.sort(k[~lab])
    below = np.searchsorted(negs, k[lab], "left")                 # negatives with a smaller key, per positive
    upto = np.searchsorted(negs, k[lab], "right")
    wins, ties = int(below.sum()), int((upto - below).sum())
    hits = int(ls[:P].sum())
    first = 1 + int((k > k[lab].max()).sum()) if P else 0
    return P, wins, ties, hits, first


def row(real, pred, a, idx=None, by="position"):
    """The five counts of row a as a tuple of ints."""
    k, lab, b = candidates(real, pred, a, idx)
    ids = np.arange(np.asarray(pred).shape[0]) if idx is None else np.asarray(idx).reshape(-1)
    return counts(k, lab, b if by == "position" else ids[b])


def row_of_vectors(real_row, pred_row, a):
    """row() for idx = None when only row a of the two matrices is at hand (the large shapes)."""
    b = np.delete(np.arange(len(pred_row)), a)
    return counts(key(np.asarray(pred_row)[b]), np.asarray(real_row)[b] == 1, b)


def rates(cols, n_idx):
    """The four rates of each row of an int [rows, 5] array of counts: float64 arrays, NaN for a zero denominator."""
    cols = np.asarray(cols, np.int64).reshape(-1, 5)
    out = {r: np.full(len(cols), np.nan) for r in RATES}
    for i, (P, wins, ties, hits, first) in enumerate(cols.tolist()):
        N = n_idx - 1 - P
        out["auc"][i] = ratio(2 * wins + ties, 2 * P * N)
        out["r_precision"][i] = ratio(hits, P)
        out["reciprocal_rank"][i] = ratio(1, first)
        out["mean_rank"][i] = ratio(P * N - wins - ties + P, P * N)
    return out


def per_node(real, pred, idx=None, rows=None, by="position"):
    """int64 [len(rows), 5]: the counts of the given rows (None: every position of idx)."""
    n_idx = np.asarray(pred).shape[0] if idx is None else len(np.asarray(idx).reshape(-1))
    rows = range(n_idx) if rows is None else rows
    return np.array([row(real, pred, a, idx, by) for a in rows], np.int64).reshape(-1, 5)


def summary(cols, n_idx):
    """The summary dict of engine.node_rank_metrics from the counts of every row: plain means in index order."""
    cols = np.asarray(cols, np.int64).reshape(-1, 5)
    r = rates(cols, n_idx)
    P = cols[:, 0]
    N = n_idx - 1 - P
    scored, has = (P > 0) & (N > 0), P > 0

    def mean(x):
        return float(np.mean(x)) if len(x) else float("nan")

    by_degree = []
    for lo, hi in DEGREE_BINS:
        sel = (P >= lo) & (P <= (hi if hi is not None else P.max(initial=0)))
        by_degree.append((lo, hi, int(sel.sum()), mean(r["auc"][sel & scored]), mean(r["r_precision"][sel])))
    return {"scored": int(scored.sum()), "macro_auc": mean(r["auc"][scored]), "mrr": mean(r["reciprocal_rank"][has]),
            "hits_at_1": mean((cols[has, 4] == 1).astype(np.float64)), "r_precision": mean(r["r_precision"][has]),
            "by_degree": by_degree}
