"""The truth of mcgra_edge_exposure (include/mcgra.h) and of engine.edge_exposure_stats: the placements from np.sort +
np.searchsorted, the common neighbours and degrees from the bool adjacency of the induced subgraph, the rates from
fractions.Fraction, each rounded to a double once.  No device, nothing of the package.

Candidates: the pairs of positions a > b of idx (None: all nodes) in packed order, score pred[idx[a], idx[b]], label
real[idx[a], idx[b]].  G has the edge {a, b} iff that label is 1: nothing but the selected strict lower triangle is read.
Scores compare as float32 values (numpy's comparison: -0.0 == +0.0, subnormals are ordinary values).

`wrong` names one misreading of the definition (WRONG); tests/test_exposure_cases_cpu.py shows that the cases tell each from the
right reading."""
import math
from fractions import Fraction

import numpy as np

from tests.delong_truth import candidates
from tests.hop_truth import adjacency

CLASSES = 16
HEADER = ("pairs", "positives", "negatives", "T", "above_pos", "above_neg")
COLUMNS = ("pairs_list", "scores", "placement", "common", "deg")
COMMON_NAMES = tuple(str(c) for c in range(15)) + ("15+",)
DEGREE_NAMES = ("0", "1", "2-3", "4-7", "8-15", "16-31", "32-63", "64-127", "128-255", "256-511", "512-1023", "1024-2047",
                "2048-4095", "4096-8191", "8192-16383", "16384+")
WRONG = ("whole_graph", "max_degree", "cap16", "bit_length_off", "ties2", "ties0", "all_candidates", "strict_cut", "row_major")


def ints(real, pred, idx=None, threshold=None, wrong=None):
    """{"header": [m, P, N, T, above_pos, above_neg], "table": [ec][dc] -> [count, T, above] (Python ints; 17 rows under the
    wrong reading cap16), and the per-edge columns in ascending packed position: "pairs_list" int64 [P, 2] (node ids),
    "scores" float32 [P], "placement" int64 [P], "common" int32 [P], "deg" int32 [P, 2]}.  threshold None: +inf."""
    assert wrong is None or wrong in WRONG
    real = np.asarray(real)
    lab, s = candidates(real, pred, idx)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx, np.int64)
    A = adjacency(real, idx)
    a, b = np.tril_indices(len(ix), -1)                       # packed order: a (a - 1) / 2 + b ascending
    ea, eb, es = a[lab], b[lab], s[lab]
    others = np.sort(s if wrong == "all_candidates" else s[~lab])
    lo, hi = (np.searchsorted(others, es, side).astype(np.int64) for side in ("left", "right"))
    place = 2 * hi if wrong == "ties2" else 2 * lo if wrong == "ties0" else lo + hi           # 2 #lower + #equal
    if wrong == "whole_graph":                                # neighbours that are not selected count too
        full = np.nan_to_num(real, nan=0.0) == 1
        full = full | full.T
        common = (full[ix[ea]] & full[ix[eb]]).sum(1)
    else:
        common = (A[ea] & A[eb]).sum(1)
    degree = A.sum(1)
    da, db = degree[ea], degree[eb]
    d = np.maximum(da, db) if wrong == "max_degree" else np.minimum(da, db)
    rows = CLASSES + 1 if wrong == "cap16" else CLASSES
    ec = np.minimum(common, rows - 1)
    length = np.asarray([int(v).bit_length() for v in d], np.int64) - (1 if wrong == "bit_length_off" else 0)
    dc = np.minimum(CLASSES - 1, length)
    thr = np.float32(np.inf if threshold is None else threshold)
    assert not np.isnan(thr)
    above = es > thr if wrong == "strict_cut" else es >= thr
    table = [[[0, 0, 0] for _ in range(CLASSES)] for _ in range(rows)]
    for e, c, p, x in zip(ec.tolist(), dc.tolist(), place.tolist(), above.tolist()):
        cell = table[e][c]
        cell[0] += 1
        cell[1] += p
        cell[2] += int(x)
    order = np.lexsort((ea, eb)) if wrong == "row_major" else np.arange(len(ea))
    P = int(lab.sum())
    header = [len(lab), P, len(lab) - P, int(place.sum()), int(above.sum()),
              int((s[~lab] > thr).sum() if wrong == "strict_cut" else (s[~lab] >= thr).sum())]
    return {"header": header, "table": table,
            "pairs_list": np.stack([ix[ea], ix[eb]], 1).astype(np.int64).reshape(-1, 2)[order], "scores": es[order],
            "placement": place[order], "common": common.astype(np.int32)[order],
            "deg": np.stack([da, db], 1).astype(np.int32).reshape(-1, 2)[order]}


def loop_ints(real, pred, idx=None, threshold=None):
    """The definition, literally (small inputs): a double loop over the edges and the non-edges, a triple loop for the common
    neighbours.  (header, table, rows) with rows = [(u, v, score, placement, common, deg_a, deg_b)] in packed order."""
    ix = list(range(len(pred))) if idx is None else [int(v) for v in idx]
    m = len(ix)
    thr = np.float32(np.inf if threshold is None else threshold)
    edge = [[False] * m for _ in range(m)]
    pos, neg = [], []
    for a in range(m):
        for b in range(a):
            sc = np.float32(pred[ix[a]][ix[b]])
            if real[ix[a]][ix[b]] == 1:
                edge[a][b] = edge[b][a] = True
                pos.append((a, b, sc))
            else:
                neg.append(sc)
    table = [[[0, 0, 0] for _ in range(CLASSES)] for _ in range(CLASSES)]
    rows = []
    for a, b, sc in pos:
        place = 0
        for q in neg:
            place += 2 if q < sc else 1 if q == sc else 0
        common = 0
        for w in range(m):
            if edge[a][w] and edge[b][w]:
                common += 1
        da, db = sum(edge[a]), sum(edge[b])
        cell = table[min(common, 15)][min(15, min(da, db).bit_length())]
        cell[0] += 1
        cell[1] += place
        cell[2] += 1 if sc >= thr else 0
        rows.append((ix[a], ix[b], sc, place, common, da, db))
    header = [len(pos) + len(neg), len(pos), len(neg), sum(r[3] for r in rows), sum(1 for r in rows if r[2] >= thr),
              sum(1 for q in neg if q >= thr)]
    return header, table, rows


def _double(num, den):
    return float(Fraction(num, den)) if den else float("nan")


def stats(header, table):
    """The dict of engine.edge_exposure_stats from the integers, every double one rounding of an exact rational."""
    m, P, N, T, above_pos, above_neg = (int(v) for v in header)
    K = CLASSES

    def doubles(c, t, x):
        return {"auc": _double(t, 2 * c * N), "recall": _double(x, c), "share": _double(c, P)}

    def marginal(names, cells_of):
        rows = [[sum(int(cell[q]) for cell in cells_of(c)) for q in range(3)] for c in range(K)]
        out = {"names": names, "count": tuple(r[0] for r in rows), "T": tuple(r[1] for r in rows), "above": tuple(r[2] for r in rows)}
        for q in ("auc", "recall", "share"):
            out[q] = tuple(doubles(*r)[q] for r in rows)
        out["lift"] = tuple(float(Fraction(r[1], 2 * r[0] * N) - Fraction(T, 2 * P * N)) if r[0] and N else float("nan") for r in rows)
        return out

    res = dict(zip(HEADER, (m, P, N, T, above_pos, above_neg)))
    res.update({"auc_pooled": _double(T, 2 * P * N), "recall": _double(above_pos, P), "precision": _double(above_pos, above_pos + above_neg),
                "by_embeddedness": marginal(COMMON_NAMES, lambda c: table[c]),
                "by_degree": marginal(DEGREE_NAMES, lambda c: [table[e][c] for e in range(K)]),
                "cells": [{"ec": e, "dc": c, "common": COMMON_NAMES[e], "degree": DEGREE_NAMES[c], "count": int(table[e][c][0]),
                           "T": int(table[e][c][1]), "above": int(table[e][c][2]), **doubles(*(int(v) for v in table[e][c]))}
                          for e in range(K) for c in range(K) if table[e][c][0]]})
    return res


def same(a, b):
    """Two values (dicts, sequences, numbers) hold the same keys, the same integers and the same bits; NaN equals NaN."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), (sorted(a), sorted(b) if isinstance(b, dict) else b)
        return all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), (a, b)
        return all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    assert type(a) is type(b) and a == b, (a, b)
    return True


def as_tuples(table):
    return tuple(tuple(tuple(int(v) for v in cell) for cell in row) for row in table)


def circulant_ints(n, threshold=0.5):
    """header and table of graph_structure_cases.circulant(n) (offsets +-1, +-2) as scores and labels at once, n >= 9: every
    degree is 4 (dc = 3); the n edges of offset 1 have two common neighbours, the n of offset 2 one; every edge scores 1 and
    every non-edge 0, so every placement is 2 N."""
    assert n >= 9 and 0 < threshold <= 1
    m, P = n * (n - 1) // 2, 2 * n
    N = m - P
    table = [[[0, 0, 0] for _ in range(CLASSES)] for _ in range(CLASSES)]
    table[1][3] = [n, 2 * N * n, n]
    table[2][3] = [n, 2 * N * n, n]
    return [m, P, N, 2 * N * P, P, 0], table
