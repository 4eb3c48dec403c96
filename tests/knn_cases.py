"""The inputs of tests/test_gpu_knn_graph.py (numpy only), shared with tests/test_knn_cases_cpu.py, which checks without a GPU
that they hold what they are named for and that they tell the wrong readings of the definition (tests/knn_truth.py VARIANTS)
from the right one.

cases() -> name -> (real, pred, idx, ks): n x n float32 labels and scores, node ids (None: all nodes) and the k's the case runs
at.  Arrays are read-only."""
import functools

import numpy as np

MAX_NIDX = 16384               # MCGRA_KNN_MAX_NIDX
MAX_K = 1024                   # MCGRA_KNN_MAX_K
CLASSES = (1024, 4096, 16384)  # the row-length classes of the select (csrc/knn_graph.hip): selected nodes per row
K_SET = (1, 2, 7, 63, 64, 65)  # and m - 1
# selection sizes where the kernels change behaviour: one lane, one word and its two sides, two words, 256 positions a step
SMALL = (2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257)
# each side of every class boundary, and k = MAX_K at 1025 and 2049
LARGE = {1023: (1, 1022), 1024: (63, 1023), 1025: (7, 64, 1024), 2049: (2, 1024), 4096: (2, 65), 4097: (7, 1024)}


def graph(rng, n, p):
    """A symmetric 0 / 1 float32 matrix with a zero diagonal."""
    up = np.triu(rng.rand(n, n) < p, 1)
    return (up | up.T).astype(np.float32)


def quantised(rng, n, levels=4):
    """An ASYMMETRIC matrix of `levels` values (every row is full of ties) whose diagonal holds the largest score."""
    pred = (rng.randint(0, levels, (n, n)) / np.float32(levels)).astype(np.float32)
    np.fill_diagonal(pred, 9.0)
    return pred


def distinct(rng, n):
    """An asymmetric matrix without two equal entries, of both signs."""
    v = (rng.permutation(n * n).astype(np.float32) - n * n // 2) / np.float32(n)
    return v.reshape(n, n)


def ks_of(m):
    return tuple(k for k in K_SET if k <= m - 1) + ((m - 1,) if m - 1 not in K_SET else ())


def capacity_row(a, n=MAX_NIDX):
    """Row a of the capacity case: 7919 b + 104729 a modulo the prime 16411 > n, distinct over b (int64; exact in float32)."""
    return (7919 * np.arange(n, dtype=np.int64) + 104729 * a) % 16411


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(20)
    C = {}
    for m in SMALL:
        C[f"q{m}"] = (graph(rng, m, 0.3), quantised(rng, m), None, ks_of(m))
    for m, ks in LARGE.items():
        C[f"q{m}"] = (graph(rng, m, 0.01), quantised(rng, m, 16), None, ks)
    n = 70
    C["constant"] = (graph(rng, n, 0.2), np.full((n, n), 0.75, np.float32), None, (1, 7, 69))
    n = 130
    C["two_valued"] = (graph(rng, n, 0.2), np.where(rng.rand(n, n) < 0.1, np.float32(0.9), np.float32(0.6)).astype(np.float32),
                       None, (2, 7, 64))
    n = 100
    hub = rng.rand(n, n).astype(np.float32)
    hub[:, 17] = 2.0                                                   # node 17 tops every row
    C["hub"] = (graph(rng, n, 0.1), hub, None, (1, 7))
    n = 66
    z = np.array([-0.0, 0.0, -1e-45, 1e-45], np.float32)[rng.randint(0, 4, (n, n))]
    C["signed_zeros"] = (graph(rng, n, 0.3), z, None, (1, 20, 33, 40))
    n = 67
    special = np.array([-2.0, -0.5, -1e-38, -3e-45, -1e-45, 1e-45, 2e-45, 1e-38], np.float32)
    C["negative_subnormal"] = (graph(rng, n, 0.3), special[rng.randint(0, len(special), (n, n))], None, (2, 7, 65))
    C["negative"] = (graph(rng, n, 0.3), (-1.0 - rng.permutation(n * n).reshape(n, n) / (n * n)).astype(np.float32), None, (7,))
    n = 129
    C["distinct_asym"] = (graph(rng, n, 0.1), distinct(rng, n), None, (1, 7, 64))
    # a subset, sorted and permuted, of a graph whose unselected rows and columns and whose diagonal hold junk
    n, m = 90, 50
    sel = np.sort(rng.permutation(n)[:m])
    off = np.ones(n, bool)
    off[sel] = False
    real, pred = graph(rng, n, 0.2), quantised(rng, n)
    for M in (real, pred):
        M[off] = np.nan
        M[:, off] = np.inf
        np.fill_diagonal(M, np.nan)
    C["subset"] = (real, pred, sel, (1, 7, 49))
    C["subset_permuted"] = (real, pred, sel[rng.permutation(m)], (1, 7, 49))
    dreal, dpred = real.copy(), distinct(rng, n)
    for M in (dpred,):
        M[off] = np.nan
        M[:, off] = np.inf
        np.fill_diagonal(M, np.nan)
    C["subset_distinct"] = (dreal, dpred, sel, (7,))
    C["subset_distinct_permuted"] = (dreal, dpred, C["subset_permuted"][2], (7,))
    for v in C.values():
        for arr in v[:3]:
            if arr is not None:
                arr.setflags(write=False)
    return C
