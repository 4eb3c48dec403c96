"""The inputs of tests/test_gpu_class_auc.py, built once: name -> (real, pred, classes, idx, pad, runs, brute), runs a tuple of
(C, how, threshold) with how one of class_truth.HOWS, brute whether the truth compares every pair (False: the sorted route).
tests/test_class_cases_cpu.py checks, without a GPU, that they have the properties they are named for and tell each wrong
reading of the definition from the right one.  pad > 0 puts both matrices' rows into buffers that many columns wider.  Every
case holds NaN everywhere outside the selected strict lower triangle, labels included, and a class outside [0, 16) on every
unselected node."""
import functools

import numpy as np

from tests.delong_cases import bits, graph
from tests.graph_structure_cases import circulant  # noqa: F401  (the capacity case, small: tests/test_class_cases_cpu.py)
from tests.hop_cases import only_lower, scores

# csrc/class_auc.hip, csrc/delong_common.h and csrc/rank_common.h
THREADS = 256            # AUC_THREADS: a row pass takes 256 columns a step
ROW_BLOCKS = 1024        # CA_ROW_BLOCKS: blocks of the passes over the selected rows (row a = 1 + block, + grid, ...)
SORT_TILE = 1024         # AUC_SORT_TILE: up to SORT_TILE edges are one sort block, one step
STAGE = 4096             # DL_STAGE: samples of the sorted edges in LDS; more edges than that: a sample stride above 1
SHARED_BINS = 2          # CA_SHARED_BINS: distinct strata of a wave that are counted once for the wave
CLASS_MAX = 16           # MCGRA_CLASS_MAX
STRATA_MAX = 136
MAX_NIDX = 65535

INF = float("inf")
SIZES = {
    2: "one candidate",
    3: "three candidates",
    63: "a row shorter than a wave",
    64: "the longest row has 63 columns: one wave, one lane idle",
    65: "the longest row fills a wave",
    255: "the longest row leaves two lanes of the block idle",
    256: "the longest row leaves one lane idle",
    257: "the longest row has THREADS columns",
}
CS = (1, 2, 3, 7, 16)
KINDS = ("levels4", "negative", "zeros", "random")
THR_OF = {"levels4": 0.5, "negative": -1.25, "zeros": 0.0, "random": 0.5}
OUTSIDE = (-3, 99)       # the classes of the unselected nodes


def spread(rng, n, C):
    """A class in [0, C) per node, every class present when n >= C, in random order."""
    return rng.permutation(np.arange(n) % C).astype(np.int64)


def case(real, pred, classes, idx=None, pad=0, runs=(), brute=True):
    real, pred = only_lower(real, idx), only_lower(pred, idx)
    classes = np.asarray(classes, np.int64).copy()
    if idx is not None:
        out = np.setdiff1d(np.arange(len(classes)), idx)
        classes[out] = np.resize(OUTSIDE, len(out))
    return (real, pred, classes, None if idx is None else np.asarray(idx, np.int64), pad, tuple(runs), brute)


def all_hows(C, thr):
    return [(C, how, thr) for how in ("one", "same", "own", "blocks")]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(71)
    out = {}
    # the sizes, every node selected, for every C and every table
    for i, m in enumerate(SIZES):
        kind = KINDS[i % 4]
        real = graph(rng, m, min(1.0, 6.0 / m) if m > 3 else 0.6)
        pred = scores(rng, real, kind)
        for C in CS:
            out[f"m{m}_c{C}"] = case(real, pred, spread(rng, m, C), None, 0, all_hows(C, THR_OF[kind]))
    # the same sizes as a permuted strict subset of a larger graph, rows padded (ld > n), the rest's classes out of range
    for i, m in enumerate(SIZES):
        kind = KINDS[(i + 1) % 4]
        n = m + 37
        real = graph(rng, n, 8.0 / n if m > 3 else 0.5)
        pred = scores(rng, real, kind)
        sel = rng.permutation(n)[:m].copy()
        if (np.diff(sel) > 0).all():
            sel = sel[::-1].copy()                                         # never in ascending order
        for C in CS:
            out[f"sub{m}_c{C}"] = case(real, pred, spread(rng, n, C), sel, 11, all_hows(C, THR_OF[kind]))
    lv = lambda real: scores(rng, real, "levels4")
    # a class with one selected node: its diagonal stratum is empty
    n = 40
    real = graph(rng, n, 0.2)
    cl = spread(rng, n, 3)
    cl[cl == 2] = 0
    cl[17] = 2
    out["single_node_class"] = case(real, lv(real), cl, None, 0, all_hows(3, 0.5))
    # strata without an edge and without a non-edge: class 0 is a clique, no edge joins class 1 and class 2
    n = 45
    cl = spread(rng, n, 3)
    real = graph(rng, n, 0.25)
    real[np.ix_(cl == 0, cl == 0)] = 1
    real[np.ix_(cl == 1, cl == 2)] = 0
    real[np.ix_(cl == 2, cl == 1)] = 0
    np.fill_diagonal(real, 0)
    out["no_edges_no_non_edges"] = case(real, lv(real), cl, None, 0, all_hows(3, 0.5))
    real = 1 - np.eye(66, dtype=np.float32)
    out["complete_n66"] = case(real, lv(real), spread(rng, 66, 7), None, 0, all_hows(7, 0.5))          # N_g = 0 everywhere
    real = np.zeros((66, 66), np.float32)
    out["empty_n66"] = case(real, lv(real), spread(rng, 66, 7), None, 0, all_hows(7, -INF))             # P = 0
    # more edges than samples: a stride of 3.  C = 3: long segments whose ends fall off the stride; C = 16: segments shorter
    # than one stride, some of one edge
    n = 200
    real = graph(rng, n, 0.5)
    pred = scores(rng, real, "random")
    out["dense_n200_c3"] = case(real, pred, spread(rng, n, 3), None, 0, all_hows(3, 0.5))
    cl = spread(rng, n, 16)
    cl[cl == 15] = 14
    cl[[5, 150]] = 15                                                       # class 15: two nodes
    real2 = real.copy()
    real2[5, 150] = real2[150, 5] = 1                                       # block 15-15: one candidate, an edge
    out["dense_n200_c16"] = case(real2, pred, cl, None, 0, [(16, "blocks", 0.5), (16, "own", 0.5), (16, "same", 0.5)])
    out["dense_n200_levels"] = case(real, lv(real), spread(rng, n, 7), None, 0, [(7, "blocks", 0.5), (7, "same", 0.75)])
    # the scores
    real = graph(rng, 90, 0.1)
    cl = spread(rng, 90, 4)
    out["negative"] = case(real, scores(rng, real, "negative"), cl, None, 0, all_hows(4, -1.25))
    zero = [float(bits(w)[0]) for w in (0x80000000, 0, 1, 0x80000001)]
    out["signed_zeros"] = case(real, scores(rng, real, "zeros"), cl, None, 0, [(4, "blocks", t) for t in zero] + [(4, "same", zero[0])])
    out["thresholds"] = case(real, lv(real), cl, None, 0, [(4, "blocks", t) for t in (-INF, INF, 0.5, 0.75, None)] + [(4, "same", None)])
    # wrong readings (tests/test_class_cases_cpu.py names what each tells apart)
    n = 30
    real = graph(rng, n, 0.25)
    sel = rng.permutation(n)[:21].copy()
    out["wrong_readings"] = case(real, lv(real), spread(rng, n, 3), sel, 0, all_hows(3, 0.5))
    # the passes' grids: more rows than ROW_BLOCKS, more edges than one sort tile
    n = 1100
    real = graph(rng, n, 0.004)
    cl = spread(rng, n, 7)
    out["sparse_n1100"] = case(real, scores(rng, real, "levels4", 0.05), cl, None, 0, [(7, "blocks", 0.5), (7, "same", 0.5)], False)
    sel = rng.permutation(n)[:ROW_BLOCKS + 30].copy()
    out["sparse_sub1054"] = case(real, scores(rng, real, "random", 0.05), spread(rng, n, 16), sel, 4,
                                 [(16, "blocks", 0.5), (16, "own", 0.5)], False)
    for v in out.values():
        for mtx in v[:3]:
            mtx.setflags(write=False)
    return out
