"""The inputs of tests/test_gpu_hops.py, built once: name -> (real, pred, idx, pad, runs), runs a tuple of (hops, threshold).
tests/test_hop_cases_cpu.py checks, without a GPU, that they have the properties they are named for and tell each wrong reading
of the definition from the right one.  pad > 0 puts both matrices' rows into buffers that many columns wider.  Every case
holds NaN everywhere outside the selected strict lower triangle, labels included, unless it says otherwise."""
import functools

import numpy as np

from tests.delong_cases import bits, graph
from tests.graph_structure_cases import circulant  # noqa: F401  (the capacity case, small: tests/test_hop_cases_cpu.py)

# csrc/hop_auc.hip and csrc/rank_common.h
WORD = 64                # HA_TILE: positions per tile side, bits per word
THREADS = 256            # AUC_THREADS: a row pass takes 256 columns a step; a lane of the expansion owns the words t, t + 256, ..
BATCH = 8                # HA_BATCH: a word of a row with at least 8 neighbours is expanded 8 rows a step, the rest one a step
ROW_BLOCKS = 1024        # HA_ROW_BLOCKS: blocks of the passes over the selected rows (row a = 1 + block, + grid, ...)
SORT_TILE = 1024         # AUC_SORT_TILE: up to SORT_TILE positives are one sort block, one step
HOP_MAX = 8              # MCGRA_HOP_MAX
MAX_NIDX = 65535         # the capacity: W = 1024 words per row, four per lane of the expansion
SECOND_WORD_N = 64 * THREADS + 63      # W = THREADS + 1: the first lane of the expansion owns a second word

INF = float("inf")
THROUGH_EDGES = ((0, 1), (1, 2), (2, 3), (4, 1), (4, 5))        # through_unselected: node 1 joins 0, 2 and 4
SIZES = {
    2: "one candidate",
    3: "three candidates",
    63: "one word, a pad bit",
    64: "one full word",
    65: "two words: an off-diagonal tile of one row",
    127: "two words, one pad bit",
    128: "two full words: three tiles",
    129: "three words: six tiles",
    257: "the longest row has THREADS columns; five words",
}
HOPS = (1, 3, 8)


def words(m):
    return -(-m // WORD)


def only_lower(mat, idx=None, junk=np.nan):
    """A copy of mat that keeps the selected strict lower triangle and holds junk everywhere else."""
    mat = np.asarray(mat, np.float32)
    ix = np.arange(len(mat)) if idx is None else np.asarray(idx, np.int64)
    a, b = np.tril_indices(len(ix), -1)
    out = np.full(mat.shape, junk, np.float32)
    out[ix[a], ix[b]] = mat[ix[a], ix[b]]
    return out


def edges_graph(n, edges):
    real = np.zeros((n, n), np.float32)
    for a, b in edges:
        real[a, b] = real[b, a] = 1
    return real


def path(n, order=None):
    """The path order[0] - order[1] - ... - order[n - 1]."""
    o = list(range(n)) if order is None else list(order)
    return edges_graph(n, zip(o[:-1], o[1:]))


def cycle(n, order=None):
    o = list(range(n)) if order is None else list(order)
    return edges_graph(n, zip(o, o[1:] + o[:1]))


def star(n, hub):
    return edges_graph(n, [(hub, v) for v in range(n) if v != hub])


def scores(rng, real, kind, flips=0.2):
    """A symmetric score matrix that ranks most edges of `real` and the pairs next to them above the rest.  kind "levels4":
    multiples of 1 / 4 (massive ties); "negative": every score below zero; "zeros": +-0.0 and the smallest subnormals of both
    signs; "random": no ties."""
    n = len(real)
    a, b = np.tril_indices(n, -1)
    lab = real[a, b] > 0
    high = lab ^ (rng.rand(len(a)) < flips)
    if kind == "levels4":
        s = np.where(high, rng.randint(2, 4, len(a)), rng.randint(0, 3, len(a))) / 4.0
    elif kind == "negative":
        s = -1.0 - np.where(high, rng.randint(0, 3, len(a)), rng.randint(2, 6, len(a))) / 8.0
    elif kind == "zeros":
        odd = bits(0x80000001, 0x80000000, 0, 1)                       # -tiny < -0.0 == +0.0 < tiny
        s = odd[np.where(high, rng.randint(1, 4, len(a)), rng.randint(0, 3, len(a)))]
    else:
        s = np.where(high, 0.5, 0.0) + rng.rand(len(a)) * 0.6
    out = np.zeros((n, n), np.float32)
    out[a, b] = out[b, a] = s                                          # (no addition: -0.0 stays -0.0)
    return out


def case(real, pred, idx=None, pad=0, runs=((3, 0.5),)):
    real, pred = only_lower(real, idx), only_lower(pred, idx)
    return (real, pred, None if idx is None else np.asarray(idx, np.int64), pad, tuple(runs))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(53)
    out = {}
    kinds = ("levels4", "negative", "zeros", "random")
    thr_of = {"levels4": 0.5, "negative": -1.25, "zeros": 0.0, "random": 0.5}
    # the sizes, every node selected: a sparse random graph (mean degree about 3: distances up to ten and several components)
    for i, m in enumerate(SIZES):
        kind = kinds[i % 4]
        real = graph(rng, m, min(1.0, 3.0 / m) if m > 3 else 0.6)
        if m == 2:
            real = edges_graph(2, [(1, 0)])
        out[f"m{m}"] = case(real, scores(rng, real, kind), None, 0, [(h, thr_of[kind]) for h in HOPS] + [(3, None)])
    # the same sizes as a permuted strict subset of a larger graph, rows padded (ld > n): no path runs through the rest
    for i, m in enumerate(SIZES):
        kind = kinds[(i + 1) % 4]
        n = m + 37
        real = graph(rng, n, 4.0 / n if m > 3 else 0.5)
        sel = rng.permutation(n)[:m].copy()
        if (np.diff(sel) > 0).all():
            sel = sel[::-1].copy()                                         # never in ascending order
        out[f"sub{m}"] = case(real, scores(rng, real, kind), sel, 11, [(3, thr_of[kind]), (8, -INF)])
    # the graphs
    lv = lambda real: scores(rng, real, "levels4")
    real = path(11)                                                        # distances 1 .. 10: every class holds pairs, beyond too
    out["path_n11"] = case(real, lv(real), None, 0, [(1, 0.5), (3, 0.5), (8, 0.5)])
    real = path(130, rng.permutation(130))                                 # a long path whose neighbours lie in other words
    out["path_n130_shuffled"] = case(real, lv(real), None, 0, [(3, 0.5), (8, 0.75)])
    real = np.zeros((75, 75), np.float32)
    real[:40, :40] = cycle(40)
    real[40:, 40:] = graph(rng, 35, 0.1)
    out["two_components"] = case(real, lv(real), None, 0, [(3, 0.5), (8, 0.5)])
    real = star(70, 33)                                                    # a hub row; every non-edge at distance 2
    out["star_n70"] = case(real, lv(real), None, 0, [(1, 0.5), (3, 0.5)])
    real = 1 - np.eye(66, dtype=np.float32)
    out["complete_n66"] = case(real, lv(real), None, 0, [(1, 0.5), (3, -INF)])        # N = 0
    real = np.zeros((66, 66), np.float32)
    out["empty_n66"] = case(real, lv(real), None, 0, [(1, 0.5), (8, -INF)])           # P = 0: everything beyond
    for n in (5, 16, 17):                                                  # the distance wraps; n = 16 is bipartite
        real = cycle(n)
        out[f"cycle_n{n}"] = case(real, lv(real), None, 0, [(1, 0.5), (3, 0.5), (8, 0.5)])
    # a hub joined to every node of a sparse rest, an isolated node, words with 8 and more neighbours beside words with fewer
    n = 300
    real = graph(rng, n, 0.01)
    real[5, :] = real[:, 5] = 1
    real[5, 5] = 0
    real[23, :] = real[:, 23] = 0
    out["hub_and_isolated"] = case(real, lv(real), None, 0, [(3, 0.5)])
    real = graph(rng, 200, 0.13)                                           # about eight neighbours a word: batches and leftovers
    out["dense_n200"] = case(real, scores(rng, real, "random"), None, 0, [(3, 0.5), (1, 0.8)])
    # the thresholds: -inf, +inf, a score that is present, -0.0 against +0.0
    real = graph(rng, 40, 0.08)
    out["thresholds"] = case(real, lv(real), None, 0, [(3, -INF), (3, INF), (3, 0.5), (3, 0.75), (3, None)])
    out["signed_zeros"] = case(real, scores(rng, real, "zeros"), None, 0,
                               [(3, float(bits(0x80000000)[0])), (3, 0.0), (3, float(bits(1)[0])), (3, float(bits(0x80000001)[0]))])
    # wrong readings (tests/test_hop_cases_cpu.py names what each tells apart)
    real = edges_graph(6, THROUGH_EDGES)
    out["through_unselected"] = case(real, lv(real), [0, 2, 3, 5, 4], 0, [(3, 0.5)])          # node 1 joins 0, 2 and 4: unselected
    n = 30
    real = graph(rng, n, 0.12)
    pred = scores(rng, real, "levels4")
    up = np.triu(np.ones((n, n), bool), 1)
    real, pred = real.copy(), pred.copy()
    real[up] = 1 - real[up]                                                # the upper triangle: the opposite label, valid scores
    pred[up] = (0.75 - pred)[up]
    np.fill_diagonal(real, 1.0)
    np.fill_diagonal(pred, 0.75)
    out["asymmetric"] = (real, pred, None, 0, ((3, 0.5),))                 # not masked: what is outside is valid, and wrong
    real = graph(rng, 50, 0.07)
    out["recovered_differs"] = case(real, scores(rng, real, "levels4", 0.3), None, 0, [(3, 0.5)])
    # the passes' grids: more rows than ROW_BLOCKS, more positives than one sort tile, 18 words
    n = 1100
    real = graph(rng, n, 0.004)
    out["sparse_n1100"] = case(real, scores(rng, real, "levels4", 0.05), None, 0, [(3, 0.5), (8, 0.5)])
    sel = rng.permutation(n)[:ROW_BLOCKS + 30].copy()
    out["sparse_sub1054"] = case(real, scores(rng, real, "random", 0.05), sel, 4, [(3, 0.5)])
    for v in out.values():
        for mtx in v[:2]:
            mtx.setflags(write=False)
    return out

