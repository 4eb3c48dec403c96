"""The inputs of tests/test_gpu_exposure.py, built once: name -> (real, pred, idx, pad, thresholds).
tests/test_exposure_cases_cpu.py checks, without a GPU, that they have the properties they are named for and tell each wrong
reading of the definition from the right one.  pad > 0 puts both matrices' rows into buffers that many columns wider.  Every
case holds NaN everywhere outside the selected strict lower triangle, labels included, unless it says otherwise."""
import functools

import numpy as np

from tests.delong_cases import bits, graph
from tests.graph_structure_cases import circulant  # noqa: F401  (the capacity case, small: tests/test_exposure_cases_cpu.py)
from tests.hop_cases import case as _hop_case
from tests.hop_cases import edges_graph, path, scores, star

# csrc/edge_exposure.hip, csrc/delong_common.h and csrc/rank_common.h
WORD = 64                # BG_TILE: positions per tile side, bits per word, lanes that stride a row
ROW_BLOCKS = 1024        # EE_ROW_BLOCKS: blocks of the passes over the selected rows (row a = 1 + block, + grid, ...)
EDGE_WAVES = 1024 * 4    # EE_EDGE_BLOCKS blocks of four waves, a wave an edge: more edges than this and a wave takes a second one
STAGE = 4096             # DL_STAGE: more positives than this and the staged samples are a stride apart
MAX_NIDX = 65535         # the capacity: 1024 words per row

INF = float("inf")
SIZES = {
    2: "one candidate",
    3: "three candidates",
    63: "one word, a pad bit",
    64: "one full word",
    65: "two words: an off-diagonal tile of one row",
    127: "two words, one pad bit",
    128: "two full words: three tiles",
    129: "three words: six tiles",
}
THROUGH_EDGES = ((0, 2), (0, 1), (1, 2), (2, 3), (4, 1), (4, 0), (4, 5))        # node 1 is a common neighbour of 0-2 and of 0-4


def case(real, pred, idx=None, pad=0, thresholds=(0.5,)):
    real, pred, idx, pad, _ = _hop_case(real, pred, idx, pad)
    return real, pred, idx, pad, tuple(thresholds)


def cliques(n, groups, extra=()):
    """Complete graphs on each of `groups` (lists of nodes) and the edges of `extra`."""
    return edges_graph(n, [(a, b) for g in groups for i, a in enumerate(g) for b in g[:i]] + list(extra))


def constant(n, value):
    return np.full((n, n), value, np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(61)
    out = {}
    kinds = ("levels4", "negative", "zeros", "random")
    thr_of = {"levels4": 0.5, "negative": -1.25, "zeros": 0.0, "random": 0.5}
    # the sizes, every node selected: mean degree about 8, so that edges have common neighbours
    for i, m in enumerate(SIZES):
        kind = kinds[i % 4]
        real = graph(rng, m, min(0.7, 8.0 / m))
        if m == 2:
            real = edges_graph(2, [(1, 0)])
        out[f"m{m}"] = case(real, scores(rng, real, kind), None, 0, (thr_of[kind], None))
    # the same sizes as a permuted strict subset of a larger graph, rows padded (ld > n): the rest lends no neighbour
    for i, m in enumerate(SIZES):
        kind = kinds[(i + 1) % 4]
        n = m + 37
        real = graph(rng, n, min(0.7, 10.0 / n))
        sel = rng.permutation(n)[:m].copy()
        if (np.diff(sel) > 0).all():
            sel = sel[::-1].copy()                                         # never in ascending order
        out[f"sub{m}"] = case(real, scores(rng, real, kind), sel, 11, (thr_of[kind], -INF))
    lv = lambda real: scores(rng, real, "levels4")
    # the graphs
    real = np.zeros((66, 66), np.float32)
    out["empty_n66"] = case(real, lv(real), None, 0, (0.5, -INF))                  # P = 0
    real = 1 - np.eye(66, dtype=np.float32)
    out["complete_n66"] = case(real, lv(real), None, 0, (0.5, -INF))               # N = 0: every T is 0; c = 64, d = 65
    real = edges_graph(5, [(3, 1)])
    out["one_edge"] = case(real, lv(real), None, 0, (0.5, INF))
    real = star(70, 33)                                                            # c = 0 and min degree 1 everywhere, max 69
    out["star_n70"] = case(real, lv(real))
    real = cliques(40, [list(range(3, 20))])                                       # a clique of 17: c = 15, the first of "15+"
    out["clique17"] = case(real, lv(real))
    real = cliques(40, [list(range(20, 38))])                                      # a clique of 18: c = 16, in "15+" too
    out["clique18"] = case(real, lv(real))
    real = cliques(70, [list(range(0, 20)), list(range(50, 68))], [(19, 50)])      # the bridge: c = 0 between degrees 20 and 18
    out["two_cliques_bridge"] = case(real, lv(real))
    real = path(11)
    out["path_n11"] = case(real, lv(real))
    # the scores
    real = graph(rng, 40, 0.2)
    out["all_equal"] = case(real, constant(40, 0.25), None, 0, (0.25, 0.5))        # every placement is N
    coin = np.tril(rng.rand(40, 40), -1)
    out["two_valued"] = case(real, np.where(coin + coin.T < 0.5, 0.25, 0.75).astype(np.float32), None, 0, (0.75, 0.25))
    out["signed_zeros"] = case(real, scores(rng, real, "zeros"), None, 0,          # with the smallest subnormals of both signs
                               (float(bits(0x80000000)[0]), 0.0, float(bits(1)[0]), float(bits(0x80000001)[0])))
    out["negative"] = case(real, scores(rng, real, "negative"), None, 0, (-1.25, -1.0))
    # wrong readings (tests/test_exposure_cases_cpu.py names what each tells apart)
    real = edges_graph(6, THROUGH_EDGES)                                           # not masked: node 1 is there, and not selected
    out["through_unselected"] = (real, lv(real), np.asarray([0, 2, 3, 5, 4], np.int64), 0, (0.5,))
    # the passes' grids: one row past ROW_BLOCKS; more edges than EDGE_WAVES and than STAGE, about 19 a word
    n = ROW_BLOCKS + 1
    real = graph(rng, n, 0.006)
    out["sparse_n1025"] = case(real, scores(rng, real, "levels4", 0.05), None, 0, (0.5,))
    sel = rng.permutation(n + 60)[:n].copy()
    real = graph(rng, n + 60, 0.006)
    out["sparse_sub1025"] = case(real, scores(rng, real, "random", 0.05), sel, 4, (0.5,))
    real = graph(rng, 200, 0.3)
    out["dense_n200"] = case(real, scores(rng, real, "random"), None, 0, (0.5, 0.8))
    for v in out.values():
        for mtx in v[:2]:
            mtx.setflags(write=False)
    return out
