"""The inputs of the edge-DP tests (tests/test_gpu_dp_graph.py runs them on the device, tests/test_dp_cases_cpu.py shows without
one that they have the properties they are there for).  Everything is generated from seeds; nothing is read from a file.

The kernel works on 64 x 64 tiles, one block each, numbered along the lower triangle of tiles, so the node counts sit on both
sides of one tile (63, 64, 65), of two (127, 128, 129) and of many (1 025, 4 097: 2 145 tiles, 8.4e6 pairs, the largest whose
truth numpy builds in about two seconds); 2 and 3 are the smallest graphs there are."""
import functools
import math

import numpy as np

from tests import dp_truth as T

SEED_LO = 15
SEED_HI = 15 | (0x9e3779b9 << 32)             # differs from SEED_LO in the high 32 bits only
SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 1025)
BIG = 4097
LARGE = 65535                                 # the capacity
LARGE_ROWS = (1, 46341, 65534)                # the first row, the row at which p passes 2^30, the last
GRAPHS = ("empty", "complete", "random")
EDGERAND_EPS = (0.1, 1.0, 8.0, 50.0)          # 50: T = 0, the identity
LAP_EPS = (0.1, 1.0, 8.0)
LAP_NOISE_EPS = 1e-3                          # the noise dominates: the target clamps
LAP_EXACT_EPS = 1e4                           # no cell crosses 1/2 and the count's noise is below 1/2: the graph itself
# found by a search on the CPU and checked by test_dp_cases_cpu.py: seeds whose count draw at LAP_NOISE_EPS clamps to 0 / to m at n = 65,
# and a seed at n = 1 025, eps = 1 whose E~-th and (E~ + 1)-th best cells are equal (the tie rule decides the result)
CLAMP_N = 65
CLAMP_ZERO_SEED = 0
CLAMP_ALL_SEED = 3
TIE_N = 1025
TIE_SEED = 366


@functools.lru_cache(maxsize=None)
def graph(kind, n):
    """A symmetric 0 / 1 float32 matrix with zero diagonal (read-only)."""
    if kind == "empty":
        A = np.zeros((n, n), np.float32)
    elif kind == "complete":
        A = np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32)
    elif kind == "asymmetric":      # lower triangle: the random graph; upper triangle: its complement.  Only the lower one may be read
        A = np.array(graph("random", n))
        iu = np.triu_indices(n, 1)
        A[iu] = 1.0 - A[iu]
    else:
        rng = np.random.RandomState(1000 + n)
        low = np.tril(rng.rand(n, n) < 0.01, -1)
        A = (low | low.T).astype(np.float32)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def boundary_eps(n=65, seed=SEED_LO):
    """(eps, p): an eps whose EdgeRand threshold T EQUALS the draw w0 of pair p of an n-node graph under `seed`, replicate 0:
    `w0 < T` leaves that pair alone, `w0 <= T` flips it."""
    w0, _ = T.draws(T.positions(n)[2], seed, 0)
    for p in np.flatnonzero((w0 > 1 << 24) & (w0 < 1 << 31)):
        t = int(w0[p])
        eps = math.log(4294967296.0 / t - 1.0)
        for _ in range(64):
            got = T.threshold(eps)[0]
            if got == t:
                return eps, int(p)
            eps = math.nextafter(eps, -math.inf if got < t else math.inf)
    raise AssertionError("no draw is a threshold")


def edgerand_cases():
    """(n, graph, eps, seed, replicate): every size on the random graph, every graph, eps and seed at the sizes around one tile
    edge and two, both replicates."""
    cases = [(n, "random", 1.0, SEED_LO, 0) for n in SIZES + (BIG,)]
    for n in (65, 129):
        cases += [(n, g, eps, SEED_LO, 0) for g in GRAPHS for eps in EDGERAND_EPS if (g, eps) != ("random", 1.0)]
    cases += [(129, "random", 1.0, SEED_HI, 0), (129, "random", 1.0, SEED_LO, 1), (2, "complete", 0.1, SEED_HI, 1),
              (3, "empty", 0.1, SEED_LO, 0), (129, "asymmetric", 1.0, SEED_LO, 0), (65, "random", boundary_eps()[0], SEED_LO, 0)]
    return cases


def lapgraph_cases():
    """(n, graph, eps, seed, replicate)"""
    cases = [(n, "random", 1.0, SEED_LO, 0) for n in SIZES]
    cases += [(129, g, eps, SEED_LO, 0) for g in GRAPHS for eps in LAP_EPS if (g, eps) != ("random", 1.0)]
    cases += [(129, "random", 1.0, SEED_HI, 0), (129, "random", 1.0, SEED_LO, 1),
              (CLAMP_N, "random", LAP_NOISE_EPS, CLAMP_ZERO_SEED, 0), (CLAMP_N, "random", LAP_NOISE_EPS, CLAMP_ALL_SEED, 0),
              (129, "random", LAP_EXACT_EPS, SEED_LO, 0), (129, "complete", LAP_EXACT_EPS, SEED_LO, 0),
              (129, "asymmetric", 1.0, SEED_LO, 0), (TIE_N, "random", 1.0, TIE_SEED, 0)]
    return cases


def case_id(c):
    return "n{}-{}-eps{:g}-seed{:x}-r{}".format(*c)
