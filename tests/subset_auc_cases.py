"""The inputs of tests/test_gpu_subset_auc.py, and what tests/test_subset_auc_cases_cpu.py checks about them without a GPU.

A case is (real [n x n], comps [K x n x n] float32, idx or None, pad, mask lists).  The selections are the sizes at which the
kernels change behaviour: one pair, one row of two, a row shorter than, as long as and longer than a wave (63, 64, 65), longer
than half a block (129) and longer than a block (257).  K is 1, 3 or 8; the mask lists are one mask, the 25-mask ablation table,
all 2^K - 1 masks and a list with repeats.  SAMPLES_AT_255 is what one segment keeps in LDS when a call has 255 distinct masks:
the dense case has far more edges than that, the sparse ones fewer."""
import numpy as np

SIZES = (2, 3, 63, 64, 65, 129, 257)
KS = (1, 3, 8)
MAX_NIDX = 65535
SMP_WORDS = 8192                            # SA_SMP_WORDS of csrc/subset_auc.hip
SAMPLES_AT_255 = SMP_WORDS // 255           # 32


def graph(rng, n, p):
    """A symmetric 0 / 1 float32 adjacency with an empty diagonal, edge probability p."""
    up = np.triu(rng.rand(n, n) < p, 1)
    return (up | up.T).astype(np.float32)


def all_masks(K):
    return list(range(1, 1 << K))


def table_masks():
    """The table (at most 25 masks) of a run with every prior: present = used = 0xff (tests/subset_auc_truth.ablation_masks' rules)."""
    from tests import subset_auc_truth as T
    table = T.ablation_masks(0xff, 0xff)
    assert len(table) == 21                      # (four rows of the flag table are `used` or `used` without one summand)
    return table


def repeats(K):
    top = (1 << K) - 1
    return [top, 1, top, 1 << (K - 1), 1, top]


def floats(rng, K, n):
    """Asymmetric, signed, distinct magnitudes: the order of the adds shows in the last bit."""
    c = rng.randn(K, n, n).astype(np.float32)
    return c * (10.0 ** rng.randint(-3, 4, size=(K, 1, 1))).astype(np.float32)


def small_ints(rng, K, n):
    """Every sum exact, ties everywhere; component K - 1 is a {0, 1} matrix; signed zeros among the entries."""
    c = rng.randint(-2, 3, size=(K, n, n)).astype(np.float32)
    c[K - 1] = rng.randint(0, 2, size=(n, n))
    c[0][rng.rand(n, n) < 0.1] = -0.0
    return c


def cancellation(real, edges=(1e8, 1.0, -1e8)):
    """(1e8, 1, -1e8) on the edges against (0, 0.5, 0) on the non-edges: the ascending sum of mask 0b111 is (1e8 + 1) - 1e8 =
    0.0f on the edges (T = 0); the float64 sum and the order (1e8 - 1e8) + 1 give 1 (T = 2 P N).  edges = (1, 1e8, -1e8): the
    ascending sum is 0.0f again and the DESCENDING one (-1e8 + 1e8) + 1 = 1."""
    e = real == 1
    k = int(np.argmin(np.abs(edges)))
    return np.stack([np.where(e, v, 0.5 if j == k else 0.0) for j, v in enumerate(edges)]).astype(np.float32)


def symmetric(c):
    """The lower triangles mirrored: what is read does not depend on the order of a pair's ends in idx."""
    low = np.tril(c, -1)
    return low + np.transpose(low, (0, 2, 1))


def cases():
    rng = np.random.RandomState(20240607)
    out = {}
    for i, m in enumerate(SIZES):
        K = KS[i % 3]
        kind = (floats, small_ints)[i % 2]
        lists = [all_masks(K), [all_masks(K)[-1]], repeats(K)] + ([table_masks()] if K == 8 else [])
        out[f"all{m}_k{K}"] = (graph(rng, m, 0.3 if m > 3 else 1.0 if m == 2 else 0.6), kind(rng, K, m), None, 0, lists)
    # K = 8 at every size where a row is longer than a wave; K = 1 and 3 beside it
    out["ints129_k8"] = (graph(rng, 129, 0.1), small_ints(rng, 8, 129), None, 0, [all_masks(8), table_masks()])
    out["floats65_k1"] = (graph(rng, 65, 0.2), floats(rng, 1, 65), None, 3, [[1], [1, 1]])
    out["ints64_k3"] = (graph(rng, 64, 0.2), small_ints(rng, 3, 64), None, 0, [all_masks(3), repeats(3)])
    # a subset and its permutation, n > n_idx, padded rows
    n = 300
    sub = rng.permutation(n)[:257]
    real, comps = graph(rng, n, 0.05), symmetric(floats(rng, 8, n))      # symmetric: a permutation of idx changes nothing
    out["sub257_k8"] = (real, comps, sub, 5, [table_masks(), repeats(8)])
    out["sub257_k8_permuted"] = (real, comps, sub[rng.permutation(257)], 5, [table_masks(), repeats(8)])
    sub = rng.permutation(100)[:63]
    real, comps = graph(rng, 100, 0.2), small_ints(rng, 3, 100)
    out["sub63_k3"] = (real, comps, sub, 1, [all_masks(3)])                # asymmetric: [idx[a]][idx[b]], not its mirror
    out["sym63_k3"] = (real, symmetric(comps), sub, 1, [all_masks(3)])
    out["sym63_k3_permuted"] = (real, symmetric(comps), sub[::-1].copy(), 1, [all_masks(3)])
    # the classes: one edge, none, no non-edge; far more edges than a segment's samples under 255 masks
    one = np.zeros((65, 65), np.float32)
    one[40, 7] = one[7, 40] = 1
    out["one_edge"] = (one, floats(rng, 3, 65), None, 0, [all_masks(3)])
    out["no_edge"] = (np.zeros((64, 64), np.float32), small_ints(rng, 3, 64), None, 0, [all_masks(3)])
    out["complete"] = (1 - np.eye(63, dtype=np.float32), floats(rng, 3, 63), None, 0, [all_masks(3)])
    out["dense257_k8"] = (graph(rng, 257, 0.5), floats(rng, 8, 257), None, 0, [all_masks(8)])
    out["dense257_k8_ints"] = (graph(rng, 257, 0.5), small_ints(rng, 8, 257), None, 2, [all_masks(8)])
    real = graph(rng, 65, 0.15)
    out["cancellation"] = (real, cancellation(real), None, 0, [all_masks(3), [7]])
    out["cancellation_descending"] = (real, cancellation(real, (1.0, 1e8, -1e8)), None, 0, [all_masks(3), [7]])
    return out
