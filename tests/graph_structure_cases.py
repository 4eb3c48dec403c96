"""The inputs of tests/test_gpu_graph_structure.py, built once: name -> (real, pred, idx, thresholds).  Every case is run with
and without `real`, at each of its thresholds.  tests/test_graph_structure_cases_cpu.py checks, without a GPU, that they have the
properties they are named for and tell each wrong reading of the definition from the right one.  Crafted cases hold NaN
everywhere outside the selected strict lower triangle, labels included."""
import functools

import numpy as np

from tests.delong_cases import bits, graph, lower, pairs_of

# csrc/graph_structure.hip
WORD = 64                # GS_TILE: positions per tile side, bits per word, lanes per wave
THREADS = 256            # AUC_THREADS: a block is four waves; a wave packs 16 rows of a tile and counts every fourth word of a row
BATCH = 8                # GS_BATCH: a word of a row with at least 8 neighbours is counted 8 rows a step, the rest one a step
MAX_NIDX = 65535         # the capacity (include/mcgra.h): W = 1024 words per row

# selections on both sides of each size at which the kernels change behaviour
SIZES = {
    63: "one word, one diagonal tile, a pad bit",
    64: "one full word, no pad bits",
    65: "two words: an off-diagonal tile of one row, 63 pad bits in the second word",
    127: "two words, one pad bit",
    128: "two full words: three tiles",
    129: "three words: six tiles",
}
SPARSE_SIZES = {
    4095: "W = 64 words: one word per lane of the count's stride, one pad bit",
    4096: "W = 64 full words",
    4097: "W = 65: the first lane takes a second word",
    4160: "W = 65 full words",
}
COMPLETE = (65, 100, 127, 130)      # complete graphs (threshold -inf): every pad bit a wrong kernel could set is counted


def words(m):
    return -(-m // WORD)


def noisy_copy(rng, real, flips, levels=8):
    """Scores in multiples of 1 / levels (many ties): high where `real` has an edge, low elsewhere, `flips` of the pairs swapped;
    symmetric, the diagonal 0."""
    n = real.shape[0]
    a, b = np.tril_indices(n, -1)
    lab = real[a, b] > 0
    swap = rng.rand(len(a)) < flips
    s = np.where(lab ^ swap, rng.randint(levels // 2, levels, len(a)), rng.randint(0, levels // 2, len(a))) / levels
    out = np.zeros((n, n), np.float32)
    out[a, b] = s
    return out + out.T


def circulant(n):
    """The capacity case, as numpy (small n): 1 where (a - b) mod n is +-1 or +-2, else 0; scores and labels at once."""
    a, b = np.indices((n, n))
    d = (a - b) % n
    return ((d == 1) | (d == 2) | (d == n - 1) | (d == n - 2)).astype(np.float32)


def circulant_truth(n):
    """The integers of circulant(n) at threshold 0.5, n >= 7: every node has degree 4 and lies in the three triangles
    {v - 2, v - 1, v}, {v - 1, v, v + 1}, {v, v + 1, v + 2}; R = G = C."""
    assert n >= 7
    out = {"pairs": pairs_of(n)}
    for g in "RGC":
        out[f"d_{g}"], out[f"t_{g}"], out[f"E_{g}"], out[f"T_{g}"] = [4] * n, [3] * n, 2 * n, n
    out["W_R"] = out["W_G"] = 6 * n
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(47)
    inf = float("inf")
    out = {}
    out["m2_edge"] = (lower([1], 2), lower([0.5], 2), None, (0.5, 0.75))
    out["m2_no_label"] = (lower([0], 2), lower([0.5], 2), None, (0.5,))
    out["m3_triangle"] = (lower([1, 1, 1], 3), lower([0.5, 0.75, 0.5], 3), None, (0.5, 0.625))
    out["m3_path"] = (lower([1, 0, 1], 3), lower([0.5, 0.25, 0.5], 3), None, (0.5,))
    out["m4_missing_triangle"] = (lower([1, 1, 1, 0, 0, 0], 4), lower([0.9, 0.9, 0.1, 0.9, 0.1, 0.1], 4), None, (0.5,))
    # ties at the threshold: `>` for `>=` loses every pair that scores exactly the threshold
    for m, why in SIZES.items():
        real = graph(rng, m, 0.3)
        out[f"m{m}"] = (real, noisy_copy(rng, real, 0.15), None, (0.5, 0.75, -inf, inf))
    for m in COMPLETE:
        if f"m{m}" not in out:
            real = graph(rng, m, 0.5)
            out[f"m{m}"] = (real, noisy_copy(rng, real, 0.1), None, (0.5, -inf))
    # -0.0 beside +0.0 and subnormals of both signs: -0.0 >= +0.0 holds, a negative subnormal is below both
    odd = bits(0x80000000, 0, 1, 0x80000001)
    n = 40
    out["signed_zeros"] = (graph(rng, n, 0.3), lower(odd[rng.randint(0, 4, pairs_of(n))], n), None,
                           (float(odd[0]), 0.0, float(odd[2]), float(odd[3])))
    # asymmetric: the upper triangle holds the opposite decision (and NaN), the labels' upper triangle the opposite label; the
    # diagonal passes every threshold and is labelled 1
    n = 70
    real = graph(rng, n, 0.25)
    pred = noisy_copy(rng, real, 0.1)
    up = np.triu(np.ones((n, n), bool), 1)
    pred[up] = (1.0 - pred)[up]
    pred[up & (rng.rand(n, n) < 0.2)] = np.nan
    real = real.copy()
    real[up] = 1 - real[up]
    np.fill_diagonal(pred, 2.0)
    np.fill_diagonal(real, 1.0)
    out["asymmetric"] = (real, pred, None, (0.5,))
    # n > m with a permuted idx; nothing outside the selection is valid
    n = 300
    real = graph(rng, n, 0.1)
    pred = noisy_copy(rng, real, 0.05)
    sel = rng.permutation(n)[:100].copy()
    off = np.ones(n, bool); off[sel] = False
    real, pred = real.copy(), pred.copy()
    for mtx in (real, pred):
        mtx[off] = np.nan
        mtx[:, off] = np.inf
    out["subset_permuted"] = (real, pred, sel, (0.5, 0.875))
    n = 40
    real = graph(rng, n, 0.3)
    out["idx_descending"] = (real, rng.rand(n, n).astype(np.float32), np.arange(n - 1, -1, -2).copy(), (0.5,))
    # node kinds: a hub joined to every node plus a sparse rest, an isolated node
    n = 400
    real = graph(rng, n, 0.01)
    real[5, :] = real[:, 5] = 1
    real[5, 5] = 0
    real[23, :] = real[:, 23] = 0
    pred = noisy_copy(rng, real, 0.002)
    pred[5, :] = pred[:, 5] = 0.875
    pred[23, :] = pred[:, 23] = 0.0
    out["hub_and_isolated"] = (real, pred, None, (0.5,))
    # G == R: the six columns are three times the same two
    real = graph(rng, 90, 0.2)
    out["g_equals_r"] = (real, (real * 0.75).astype(np.float32), None, (0.5,))
    # the closed form of the capacity case, small
    out["circulant_n70"] = (circulant(70), circulant(70), None, (0.5,))
    # W on both sides of one 64-lane stride: the leading blocks of one sparse graph
    n = max(SPARSE_SIZES)
    real = graph(rng, n, 0.003)
    keep = np.tril(rng.rand(n, n) < 0.9, -1)
    pred = noisy_copy(rng, real * (keep | keep.T), 0.0005)       # a tenth of the true edges missed, as many false ones added
    for m in sorted(SPARSE_SIZES):
        out[f"sparse_m{m}"] = (real[:m, :m], pred[:m, :m], None, (0.5,))
    for v in out.values():
        for mtx in v[:2]:
            mtx.setflags(write=False)
    return out
