"""The inputs of tests/test_gpu_influence.py and tests/test_influence_cases_cpu.py: small victims and graphs for
mcgra_influence_scores, each a dict {"A" (the float32 propagation matrix the victim answers from), "A_raw" (the 0 / 1 graph), "X",
"W", "b", "Wlin", "blin", "delta", "labels" (the true graph, for the AUC)}.  case(name) builds (and memoises) one; CASES lists them:

    name: (n, graph, mode, L, widths, nclass, nfeat, delta, what it is there for)

The sizes are the smallest at which the kernels can go wrong: one node, one word of the frontier mask (n <= 32), 63 / 64 / 65 around
the wave and the symmetrise tile, 130 and 257 past two and four tiles, 515 past the 512 persistent workgroups of a 256-CU device (a
workgroup then takes a second source); a star and a complete graph whose frontier is every node; widths 1, 7, 16, 33 and 64 (a lane a
column), per-layer widths that differ, 64 classes; 3 layers of width 64, whose staged weights fit the LDS budget (34.5 KB of 40 KB),
and 8 layers of width 40 on a 64-node path, whose weights (44.8 KB) do not and are read in place.
Weights and biases are drawn as models.gcn.GraphConvolution.reset_parameters draws them (uniform in +-1 / sqrt(out width)), the
features are sparse 0 / 1 rows scaled to sum 1, as the datasets' are; a `gapped` victim has its biases moved to +-(1 .. 2) and
its inner weights halved, so that no pre-activation of a long chain sits at a relu's corner and the magnitudes grow slowly with the
depth (tests/influence_truth.py: the exclusions)."""
import numpy as np

DELTA = 1e-4

CASES = {
    "one_node":       (1, "empty", "normalised", 2, (16, 16), 7, 24, DELTA, "n = 1: the self-influence alone"),
    "two_nodes":      (2, "path", "normalised", 2, (7, 7), 2, 1, DELTA, "n = 2, one feature"),
    "cycle63":        (63, "cycle", "normalised", 2, (16, 16), 7, 24, DELTA, "one row short of a wave"),
    "path64_deep":    (64, "path", "normalised", 8, (40,) * 8, 7, 24, DELTA, "8 layers; the weights do not fit the LDS budget"),
    "wide63":         (63, "planted", "normalised", 3, (64, 64, 64), 7, 24, DELTA, "width 64; the weights just fit the LDS budget"),
    "star65_raw":     (65, "star", "raw", 2, (33, 33), 64, 80, DELTA, "raw star: walks of exactly two steps; 64 classes; width 33"),
    "empty65_raw":    (65, "empty", "raw", 2, (16, 16), 7, 24, DELTA, "no cell at all: every influence is +0.0"),
    "complete130":    (130, "complete", "normalised", 2, (16, 16), 7, 24, DELTA, "every frontier is every node"),
    "planted130":     (130, "planted", "normalised", 2, (16, 16), 7, 24, DELTA, "the accuracy case of the command line's shape"),
    "planted130_raw": (130, "planted", "raw", 2, (16, 16), 7, 24, DELTA, "the same victim queried on the raw graph"),
    "planted130_l1":  (130, "planted", "normalised", 1, (64,), 7, 24, DELTA, "one layer: the support is the edges and the diagonal"),
    "mixed130":       (130, "planted", "normalised", 3, (33, 7, 16), 2, 24, DELTA, "widths that differ from layer to layer"),
    "components130":  (130, "two_components", "normalised", 3, (7, 7, 7), 2, 24, DELTA, "nothing crosses between the components"),
    "zero_row130":    (130, "planted", "normalised", 2, (16, 16), 7, 24, DELTA, "two nodes without features: their rows are +0.0"),
    "narrow64":       (64, "planted", "normalised", 2, (1, 1), 1, 24, DELTA, "width 1, one class: every influence is 0 up to rounding"),
    "planted257":     (257, "planted", "normalised", 3, (16, 16, 16), 7, 24, DELTA, "three layers past four tiles"),
    "planted515":     (515, "planted", "normalised", 2, (16, 16), 7, 80, DELTA, "more sources than persistent workgroups"),
    "star515":        (515, "star", "normalised", 2, (16, 16), 2, 1, DELTA, "a hub: every frontier is every node at n = 515"),
    "coarse130":      (130, "planted", "normalised", 2, (16, 16), 7, 24, 2.0 ** -7, "a large Delta: the finite difference is not its Jacobian"),
    "crossing":       (9, "path", "normalised", 2, (4, 4), 3, 2, 2.0 ** -7, "units that the perturbation switches on and off"),
    "softmax9":       (9, "path", "normalised", 2, (4, 4), 3, 2, 2.0 ** -4, "the crossing victim under a Delta that bends the softmax"),
}
EXACT = ("crossing", "softmax9")      # float32 computes their base pre-activations exactly: no entry is excluded
GAPPED = ("path64_deep", "wide63", "mixed130", "components130")
# the cases that look like a run of the command line: their exclusions and their AUC resolution are held to 1e-3
ACCURACY = ("planted130", "planted130_raw", "planted515", "zero_row130")

_memo = {}


def graph(kind, n, rng):
    """The 0 / 1 adjacency (symmetric, zero diagonal), float32."""
    A = np.zeros((n, n), np.float32)
    i = np.arange(n - 1)
    if kind == "path":
        A[i, i + 1] = 1
    elif kind == "cycle":
        A[i, i + 1] = 1
        A[n - 1, 0] = 1
    elif kind == "star":
        A[0, 1:] = 1
    elif kind == "two_components":
        h = n // 2 - 2                                            # a cycle of h nodes and a path of the rest
        A[np.arange(h - 1), np.arange(1, h)] = 1
        A[h - 1, 0] = 1
        A[np.arange(h, n - 1), np.arange(h + 1, n)] = 1
    elif kind == "complete":
        A[:] = 1
    elif kind == "planted":                                       # four communities, mean degree about 6, a few hubs by chance
        comm = rng.randint(0, 4, n)
        same = comm[:, None] == comm[None, :]
        p = np.where(same, min(1.0, 18.0 / n), min(1.0, 2.0 / n))
        A = np.triu((rng.rand(n, n) < p).astype(np.float32), 1)
    elif kind != "empty":
        raise ValueError(kind)
    A = np.maximum(A, A.T)
    np.fill_diagonal(A, 0)
    return A


def normalise(A):
    """utils.normalize_adj_tensor: D^-1/2 (A + I) D^-1/2, as float32."""
    B = A.astype(np.float64) + np.eye(A.shape[0])
    r = 1.0 / np.sqrt(B.sum(axis=1))
    return (B * r[:, None] * r[None, :]).astype(np.float32)


def _crossing():
    """A 9-node path, 2 features, widths 4, 3 classes, Delta = 2^-7, every value a small dyadic number so that float32 and float64
    compute the same base pre-activations EXACTLY.  A is the unnormalised path with self-loops (cells 1).  Layer 0's biases put named
    units at -dP / 2 (they switch on) and at +dP / 2 under a negative dP (they switch off) for the source 4."""
    n, delta = 9, 2.0 ** -7
    A = graph("path", n, None) + np.eye(n, dtype=np.float32)
    X = np.zeros((n, 2), np.float32)
    X[:, 0] = 1.0
    X[:, 1] = (np.arange(n) % 3).astype(np.float32) * 0.5
    W0 = np.array([[1.0, -1.0, 0.5, 0.25], [0.5, 1.0, -2.0, 0.0]], np.float32)
    W1 = np.array([[0.5, -0.5, 1.0, 0.25], [1.0, 0.5, -1.0, 0.5], [-0.5, 1.0, 0.5, -1.0], [0.25, 0.5, 1.0, 1.0]], np.float32)
    Wlin = np.array([[1.0, -0.5, 0.25, 0.5], [-1.0, 0.5, 1.0, -0.25], [0.5, 0.5, -0.5, 1.0]], np.float32)
    T0 = X.astype(np.float64) @ W0.astype(np.float64)
    AT = A.astype(np.float64) @ T0                                # row 4 = T0_3 + T0_4 + T0_5
    dP = delta * T0[4]                                            # what the source 4 adds to its own row, and to rows 3 and 5
    b0 = np.zeros(4)
    b0[0] = -AT[4, 0] - dP[0] / 2                                  # unit (0, 4, 0): P = -dP / 2 < 0 < P + dP when dP > 0: switches ON
    b0[1] = -AT[4, 1] - dP[1] / 2                                  # unit (0, 4, 1): dP < 0, P = -dP / 2 > 0 > P + dP: switches OFF
    b0[2] = 0.5
    b0[3] = 0.25
    return {"A": A, "A_raw": A.copy(), "X": X, "W": [W0, W1], "b": [b0.astype(np.float32), np.array([0.5, -0.25, 0.125, 1.0], np.float32)],
            "Wlin": Wlin, "blin": np.array([0.0, 0.25, -0.5], np.float32), "delta": delta, "labels": graph("path", n, None)}


def case(name):
    if name in _memo:
        return _memo[name]
    n, kind, mode, L, widths, nclass, nfeat, delta, _ = CASES[name]
    if name in EXACT:
        _memo[name] = dict(_crossing(), delta=delta)
        return _memo[name]
    rng = np.random.RandomState(sum(map(ord, name)) * 7919 % (2 ** 31))
    raw = graph(kind, n, rng)
    A = normalise(raw) if mode == "normalised" else raw
    X = (rng.rand(n, nfeat) < min(1.0, 5.0 / nfeat)).astype(np.float32)
    X[np.arange(n), rng.randint(0, nfeat, n)] = 1.0               # no empty row by chance
    X = (X / X.sum(axis=1, keepdims=True)).astype(np.float32)
    if name == "zero_row130":
        X[5] = 0.0
        X[int(raw.sum(axis=1).argmax())] = 0.0                    # the largest hub too
    dims = (nfeat,) + tuple(widths)
    W, b = [], []
    for l in range(L):
        s = 1.0 / np.sqrt(dims[l + 1])
        W.append(rng.uniform(-s, s, (dims[l], dims[l + 1])).astype(np.float32))
        b.append(rng.uniform(-s, s, dims[l + 1]).astype(np.float32))
        if name in GAPPED:
            b[-1] = (np.where(rng.rand(dims[l + 1]) < 0.7, 1.0, -1.0) * rng.uniform(1.0, 2.0, dims[l + 1])).astype(np.float32)
            if l > 0:
                W[-1] = (W[-1] * np.float32(0.5)).astype(np.float32)       # the magnitudes grow slowly from layer to layer
    s = 1.0 / np.sqrt(dims[L])
    Wlin = rng.uniform(-s, s, (nclass, dims[L])).astype(np.float32)
    blin = rng.uniform(-s, s, nclass).astype(np.float32)
    _memo[name] = {"A": A, "A_raw": raw, "X": X, "W": W, "b": b, "Wlin": Wlin, "blin": blin, "delta": delta, "labels": raw}
    return _memo[name]
