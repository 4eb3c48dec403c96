"""The truth the edge-DP tests compare against (numpy and math only, no GPU, no project code).

The pairs are the m = n (n - 1) / 2 unordered pairs of positions a > b in packed order p = a (a - 1) / 2 + b, the order of
np.tril_indices(n, -1); pair p's label is A[a, b] (the strict lower triangle of A).

Generator: Philox4x32-10 (Salmon et al., SC'11), key = (seed & 0xffffffff, seed >> 32), counter = (p, 0, replicate, 0), result
words w0 .. w3; one call per pair.

EdgeRand(eps): T = floor(2^32 / (1 + e^eps) + 1/2) in double; pair p flips iff w0 < T.  q = T / 2^32, eps_realised =
ln((1 - q) / q), inf when T = 0.

LapGraph(eps): eps1 = 0.01 eps, eps2 = 0.99 eps.  u = ((w0 >> 8) + 1/2) 2^-24, sigma = +1 iff bit 31 of w1 is clear, Lap(beta) =
sigma beta (-ln u), in float64.  v_p = float32(A_p + Lap(1 / eps2)); target = clamp(rint(E + Lap(1 / eps1)), 0, m) from the
draw at counter (m, 0, replicate, 0); the result is the `target` best pairs of np.argsort(-v, kind="stable"): v descending as
float32 values, ties by ascending p (tests/topk_truth.py's ranking).

`variant` selects one of the deliberately WRONG readings; tests/test_dp_cases_cpu.py shows that the test inputs tell each of
them from the truth:
    "le"            EdgeRand flips on w0 <= T
    "sign_w0"       the Laplace sign taken from bit 31 of w0
    "seed_counter"  the seed placed in the counter (p, 0, seed lo, seed hi) under the key (replicate, 0)
    "upper"         the label read from the upper triangle, A[b, a]
    "row_major"     p = a n + b in place of the packed position
    "eps_swapped"   eps1 and eps2 swapped
    "count_at_0"    the count's draw taken at counter 0 in place of m
    "ties_last"     ties taken last-in-packed-order first"""
import math

import numpy as np

from tests import topk_truth as TK

VARIANTS = ("le", "sign_w0", "seed_counter", "upper", "row_major", "eps_swapped", "count_at_0", "ties_last")
MECHANISMS = ("edgerand", "lapgraph")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (arrays or scalars, broadcast together) under one key: four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1, mask = int(k0), int(k1), np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return tuple(x.astype(np.uint32) for x in c)


def draws(p, seed, replicate, variant=None):
    """(w0, w1) of the pairs at packed positions p."""
    seed = int(seed)
    lo, hi = seed & 0xffffffff, seed >> 32
    if variant == "seed_counter":
        w = philox(p, 0, lo, hi, int(replicate), 0)
    else:
        w = philox(p, 0, int(replicate), 0, lo, hi)
    return w[0], w[1]


def positions(n, variant=None):
    """(a, b, p) of every pair in packed order."""
    a, b = np.tril_indices(n, -1)
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    p = a * np.uint64(n) + b if variant == "row_major" else a * (a - np.uint64(1)) // np.uint64(2) + b
    return a.astype(np.int64), b.astype(np.int64), p


def labels(A, variant=None):
    """The pairs' labels in packed order, as bool."""
    A = np.asarray(A)
    a, b = np.tril_indices(A.shape[0], -1)
    lab = A[b, a] if variant == "upper" else A[a, b]
    assert np.all((lab == 0) | (lab == 1))
    return lab == 1


def threshold(eps):
    """(T, q, eps_realised) of EdgeRand."""
    try:
        e = math.exp(eps)
    except OverflowError:
        e = math.inf
    T = int(math.floor(4294967296.0 / (1.0 + e) + 0.5))
    q = T / 4294967296.0
    return T, q, (math.log((1.0 - q) / q) if T else math.inf)


def laplace(w0, w1, beta, variant=None):
    """Lap(beta) of the draws, float64."""
    u = ((w0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    mag = beta * -np.log(u)
    neg = ((w0 if variant == "sign_w0" else w1) >> np.uint32(31)) == 1
    return np.where(neg, -mag, mag)


def from_packed(bits, n, dtype=np.float32):
    """The symmetric n x n matrix, zero diagonal, of the packed values."""
    out = np.zeros((n, n), dtype)
    a, b = np.tril_indices(n, -1)
    out[a, b] = bits
    out[b, a] = bits
    return out


def _result(n, lab, new, extra):
    m = n * (n - 1) // 2
    res = {"pairs": m, "edges": int(lab.sum()), "kept": int((lab & new).sum()), "added": int((~lab & new).sum()),
           "removed": int((lab & ~new).sum()), "bits": new, "out": from_packed(new, n)}
    res.update(extra)
    res["edges_out"] = res["kept"] + res["added"]
    res["counts"] = [m, res["edges"], res["target"], res["kept"], res["added"], res["removed"]]
    return res


def edgerand(A, eps, seed, replicate=0, variant=None):
    n = np.asarray(A).shape[0]
    lab = labels(A, variant)
    _, _, p = positions(n, variant)
    w0, _ = draws(p, seed, replicate, variant)
    T, q, er = threshold(eps)
    flip = (w0.astype(np.uint64) <= np.uint64(T)) if variant == "le" else (w0.astype(np.uint64) < np.uint64(T))
    return _result(n, lab, lab ^ flip, {"target": -1, "T": T, "flip_probability": q, "eps_realised": er, "flips": int(flip.sum()),
                                        "realised": (q, er)})


def count_draw(E, m, eps, seed, replicate=0, variant=None):
    """(noise, E + noise, target) of LapGraph's count."""
    eps1 = (0.99 if variant == "eps_swapped" else 0.01) * eps
    w0, w1 = draws(np.array([0 if variant == "count_at_0" else m], np.uint64), seed, replicate, variant)
    noise = float(laplace(w0, w1, 1.0 / eps1, variant)[0])
    noisy = E + noise
    return noise, noisy, int(min(max(np.rint(noisy), 0), m))


def lapgraph(A, eps, seed, replicate=0, variant=None):
    n = np.asarray(A).shape[0]
    m = n * (n - 1) // 2
    lab = labels(A, variant)
    _, _, p = positions(n, variant)
    w0, w1 = draws(p, seed, replicate, variant)
    eps2 = (0.01 if variant == "eps_swapped" else 0.99) * eps
    v64 = lab.astype(np.float64) + laplace(w0, w1, 1.0 / eps2, variant)
    v = v64.astype(np.float32)
    noise, noisy_count, target = count_draw(int(lab.sum()), m, eps, seed, replicate, variant)
    new = select(v, target, variant)
    return _result(n, lab, new, {"target": target, "count_noise": noise, "count_noisy": noisy_count, "v64": v64, "v": v,
                                 "noisy": from_packed(v, n), "realised": (noise, math.nan)})


def select(v, target, variant=None):
    """The packed mask of the `target` best of the float32 cells v."""
    new = np.zeros(len(v), bool)
    new[TK.ranking(np.asarray(v, np.float32), "ties_last" if variant == "ties_last" else None)[:target]] = True
    return new


def perturb(A, mechanism, eps, seed, replicate=0, variant=None):
    return {"edgerand": edgerand, "lapgraph": lapgraph}[mechanism](A, eps, seed, replicate, variant)


def ulp32(x):
    """The spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)
