"""The inputs of tests/test_gpu_node_jackknife.py, built once: name -> (real, pred_a, pred_b, idx, pad), in the layout of
tests/delong_cases.py (whose builders are used).  tests/test_node_jackknife_cases_cpu.py checks, without a GPU, that they have
the properties they are there for.  Crafted cases hold NaN everywhere outside the selected strict lower triangle, labels
included."""
import functools

import numpy as np

from tests.delong_cases import bench_shaped, bits, graph, lower, pairs_of, _scored_labels

# csrc/node_jackknife.hip, csrc/delong_common.h and csrc/rank_common.h
THREADS = 256            # AUC_THREADS: lanes of a block; a row pass takes 256 columns a step, the positives' passes 256 positives
ROW_BLOCKS = 512         # NJ_ROW_BLOCKS: blocks of the three passes over the selected rows (row a = 1 + block, + grid, ...)
COLS = 2048              # NJ_COLS: columns of one LDS chunk of the negatives' pass (columns 0 .. n_idx - 2 have a row above them)
POS_BLOCKS = 1024        # NJ_POS_BLOCKS: beyond POS_BLOCKS * THREADS positives a lane of the positives' passes takes a second
STAGE = 4096             # DL_STAGE: samples of the sorted positives in LDS; beyond STAGE positives every second one is a sample
SCAN_LANES = 1024        # k_auc_digit_scan: one block; it scans n_idx + 1 degrees and P counts
SORT_TILE = 1024         # AUC_SORT_TILE: keys per step of a sort block.  Sorted: the P positives and their 2 P list entries
SORT_BLOCKS = 1024       # AUC_SORT_BLOCKS: beyond SORT_BLOCKS * SORT_TILE keys a sort block takes a second step
MAX_NIDX = 65535         # the capacity (include/mcgra.h)

# selections on both sides of each constant of the passes over the rows and the nodes, beside the constant that puts them there
TILING = {
    257: "the longest row has THREADS columns: one step of the row passes; one block of k_nj_finish takes a second node",
    258: "the longest row has THREADS + 1 columns: a second step",
    513: "ROW_BLOCKS rows with candidates: one row per block of the row passes",
    514: "ROW_BLOCKS + 1 rows with candidates: the first block takes a second row",
    1023: "n_idx + 1 = SCAN_LANES degrees: one per lane of the scan",
    1024: "n_idx + 1 = SCAN_LANES + 1 degrees: two per lane",
    2049: "columns 0 .. COLS - 1 have a row above them: one full LDS chunk",
    2050: "column COLS has a row above it: a second chunk of one column and one row",
}

# class sizes on both sides of each constant of the sorts, the scan and the positives' passes: name -> (n, P, scores, why)
CLASS_SIZES = {
    "P256": (60, THREADS, "random", "the positives are one block of their passes"),
    "P257": (60, THREADS + 1, "random", "a second block"),
    "P512": (60, SORT_TILE // 2, "random", "2 P = SORT_TILE list entries: one full step of one sort block"),
    "P513": (60, SORT_TILE // 2 + 1, "random", "2 P = SORT_TILE + 2 list entries: a second sort block"),
    "P1024": (100, SORT_TILE, "random", "P = SORT_TILE positives: one sort block; one count per lane of the scan"),
    "P1025": (100, SORT_TILE + 1, "random", "a second sort block of the positives; two counts per lane of the scan"),
    "N1024": (100, pairs_of(100) - 1024, "random", "1024 negatives among 3926 positives: long per-node lists"),
    "P4096_ties": (150, STAGE, "levels1", "all scores equal; every positive is a sample"),
    "P4097_levels": (150, STAGE + 1, "levels3", "every second positive is a sample; three levels: ties that span many samples"),
    "P8193": (150, 2 * STAGE + 1, "random", "every third positive is a sample; the last stretch is short"),
    "P262144": (1100, POS_BLOCKS * THREADS, "random", "P = POS_BLOCKS * THREADS: one positive per lane of the positives' passes"),
    "P262145": (1100, POS_BLOCKS * THREADS + 1, "random", "one more positive: the first lane takes a second one"),
    "P524288": (1100, SORT_BLOCKS * SORT_TILE // 2, "random", "2 P = SORT_BLOCKS * SORT_TILE list entries: one step per sort block"),
    "P524289": (1100, SORT_BLOCKS * SORT_TILE // 2 + 1, "random", "two more entries: sort blocks of two steps"),
}

RELATIONS_N = 150


def star(n, hub):
    """Every positive contains `hub`."""
    real = np.zeros((n, n), np.float32)
    real[hub, :] = real[:, hub] = 1
    real[hub, hub] = 0
    return real


def path_scores(n):
    """(real, pred) of the capacity case, as numpy (small n): label 1 for the pairs (a, a - 1); a positive scores 1 when
    a % 3 == 0, else 2; a negative scores 1 when a - b is even, else 0.  Upper triangle: the same by the pair's position."""
    a, b = np.indices((n, n))
    d = a - b
    real = (d == 1).astype(np.float32)
    pred = np.where(d == 1, np.where(a % 3 == 0, 1.0, 2.0), np.where(d % 2 == 0, 1.0, 0.0)).astype(np.float32)
    return real, pred


def path_truth(n):
    """The integers of path_scores(n) in closed form, O(n): the truth at the capacity."""
    v = np.arange(n, dtype=np.int64)
    P = n - 1
    tied = (v[1:] % 3 == 0)                                    # positive (a, a - 1), a = 1 .. n - 1, scores 1
    K1 = int(tied.sum()); K2 = P - K1
    d = np.arange(2, n, dtype=np.int64)                        # a - b of the negatives; n - d pairs each
    N1 = int((n - d)[d % 2 == 0].sum()); N0 = int((n - d)[d % 2 == 1].sum())
    N = N0 + N1
    a_tied, a_top = 2 * N0 + N1, 2 * N
    b_tied, b_low = 2 * K2 + K1, 2 * P
    evens, odds = (n + 1) // 2, n // 2
    Pv = (v >= 1).astype(np.int64) + (v <= n - 2)
    e = np.where(v % 2 == 0, evens, odds) - 1                  # the others of v's parity: negatives that score 1
    o = np.where(v % 2 == 0, odds, evens) - Pv                 # the other parity without v's neighbours: negatives that score 0
    up_tied = np.zeros(n, bool); up_tied[1:] = tied            # v's positive (v, v - 1)
    dn_tied = np.zeros(n, bool); dn_tied[:-1] = tied           # v's positive (v + 1, v)
    has_up, has_dn = v >= 1, v <= n - 2
    A = has_up * np.where(up_tied, a_tied, a_top) + has_dn * np.where(dn_tied, a_tied, a_top)
    C = has_up * np.where(up_tied, 2 * o + e, 2 * (e + o)) + has_dn * np.where(dn_tied, 2 * o + e, 2 * (e + o))
    out = {"pairs": n * (n - 1) // 2, "positives": P, "negatives": N, "T": K1 * a_tied + K2 * a_top}
    out.update({"P_v": Pv.tolist(), "N_v": (e + o).tolist(), "A_v": A.tolist(), "B_v": (e * b_tied + o * b_low).tolist(),
                "C_v": C.tolist()})
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(91)
    out = {}
    out["n2_one_positive"] = (lower([1], 2), lower([0.5], 2), lower([0.25], 2), None, 0)
    out["n2_one_negative"] = (lower([0], 2), lower([0.5], 2), lower([0.25], 2), None, 0)
    out["n3"] = (lower([1, 0, 1], 3), lower([0.5, 0.5, 0.25], 3), lower([0.75, 0.5, 0.5], 3), None, 0)
    out["n3_one_positive"] = (lower([0, 1, 0], 3), lower([0.1, 0.5, 0.7], 3), lower([0.3, 0.2, 0.1], 3), None, 0)
    out["n4"] = (lower([1, 0, 0, 1, 1, 0], 4), lower(rng.rand(6), 4), lower(rng.rand(6), 4), None, 0)
    out["n4_ties"] = (lower([1, 0, 0, 1, 1, 0], 4), lower([0.5, 0.5, 0.25, 0.25, 0.5, 0.75], 4), lower([1, 1, 1, 1, 1, 1], 4), None, 0)
    out["n64_all_equal"] = (graph(rng, 64, 0.2), np.full((64, 64), 0.375, np.float32), np.full((64, 64), -2.0, np.float32), None, 0)
    out["n64_no_positive"] = (np.zeros((64, 64), np.float32), rng.rand(64, 64).astype(np.float32), rng.rand(64, 64).astype(np.float32), None, 0)
    out["n64_no_negative"] = (np.ones((64, 64), np.float32), rng.rand(64, 64).astype(np.float32), rng.rand(64, 64).astype(np.float32), None, 0)
    n = 200
    out["five_levels"] = (graph(rng, n, 0.1), lower(rng.randint(0, 5, pairs_of(n)) * 0.25, n),
                          lower(rng.randint(0, 5, pairs_of(n)) * 0.125, n), None, 0)
    # -0.0 beside +0.0, subnormals of both signs, the smallest normal, negative scores
    odd = bits(0x80000000, 0, 1, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0xbfc00000, 0x40000000, 0xbe800000)
    n = 16
    out["zeros_subnormals_negatives"] = (lower(rng.randint(0, 2, pairs_of(n)), n), lower(odd[rng.randint(0, len(odd), pairs_of(n))], n),
                                         lower(odd[rng.randint(0, len(odd), pairs_of(n))], n), None, 0)
    out["signed_zeros_only"] = (lower(rng.randint(0, 2, pairs_of(n)), n), lower(odd[rng.randint(0, 2, pairs_of(n))], n),
                                lower(odd[rng.randint(0, 3, pairs_of(n))], n), None, 0)
    # layout
    out["n257_ld288"] = (graph(rng, 257, 0.05), rng.rand(257, 257).astype(np.float32) ** 6,
                         rng.randn(257, 257).astype(np.float32), None, 31)
    n = 120
    mats = [(rng.rand(n, n) < 0.1).astype(np.float32), rng.rand(n, n).astype(np.float32) ** 4, rng.randn(n, n).astype(np.float32)]
    sel = np.sort(rng.permutation(n)[:90])
    off = np.ones(n, bool); off[sel] = False
    for mtx in mats:                                     # asymmetric; nothing outside the selected lower triangle is valid
        junk = np.array([np.nan, np.inf, 0.5], np.float32)[rng.randint(0, 3, (n, n))]
        up = np.triu(np.ones((n, n), bool))
        mtx[up] = junk[up]
        mtx[off] = junk[off]
        mtx[:, off] = junk[:, off]
    out["junk_outside_selection"] = (mats[0], mats[1], mats[2], sel, 0)
    n = 90
    out["asymmetric"] = (graph(rng, n, 0.1), rng.rand(n, n).astype(np.float32), rng.rand(n, n).astype(np.float32), None, 0)
    out["asymmetric_labels"] = ((rng.rand(n, n) < 0.15).astype(np.float32), (rng.randint(0, 8, (n, n)) / 8).astype(np.float32),
                                rng.rand(n, n).astype(np.float32), None, 0)
    real = graph(rng, 300, 0.05)
    pa, pb = (np.tril(p, -1) + np.tril(p, -1).T for p in (rng.rand(300, 300).astype(np.float32) ** 5, rng.randn(300, 300).astype(np.float32)))
    sub = rng.permutation(300)[:100].copy()              # symmetric matrices: a reordered idx names the same pair set
    out["subset_permuted"] = (real, pa, pb, sub, 0)
    out["subset_reordered"] = (real, pa, pb, sub[rng.permutation(100)].copy(), 0)
    # a descending idx: the position is not the node id, and the lower triangle of the selection is the matrix's upper one
    n = 40
    out["idx_descending"] = (graph(rng, n, 0.2), rng.rand(n, n).astype(np.float32), rng.rand(n, n).astype(np.float32),
                             np.arange(n - 1, -1, -2).copy(), 0)
    # node kinds: a hub that holds every positive (its deletion leaves no AUC), an isolated node, a node of degree > THREADS
    n = 50
    out["star"] = (star(n, 17), rng.rand(n, n).astype(np.float32), (rng.randint(0, 3, (n, n)) / 2).astype(np.float32), None, 0)
    real = graph(rng, n, 0.2)
    real[23, :] = real[:, 23] = 0
    out["isolated_node"] = (real, rng.rand(n, n).astype(np.float32), rng.rand(n, n).astype(np.float32), None, 0)
    n = 400
    real = graph(rng, n, 0.01)
    real[5, :300] = real[:300, 5] = 1
    real[5, 5] = 0
    out["hub_degree_299"] = (real, (rng.randint(0, 50, (n, n)) / 50).astype(np.float32), rng.rand(n, n).astype(np.float32), None, 0)
    # paired relations, on scores that are multiples of 2^-12 in [0, 1): -A is exact
    n = RELATIONS_N
    real = graph(rng, n, 0.08)
    a = lower(rng.randint(0, 4096, pairs_of(n)) / 4096.0, n)
    out["b_equals_a"] = (real, a, a.copy(), None, 0)
    out["b_minus_a"] = (real, a, (-a).astype(np.float32), None, 0)
    lab = np.tril(real, -1)[np.tril_indices(n, -1)]
    out["two_independent_scorings"] = (real, lower(_scored_labels(rng, lab, 1.5), n), lower(_scored_labels(rng, lab, 1.0), n), None, 0)
    # the closed form of the capacity case, small
    out["path_n50"] = path_scores(50) + (path_scores(50)[1].copy(), None, 0)
    # tiling: the leading rows x rows block of one bench-shaped matrix
    pa, pb, real = bench_shaped(rng, max(TILING), 0.004)
    for rows in sorted(TILING):
        out[f"tiling_n{rows}"] = (real[:rows, :rows], pa[:rows, :rows], pb[:rows, :rows], None, 0)
    for name, (n, P, kind, _) in CLASS_SIZES.items():
        m = pairs_of(n)
        lab = np.zeros(m, np.float32)
        lab[rng.permutation(m)[:P]] = 1
        if kind == "random":
            sa, sb = _scored_labels(rng, lab, 1.0), _scored_labels(rng, lab, 0.5)
        else:
            k = int(kind[len("levels"):])
            sa, sb = rng.randint(0, k, m) * 0.5, rng.randint(0, 3, m) * 0.25
        out[f"class_{name}"] = (lower(lab, n), lower(sa, n), lower(sb, n), None, 0)
    for v in out.values():
        for mtx in v[:3]:
            mtx.setflags(write=False)
    return out
