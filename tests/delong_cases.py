"""The inputs of tests/test_gpu_delong.py, built once: name -> (real, pred_a, pred_b, idx, pad).  tests/test_delong_cases_cpu.py
checks, without a GPU, that they have the properties they are there for.  pad > 0 puts the three matrices' rows into buffers
that many columns wider.  Crafted cases hold NaN everywhere outside the selected strict lower triangle, labels included."""
import functools

import numpy as np

# csrc/delong.hip and csrc/rank_common.h
THREADS = 256            # AUC_THREADS: lanes of a block; a row pass takes 256 columns a step, the positives' pass 256 slots
ROW_BLOCKS = 1024        # DL_ROW_BLOCKS: blocks of the three passes over the selected rows (row a = 1 + block, + grid, ...)
POS_BLOCKS = 2048        # DL_POS_BLOCKS: blocks of the positives' pass; beyond POS_BLOCKS * THREADS positives a lane takes a second
STAGE = 4096             # DL_STAGE: samples of the sorted positives in LDS; beyond STAGE positives every second one is a sample
SCAN_LANES = 1024        # k_auc_digit_scan: one block; beyond SCAN_LANES positives a lane scans two counts
SORT_TILE = 1024         # AUC_SORT_TILE: keys per step of a sort block; up to SORT_TILE positives are one block, one step
SORT_BLOCKS = 1024       # AUC_SORT_BLOCKS: beyond SORT_BLOCKS * SORT_TILE positives a sort block takes a second step


def pairs_of(rows):
    return rows * (rows - 1) // 2


# selections on both sides of each constant of the passes over the rows, beside the constant that puts them there
TILING = {
    257: "the longest row has THREADS columns: one step of the row passes",
    258: "the longest row has THREADS + 1 columns: a second step",
    1025: "ROW_BLOCKS rows with candidates: one row per block of the row passes",
    1026: "ROW_BLOCKS + 1 rows with candidates: the first block takes a second row",
    1448: "m = 1 047 628 < 2^20 pairs",
    1449: "m = 1 049 076 > 2^20 pairs (only the positives are sorted: class_P1048576 / 7 put them across the sort's constant)",
}

# class sizes on both sides of each constant of the sort, the scan and the positives' pass: name -> (n, P, scores, why)
CLASS_SIZES = {
    "P1023": (100, SCAN_LANES - 1, "random", "the scan's last lane has no count"),
    "P1024": (100, SORT_TILE, "random", "one full step of one sort block; one count per lane of the scan"),
    "P1025": (100, SORT_TILE + 1, "random", "a second sort block; two counts per lane of the scan"),
    "N1024": (100, pairs_of(100) - SORT_TILE, "random", "1024 negatives among 3926 positives"),
    "N1025": (100, pairs_of(100) - SORT_TILE - 1, "random", "1025 negatives"),
    "P256": (60, THREADS, "random", "the positives are one block of their pass"),
    "P257": (60, THREADS + 1, "random", "a second block"),
    "P4096_ties": (150, STAGE, "levels1", "all scores equal; every positive is a sample"),
    "P4097_ties": (150, STAGE + 1, "levels1", "P = STAGE + 1: every second positive is a sample, the rest is searched in place"),
    "P4097_levels": (150, STAGE + 1, "levels3", "three levels: ties that span many samples"),
    "P8193": (150, 2 * STAGE + 1, "random", "every third positive is a sample; the last stretch is short"),
    "P524288": (1100, POS_BLOCKS * THREADS, "random", "P = POS_BLOCKS * THREADS: one slot per lane of the positives' pass"),
    "P524289": (1100, POS_BLOCKS * THREADS + 1, "random", "one more positive: the first lane takes a second slot"),
    "P1048576": (1500, SORT_BLOCKS * SORT_TILE, "random", "P = SORT_BLOCKS * SORT_TILE: every sort block takes one step"),
    "P1048577": (1500, SORT_BLOCKS * SORT_TILE + 1, "random", "one more positive: sort blocks of two steps"),
}

CARRY_N = 3000


def graph(rng, n, p):
    a = np.triu(rng.rand(n, n) < p, 1)
    return (a | a.T).astype(np.float32)


def lower(values, n, junk=np.nan):
    """An n x n matrix whose strict lower triangle holds `values` in packed order (cycled) and `junk` everywhere else."""
    m = np.full((n, n), junk, np.float32)
    a, b = np.tril_indices(n, -1)
    m[a, b] = np.resize(np.asarray(values, np.float32), len(a))
    return m


def bits(*words):
    return np.array(words, np.uint32).view(np.float32)


def bench_shaped(rng, n, p_high=0.002):
    """(pred_a, pred_b, real): a modified_adj as the attack leaves it -- p_high of the pairs near 0.8, the rest small -- a
    second, weaker scoring of the same graph, and the graph."""
    hi = np.tril(rng.rand(n, n) < p_high, -1)
    real = ((hi | hi.T) ^ _flip(rng, n)).astype(np.float32)

    def scoring(noise):
        s = np.abs(rng.randn(n, n)).astype(np.float32) * np.float32(noise)
        s[hi] = (0.8 + 0.05 * rng.randn(int(hi.sum()))).astype(np.float32)
        s = np.tril(s, -1)
        return (s + s.T).astype(np.float32)

    return scoring(0.01), scoring(0.3), real


def _flip(rng, n, p=0.001):
    f = np.tril(rng.rand(n, n) < p, -1)
    return f | f.T


def _scored_labels(rng, lab, sep):
    """A float32 score per label: N(sep, 1) for a 1, N(0, 1) for a 0 (AUC = Phi(sep / sqrt 2))."""
    return (rng.randn(len(lab)) + sep * lab).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(88)
    out = {}
    out["n2_one_positive"] = (lower([1], 2), lower([0.5], 2), lower([0.25], 2), None, 0)
    out["n2_one_negative"] = (lower([0], 2), lower([0.5], 2), lower([0.25], 2), None, 0)
    out["n3"] = (lower([1, 0, 1], 3), lower([0.5, 0.5, 0.25], 3), lower([0.75, 0.5, 0.5], 3), None, 0)
    out["n3_one_positive"] = (lower([0, 1, 0], 3), lower([0.1, 0.5, 0.7], 3), lower([0.3, 0.2, 0.1], 3), None, 0)
    out["n4"] = (lower([1, 0, 0, 1, 1, 0], 4), lower(rng.rand(6), 4), lower(rng.rand(6), 4), None, 0)
    out["n64_all_equal"] = (graph(rng, 64, 0.2), np.full((64, 64), 0.375, np.float32), np.full((64, 64), -2.0, np.float32), None, 0)
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
    real = graph(rng, 300, 0.05)
    pa, pb = (np.tril(p, -1) + np.tril(p, -1).T for p in (rng.rand(300, 300).astype(np.float32) ** 5, rng.randn(300, 300).astype(np.float32)))
    sub = rng.permutation(300)[:100].copy()              # symmetric matrices: a reordered idx names the same pair set
    out["subset_permuted"] = (real, pa, pb, sub, 0)
    out["subset_reordered"] = (real, pa, pb, sub[rng.permutation(100)].copy(), 0)
    # paired relations, on scores that are multiples of 2^-12 in [0, 1): 2 A + 1 and -A are exact
    n = 150
    real = graph(rng, n, 0.08)
    a = lower(rng.randint(0, 4096, pairs_of(n)) / 4096.0, n)
    out["b_equals_a"] = (real, a, a.copy(), None, 0)
    out["b_increasing_map_of_a"] = (real, a, (2 * a + 1).astype(np.float32), None, 0)
    out["b_minus_a"] = (real, a, (-a).astype(np.float32), None, 0)
    lab = np.tril(real, -1)[np.tril_indices(n, -1)]
    out["two_independent_scorings"] = (real, lower(_scored_labels(rng, lab, 1.5), n), lower(_scored_labels(rng, lab, 1.0), n), None, 0)
    # tiling: the leading rows x rows block of one bench-shaped matrix
    pa, pb, real = bench_shaped(rng, max(TILING))
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
    # every sum of squares and of products carries into the high limb: half the pairs positive, AUC about 0.9 and 0.8
    n = CARRY_N
    lab = (rng.rand(pairs_of(n)) < 0.5).astype(np.float32)
    out["carry_n3000"] = (lower(lab, n), lower(_scored_labels(rng, lab, 1.8), n), lower(_scored_labels(rng, lab, 1.2), n), None, 0)
    for v in out.values():
        for mtx in v[:3]:
            mtx.setflags(write=False)
    return out
