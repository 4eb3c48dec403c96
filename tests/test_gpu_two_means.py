"""The recovered graph without the truth on the device (mcgra_two_means_split, mcgra_threshold_pairs, engine.two_means_split /
threshold_pairs, main.py --binarize / --save_graph) against tests/two_means_truth.py: every reported integer and every
threshold bit compared for equality, over the smallest selections, crafted multiples of 2^-10 (a value exactly between the
two centres, a split that needs several rounds, the same split capped), the edges of the quantisation, layouts (padding,
junk outside the selected lower triangle, permuted subsets) and selections on both sides of every constant the kernels' grids
and steps use.  Run with -m gpu.

tests/test_two_means_cases_cpu.py checks, without a GPU, that these inputs have the properties the cases are there for and that
they tell five wrong readings of the definition from the right one."""
import functools
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import two_means_truth as T

pytestmark = pytest.mark.gpu

# csrc/two_means.hip and csrc/rank_common.h
THREADS = 256            # AUC_THREADS: lanes of a block; a row pass takes 256 columns a step
ROW_BLOCKS = 1024        # TM_ROW_BLOCKS: blocks of the passes over the selected rows (row a = 1 + block, + grid, ...)
STEP = 1024              # TM_STEP: q per step of a block of the streaming pass
BLOCKS = 1024            # TM_BLOCKS: blocks of the streaming pass; beyond BLOCKS * STEP pairs a block takes a second step
BATCH = 4                # TM_BATCH: rounds between two reads of the state
TP_BLOCKS = 1024         # contiguous packed ranges of mcgra_threshold_pairs; beyond TP_BLOCKS * THREADS pairs a range takes 512


def pairs_of(rows):
    return rows * (rows - 1) // 2


# selections on both sides of each constant, beside the constant that puts them there
TILING = {
    45: "m = 990 < STEP: the streaming pass is one partial step of one block",
    46: "m = 1035 > STEP: a second block",
    257: "the longest row has THREADS columns: one step of the row pass",
    258: "the longest row has THREADS + 1 columns: a second step",
    724: "m = 261 726 <= TP_BLOCKS * THREADS: ranges of 256 pairs",
    725: "m = 262 450 > TP_BLOCKS * THREADS: ranges of 512 pairs",
    1025: "ROW_BLOCKS rows with candidates: one row per block of the row pass",
    1026: "ROW_BLOCKS + 1 rows with candidates: more rows than the row pass has blocks",
    1448: "m = 1 047 628 < BLOCKS * STEP: every streaming block takes one step",
    1449: "m = 1 049 076 > BLOCKS * STEP: the first blocks take a second step",
}


def _graph(rng, n, p):
    a = np.triu(rng.rand(n, n) < p, 1)
    return (a | a.T).astype(np.float32)


def _lower(values, n, junk=np.nan):
    """An n x n matrix whose strict lower triangle holds `values` in packed order (cycled) and `junk` everywhere else."""
    m = np.full((n, n), junk, np.float32)
    a, b = np.tril_indices(n, -1)
    m[a, b] = np.resize(np.asarray(values, np.float32), len(a))
    return m


def _bits(*words):
    return np.array(words, np.uint32).view(np.float32)


TIE_VALUES = [2, 12, 13, 19, 33, 35]                 # x 2^-10: round 0 gives c0 = 9, c1 = 29, and 19 sits on (9 + 29) / 2
ROUNDS_VALUES = [0, 0, 0, 0, 0, 0, 0, 1, 1, 3, 5, 9, 13, 17, 32, 36, 99, 101, 146, 159, 174, 181, 211, 219, 233, 261, 437, 438]


def bench_shaped(rng, n, p_high=0.001):
    """A modified_adj as the attack leaves it: p_high of the pairs near 0.8, the rest small; symmetric, zero diagonal."""
    s = np.abs(rng.randn(n, n)).astype(np.float32) * np.float32(0.01)
    hi = rng.rand(n, n) < p_high
    s[hi] = (0.8 + 0.05 * rng.randn(int(hi.sum()))).astype(np.float32)
    s = np.tril(s, -1)
    return (s + s.T).astype(np.float32), ((np.tril(hi, -1) | np.tril(hi, -1).T) ^ _flip(rng, n)).astype(np.float32)


def _flip(rng, n, p=0.0005):
    f = np.tril(rng.rand(n, n) < p, -1)
    return f | f.T


def _cases():
    """name -> (real, pred, idx, pad, max_iter): pad > 0 puts pred's rows into a buffer that many columns wider."""
    rng = np.random.RandomState(41)
    out = {}
    out["n2_one_pair"] = (np.array([[0, 1], [1, 0]], np.float32), rng.rand(2, 2).astype(np.float32), None, 0, 256)
    out["n3_two_values"] = (_graph(rng, 3, 0.6), _lower([0.25, 0.75, 0.25], 3, 0.0), None, 0, 256)
    out["n64_all_equal"] = (_graph(rng, 64, 0.2), np.full((64, 64), 0.375, np.float32), None, 0, 256)
    tie = np.array(TIE_VALUES, np.float32) * np.float32(2.0 ** -10)
    out["tie_on_the_midpoint"] = (_graph(rng, 4, 0.5), _lower(tie, 4), None, 0, 256)
    rounds = np.array(ROUNDS_VALUES, np.float32) * np.float32(2.0 ** -10)
    out["several_rounds"] = (_graph(rng, 8, 0.3), _lower(rounds, 8), None, 0, 256)
    out["several_rounds_cap2"] = (out["several_rounds"][0], out["several_rounds"][1], None, 0, 2)
    # quantisation: 2^-29, 3 2^-29, 5 2^-29 and 7 2^-29 are half-way (to 0, 2, 2, 4); subnormals and -0.0 are 0
    small = np.concatenate([_bits(0x80000000, 0, 1, 0x007fffff, 0x00800000),
                            np.array([2.0 ** -29, 3 * 2.0 ** -29, 5 * 2.0 ** -29, 7 * 2.0 ** -29, 2.0 ** -28], np.float32)])
    out["quant_halfway_small"] = (_graph(rng, 5, 0.5), _lower(small, 5), None, 0, 256)
    top = np.concatenate([small, _bits(0x417fffff, 0x417fffff), np.array([15.5, 1.0, 0.5 + 2.0 ** -24, 3 * 2.0 ** -29], np.float32)])
    out["quant_largest_below_16"] = (_graph(rng, 7, 0.4), _lower(top, 7), None, 0, 256)
    odd = (rng.randint(0, 2 ** 20, pairs_of(40)) * 2 + 1).astype(np.float64) * 2.0 ** -29     # every value half-way
    out["quant_halfway_many"] = (_graph(rng, 40, 0.2), _lower(odd, 40), None, 0, 256)
    # layout
    real, pred = _graph(rng, 257, 0.05), rng.rand(257, 257).astype(np.float32) ** 6
    out["n257_ld288"] = (real, pred, None, 31, 256)
    n = 120
    pred = rng.rand(n, n).astype(np.float32) ** 4
    real = (rng.rand(n, n) < 0.1).astype(np.float32)
    sel = np.sort(rng.permutation(n)[:90])
    off = np.ones(n, bool); off[sel] = False
    for mtx in (pred, real):                                             # asymmetric; nothing outside the selection is valid
        junk = np.array([np.nan, -1.0, 99.0], np.float32)[rng.randint(0, 3, (n, n))]
        up = np.triu(np.ones((n, n), bool))
        mtx[up] = junk[up]
        mtx[off] = junk[off]
        mtx[:, off] = junk[:, off]
    out["junk_outside_selection"] = (real, pred, sel, 0, 256)
    real, pred = _graph(rng, 300, 0.05), rng.rand(300, 300).astype(np.float32) ** 5
    pred = np.tril(pred, -1) + np.tril(pred, -1).T                       # symmetric: a reordered idx names the same pair set
    sub = rng.permutation(300)[:100].copy()
    out["subset_permuted"] = (real, pred, sub, 0, 256)
    out["subset_reordered"] = (real, pred, sub[rng.permutation(100)].copy(), 0, 256)
    # tiling: the leading n x n block of one bench-shaped matrix
    pred, real = bench_shaped(rng, 2048)
    for rows in sorted(TILING):
        out[f"tiling_n{rows}"] = (real[:rows, :rows], pred[:rows, :rows], None, 0, 256)
    out["bench_shaped_n2048"] = (real, pred, None, 0, 256)
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def truth(name):
    """The truth of a case, computed once and shared (read-only)."""
    real, pred, idx, _, max_iter = CASES[name]
    return T.split(real, pred, idx, max_iter)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x, pad=0):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    if pad:
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda:0")      # the padding is never read
        buf[:, :t.shape[1]] = t
        t = buf[:, :t.shape[1]]
    return t


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_split(got, want, what):
    print(f"{what}: got { {k: got[k] for k in T.INTS} } threshold={got['threshold']} low={got['threshold_low']}")
    for key in T.INTS + ("positives", "hits"):
        assert int(got[key]) == int(want[key]), (what, key, got[key], want[key])
    for key in ("threshold", "threshold_low"):
        if want["degenerate"]:
            assert got[key] is None and want[key] is None, (what, key)
        else:
            assert isinstance(got[key], float) and K_bits(got[key]) == K_bits(want[key]), (what, key, got[key], want[key])
    for key in ("center_low", "center_high", "precision", "recall", "f1"):
        assert _same_float(got[key], want[key]), (what, key, got[key], want[key])


def K_bits(x):
    return int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])


def _check_pairs(got, want, what):
    import torch
    pairs, scores, hits = got
    assert pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2 and scores.dtype == torch.float32
    assert pairs.is_cuda and scores.is_cuda and (hits is None) == (want[2] is None)
    assert np.array_equal(pairs.cpu().numpy(), want[0]), what
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), what
    if hits is not None:
        assert hits.dtype == torch.bool and np.array_equal(hits.cpu().numpy(), want[2]), what


# ------------------------------------------------------------------------------------------------ 1. the split
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_means_against_the_truth(pkg, name):
    """Every integer, both threshold bits, and the high cluster as mcgra_threshold_pairs returns it on the threshold."""
    from mc_gra_amd import engine as E
    real, pred, idx, pad, max_iter = CASES[name]
    r, p, ix = _dev(real), _dev(pred, pad), None if idx is None else _dev(idx)
    if pad:
        assert p.stride(0) == pred.shape[1] + pad
    want = truth(name)
    got = E.two_means_split(p, ix, r, max_iter)
    _check_split(got, want, name)
    bare = E.two_means_split(p, ix, None, max_iter)                     # without labels: the same split, nothing about edges
    assert "hits" not in bare and {k: bare[k] for k in T.INTS} == {k: got[k] for k in T.INTS}
    assert bare["threshold"] == got["threshold"] and bare["threshold_low"] == got["threshold_low"]
    if want["degenerate"]:
        assert got["edges"] == 0 and got["iterations"] == 0 and got["converged"] is True
        return
    edges = E.threshold_pairs(p, got["threshold"], ix, r)
    _check_pairs(edges, T.threshold_pairs(real, pred, want["threshold"], idx), name)
    assert edges[0].shape[0] == got["edges"] and int(edges[2].sum()) == got["hits"]
    assert int(want["high"].sum()) == got["edges"]


def test_capped_split_reports_the_partition_it_counted(pkg):
    from mc_gra_amd import engine as E
    full, capped = truth("several_rounds"), truth("several_rounds_cap2")
    assert full["iterations"] >= 4 and full["converged"] == 1 and capped["iterations"] == 2 and capped["converged"] == 0
    real, pred, _, _, _ = CASES["several_rounds"]
    r, p = _dev(real), _dev(pred)
    for cap in range(1, full["iterations"] + BATCH + 2):                # also every cap inside and past a batch of rounds
        got = E.two_means_split(p, None, r, cap)
        _check_split(got, T.split(real, pred, None, cap), ("cap", cap))
        assert got["converged"] == (cap >= full["iterations"]) and got["iterations"] == min(cap, full["iterations"])


def test_reordered_selection_gives_the_same_split(pkg):
    """The same node set in another order: another packing, the same multiset of scores, so the same integers."""
    from mc_gra_amd import engine as E
    real, pred, a, _, _ = CASES["subset_permuted"]
    b = CASES["subset_reordered"][2]
    assert sorted(a.tolist()) == sorted(b.tolist()) and not np.array_equal(a, b)
    r, p = _dev(real), _dev(pred)
    ga, gb = E.two_means_split(p, a, r), E.two_means_split(p, b, r)
    for key in T.INTS + ("positives", "hits", "threshold", "threshold_low"):
        assert ga[key] == gb[key], key
    ea, eb = E.threshold_pairs(p, ga["threshold"], a)[0].cpu().numpy(), E.threshold_pairs(p, gb["threshold"], b)[0].cpu().numpy()
    assert {frozenset(e) for e in ea.tolist()} == {frozenset(e) for e in eb.tolist()} and len(ea) == ga["edges"] > 0


@pytest.mark.parametrize("name", ["bench_shaped_n2048", "subset_permuted"])
def test_two_calls_give_identical_bits(pkg, name):
    import torch
    from mc_gra_amd import engine as E
    real, pred, idx, pad, max_iter = CASES[name]
    r, p, ix = _dev(real), _dev(pred, pad), None if idx is None else _dev(idx)
    a, b = E.two_means_split(p, ix, r, max_iter), E.two_means_split(p, ix, r, max_iter)
    assert {k: (v.hex() if isinstance(v, float) else v) for k, v in a.items()} == \
           {k: (v.hex() if isinstance(v, float) else v) for k, v in b.items()}
    x, y = E.threshold_pairs(p, a["threshold"], ix, r), E.threshold_pairs(p, a["threshold"], ix, r)
    for s, t in zip(x, y):
        assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)


# --------------------------------------------------------------------------------------------- 2. threshold pairs
@pytest.mark.parametrize("name", ["n257_ld288", "junk_outside_selection", "subset_permuted", "tiling_n724", "tiling_n725"])
def test_threshold_pairs_against_the_truth(pkg, name):
    """Pairs, scores and hits element for element in ascending packed position, at thresholds of every kind."""
    from mc_gra_amd import engine as E
    real, pred, idx, pad, _ = CASES[name]
    r, p, ix = _dev(real), _dev(pred, pad), None if idx is None else _dev(idx)
    s = T.K.packed(real, pred, idx)[0]
    for thr in (0.9, float(np.median(s)), float(s.max()), float(np.nextafter(s.max(), np.float32(np.inf))), float("inf"),
                float(s.min()), -1.0, float("-inf")):
        want = T.threshold_pairs(real, pred, thr, idx)
        _check_pairs(E.threshold_pairs(p, thr, ix, r), want, (name, thr))
        _check_pairs(E.threshold_pairs(p, thr, ix), (want[0], want[1], None), (name, thr, "bare"))
    assert len(T.threshold_pairs(real, pred, np.nextafter(s.max(), np.float32(np.inf)), idx)[0]) == 0      # above every score
    assert len(T.threshold_pairs(real, pred, s.min(), idx)[0]) == len(s)


def test_threshold_pairs_of_1100_selected_nodes(pkg):
    """n_idx = 1100 of n = 1200 nodes in a shuffled order: m = 604 450 pairs, ranges of 768 pairs (three 256-lane steps a block),
    positions a beyond 1024.  64 score levels, about 1 % edges, the scores in a wider buffer; a level as the threshold."""
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(1100)
    real = _graph(rng, 1200, 0.01)
    pred = (rng.randint(0, 64, (1200, 1200)) / 64.0).astype(np.float32)
    idx = rng.permutation(1200)[:1100].copy()
    r, p, ix = _dev(real), _dev(pred, 7), _dev(idx)
    for thr in (0.875, 0.5):
        want = T.threshold_pairs(real, pred, thr, idx)
        assert 0 < len(want[0]) < 604450
        _check_pairs(E.threshold_pairs(p, thr, ix, r), want, ("n_idx 1100", thr))


def test_threshold_pairs_negative_scores_and_signed_zeros(pkg):
    """Any finite score is a candidate, and -0.0 >= +0.0 holds: a threshold of +0.0 takes the -0.0 scores."""
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    vals = np.concatenate([_bits(0x80000000, 0, 1, 0x80000001), np.array([-2.5, -1e-30, 3e-39, 0.5, 7.0], np.float32)])
    pred = _lower(vals[rng.randint(0, len(vals), pairs_of(70))], 70)
    real = _graph(rng, 70, 0.2)
    s = T.K.packed(real, pred)[0]
    assert (s.view(np.uint32) == 0x80000000).sum() > 100 and (s < 0).sum() > 100
    r, p = _dev(real), _dev(pred)
    for thr in _bits(0, 0x80000000, 1, 0x80000001).tolist() + [-2.5, 0.5]:
        want = T.threshold_pairs(real, pred, thr)
        _check_pairs(E.threshold_pairs(p, thr, None, r), want, thr)
    zero = E.threshold_pairs(p, 0.0)[1].cpu().numpy().view(np.uint32)
    assert (zero == 0x80000000).sum() == (s.view(np.uint32) == 0x80000000).sum()


def test_threshold_pairs_capacity(pkg):
    """The C entry itself: counts alone with cap = 0, cap one too small (MCGRA_ENOMEM, untouched buffers, the needed count), the
    exact cap."""
    import ctypes as C
    import torch
    from mc_gra_amd.engine import _p, _stream
    real, pred, _, _, _ = CASES["tiling_n258"]
    r, p = _dev(real), _dev(pred)
    thr = truth("tiling_n258")["threshold"]
    want = T.threshold_pairs(real, pred, thr)
    k = len(want[0])
    assert k == truth("tiling_n258")["edges"] > 3
    L = pkg._lib.lib

    def call(cap, pairs, scores, hits, counts):
        return L.mcgra_threshold_pairs(_stream(), 258, _p(p), p.stride(0), _p(r), r.stride(0), None, 258, float(thr), cap,
                                       _p(pairs), _p(scores), _p(hits), counts)

    counts = (C.c_int64 * 3)(-7, -7, -7)
    assert call(0, None, None, None, counts) == 0 and list(counts) == [pairs_of(258), k, int(want[2].sum())]
    pairs = torch.full((k, 2), -5, device="cuda:0", dtype=torch.int64)
    scores = torch.full((k,), -5.0, device="cuda:0")
    hits = torch.full((k,), 9, device="cuda:0", dtype=torch.uint8)
    counts = (C.c_int64 * 3)(-7, -7, -7)
    assert call(k - 1, pairs, scores, hits, counts) == -4
    msg = L.mcgra_last_error()
    assert b"threshold_pairs" in msg and str(k).encode() in msg and str(k - 1).encode() in msg
    assert list(counts) == [pairs_of(258), k, int(want[2].sum())]
    assert bool((pairs == -5).all()) and bool((scores == -5.0).all()) and bool((hits == 9).all())
    assert call(k, pairs, scores, hits, counts) == 0
    _check_pairs((pairs, scores, hits.view(torch.bool)), want, "exact cap")


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_on_the_device_leave_the_outputs_untouched(pkg):
    import ctypes as C
    import torch
    from mc_gra_amd.engine import _p, _stream
    rng = np.random.RandomState(9)
    n = 80
    real, pred = _graph(rng, n, 0.2), rng.rand(n, n).astype(np.float32)
    L = pkg._lib.lib
    ids = torch.arange(n, device="cuda:0")

    def split(rr, pp, ix=None, n_idx=n):
        out, hi, lo = (C.c_int64 * 10)(*([-7] * 10)), C.c_float(-7.0), C.c_float(-7.0)
        rc = L.mcgra_two_means_split(_stream(), n, _p(pp), pp.stride(0), _p(rr), n, _p(ix), n_idx, 256, out, C.byref(hi), C.byref(lo))
        assert rc == 0 or (list(out) == [-7] * 10 and hi.value == -7.0 and lo.value == -7.0), (rc, list(out))
        return rc

    def pairs(rr, pp, ix=None, n_idx=n):
        counts = (C.c_int64 * 3)(-7, -7, -7)
        buf = torch.full((pairs_of(n), 2), -5, device="cuda:0", dtype=torch.int64)
        rc = L.mcgra_threshold_pairs(_stream(), n, _p(pp), pp.stride(0), _p(rr), n, _p(ix), n_idx, 0.5, pairs_of(n), _p(buf), None,
                                     None, counts)
        assert rc == 0 or (list(counts) == [-7] * 3 and bool((buf == -5).all())), (rc, list(counts))
        return rc

    r, p = _dev(real), _dev(pred)
    assert split(r, p) == 0 and pairs(r, p) == 0 and split(r, p, ids) == 0 and pairs(r, p, ids) == 0
    for v in (np.nan, np.inf, -np.inf):
        bad = pred.copy(); bad[7, 3] = v                                 # selected: row 7, column 3 of the lower triangle
        assert split(r, _dev(bad)) == -1 and b"NaN or infinite" in L.mcgra_last_error()
        assert pairs(r, _dev(bad)) == -1 and b"NaN or infinite" in L.mcgra_last_error()
        ok = pred.copy(); ok[3, 7] = v; ok[5, 5] = v                     # its mirror and the diagonal are not looked at
        assert split(r, _dev(ok)) == 0 and pairs(r, _dev(ok)) == 0
    for v in (-1.0, 16.0, -1e-45, 1e30):
        bad = pred.copy(); bad[40, 39] = v
        assert split(r, _dev(bad)) == -3 and b"below 16" in L.mcgra_last_error()
        assert pairs(r, _dev(bad)) == 0                                   # any finite score is a candidate there
    bad = real.copy(); bad[9, 2] = 0.5
    assert split(_dev(bad), p) == -1 and b"neither 0 nor 1" in L.mcgra_last_error()
    assert pairs(_dev(bad), p) == -1 and b"neither 0 nor 1" in L.mcgra_last_error()
    ok = real.copy(); ok[2, 9] = 0.5
    assert split(_dev(ok), p) == 0 and pairs(_dev(ok), p) == 0
    for ix in ([4, 9, 4], [7, 7], [0, n], [-1, 2]):                      # repeated; out of range
        t = torch.as_tensor(ix, device="cuda:0")
        assert split(r, p, t, len(ix)) == -1 and pairs(r, p, t, len(ix)) == -1, ix
    from mc_gra_amd import engine as E
    bad = pred.copy(); bad[7, 3] = 16.0
    with pytest.raises(pkg._lib.McgraNotSupported):
        E.two_means_split(_dev(bad))
    bad[7, 3] = np.nan
    with pytest.raises(pkg._lib.McgraError):
        E.two_means_split(_dev(bad))
    with pytest.raises(pkg._lib.McgraError):
        E.threshold_pairs(_dev(bad), 0.5)
    with pytest.raises(pkg._lib.McgraError):
        E.threshold_pairs(p, float("nan"))


# ------------------------------------------------------------------------------------------------------ 4. main.py
def test_main_evaluate_binarize_and_save_graph(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --binarize adds the three
    split_* dicts, each the truth on the modified_adj that was split; --save_graph is engine.threshold_pairs on the whole
    graph's threshold; a run without the flags returns and logs what it did before the flags existed.  (Not brazil, the
    graph of the --topk main test: its decode branch, relu(Z Z^T - I), is unbounded, and that run's modified_adj holds scores
    outside [0, 16), which the split refuses by definition with MCGRA_ENOSUP.)"""
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain = M.run(M.build_parser().parse_args(argv + ["--log_name", "plain.txt"]))
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.two_means_split

    def record(pred, idx=None, real=None, max_iter=256):
        v = orig(pred, idx, real, max_iter)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx), pred, real, v))
        return v

    monkeypatch.setattr(M.engine, "two_means_split", record)
    path = str(tmp_path / "graph.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "split.txt", "--binarize", "--save_graph", path]))
    out = capsys.readouterr().out
    assert sorted(res) == sorted(list(plain) + ["split_attack", "split_train", "split_all"]) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flag, bit for bit
    for (real, pred, idx, _, _, v), name in zip(seen, ("attack", "train", "all")):
        assert res[f"split_{name}"] is v
        _check_split(v, T.split(real, pred, idx), name)
    real, pred, idx, dpred, dreal, d = seen[2]
    assert idx is None and d["pairs"] == pairs_of(1190) and not d["degenerate"] and 0 < d["edges"] < d["pairs"]
    z = np.load(path)
    assert sorted(z.files) == ["hits", "iterations", "pairs", "scores", "threshold"]
    want = E.threshold_pairs(dpred, d["threshold"], None, dreal)
    _check_pairs(want, T.threshold_pairs(real, pred, d["threshold"]), "whole graph")
    assert np.array_equal(z["pairs"], want[0].cpu().numpy()) and z["pairs"].dtype == np.int64 and len(z["pairs"]) == d["edges"]
    assert np.array_equal(z["scores"].view(np.uint32), want[1].cpu().numpy().view(np.uint32)) and z["scores"].dtype == np.float32
    assert np.array_equal(z["hits"], want[2].cpu().numpy()) and z["hits"].dtype == np.bool_ and int(z["hits"].sum()) == d["hits"]
    assert K_bits(z["threshold"]) == K_bits(d["threshold"]) and int(z["iterations"]) == d["iterations"]
    assert (f"current auc={res['auc_all']}\ncurrent split_f1={d['f1']} (edges={d['edges']}, threshold={d['threshold']})\n" in out
            and "split_f1" not in out_plain)
    log = open(tmp_path / "results" / "split.txt").read().split("\n")
    for line, (name, key) in zip(log[2:5], (("attack graph", "split_attack"), ("train graph", "split_train"), ("Whole Graph", "split_all"))):
        s = res[key]
        assert line == (f"In {name}: split edges={s['edges']} threshold={s['threshold']} rounds={s['iterations']} "
                        f"P={s['precision']} R={s['recall']} F1={s['f1']}")
    assert log[5].startswith("current density:") and "binarize=True" in log[0] and "save_graph=" in log[0] and "topk" not in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "binarize" not in old and "save_graph" not in old and "split" not in old and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[5:]
