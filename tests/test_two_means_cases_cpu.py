"""CPU-side checks of the 2-means entries (mcgra_two_means_split, mcgra_threshold_pairs, engine.two_means_split /
threshold_pairs, main.py --binarize / --save_graph): the truth helper against the properties of its own definition and
against an independently written float64 Lloyd; the resolving power of the inputs tests/test_gpu_two_means.py uses; the C ABI,
its binding and every refusal that the arguments alone decide (the pointers here are never followed); the command line.  No
compute: there is no GPU here."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from tests import two_means_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


@pytest.fixture(scope="module")
def gpu_cases():
    from tests import test_gpu_two_means as G
    return G


def _q(G, name, variant=None):
    real, pred, idx, _, _ = G.CASES[name]
    return T.quantise(T.K.packed(real, pred, idx)[0], variant)


# ---------------------------------------------------------------------------------------------------- truth helper
def test_quantisation_rounds_half_to_even_and_is_exact():
    v = np.array([2.0 ** -29, 3 * 2.0 ** -29, 5 * 2.0 ** -29, 7 * 2.0 ** -29, 2.0 ** -28, 1.0, 0.5 + 2.0 ** -24], np.float32)
    assert T.quantise(v).tolist() == [0, 2, 2, 4, 1, 2 ** 28, 2 ** 27 + 16]
    assert T.quantise(v, "truncate").tolist() == [0, 1, 2, 3, 1, 2 ** 28, 2 ** 27 + 16]
    z = np.array([0x80000000, 0, 1, 0x007fffff, 0x00800000], np.uint32).view(np.float32)       # -0.0, 0, subnormals, 2^-126
    assert T.quantise(z).tolist() == [0] * 5
    top = np.array([0x417fffff], np.uint32).view(np.float32)
    assert top[0] < 16 and T.quantise(top).tolist() == [2 ** 32 - 2 ** 8]


def test_truth_on_a_split_worked_by_hand(gpu_cases):
    """[2, 12, 13, 19, 33, 35] x 2^-10: t_0 = 19 units + 1 -> low {2, 12, 13}, high {19, 33, 35}, c0 = 9, c1 = 29; 19 sits
    exactly on (9 + 29) / 2 and goes low: t_1 = 19 units + 1 ... the next partition is {2, 12, 13, 19} | {33, 35}."""
    u = 2 ** 18
    q = np.array(gpu_cases.TIE_VALUES, np.uint64) * np.uint64(u)
    r = T.lloyd(q)
    assert (r["edges"], r["c0"], r["c1"], r["converged"]) == (2, 46 * u // 4, 34 * u, 1) and r["t"] == (r["c0"] + r["c1"]) // 2 + 1
    first = T.lloyd(q, 1)
    assert (first["iterations"], first["converged"], first["t"], first["edges"], first["c0"], first["c1"]) == \
           (1, 0, 18 * u + u // 2 + 1, 3, 9 * u, 29 * u)
    assert 2 * 19 * u == first["c0"] + first["c1"]                      # the tie
    assert T.lloyd(q, variant="ties_high")["edges"] == 3


def test_the_reported_state_is_a_fixed_point(gpu_cases):
    """Counting again at the reported t reproduces n_high and the centres; where the iteration converged the centres give t
    back; both clusters are non-empty."""
    for name in gpu_cases.CASES:
        r = gpu_cases.truth(name)
        if r["degenerate"]:
            continue
        q = _q(gpu_cases, name)
        high = q >= np.uint64(r["t"])
        obj = q.astype(object)
        assert 0 < int(high.sum()) < len(q) and int(high.sum()) == r["edges"], name
        assert int(obj[~high].sum()) // int((~high).sum()) == r["c0"] and int(obj[high].sum()) // int(high.sum()) == r["c1"], name
        assert r["c0"] < r["t"] <= r["c1"], name
        if r["converged"]:
            assert (r["c0"] + r["c1"]) // 2 + 1 == r["t"], name
        else:
            assert r["iterations"] == gpu_cases.CASES[name][4], name


def float_lloyd(s):
    """An independent Lloyd in float64 on the scores themselves: real means, the centres start at the extremes (so the first
    boundary is their midpoint), a score equidistant from the two centres goes low; runs until the partition repeats."""
    x = np.asarray(s, np.float64)
    c_low, c_high = x.min(), x.max()
    prev = None
    for _ in range(1000):
        high = np.abs(x - c_high) < np.abs(x - c_low)
        if prev is not None and np.array_equal(high, prev):
            return high
        prev = high
        c_low, c_high = x[~high].mean(), x[high].mean()
    raise AssertionError("no fixed point")


def test_an_independent_float64_lloyd_finds_the_same_partition(gpu_cases):
    checked = 0
    for name, (real, pred, idx, _, max_iter) in gpu_cases.CASES.items():
        r = gpu_cases.truth(name)
        if r["degenerate"] or not r["converged"]:
            continue
        gap = float(r["threshold"]) - float(r["threshold_low"])
        assert gap > 0, name
        if gap <= 2.0 ** -26:
            continue
        s = T.K.packed(real, pred, idx)[0]
        assert np.array_equal(float_lloyd(s), r["high"]), name
        checked += 1
    assert checked >= 20, checked


def test_the_high_cluster_is_everything_at_or_above_the_threshold(gpu_cases):
    for name, (real, pred, idx, _, _) in gpu_cases.CASES.items():
        r = gpu_cases.truth(name)
        if r["degenerate"]:
            assert r["threshold"] is None and not r["high"].any()
            continue
        s = T.K.packed(real, pred, idx)[0]
        assert np.array_equal(s >= r["threshold"], r["high"]) and np.array_equal(s <= r["threshold_low"], ~r["high"]), name
        pairs, scores, hits = T.threshold_pairs(real, pred, r["threshold"], idx)
        assert len(pairs) == r["edges"] and int(hits.sum()) == r["hits"], name


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_the_cases_tell_each_wrong_reading_from_the_truth(gpu_cases, variant):
    """Resolving power: each mutant of the definition changes a reported integer on at least one case of the shared list."""
    told = []
    for name, (real, pred, idx, _, max_iter) in gpu_cases.CASES.items():
        if len(pred) > 300:
            continue                                                      # (the small cases carry this; the large ones cost time)
        right, wrong = gpu_cases.truth(name), T.split(real, pred, idx, max_iter, variant)
        if any(int(right[k]) != int(wrong[k]) for k in T.INTS + ("hits",)):
            told.append(name)
    print(variant, told)
    assert told, variant
    named = {"ties_high": "tie_on_the_midpoint", "truncate": "quant_halfway_small", "report_next": "several_rounds_cap2"}
    assert named.get(variant, told[0]) in told


def test_the_gpu_cases_hold_what_they_are_named_for(gpu_cases):
    G, C = gpu_cases, gpu_cases.CASES
    assert G.truth("n2_one_pair")["degenerate"] and G.truth("n2_one_pair")["pairs"] == 1
    assert len(np.unique(_q(G, "n3_two_values"))) == 2 and not G.truth("n3_two_values")["degenerate"]
    r = G.truth("n64_all_equal")
    assert r["degenerate"] and (r["iterations"], r["converged"], r["edges"], r["hits"]) == (0, 1, 0, 0) and r["c0"] == r["c1"] == r["t"] - 1
    for name in ("tie_on_the_midpoint", "several_rounds"):                # multiples of 2^-10: q is exact
        s = T.K.packed(*C[name][:3])[0]
        assert np.array_equal(s * 1024, np.round(s * 1024)) and np.array_equal(T.quantise(s), (s * 1024).astype(np.uint64) << np.uint64(18))
    full, capped = G.truth("several_rounds"), G.truth("several_rounds_cap2")
    assert full["iterations"] >= 4 and full["converged"] == 1
    assert (capped["iterations"], capped["converged"]) == (2, 0) and capped["t"] != full["t"]
    small = T.K.packed(*C["quant_halfway_small"][:3])[0]
    bits = small.view(np.uint32)
    assert (bits == 0x80000000).any() and ((bits & 0x7f800000) == 0).sum() >= 4 and set(T.quantise(small).tolist()) == {0, 1, 2, 4}
    top = T.K.packed(*C["quant_largest_below_16"][:3])[0]
    assert (top.view(np.uint32) == 0x417fffff).any() and int(T.quantise(top).max()) == 2 ** 32 - 256
    many = T.K.packed(*C["quant_halfway_many"][:3])[0]
    assert np.array_equal((many.astype(np.float64) * 2.0 ** 29) % 2, np.ones(len(many)))      # every value half-way
    real, pred, idx, pad, _ = C["n257_ld288"]
    assert len(pred) == 257 and idx is None and 257 + pad == 288
    real, pred, idx, _, _ = C["junk_outside_selection"]
    assert not np.array_equal(np.sort(idx), np.arange(len(pred))) and np.array_equal(idx, np.sort(idx))
    off = np.ones(len(pred), bool); off[idx] = False
    for mtx in (real, pred):
        up = mtx[np.triu(np.ones(mtx.shape, bool))]
        assert np.isnan(up).any() and (up == -1).any() and (up == 99).any()
        assert not np.isin(mtx[off], (0.0, 1.0)).any() and not np.isin(mtx[:, off], (0.0, 1.0)).any() and off.sum() == 30
    a, b = C["subset_permuted"][2], C["subset_reordered"][2]
    assert len(a) == 100 and len(set(a.tolist())) == 100 and sorted(a.tolist()) == sorted(b.tolist()) and not np.array_equal(a, b)
    assert not np.array_equal(a, np.sort(a)) and np.array_equal(C["subset_permuted"][1], C["subset_permuted"][1].T)
    ra, rb = G.truth("subset_permuted"), G.truth("subset_reordered")
    assert all(ra[k] == rb[k] for k in T.INTS + ("hits", "threshold", "threshold_low")) and not np.array_equal(ra["high"], rb["high"])
    r = G.truth("bench_shaped_n2048")
    assert 0.0005 < r["edges"] / r["pairs"] < 0.002 and 0.6 < r["threshold"] < 0.8 and r["f1"] > 0.5 and r["iterations"] >= 2


def test_the_tiling_cases_sit_on_both_sides_of_the_kernels_constants(gpu_cases):
    """The constants are read from the source, and each boundary they put into the launch arithmetic has a case on each side."""
    G = gpu_cases
    src = open(os.path.join(ROOT, "mc-gra_amd", "csrc", "two_means.hip")).read()
    com = open(os.path.join(ROOT, "mc-gra_amd", "csrc", "rank_common.h")).read()
    const = lambda text, name: re.search(rf"constexpr int {name} = ([^;]+);", text).group(1)
    assert int(const(com, "AUC_THREADS")) == G.THREADS and int(const(src, "TM_ROW_BLOCKS")) == G.ROW_BLOCKS
    assert const(src, "TM_STEP") == "4 * AUC_THREADS" and G.STEP == 4 * G.THREADS
    assert int(const(src, "TM_BLOCKS")) == G.BLOCKS and int(const(src, "TM_BATCH")) == G.BATCH and int(const(src, "TP_BLOCKS")) == G.TP_BLOCKS
    p = G.pairs_of
    for below, limit in ((45, G.STEP), (724, G.TP_BLOCKS * G.THREADS), (1448, G.BLOCKS * G.STEP)):
        assert p(below) <= limit < p(below + 1) and below in G.TILING and below + 1 in G.TILING
    assert 257 - 1 == G.THREADS and 1025 - 1 == G.ROW_BLOCKS and {257, 258, 1025, 1026} <= set(G.TILING)
    for rows in G.TILING:
        assert len(G.CASES[f"tiling_n{rows}"][1]) == rows and not G.truth(f"tiling_n{rows}")["degenerate"]
    assert G.truth("several_rounds")["iterations"] > G.BATCH           # the rounds of one case span two reads of the state


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entries_are_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    lib = ctypes.CDLL(LIB)
    for s, nargs in (("mcgra_two_means_split", 12), ("mcgra_threshold_pairs", 14)):
        assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s)
        assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == nargs
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    for f in (E.two_means_split, E.threshold_pairs):
        assert callable(f) and hasattr(f, "__wrapped__") and "baseline.py" in f.__doc__                # the device guard
    assert E.TWO_MEANS_SCALE == 2.0 ** -28


def test_entries_refuse_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to the host outputs."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)

    def split(n=8, lds=8, ldl=8, idx=None, n_idx=None, sc=p, lab=p, max_iter=256, out=True):
        o, hi, lo = (ctypes.c_int64 * 10)(*([-7] * 10)), ctypes.c_float(-7.0), ctypes.c_float(-7.0)
        rc = L.mcgra_two_means_split(None, n, sc, lds, lab, ldl, idx, n if n_idx is None else n_idx, max_iter, o if out else None,
                                     ctypes.byref(hi), ctypes.byref(lo))
        assert list(o) == [-7] * 10 and hi.value == -7.0 and lo.value == -7.0
        return rc

    def pairs(n=8, lds=8, ldl=8, idx=None, n_idx=None, sc=p, lab=p, thr=0.5, cap=4, buf=p, hits=None, counts=True):
        c = (ctypes.c_int64 * 3)(-7, -7, -7)
        rc = L.mcgra_threshold_pairs(None, n, sc, lds, lab, ldl, idx, n if n_idx is None else n_idx, thr, cap, buf, None, hits,
                                     c if counts else None)
        assert list(c) == [-7] * 3
        return rc

    shared = (dict(n=0), dict(n=-3), dict(n=1), dict(lds=7), dict(ldl=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
              dict(idx=p, n_idx=-5), dict(sc=None))
    for kw in shared + (dict(max_iter=0), dict(max_iter=-1), dict(out=False)):
        assert split(**kw) == -1 and b"two_means_split" in L.mcgra_last_error(), kw
    for kw in shared + (dict(cap=-1), dict(thr=float("nan")), dict(lab=None, hits=p), dict(buf=None), dict(counts=False)):
        assert pairs(**kw) == -1 and b"threshold_pairs" in L.mcgra_last_error(), kw
    assert pairs(thr=float("nan")) == -1 and b"NaN" in L.mcgra_last_error()
    big = 65536
    for f in (split, pairs):
        assert f(n=big, lds=big, ldl=big) == -3 and b"65535" in L.mcgra_last_error()
        assert f(n=10 ** 6, lds=10 ** 6, ldl=10 ** 6, idx=p, n_idx=big) == -3
        assert f(n=big, lds=big - 1, ldl=big) == -1                      # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(split(n=big, lds=big, ldl=big))


def test_engine_entries_refuse_wrong_shapes_and_host_tensors(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for pred, real in ((wide, None), (torch.zeros(5), None), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.two_means_split.__wrapped__(pred, None, real)
        with pytest.raises(AssertionError):
            E.threshold_pairs.__wrapped__(pred, 0.5, None, real)
    with pytest.raises(ValueError, match="device tensors"):
        E.two_means_split(sq)                                             # a host tensor: refused before anything is called
    with pytest.raises(ValueError, match="device tensors"):
        E.threshold_pairs(sq, 0.5)


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_binarize_is_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    assert p.parse_args([]).binarize is False and p.parse_args([]).save_graph is None
    a = p.parse_args(["--binarize", "--save_graph", "g.npz"])
    assert a.binarize is True and a.save_graph == "g.npz"
    with pytest.raises(SystemExit):
        p.parse_args(["--save_graph", "g.npz"])
    assert "--save_graph needs --binarize" in capsys.readouterr().err
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--binarize", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err   # the wording of --topk's refusal
    assert "--binarize" in M.__doc__ and "--save_graph" in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(binarize=True, mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --binarize"):
        M._run(argparse.Namespace(binarize=False, save_graph="g.npz", mode="evaluate"), 0, 1)
    calls = []
    R.check_binarize_args(argparse.Namespace(binarize=False, save_graph=None, mode="prepare"), calls.append)
    R.check_binarize_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_binarize_args(argparse.Namespace(binarize=True, save_graph="x", mode="evaluate"), calls.append)
    assert calls == []


def test_binarize_is_hidden_from_the_parameter_line_when_unset(pkg):
    """The log's parameter line prints reports.shown_parameters(args): the two flags are in it exactly when --binarize is set,
    and none of the other flags that are hidden while unset comes with them."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    older = ("ap", "topk", "save_edges", "curves", "per_node", "binarize", "save_graph")
    args = M.build_parser().parse_args([])
    assert all(f" {k}=" in str(args) for k in older)
    assert not any(f" {k}=" in str(R.shown_parameters(args)) for k in older)
    for argv, own in ((["--binarize"], ("binarize", "save_graph")), (["--binarize", "--save_graph", "g.npz"], ("binarize", "save_graph"))):
        args = M.build_parser().parse_args(argv)
        text = str(R.shown_parameters(args))
        assert [k for k in older if f" {k}=" in text] == list(own), (argv, text)
        assert f"binarize=True, save_graph={args.save_graph!r}" in text
        assert vars(R.shown_parameters(args)) == {k: v for k, v in vars(args).items() if k not in set(older) - set(own)}
