"""CPU-side checks of the k-nearest-neighbour graph entry (mcgra_knn_graph, engine.knn_graph, main.py --knn / --save_knn): the
truth helper against the definition's literal double loop, its identities, the structure and per-node truths where they
overlap and sklearn's kneighbors_graph; the resolving power of the inputs tests/test_gpu_knn_graph.py uses; the host
arithmetic of engine.knn_graph_stats; the C ABI, its binding and every refusal that the arguments alone decide (the pointers
here are never followed); the command line; the report's text and file from a dict built with the truth (no compute: there is
no GPU here)."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import graph_structure_truth as GS
from tests import knn_cases as KC
from tests import knn_truth as T
from tests import node_rank_truth as NR
from tests import topk_truth as TK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")
CASES = KC.cases()
SMALL = [name for name in sorted(CASES) if len(CASES[name][1]) <= 130]


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


# ---------------------------------------------------------------------------------------------------- truth helper
def test_truth_lists_are_the_definitions_double_loop():
    """L_k(a) by counting, for every candidate, who is ahead of it (float32 comparisons: -0.0 == +0.0, distinct subnormals)."""
    rows = 0
    for name in SMALL:
        real, pred, idx, ks = CASES[name]
        m = len(pred) if idx is None else len(idx)
        for k in ks[:2] + ks[-1:]:
            L = T.lists(pred, k, idx)
            for a in sorted({0, 1, m // 2, m - 1}):
                assert L[a].tolist() == T.row_by_definition(pred, k, a, idx), (name, k, a)
                rows += 1
    assert rows > 100


def test_truth_obeys_the_identities_of_the_definition():
    for name in SMALL + ["q1025"]:
        real, pred, idx, ks = CASES[name]
        for k in ks:
            g = T.ints(real, pred, k, idx)
            T.check_identities(g)
            T.check_identities(T.ints(None, pred, k, idx))
            m = len(g["in"])
            assert all(len(set(row)) == k and a not in row for a, row in enumerate(g["lists"].tolist()))
            assert len(g["edges"][0]) == g["E_U"] and int((g["edges"][2] == 3).sum()) == g["E_M"]
            assert int(g["edges"][3].sum()) == g["H_U"] and set(np.unique(g["edges"][2]).tolist()) <= {1, 2, 3}
            a_b = g["edges"][0]
            if idx is None:                                                # ascending packed position
                p = a_b[:, 0] * (a_b[:, 0] - 1) // 2 + a_b[:, 1]
                assert (a_b[:, 0] > a_b[:, 1]).all() and (np.diff(p) > 0).all()
            want = T.ints_from_lists(g["lists"], m)
            assert all(g[q] == want[q] for q in want), name


def test_truth_agrees_with_the_structure_truth_on_u_and_g():
    """d_G, E_G are graph_structure_truth's on the labels; U as a 0 / 1 matrix cut at threshold 1 gives E_U and d_U."""
    for name in ("q65", "q129", "subset_permuted", "hub", "two_valued"):
        real, pred, idx, ks = CASES[name]
        for k in ks[:2]:
            g = T.ints(real, pred, k, idx)
            m = len(g["in"])
            D = T.directed(pred, k, idx)
            U = (D | D.T).astype(np.float32)
            ix = np.arange(m) if idx is None else np.asarray(idx)
            clean = np.where(np.asarray(real)[np.ix_(ix, ix)] == 1, 1, 0).astype(np.float32)
            s = GS.ints(clean, U, 1.0)
            assert (s["E_R"], s["d_R"], s["E_G"], s["d_G"]) == (g["E_U"], g["d_U"], g["E_G"], g["d_G"])
            assert (s["E_C"], s["d_C"]) == (g["H_U"], g["h_U"])


def test_truth_agrees_with_the_per_node_truth_where_they_overlap():
    """With k = a row's positive count P, h_D is that row's `hits` of mcgra_node_rank_metrics (symmetric labels)."""
    checked = 0
    for name in ("q65", "q129", "two_valued", "subset_permuted", "signed_zeros"):
        real, pred, idx, _ = CASES[name]
        m = len(pred) if idx is None else len(idx)
        per_node = NR.per_node(np.nan_to_num(real, nan=0, posinf=0), pred, idx)
        for P in sorted(set(per_node[:, 0].tolist()))[:6]:
            if not 1 <= P <= m - 1:
                continue
            g = T.ints(real, pred, P, idx)
            for a in np.nonzero(per_node[:, 0] == P)[0]:
                assert g["h_D"][a] == per_node[a, 3], (name, P, a)
                checked += 1
    assert checked > 50


def test_truth_is_sklearns_kneighbors_graph_on_tie_free_scores():
    neighbors = pytest.importorskip("sklearn.neighbors")
    for name in ("distinct_asym", "negative"):
        real, pred, idx, ks = CASES[name]
        assert len(np.unique(pred)) == pred.size
        dist = (pred.max() - pred).astype(np.float64)
        np.fill_diagonal(dist, 0)
        for k in ks:
            want = neighbors.kneighbors_graph(dist, k, metric="precomputed", mode="connectivity", include_self=False).toarray() > 0
            assert np.array_equal(T.directed(pred, k), want), (name, k)


# ---------------------------------------------------------------------------------------------------- resolving power
def _differs(a, b):
    return any(a[q] != b[q] for q in T.HEADER + T.COLUMNS) or ("lists" in a and "lists" in b
                                                              and not np.array_equal(a["lists"], b["lists"]))


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_the_cases_tell_each_wrong_reading_from_the_truth(variant):
    """Every wrong reading of the definition changes an integer of at least three (case, k) of the shared list -- and the first
    five already on the quantised matrices at m in {5, 63, 64, 65, 129}, k in {1, 2, 7} (node ids: under the permuted idx)."""
    told = []
    for name in SMALL:
        real, pred, idx, ks = CASES[name]
        m = len(pred) if idx is None else len(idx)
        for k in ks:
            if variant == "k_plus" and k + 1 > m - 1:
                continue
            if _differs(T.ints(real, pred, k, idx), T.ints(real, pred, k, idx, variant)):
                told.append((name, k))
    assert len(told) >= 3, told
    names = {n for n, _ in told}
    if variant in ("ties_desc", "columns", "diagonal", "k_plus", "k_minus", "swapped", "global"):
        assert {(f"q{m}", k) for m in (5, 63, 64, 65, 129) for k in (1, 2, 7) if k <= m - 1} - {("q5", 7)} <= set(told), told
    if variant == "node_id":
        assert "subset_permuted" in names and "subset" not in names
    if variant == "neg_zero":
        assert names == {"signed_zeros"}


def test_the_gpu_cases_hold_what_they_are_named_for():
    assert set(KC.SMALL) >= {2, 3, 63, 64, 65, 127, 128, 129} and set(KC.K_SET) == {1, 2, 7, 63, 64, 65}
    for c in KC.CLASSES[:-1]:
        assert {c - 1, c, c + 1} & set(KC.LARGE) >= {c, c + 1}            # the last size of a class and the first of the next
    assert 1023 in KC.LARGE and KC.CLASSES[-1] == KC.MAX_NIDX
    assert KC.MAX_K in KC.LARGE[1025] and KC.MAX_K in KC.LARGE[2049] and KC.MAX_K in KC.LARGE[4097]
    for m in KC.SMALL:
        real, pred, idx, ks = CASES[f"q{m}"]
        assert m - 1 in ks and set(ks) <= set(KC.K_SET) | {m - 1} and not np.array_equal(pred, pred.T) or m == 2
        assert (np.diagonal(pred) == 9).all() and pred[~np.eye(m, dtype=bool)].max() < 9
    assert len(np.unique(CASES["constant"][1])) == 1 and len(np.unique(CASES["two_valued"][1])) == 2
    hub = CASES["hub"][1]
    assert all(np.argmax(np.delete(hub[a], a)) == 17 - (17 > a) for a in range(len(hub)) if a != 17)
    z = CASES["signed_zeros"][1].view(np.uint32)
    assert (z == 0x80000000).any() and (z == 0).any() and (z == 1).any() and (z == 0x80000001).any()
    s = CASES["negative_subnormal"][1]
    assert (s < 0).any() and ((s.view(np.uint32) & 0x7f800000) == 0).any() and (CASES["negative"][1] < 0).all()
    real, pred, idx, _ = CASES["subset"]
    pidx = CASES["subset_permuted"][2]
    assert sorted(pidx.tolist()) == idx.tolist() and not np.array_equal(pidx, idx) and len(idx) < len(pred)
    off = np.ones(len(pred), bool)
    off[idx] = False
    for M in (real, pred):
        assert not np.isfinite(M[off]).any() and not np.isfinite(M[:, off]).any() and np.isnan(np.diagonal(M)).all()
        sel = M[np.ix_(idx, idx)][~np.eye(len(idx), dtype=bool)]
        assert np.isfinite(sel).all()
    d = CASES["subset_distinct"][1]
    sel = d[np.ix_(idx, idx)][~np.eye(len(idx), dtype=bool)]
    assert len(np.unique(sel)) == sel.size
    rows = [KC.capacity_row(a) for a in (0, 1, KC.MAX_NIDX - 1)]
    assert all(len(np.unique(r)) == KC.MAX_NIDX and r.max() < 2 ** 24 for r in rows)


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_knn_graph_stats_on_five_nodes_by_hand(pkg):
    """Five nodes, k = 2.  Lists: 0: 1 2 | 1: 0 2 | 2: 0 1 | 3: 0 1 | 4: 0 3.  True edges: 01 02 34."""
    from mc_gra_amd import engine as E
    pred = np.array([[0, 9, 8, 1, 1], [9, 0, 8, 1, 1], [9, 8, 0, 1, 1], [9, 8, 1, 0, 2], [9, 1, 1, 8, 0]], np.float32)
    real = np.zeros((5, 5), np.float32)
    for a, b in ((0, 1), (0, 2), (3, 4)):
        real[a, b] = real[b, a] = 1
    g = T.ints(real, pred, 2)
    assert g["lists"].tolist() == [[1, 2], [0, 2], [0, 1], [0, 1], [0, 3]]
    assert g["in"] == [4, 3, 2, 1, 0] and g["d_U"] == [4, 3, 2, 3, 2] and g["d_M"] == [2, 2, 2, 0, 0]
    assert [g[q] for q in T.HEADER] == [10, 2, 7, 3, 3, 5, 3, 2]          # U: 01 02 03 04 12 13 34; Mu: 01 02 12
    assert g["edges"][0].tolist() == [[1, 0], [2, 0], [2, 1], [3, 0], [3, 1], [4, 0], [4, 3]]
    assert g["edges"][2].tolist() == [3, 3, 3, 1, 1, 1, 1] and g["edges"][3].tolist() == [True, True, False, False, False, False, True]
    s = E.knn_graph_stats(g, g)
    assert s["directed"] == {"edges": 10, "positives": 6, "hits": 5, "precision": 0.5, "recall": 5 / 6, "f1": 10 / 16}
    assert s["union"] == {"edges": 7, "positives": 3, "hits": 3, "precision": 3 / 7, "recall": 1.0, "f1": 0.6, "isolated": 0}
    assert s["mutual"] == {"edges": 3, "positives": 3, "hits": 2, "precision": 2 / 3, "recall": 2 / 3, "f1": 2 / 3, "isolated": 2}
    hub = s["hubness"]
    assert (hub["max_in"], hub["orphans"], hub["skewness"]) == (4, 1, 0.0)           # in - k = 2 1 0 -1 -2: symmetric
    assert hub["in_hist"] == [(0, 0, 1), (1, 1, 1), (2, 2, 1), (3, 4, 2), (5, 8, 0), (9, 16, 0), (17, 32, 0), (33, None, 0)]
    assert repr(s) == repr(T.stats(g)) and s["nodes"] == 5 and s["k"] == 2


def test_knn_graph_stats_nan_rules_and_refusals(pkg):
    from mc_gra_amd import engine as E
    real, pred, idx, _ = CASES["q65"]
    g = T.ints(None, pred, 7)
    s = E.knn_graph_stats(g, g)
    for which in ("directed", "union", "mutual"):
        assert s[which]["hits"] is None and all(math.isnan(s[which][q]) for q in T.GRAPH_DOUBLES)
    assert repr(s) == repr(T.stats(g))
    g = T.ints(np.zeros_like(real), pred, 7)                              # no true edge: recall 0 / 0, precision 0 / edges
    s = E.knn_graph_stats(g, g)
    assert math.isnan(s["union"]["recall"]) and s["union"]["precision"] == 0.0 and s["union"]["f1"] == 0.0
    g = T.ints(real[:2, :2], CASES["q2"][1], 1)                           # every in-degree is k: m2 == 0
    assert math.isnan(E.knn_graph_stats(g, g)["hubness"]["skewness"])
    bad = dict(T.ints(real, pred, 7))
    bad["in"] = bad["in"][:-1] + [bad["in"][-1] + 1]
    with pytest.raises(ValueError, match="do not belong"):
        E.knn_graph_stats(bad, bad)
    for name in SMALL:
        real, pred, idx, ks = CASES[name]
        for k in ks:
            g = T.ints(real, pred, k, idx)
            assert repr(E.knn_graph_stats(g, g)) == repr(T.stats(g)), (name, k)


def test_skewness_is_scipys_biased_sample_skewness(pkg):
    stats = pytest.importorskip("scipy.stats")
    from mc_gra_amd import engine as E
    seen = 0
    for name in ("hub", "q129", "two_valued", "distinct_asym", "q65"):
        real, pred, idx, ks = CASES[name]
        for k in ks:
            g = T.ints(real, pred, k, idx)
            got = E.knn_graph_stats(g, g)["hubness"]["skewness"]
            if math.isnan(got):
                assert len(set(g["in"])) == 1
                continue
            want = float(stats.skew(np.asarray(g["in"], np.float64), bias=True))
            assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (name, k, got, want)
            seen += 1
    assert seen >= 10


def test_the_k_of_the_mean_true_degree(pkg):
    """--knn 0: 2 P / m rounded half UP in integers, at least 1, clamped to min(m - 1, 1024); K >= 1 as given, clamped alike."""
    from mc_gra_amd import engine as E
    from mc_gra_amd import reports as R
    assert R.knn_k(0, 10, 0) == 1 and R.knn_k(0, 10, 7) == 1 and R.knn_k(0, 10, 8) == 2          # 1.4 -> 1, 1.6 -> 2
    assert R.knn_k(0, 4, 3) == 2 and R.knn_k(0, 4, 5) == 3 and R.knn_k(0, 4, 2) == 1              # 1.5 -> 2, 2.5 -> 3, 1.0
    assert R.knn_k(0, 2708, 5278) == 4                                                             # 3.898
    for m in (2, 3, 4, 7, 10, 101):
        for P in range(0, m * (m - 1) // 2 + 1):
            assert R.knn_k(0, m, P) == min(T.k_of_mean_degree(m, P), m - 1), (m, P)
    assert R.knn_k(5, 100, 0) == 5 and R.knn_k(5, 4, 0) == 3 and R.knn_k(5000, 10 ** 4, 0) == E.KNN_MAX_K == 1024
    assert R.knn_k(0, 5000, 5000 * 4999 // 2) == 1024


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_knn_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    lib = ctypes.CDLL(LIB)
    s = "mcgra_knn_graph"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s)
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 17
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    assert callable(E.knn_graph) and hasattr(E.knn_graph, "__wrapped__")      # the device guard
    assert E.KNN_HEADER == T.HEADER and E.KNN_COLUMNS == T.COLUMNS and E.KNN_IN_BINS == T.IN_BINS


def test_constants_agree_between_header_kernel_engine_and_tests(pkg):
    from mc_gra_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "mcgra.h")).read()
    src = open(os.path.join(ROOT, "mc-gra_amd", "csrc", "knn_graph.hip")).read()
    bound = int(re.search(r"#define MCGRA_KNN_MAX_NIDX (\d+)", hdr).group(1))
    max_k = int(re.search(r"#define MCGRA_KNN_MAX_K (\d+)", hdr).group(1))
    node_rank = int(re.search(r"#define MCGRA_NODE_RANK_MAX_NIDX (\d+)", hdr).group(1))
    launched = [bound if c == "MCGRA_KNN_MAX_NIDX" else int(c) for c in re.findall(r"knn_select_launch<(\w+)>\(st", src)]
    assert bound == node_rank == E.KNN_MAX_NIDX == KC.MAX_NIDX and max_k == E.KNN_MAX_K == KC.MAX_K == 1024
    assert list(E.KNN_CLASSES) == launched == list(KC.CLASSES) and launched[-1] == bound
    assert re.findall(r"m <= (\d+)\) knn_select_launch", src) == [str(c) for c in launched[:-1]]


def test_knn_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed and
    no GPU in the machine; the host header is not written."""
    from mc_gra_amd import engine as E
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    hd = (ctypes.c_int64 * 8)(*([-7] * 8))

    def call(n=8, lds=8, ldl=8, idx=None, n_idx=None, k=3, sc=p, lab=p, header=hd, out=p, lists=p, cap=0, pairs=None, ps=None,
             kind=None, hits=None):
        rc = L.mcgra_knn_graph(None, n, sc, lds, lab, ldl, idx, n if n_idx is None else n_idx, k, header, out, lists, cap, pairs,
                               ps, kind, hits)
        return rc, L.mcgra_last_error().decode()

    for kw, cause in ((dict(header=None), "header"), (dict(out=None), "out"), (dict(sc=None), "matrices not NULL"),
                      (dict(lds=7), "ld >= n"), (dict(ldl=7), "ld >= n"), (dict(n=0), "n >= 1"), (dict(n=1), "at least 2"),
                      (dict(idx=p, n_idx=1), "at least 2"), (dict(idx=p, n_idx=-5), "at least 2"),
                      (dict(k=0), "k = 0"), (dict(k=-4), "k = -4"), (dict(k=8), "k = 8"), (dict(idx=p, n_idx=3, k=3), "k = 3"),
                      (dict(cap=-1), "cap = -1"), (dict(cap=5), "pairs NULL"), (dict(lab=None, hits=p, cap=5, pairs=p), "hits needs labels")):
        rc, e = call(**kw)
        assert rc == -1 and "knn_graph" in e and cause in e, (kw, e)
    big = E.KNN_MAX_NIDX + 1
    rc, e = call(n=big, lds=big, ldl=big)
    assert rc == -3 and str(E.KNN_MAX_NIDX) in e and "knn_graph" in e
    rc, e = call(n=10 ** 6, lds=10 ** 6, ldl=10 ** 6, idx=p, n_idx=big)
    assert rc == -3 and str(E.KNN_MAX_NIDX) in e
    rc, e = call(n=2000, lds=2000, ldl=2000, k=E.KNN_MAX_K + 1)
    assert rc == -3 and str(E.KNN_MAX_K) in e and "knn_graph" in e
    assert call(n=big, lds=big - 1, ldl=big)[0] == -1                      # a bad argument is named before the capacity
    assert call(n=1025, lds=1025, ldl=1025, k=1025)[0] == -1               # k > m - 1 is a bad argument, not a capacity
    assert list(hd) == [-7] * 8
    with pytest.raises(pkg._lib.McgraNotSupported, match=str(E.KNN_MAX_K)):
        pkg._lib.check(call(n=2000, lds=2000, ldl=2000, k=E.KNN_MAX_K + 1)[0])


def test_engine_entry_refuses_without_a_device(pkg, monkeypatch):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for pred, real in ((wide, None), (sq, other), (sq, wide), (torch.zeros(5), None)):
        with pytest.raises(AssertionError):
            E.knn_graph.__wrapped__(pred, 2, None, real)
    with pytest.raises(ValueError, match="device tensors"):
        E.knn_graph(sq, 2)                                                # a host tensor: refused before anything is called
    # the refusals of the C entry reach the caller as exceptions that name the cause (no stream is needed to be refused)
    monkeypatch.setattr(E, "_stream", lambda: None)
    for k in (0, -1, 5, 6):
        with pytest.raises(pkg._lib.McgraError, match=f"k = {k}"):
            E.knn_graph.__wrapped__(sq, k, None, sq, lists=True, edges=True)
    with pytest.raises(pkg._lib.McgraError, match="at least 2"):
        E.knn_graph.__wrapped__(sq, 1, [3])
    with pytest.raises(pkg._lib.McgraNotSupported, match=str(E.KNN_MAX_NIDX)):
        E.knn_graph.__wrapped__(sq, 3, list(range(E.KNN_MAX_NIDX + 1)))      # the count is refused before an id is read


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_knn_is_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not hasattr(plain, "knn") and not hasattr(plain, "save_knn")
    args = p.parse_args(["--knn", "0", "--save_knn", "k.npz"])
    assert (args.knn, args.save_knn) == (0, "k.npz") and p.parse_args(["--knn", "12"]).knn == 12
    for argv, text in ((["--save_knn", "k.npz"], "--save_knn needs --knn"), (["--knn", "3", "--save_knn", ""], "path"),
                       (["--knn", "-1"], "K >= 0")):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    for mode in ("notrain_test", "prepare", "link_stealing"):
        with pytest.raises(SystemExit):
            p.parse_args(["--knn", "4", "--mode", mode])
        assert f"--mode evaluate only, not --mode {mode}" in capsys.readouterr().err
    assert "--knn" in M.__doc__ and "--save_knn" in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(knn=3, mode="prepare"), 0, 1)
    calls = []
    R.check_knn_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_knn_args(argparse.Namespace(knn=0, save_knn="x", mode="evaluate"), calls.append)
    assert calls == []


def test_knn_is_hidden_from_the_parameter_line_when_unset(pkg):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    args = M.build_parser().parse_args([])
    assert "knn" not in str(R.shown_parameters(args)) and str(R.shown_parameters(args)) == str(
        argparse.Namespace(**{q: v for q, v in vars(args).items() if q not in ("ap", "topk", "save_edges", "curves", "per_node",
                                                                              "binarize", "save_graph")}))
    text = str(R.shown_parameters(M.build_parser().parse_args(["--knn", "0"])))
    assert " knn=0" in text and "save_knn" not in text
    text = str(R.shown_parameters(M.build_parser().parse_args(["--knn", "3", "--save_knn", "k.npz"])))
    assert " knn=3" in text and " save_knn='k.npz'" in text


def test_the_report_table_is_extended_not_changed(pkg):
    from mc_gra_amd import reports as R
    assert R.EVALUATE_REPORTS[:len(R.REPORT_TABLE)] == R.REPORT_TABLE and len(R.EVALUATE_REPORTS) == len(R.REPORT_TABLE) + 1
    assert R.EVALUATE_REPORTS[-1].flags == ("knn", "save_knn") and R.REPORT_TABLE[-1].flags == ("ablate", "save_ablation")
    last = R.EVALUATE_REPORTS[-1]
    assert last.wanted(argparse.Namespace(knn=0)) and last.wanted(argparse.Namespace(knn=3)) and not last.wanted(argparse.Namespace())
    flags = [f for r in R.EVALUATE_REPORTS for f in r.flags]
    assert len(flags) == len(set(flags))
    src = open(os.path.join(ROOT, "mc-gra_amd", "main.py")).read()
    assert src.count("reports.EVALUATE_REPORTS") == 4 and "reports.REPORT_TABLE" not in src
    assert "EVALUATE_REPORTS" in R.__doc__


# ----------------------------------------------------------------------------------- the report, from the truth
def _fake_engine(monkeypatch, E):
    """engine.knn_graph and engine.topk_metrics as the truths, on host tensors."""
    import torch

    def knn_graph(pred, k, idx=None, real=None, lists=False, edges=False):
        g = T.ints(None if real is None else real.numpy(), pred.numpy(), k, idx)
        res = {"k": k, "nodes": len(g["in"])}
        res.update({q: g[q] for q in T.HEADER})
        res.update({q: torch.tensor(g[q]) for q in T.COLUMNS})
        res["stats"] = T.stats(g)
        if edges:
            pairs, scores, kind, hits = g["edges"]
            res.update({"pairs_list": torch.tensor(pairs), "scores": torch.tensor(scores), "kind": torch.tensor(kind),
                        "hits": torch.tensor(hits)})
        return res

    monkeypatch.setattr(E, "knn_graph", knn_graph)
    monkeypatch.setattr(E, "topk_metrics", lambda real, pred, k=None, idx=None: {
        q: v for q, v in TK.top_k(real.numpy(), pred.numpy(), k, idx).items() if q in ("k", "positives", "hits", "pairs", "f1")})


def test_the_report_text_and_file_from_the_truth(pkg, monkeypatch, tmp_path):
    import torch
    from mc_gra_amd import engine as E
    from mc_gra_amd import reports as R
    _fake_engine(monkeypatch, E)
    rng = np.random.RandomState(4)
    n = 40
    real = KC.graph(rng, n, 0.15)
    pred = (0.5 * real + rng.rand(n, n)).astype(np.float32)
    sets = {"attack": rng.permutation(n)[:30], "train": np.arange(5, 17), "all": None}
    path = str(tmp_path / "k.npz")
    ctx = R.RunContext(real=torch.tensor(real), inference_adj=torch.tensor(pred), sets=sets, n=n, rank=0, other=None, versus=None,
                       args=argparse.Namespace(knn=0, save_knn=path, mode="evaluate"))
    report = R.EVALUATE_REPORTS[-1]
    res = report.compute(ctx)
    assert sorted(res) == ["knn_all", "knn_attack", "knn_train"]
    for name, ix in sets.items():
        d = res[f"knn_{name}"]
        m = n if ix is None else len(ix)
        P = TK.top_k(real, pred, 0, ix)["positives"]
        g = T.ints(real, pred, T.k_of_mean_degree(m, P), ix)
        assert sorted(d) == sorted(["stats", "k", "nodes", "pairs", "positives", "global_f1_union", "global_f1_mutual", "columns"])
        assert (d["k"], d["nodes"], d["pairs"], d["positives"]) == (g["k"], m, m * (m - 1) // 2, P) and repr(d["stats"]) == repr(T.stats(g))
        assert d["global_f1_union"] == TK.top_k(real, pred, g["E_U"], ix)["f1"]
        assert d["global_f1_mutual"] == TK.top_k(real, pred, g["E_M"], ix)["f1"] and g["E_M"] > 0
    d = res["knn_all"]
    u, mu, hub = d["stats"]["union"], d["stats"]["mutual"], d["stats"]["hubness"]
    line = (f"k={d['k']} union f1={u['f1']} (edges={u['edges']}, isolated={u['isolated']}; global f1={d['global_f1_union']}) "
            f"mutual f1={mu['f1']} (edges={mu['edges']}, isolated={mu['isolated']}; global f1={d['global_f1_mutual']}) "
            f"max_in={hub['max_in']} orphans={hub['orphans']} skew={hub['skewness']}")
    assert report.console(res, ctx) == [f"current knn {line}"]
    log = report.log(res, ctx)
    assert len(log) == 3 and [l.split(":")[0] for l in log] == ["In attack graph", "In train graph", "In Whole Graph"]
    assert log[2].startswith(f"In Whole Graph: knn {line} | nodes={n} positives={d['positives']} lists P=")
    report.save(res, ctx)
    saved = np.load(path)
    assert sorted(saved.files) == sorted([f"{q}_{s}" for q in ("nodes", "k") + T.COLUMNS for s in sets] + ["pairs", "scores", "kind", "hits"])
    g = T.ints(real, pred, d["k"])
    assert np.array_equal(saved["pairs"], g["edges"][0]) and np.array_equal(saved["kind"], g["edges"][2])
    assert np.array_equal(saved["hits"], g["edges"][3]) and saved["in_all"].tolist() == g["in"] and int(saved["k_all"]) == d["k"]
    assert np.array_equal(saved["nodes_attack"], sets["attack"]) and np.array_equal(saved["nodes_all"], np.arange(n))
    # a zero edge count: the global F1 is NaN; a set above the capacity is refused by name
    monkeypatch.setattr(E, "knn_graph", lambda *a, **k: {**T.ints(real, pred, 1), "stats": T.stats(T.ints(real, pred, 1)), "k": 1,
                                                         "E_M": 0, **{q: torch.zeros(n) for q in T.COLUMNS}})
    assert math.isnan(report.compute(ctx)["knn_all"]["global_f1_mutual"])
    monkeypatch.setattr(E, "KNN_MAX_NIDX", 35)
    with pytest.raises(SystemExit, match="`all` has 40 nodes.*35"):
        report.compute(ctx)
    ctx_off = ctx._replace(args=argparse.Namespace(knn=3, mode="evaluate"))
    assert report.save(res, ctx_off) is None
