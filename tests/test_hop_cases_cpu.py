"""Without a GPU: the truth of the AUC by true-graph distance (tests/hop_truth.py) against the definition written as loops,
against networkx and scipy, against DeLong's and the graph-structure truths and against its own identities; that the inputs of
tests/test_gpu_hops.py (tests/hop_cases.py) have the properties they are named for and tell each wrong reading of the
definition from the right one; the host arithmetic of engine.hop_auc_stats and its NaN rules; the entry's device-free refusals;
main.py's --hops / --hops_cut / --save_hops checks."""
import argparse
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import delong_truth as DL
from tests import graph_structure_truth as GS
from tests import hop_cases as HC
from tests import hop_truth as T
from tests.delong_cases import pairs_of

CASES = HC.cases()
INF = float("inf")


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


@functools.lru_cache(maxsize=None)
def prep(name):
    real, pred, idx, _, _ = CASES[name]
    return T.prepare(real, pred, idx)


def rows(name, hops, thr):
    return T.rows_of(prep(name), hops, thr)


def selected(name):
    real, _, idx, _, _ = CASES[name]
    return len(real) if idx is None else len(idx)


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("name", [k for k in sorted(CASES) if selected(k) <= 66])
def test_truth_is_the_definition_written_as_loops(name):
    real, pred, idx, _, runs = CASES[name]
    for hops, thr in runs:
        assert rows(name, hops, thr) == T.loop_ints(real, pred, idx, hops, thr), (name, hops, thr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_distances_are_those_of_networkx_and_scipy(name):
    import networkx as nx
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    real, _, idx, _, _ = CASES[name]
    A = T.adjacency(real, idx)
    d = T.distances(A)
    sp = shortest_path(csr_matrix(A.astype(np.int8)), method="D", unweighted=True)
    assert np.array_equal(np.where(np.isinf(sp), -1, sp).astype(np.int64), d)
    assert np.array_equal(d, d.T) and np.array_equal(d == 1, A)
    lim = T.distances(A, 3)
    assert np.array_equal(lim, np.where(d > 3, -1, d))
    if len(A) <= 300:
        want = np.full_like(d, -1)
        for a, row in nx.shortest_path_length(nx.from_numpy_array(A)):
            for b, v in row.items():
                want[a, b] = v
        assert np.array_equal(want, d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_identities_and_the_neighbouring_truths(name):
    """sum count = m, count_1 = P; hops = 1 is DeLong's {P, N, T}; sum T_c is DeLong's T; raising H only splits beyond; the
    false positives are graph_structure's E_R - E_C."""
    real, pred, idx, _, runs = CASES[name]
    m = pairs_of(selected(name))
    dl = DL.ints(real, pred, idx)
    assert dl["pairs"] == m
    for hops, thr in runs:
        r = rows(name, hops, thr)
        assert len(r) == hops + 1 and sum(c[0] for c in r) == m and r[0][0] == dl["positives"]
        assert r[0][1] == sum(c[1] for c in r[1:]) == dl["T"]
        assert all(0 <= c[2] <= c[0] for c in r) and all(0 <= c[1] <= 2 * r[0][0] * c[0] for c in r[1:])
        if thr is not None and np.isfinite(thr):
            gs = GS.ints(real, pred, thr, idx)
            assert r[0][2] == gs["E_C"] and sum(c[2] for c in r[1:]) == gs["E_R"] - gs["E_C"]
    lab, s, _, place = prep(name)
    assert np.array_equal(place[~lab], DL.placements(lab, s)[1])           # the sorted route of the largest GPU inputs
    one = rows(name, 1, None)
    assert one == [[dl["positives"], dl["T"], 0], [dl["negatives"], dl["T"], 0]]
    for h in range(1, T.HOP_MAX):
        lo, hi = rows(name, h, 0.5), rows(name, h + 1, 0.5)
        assert lo[:h] == hi[:h] and lo[h] == [hi[h][q] + hi[h + 1][q] for q in range(3)]


def test_closed_form_of_the_capacity_case():
    """The circulant graph of offsets +-1, +-2 as scores and labels at once, at small odd and even n."""
    for n in (35, 37, 64, 71):
        c = HC.circulant(n)
        for hops in (1, 3, 8):
            assert T.ints(c, c, None, hops, 0.5) == T.circulant_rows(n, hops), (n, hops)
    assert T.circulant_rows(HC.MAX_NIDX, 3)[-1][1] < 2 ** 63


# ------------------------------------------------------------------------------- 2. what the cases are there for
def test_cases_have_the_properties_they_are_named_for():
    for m in HC.SIZES:
        for name in (f"m{m}", f"sub{m}"):
            real, pred, idx, pad, runs = CASES[name]
            assert selected(name) == m and (idx is None) == (name[0] == "m")
            assert {h for h, _ in runs} >= ({1, 3, 8} if idx is None else {3, 8})
            if idx is not None:
                assert pad > 0 and len(real) > m and len(set(idx.tolist())) == m and sorted(idx.tolist()) != idx.tolist()
    assert HC.words(63) == HC.words(64) == 1 and HC.words(65) == 2 and HC.words(129) == 3 and HC.words(257) == 5
    for name, (real, pred, idx, _, _) in CASES.items():
        if name != "asymmetric":                                           # nothing outside the selection is valid
            assert np.isnan(real).sum() == np.isnan(pred).sum() == real.size - pairs_of(selected(name)), name
    # the graphs: every class of the path holds pairs, beyond too; unreachable pairs; a hub; N = 0; P = 0; the wrap
    for hops in (1, 3, 8):
        assert all(c[0] > 0 for c in rows("path_n11", hops, 0.5))
    d = T.distances(T.adjacency(CASES["two_components"][0]))
    assert (d < 0).any() and (d > 8).any()
    star = rows("star_n70", 3, 0.5)
    assert [c[0] for c in star] == [69, pairs_of(70) - 69, 0, 0]
    assert rows("complete_n66", 3, -INF)[0][0] == pairs_of(66) and rows("empty_n66", 8, -INF)[-1][0] == pairs_of(66)
    assert [c[0] for c in rows("cycle_n17", 8, 0.5)] == [17] * 8 + [0]
    assert [c[0] for c in rows("cycle_n16", 8, 0.5)] == [16] * 7 + [8, 0]
    A = T.adjacency(CASES["hub_and_isolated"][0])
    assert A[5].sum() == 298 and A[23].sum() == 0
    per_word = T.adjacency(CASES["dense_n200"][0]).reshape(200, -1)[:, :192].reshape(200, 3, 64).sum(2)
    assert (per_word >= HC.BATCH).any() and (per_word % HC.BATCH != 0).any() and (per_word < HC.BATCH).any()
    # the scores: four levels, negative, signed zeros and subnormals
    for name, kind in (("m2", "levels4"), ("m3", "negative"), ("m63", "zeros"), ("m64", "random")):
        s = prep(name)[1]
        if kind == "levels4":
            assert set(s.tolist()) <= {0.0, 0.25, 0.5, 0.75}
        elif kind == "negative":
            assert (s < -0.9).all()
        elif kind == "zeros":
            w = s.view(np.uint32)
            assert {0x80000001, 0x80000000, 0, 1} == set(w.tolist())
    assert len(set(prep("m257")[1].tolist())) <= 4 and (prep("m127")[1] < 0).all()
    # the grids
    for name in ("sparse_n1100", "sparse_sub1054"):
        assert selected(name) - 1 > HC.ROW_BLOCKS and int(prep(name)[0].sum()) > HC.SORT_TILE
    assert HC.words(HC.SECOND_WORD_N) == HC.THREADS + 1 and HC.words(HC.MAX_NIDX) == 4 * HC.THREADS
    # the thresholds
    thrs = [t for _, t in CASES["thresholds"][4]]
    assert -INF in thrs and INF in thrs and None in thrs and 0.5 in set(prep("thresholds")[1].tolist())
    zero = [rows("signed_zeros", 3, t) for _, t in CASES["signed_zeros"][4]]
    assert zero[0] == zero[1] and zero[1] != zero[2] and zero[3] != zero[0]           # -0.0 >= +0.0 holds


def _walk_classes(A, hops):
    """For every pair the lengths h <= hops of which a walk of EXACTLY h edges joins it."""
    exact, step = [], np.eye(len(A), dtype=np.int64)
    for _ in range(hops):
        step = ((step @ A.astype(np.int64)) > 0).astype(np.int64)
        exact.append(step > 0)
    return exact


def test_each_wrong_reading_is_told_apart():
    a_, b_ = lambda m: np.tril_indices(m, -1)[0], lambda m: np.tril_indices(m, -1)[1]
    # a path through an unselected node: 0 - 1 - 2 with node 1 outside the selection
    real, pred, idx, _, _ = CASES["through_unselected"]
    full = T.distances(T.adjacency(HC.edges_graph(6, HC.THROUGH_EDGES)))
    sub = full[np.ix_(idx, idx)]
    own = T.distances(T.adjacency(real, idx))
    assert sub[1, 0] == 2 and own[1, 0] == -1 and rows("through_unselected", 3, 0.5)[1][0] == 0
    # ordered pairs or the diagonal: the upper triangle and the diagonal hold other labels and scores
    real, pred, _, _, _ = CASES["asymmetric"]
    n = len(real)
    r = rows("asymmetric", 3, 0.5)
    assert sum(c[0] for c in r) == pairs_of(n) and int((real == 1).sum()) not in (r[0][0], 2 * r[0][0])
    assert T.ints(real.T.copy(), pred.T.copy(), None, 3, 0.5) != r
    # walks instead of shortest paths: in the 5-cycle a pair two apart is also three apart the other way round
    A = T.adjacency(CASES["cycle_n5"][0])
    exact = _walk_classes(A, 3)
    counted = sum(int(e[a_(5), b_(5)].sum()) for e in exact)
    assert counted > pairs_of(5) and exact[1][2, 0] and exact[2][2, 0]
    assert [c[0] for c in rows("cycle_n5", 3, 0.5)] == [5, 5, 0, 0]
    # ties counted 0 or 2 instead of 1
    lab, s, d, place = prep("m257")
    pos, neg = s[lab], s[~lab]
    ties = int((pos[:, None] == neg[None, :]).sum())
    assert ties > 0 and int(place.sum()) == 2 * int((pos[:, None] > neg[None, :]).sum()) + ties
    # > instead of >= at the threshold
    lab, s, d, _ = prep("thresholds")
    assert int((s > np.float32(0.5)).sum()) < int((s >= np.float32(0.5)).sum()) == sum(c[2] for c in rows("thresholds", 3, 0.5))
    # distance taken in the recovered graph
    real, pred, _, _, _ = CASES["recovered_differs"]
    recovered = (_symmetric(pred) >= 0.5).astype(np.float32)
    np.fill_diagonal(recovered, 0)
    dr = T.distances(T.adjacency(recovered))
    dg = T.distances(T.adjacency(real))
    assert (dr != dg).any() and [int(((dr == k)[a_(50), b_(50)]).sum()) for k in (2, 3)] != [c[0] for c in rows("recovered_differs", 3, 0.5)[1:3]]
    # reach that is not cumulative: on a path an even-length walk leads back to a neighbour, never an odd one to a pair two apart
    A = T.adjacency(CASES["path_n11"][0])
    exact = _walk_classes(A, 3)
    assert exact[1][2, 0] and not exact[2][2, 0] and exact[0][1, 0] and not exact[1][1, 0] and exact[2][1, 0]
    wrong = 3 - sum(e[a_(11), b_(11)].astype(np.int64) for e in exact)              # levels counted as if they were nested
    assert np.bincount(wrong, minlength=4).tolist() != [c[0] for c in rows("path_n11", 3, 0.5)]


def _symmetric(lower_only):
    m = np.nan_to_num(np.asarray(lower_only, np.float32), nan=0.0)
    m = np.tril(m, -1)
    return m + m.T


# ---------------------------------------------------------------------------------------- 3. the host arithmetic
def test_hop_auc_stats_by_hand_and_its_nan_rules(pkg):
    from mc_gra_amd import engine as E
    isnan = math.isnan
    r = [(3, 40, 2), (4, 18, 3), (0, 0, 0), (10, 22, 1)]
    s = E.hop_auc_stats(r, 3, 0.5)
    assert (s["hops"], s["threshold"], s["pairs"], s["positives"], s["negatives"]) == (3, 0.5, 17, 3, 14)
    assert s["distance"] == (1, 2, 3, "beyond") and s["count"] == (3, 4, 0, 10) and s["T"] == (40, 18, 0, 22) and s["above"] == (2, 3, 0, 1)
    assert isnan(s["auc"][0]) and s["auc"][1] == 18 / 24 and isnan(s["auc"][2]) and s["auc"][3] == 22 / 60
    assert isnan(s["share"][0]) and s["share"][1:] == (4 / 14, 0.0, 10 / 14)
    assert isnan(s["fp_share"][0]) and s["fp_share"][1:] == (0.75, 0.0, 0.25)
    assert s["auc_pooled"] == 40 / 84 == float(Fraction(40, 84))                    # as delong_stats forms its "auc"
    assert s["ints"] == r and T.same(s, T.stats([list(c) for c in r], 3, 0.5))
    # the pooled AUC is the share-weighted mean of the class AUCs
    assert abs(sum(a * w for a, w in zip(s["auc"][1:], s["share"][1:]) if not isnan(a)) - s["auc_pooled"]) < 1e-15
    none = E.hop_auc_stats(r, 3)
    assert none["threshold"] is None and "above" not in none and "fp_share" not in none and none["auc"][1::2] == s["auc"][1::2]
    p0 = E.hop_auc_stats([(0, 0, 0), (6, 0, 2)], 1, 0.5)                  # P = 0
    assert isnan(p0["auc"][1]) and isnan(p0["auc_pooled"]) and p0["share"][1] == 1.0 and p0["fp_share"][1] == 1.0
    n0 = E.hop_auc_stats([(6, 0, 2), (0, 0, 0)], 1, 0.5)                  # N = 0
    assert isnan(n0["auc"][1]) and isnan(n0["auc_pooled"]) and isnan(n0["share"][1]) and isnan(n0["fp_share"][1])
    nofp = E.hop_auc_stats([(2, 8, 2), (4, 8, 0)], 1, 0.5)                # no false positives
    assert nofp["auc"][1] == 0.5 and isnan(nofp["fp_share"][1])
    for name, (_, _, _, _, runs) in CASES.items():
        for hops, thr in runs[:2]:
            assert T.same(E.hop_auc_stats(rows(name, hops, thr), hops, thr), T.stats(rows(name, hops, thr), hops, thr))
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="hops"):
            E.hop_auc_stats(r, bad)
    for bad in (r[:3], r + [(0, 0, 0)], [(3, 41, 2)] + r[1:], [(3, 40)] + r[1:], [(3, 40, -1)] + r[1:]):
        with pytest.raises(ValueError):
            E.hop_auc_stats(bad, 3)


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    s = "mcgra_hop_auc"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 11
    assert "#define MCGRA_HOP_MAX 8" in open(HEADER).read() and E.HOP_MAX == T.HOP_MAX == HC.HOP_MAX == 8
    assert callable(E.hop_auc) and hasattr(E.hop_auc, "__wrapped__")                                  # the device guard
    assert "mcgra_hop_auc" in E.hop_auc.__doc__ and "No device" in E.hop_auc_stats.__doc__


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcgra.h")


def test_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to out."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = -7

    def call(n=8, ldl=8, lds=8, idx=None, n_idx=None, lab=p, s=p, hops=3, thr=0.5, out=True):
        o = (ctypes.c_int64 * 27)(*([mark] * 27))
        rc = L.mcgra_hop_auc(None, n, lab, ldl, s, lds, idx, n if n_idx is None else n_idx, hops, thr, o if out else None)
        assert list(o) == [mark] * 27
        return rc

    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(lds=7), dict(ldl=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(s=None), dict(lab=None), dict(out=False), dict(thr=float("nan")), dict(hops=0),
               dict(hops=9), dict(hops=-1)):
        assert call(**kw) == -1 and b"hop_auc:" in L.mcgra_last_error(), kw
    assert call(thr=float("nan")) == -1 and b"NaN" in L.mcgra_last_error()
    assert call(hops=9) == -1 and b"hops = 9" in L.mcgra_last_error()
    big = HC.MAX_NIDX + 1
    assert call(n=big, lds=big, ldl=big) == -3 and b"65535" in L.mcgra_last_error()
    assert call(n=10 ** 6, lds=10 ** 6, ldl=10 ** 6, idx=p, n_idx=big) == -3
    assert call(n=big, lds=big - 1, ldl=big) == -1                            # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(call(n=big, lds=big, ldl=big))


def test_engine_entry_refuses_wrong_shapes_host_tensors_and_bad_hops(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for real, pred in ((wide, sq), (torch.zeros(5), sq), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.hop_auc.__wrapped__(real, pred)
    for hops in (0, 9, 2.5, None):
        with pytest.raises(ValueError, match="hops"):
            E.hop_auc.__wrapped__(sq, sq, None, hops)
    with pytest.raises(ValueError, match="device tensors"):
        E.hop_auc(sq, sq)                                                # a host tensor: refused before anything is called


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_hops_flags_are_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in ("hops", "hops_cut", "save_hops")) and "hops" not in str(plain)
    assert "hops" not in str(R.shown_parameters(plain))
    a = p.parse_args(["--hops", "3", "--hops_cut", "split", "--save_hops", "h.npz"])
    assert (a.hops, a.hops_cut, a.save_hops) == (3, "split", "h.npz")
    assert all(f" {k}=" in str(R.shown_parameters(a)) for k in ("hops", "hops_cut", "save_hops"))
    assert p.parse_args(["--hops", "1"]).hops == 1 and p.parse_args(["--hops", "8", "--hops_cut=-0.25"]).hops_cut == "-0.25"
    for bad in ("0", "9", "-2"):
        with pytest.raises(SystemExit):
            p.parse_args([f"--hops={bad}"])
        assert "H in [1, 8]" in capsys.readouterr().err
    for bad in ("", "Split", "nan", "inf"):
        with pytest.raises(SystemExit):
            p.parse_args(["--hops", "3", f"--hops_cut={bad}"])
        assert "`split`, `edges` or a finite threshold" in capsys.readouterr().err
    for flag, value in (("--hops_cut", "edges"), ("--save_hops", "h.npz")):
        with pytest.raises(SystemExit):
            p.parse_args([flag, value])
        assert f"{flag} needs --hops" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--hops", "3", "--save_hops", ""])
    assert ".npz" in capsys.readouterr().err
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--hops", "3", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err and "--hops" in err
    for flag in ("--hops", "--hops_cut", "--save_hops"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(hops=3, mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --hops"):
        M._run(argparse.Namespace(save_hops="h.npz", mode="evaluate"), 0, 1)
    calls = []
    R.check_hops_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_hops_args(argparse.Namespace(hops=2, hops_cut="0.5", save_hops="h.npz", mode="evaluate"), calls.append)
    assert calls == []
    assert [r.flags[0] for r in R.EVERY_REPORT] == [r.flags[0] for r in R.REPORTS] + ["hops"]


def test_report_text_and_file_of_a_result(pkg, tmp_path):
    """The console line, the log lines and the .npz that reports.py makes of hop_auc's dicts."""
    from mc_gra_amd import engine as E
    from mc_gra_amd import reports as R
    d = E.hop_auc_stats([(3, 40, 2), (4, 18, 3), (0, 0, 0), (10, 22, 1)], 3, 0.5)
    res = {f"hops_{k}": d for k in ("attack", "train", "all")}
    path = str(tmp_path / "h.npz")
    args = argparse.Namespace(hops=3, save_hops=path, mode="evaluate")
    ctx = R.Context(real=None, inference_adj=None, sets={"attack": None, "train": None, "all": None}, n=7, rank=0, other=None,
                    versus=None, args=args)
    rep = R.EVERY_REPORT[-1]
    assert rep.wanted(args) and not rep.wanted(argparse.Namespace(mode="evaluate"))
    assert rep.console(res, ctx) == [f"current auc_by_distance 2:0.75 3:nan beyond:{22 / 60} (pooled {40 / 84}) "
                                     "false positives at distance 2: 3/4"]
    log = rep.log(res, ctx)
    assert len(log) == 3 and log[2] == ("In Whole Graph: by true-graph distance at 0.5: 1: count=3 AUC=nan above=2 "
                                        f"2: count=4 AUC=0.75 above=3 3: count=0 AUC=nan above=0 beyond: count=10 AUC={22 / 60} above=1 "
                                        f"pooled AUC={40 / 84}")
    one = dict(res, hops_all=E.hop_auc_stats([(3, 40, 2), (14, 40, 4)], 1, 0.5))
    assert "false positives beyond distance 1: 4/4" in rep.console(one, ctx)[0]
    rep.save(res, ctx)
    saved = np.load(path)
    assert sorted(saved.files) == sorted(f"{k}_{s}" for k in ("distance", "count", "T", "above", "auc", "threshold")
                                         for s in ("attack", "train", "all"))
    assert saved["distance_all"].tolist() == [1, 2, 3, 0] and saved["T_all"].tolist() == [40, 18, 0, 22]
    assert saved["count_all"].dtype == saved["above_all"].dtype == np.int64 and saved["auc_all"].dtype == np.float64
    assert saved["threshold_all"].dtype == np.float32 and float(saved["threshold_all"]) == 0.5
