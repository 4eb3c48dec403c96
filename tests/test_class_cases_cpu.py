"""Without a GPU: the truth of the AUC within node classes (tests/class_truth.py) against the definition written as loops,
against DeLong's truth, sklearn's roc_auc_score, the graph-structure and threshold truths and against its own identities; that
the inputs of tests/test_gpu_class_auc.py (tests/class_cases.py) have the properties they are named for and tell each wrong
reading of the definition from the right one; the host arithmetic of engine.class_auc_stats and its NaN rules;
engine.class_strata; the entry's device-free refusals; main.py's --by_class / --by_class_cut / --save_by_class checks, the
class sources and the report's text and file."""
import argparse
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import class_cases as CC
from tests import class_truth as T
from tests import delong_truth as DL
from tests import graph_structure_truth as GS
from tests import two_means_truth as TM
from tests.delong_cases import pairs_of

CASES = CC.cases()
INF = float("inf")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcgra.h")


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


@functools.lru_cache(maxsize=None)
def prep(name):
    real, pred, classes, idx, _, _, _ = CASES[name]
    return T.prepare(real, pred, classes, idx)


def rows(name, C, how, thr, brute=None):
    table, names = T.strata(C, how)
    return T.rows_of(prep(name), table, len(names), thr, CASES[name][6] if brute is None else brute)


def selected(name):
    real, _, _, idx, _, _, _ = CASES[name]
    return len(real) if idx is None else len(idx)


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("name", [k for k in sorted(CASES) if pairs_of(selected(k)) <= 40] + ["wrong_readings", "single_node_class"])
def test_truth_is_the_definition_written_as_loops(name):
    real, pred, classes, idx, _, runs, _ = CASES[name]
    for C, how, thr in runs:
        table, names = T.strata(C, how)
        assert rows(name, C, how, thr) == T.loop_ints(real, pred, classes, idx, table, len(names), thr), (name, C, how, thr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_identities_and_the_neighbouring_truths(name):
    """sum pairs_g = m, sum P_g = P, hits_g <= min(P_g, above_g); `one` is DeLong's {m, P, T}; stratum c of `own` is DeLong's
    truth on the selected nodes of class c alone; sklearn's roc_auc_score per stratum; sum above and sum hits are the recovered
    and the shared edges of the graph-structure truth and the pairs of the threshold truth; the sorted route is the brute one."""
    from sklearn.metrics import roc_auc_score
    real, pred, classes, idx, _, runs, brute = CASES[name]
    m = pairs_of(selected(name))
    dl = DL.ints(real, pred, idx)
    lab, s, ca, cb = prep(name)
    sel = np.arange(len(real)) if idx is None else idx
    for C, how, thr in runs:
        table, names = T.strata(C, how)
        r = rows(name, C, how, thr)
        assert len(r) == len(names) and sum(c[0] for c in r) == m == dl["pairs"] and sum(c[1] for c in r) == dl["positives"]
        assert all(0 <= c[4] <= min(c[1], c[3]) and c[3] <= c[0] and 0 <= c[2] <= 2 * c[1] * (c[0] - c[1]) for c in r)
        if selected(name) <= 300:
            assert r == rows(name, C, how, thr, True) == rows(name, C, how, thr, False)
        if how == "one":
            assert r[0][:3] == [m, dl["positives"], dl["T"]]
        if how == "own":
            for c in range(C):
                nodes = sel[classes[sel] == c]
                want = DL.ints(real, pred, nodes) if len(nodes) >= 2 else {"pairs": 0, "positives": 0, "T": 0}
                assert r[c][:3] == [want["pairs"], want["positives"], want["T"]], (name, c)
        g_of = np.asarray(table)[ca, cb]
        for g, c in enumerate(r):
            if c[1] and c[0] - c[1]:
                at = g_of == g
                assert abs(roc_auc_score(lab[at], s[at].astype(np.float64)) - c[2] / (2 * c[1] * (c[0] - c[1]))) < 1e-12
        if thr is not None and np.isfinite(thr):
            gs = GS.ints(real, pred, thr, idx)
            assert sum(c[3] for c in r) == gs["E_R"] and sum(c[4] for c in r) == gs["E_C"]
        if thr is not None:
            _, _, hits = TM.threshold_pairs(real, pred, thr, idx)
            assert (sum(c[3] for c in r), sum(c[4] for c in r)) == (len(hits), int(hits.sum()))


def test_closed_form_of_the_capacity_case():
    """The circulant graph of offsets +-1, +-2 as scores and labels at once with the classes v mod 16, at small n."""
    table, names = T.strata(16, "blocks")
    for n in (35, 37, 64, 71, 160):
        c = CC.circulant(n)
        assert T.ints(c, c, np.arange(n) % 16, None, table, 136, 0.5) == T.circulant_rows(n, 16), n
    big = T.circulant_rows(CC.MAX_NIDX, 16)
    assert sum(r[0] for r in big) == pairs_of(CC.MAX_NIDX) and sum(r[1] for r in big) == 2 * CC.MAX_NIDX
    assert any(r[1] == 0 for r in big) and any(r[1] > 0 for r in big) and max(r[2] for r in big) < 2 ** 63    # e.g. block 0-0 has no edge


# ------------------------------------------------------------------------------- 2. what the cases are there for
def test_cases_have_the_properties_they_are_named_for():
    for m in CC.SIZES:
        for C in CC.CS:
            for name in (f"m{m}_c{C}", f"sub{m}_c{C}"):
                real, pred, classes, idx, pad, runs, brute = CASES[name]
                assert selected(name) == m and (idx is None) == (name[0] == "m") and brute
                assert [(c, h) for c, h, _ in runs] == [(C, h) for h in T.HOWS]
                sel = np.arange(len(real)) if idx is None else idx
                assert 0 <= classes[sel].min() and classes[sel].max() < C and (m < 63 or len(set(classes[sel].tolist())) > C // 2)
                if idx is not None:
                    assert pad > 0 and len(real) > m and len(set(idx.tolist())) == m and sorted(idx.tolist()) != idx.tolist()
                    rest = np.setdiff1d(np.arange(len(real)), idx)
                    assert set(classes[rest].tolist()) == set(CC.OUTSIDE) and all(not 0 <= c < 16 for c in CC.OUTSIDE)
    assert len(T.strata(16, "blocks")[1]) == CC.STRATA_MAX == 136
    full = rows("m257_c16", 16, "blocks", 0.5)
    assert all(c[0] > 0 for c in full)                                      # all 136 strata hold pairs
    for name, (real, pred, _, _, _, _, _) in CASES.items():
        assert np.isnan(real).sum() == np.isnan(pred).sum() == real.size - pairs_of(selected(name)), name
    # the layouts
    own = rows("single_node_class", 3, "own", 0.5)
    assert own[2] == [0, 0, 0, 0, 0] and own[0][0] > 0 and rows("single_node_class", 3, "blocks", 0.5)[5] == [0, 0, 0, 0, 0]
    blocks = rows("no_edges_no_non_edges", 3, "blocks", 0.5)
    assert blocks[0][0] == blocks[0][1] > 0 and blocks[4][1] == 0 < blocks[4][0]          # 0-0: N_g = 0; 1-2: P_g = 0
    assert all(c[0] == c[1] and c[2] == 0 for c in rows("complete_n66", 7, "blocks", 0.5))
    assert all(c[1] == 0 and c[2] == 0 and c[3] == c[0] for c in rows("empty_n66", 7, "blocks", -INF))
    # more edges than samples: a stride of 3; segment ends off the stride; segments shorter than a stride, one of one edge
    for name, C in (("dense_n200_c3", 3), ("dense_n200_c16", 16)):
        r = rows(name, C, "blocks", 0.5)
        P = sum(c[1] for c in r)
        stride = -(-P // CC.STAGE)
        assert P > 2 * CC.STAGE and stride == 3
        ends = np.cumsum([c[1] for c in r])[:-1]
        assert (ends % stride != 0).any()
        if C == 16:
            assert any(0 < c[1] < stride for c in r) and r[135][:2] == [1, 1]
    # the scores: four levels with equal keys in different strata, negative, signed zeros and subnormals
    lab, s, ca, cb = prep("dense_n200_levels")
    assert set(s.tolist()) <= {0.0, 0.25, 0.5, 0.75}
    assert (prep("negative")[1] < -0.9).all()
    assert {0x80000001, 0x80000000, 0, 1} == set(prep("signed_zeros")[1].view(np.uint32).tolist())
    zero = [rows("signed_zeros", 4, "blocks", t) for _, _, t in CASES["signed_zeros"][5][:4]]
    assert zero[0] == zero[1] and zero[1] != zero[2] and zero[3] != zero[0]              # -0.0 >= +0.0 holds
    thrs = [t for _, _, t in CASES["thresholds"][5]]
    assert -INF in thrs and INF in thrs and None in thrs and 0.5 in set(prep("thresholds")[1].tolist())
    # the grids
    for name in ("sparse_n1100", "sparse_sub1054"):
        assert selected(name) - 1 > CC.ROW_BLOCKS and int(prep(name)[0].sum()) > CC.SORT_TILE and not CASES[name][6]
    # a wave meets more strata than it counts together, and as few
    assert len(T.strata(7, "blocks")[1]) > CC.SHARED_BINS >= len(T.strata(7, "same")[1])


def test_each_wrong_reading_is_told_apart():
    real, pred, classes, idx, _, _, _ = CASES["wrong_readings"]
    lab, s, ca, cb = prep("wrong_readings")
    table, names = T.strata(3, "blocks")
    G = len(names)
    tab = np.asarray(table)
    g_of = tab[ca, cb]
    right = rows("wrong_readings", 3, "blocks", 0.5)
    # a non-edge searched among ALL edges
    b_all = DL.placements(lab, s)[1]
    assert [int(b_all[g_of[~lab] == g].sum()) for g in range(G)] != [c[2] for c in right]
    # a key that ties across two strata counted: equal keys of an edge and a non-edge sit in different strata
    pos, neg = np.nonzero(lab)[0], np.nonzero(~lab)[0]
    across = (s[pos][:, None] == s[neg][None, :]) & (g_of[pos][:, None] != g_of[neg][None, :])
    inside = (s[pos][:, None] == s[neg][None, :]) & (g_of[pos][:, None] == g_of[neg][None, :])
    assert across.any() and inside.any()
    with_foreign_ties = [c[2] + int(across[:, g_of[neg] == g].sum()) for g, c in enumerate(right)]
    assert with_foreign_ties != [c[2] for c in right]
    # ties counted 0 or 2 instead of 1
    above = (s[pos][:, None] > s[neg][None, :]) & (g_of[pos][:, None] == g_of[neg][None, :])
    assert sum(c[2] for c in right) == 2 * int(above.sum()) + int(inside.sum())
    # the class taken by position instead of by idx[a]
    by_position = T.rows_of((lab, s, classes[np.tril_indices(len(idx), -1)[0]] % 3, classes[np.tril_indices(len(idx), -1)[1]] % 3),
                            table, G, 0.5)
    assert by_position != right
    # the stratum taken from one endpoint
    assert T.rows_of((lab, s, ca, ca), table, G, 0.5) != right and T.rows_of((lab, s, cb, cb), table, G, 0.5) != right
    # > for >= at the threshold
    assert int((s > np.float32(0.5)).sum()) < int((s >= np.float32(0.5)).sum()) == sum(c[3] for c in right)
    # hits counting the non-edges above the threshold, or every candidate above it
    assert [int(((s >= np.float32(0.5)) & ~lab & (g_of == g)).sum()) for g in range(G)] != [c[4] for c in right]
    assert [c[3] for c in right] != [c[4] for c in right]
    # the pooled AUC is not the within-stratum one
    dl = DL.ints(real, pred, idx)
    assert sum(c[2] for c in right) != dl["T"]


# ---------------------------------------------------------------------------------------- 3. the host arithmetic
def test_class_auc_stats_by_hand_and_its_nan_rules(pkg):
    from mc_gra_amd import engine as E
    isnan = math.isnan
    r = [(10, 4, 40, 5, 3), (6, 0, 0, 1, 0), (3, 3, 0, 3, 3), (0, 0, 0, 0, 0), (20, 2, 10, 0, 0)]
    s = E.class_auc_stats(r, ("a", "b", "c", "d", "e"), 0.5)
    assert (s["names"], s["threshold"], s["pairs"]) == (("a", "b", "c", "d", "e"), 0.5, 39)
    assert s["count"] == (10, 6, 3, 0, 20) and s["positives"] == (4, 0, 3, 0, 2) and s["negatives"] == (6, 6, 0, 0, 18)
    assert s["T"] == (40, 0, 0, 0, 10) and s["above"] == (5, 1, 3, 0, 0) and s["hits"] == (3, 0, 3, 0, 0)
    assert s["auc"][0] == 40 / 48 and s["auc"][4] == 10 / 72 and all(isnan(s["auc"][g]) for g in (1, 2, 3))
    assert s["pair_share"] == (10 / 39, 6 / 39, 3 / 39, 0.0, 20 / 39) and s["edge_share"] == (4 / 9, 0.0, 3 / 9, 0.0, 2 / 9)
    assert s["precision"][:3] == (3 / 5, 0.0, 1.0) and isnan(s["precision"][3]) and isnan(s["precision"][4])
    assert s["recall"][0] == 0.75 and isnan(s["recall"][1]) and s["recall"][2] == 1.0 and isnan(s["recall"][3]) and s["recall"][4] == 0.0
    assert s["auc_within"] == 50 / 120
    assert s["auc_adjusted"] == float((4 * Fraction(40, 48) + 2 * Fraction(10, 72)) / 6)
    assert s["ints"] == r and T.same(s, T.stats([list(c) for c in r], ("a", "b", "c", "d", "e"), 0.5))
    none = E.class_auc_stats(r)
    assert none["threshold"] is None and none["names"] == ("0", "1", "2", "3", "4") and none["auc"][0] == s["auc"][0]
    assert not any(k in none for k in ("above", "hits", "precision", "recall"))
    dead = E.class_auc_stats([(0, 0, 0, 0, 0), (5, 0, 0, 0, 0)], None, 0.5)              # no stratum with an AUC, no edge at all
    assert isnan(dead["auc_within"]) and isnan(dead["auc_adjusted"]) and isnan(dead["edge_share"][0]) and dead["pair_share"] == (0.0, 1.0)
    assert isnan(E.class_auc_stats([(0, 0, 0, 0, 0)], None, 0.5)["pair_share"][0])
    # auc_adjusted is ONE Fraction rounded once, on every case; the dict is the truth's
    for name, (_, _, _, _, _, runs, _) in CASES.items():
        if selected(name) > 300:
            continue
        for C, how, thr in runs[:2] + runs[-1:]:
            names = T.strata(C, how)[1]
            rr = rows(name, C, how, thr)
            got = E.class_auc_stats(rr, names, thr)
            assert T.same(got, T.stats(rr, names, thr))
            live = [c for c in rr if c[1] and c[0] - c[1]]
            if live:
                exact = sum(Fraction(c[1]) * Fraction(c[2], 2 * c[1] * (c[0] - c[1])) for c in live) / sum(c[1] for c in live)
                assert got["auc_adjusted"] == float(exact)
    for bad in ([], [(1, 0, 0, 0)], [(3, 4, 0, 0, 0)], [(3, 1, 5, 0, 0)], [(3, 1, 0, 1, 2)], [(3, 1, 0, 0, 1)], [(3, 1, 0, 0, -1)],
                [(1, 0, 0, 0, 0)] * 137):
        with pytest.raises(ValueError):
            E.class_auc_stats(bad)
    with pytest.raises(ValueError, match="names"):
        E.class_auc_stats(r, ("a", "b"))


def test_class_strata(pkg):
    from mc_gra_amd import engine as E
    assert E.CLASS_MAX == T.CLASS_MAX == CC.CLASS_MAX == 16 and E.STRATA_MAX == T.STRATA_MAX == 136
    assert "#define MCGRA_CLASS_MAX 16" in open(HEADER).read()
    for C in (1, 2, 7, 16):
        for how, G in (("one", 1), ("same", 2), ("own", C + 1), ("blocks", C * (C + 1) // 2)):
            table, names = E.class_strata(C, how)
            want, want_names = T.strata(C, how)
            assert table.dtype == np.uint8 and table.shape == (C, C) and table.tolist() == want and names == want_names
            assert len(names) == G and np.array_equal(table, table.T) and table.max() < G
            if how != "one" and C > 1:
                assert set(table.ravel().tolist()) == set(range(G))
    assert E.class_strata(3, "blocks")[0].tolist() == [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    assert E.class_strata(3, "own")[0].tolist() == [[0, 3, 3], [3, 1, 3], [3, 3, 2]]
    assert E.class_strata(1, "same")[1] == ("same", "different") and E.class_strata(1, "own")[0].tolist() == [[0]]
    for C in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="classes"):
            E.class_strata(C, "same")
    with pytest.raises(ValueError, match="how"):
        E.class_strata(3, "Same")


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    s = "mcgra_class_auc"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 14
    assert callable(E.class_auc) and hasattr(E.class_auc, "__wrapped__")                              # the device guard
    assert "mcgra_class_auc" in E.class_auc.__doc__ and "No device" in E.class_auc_stats.__doc__


def test_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to out."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = -7
    good = np.asarray(T.strata(3, "blocks")[0], np.uint8)

    def call(n=8, ldl=8, lds=8, idx=None, n_idx=None, lab=p, s=p, cl=p, C=3, table=good, G=6, thr=0.5, out=True):
        o = (ctypes.c_int64 * 40)(*([mark] * 40))
        t = None if table is None else np.ascontiguousarray(table, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        rc = L.mcgra_class_auc(None, n, lab, ldl, s, lds, idx, n if n_idx is None else n_idx, cl, C, t, G, thr, o if out else None)
        assert list(o) == [mark] * 40
        return rc

    lop = good.copy()
    lop[2, 0] = 4
    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(lds=7), dict(ldl=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(s=None), dict(lab=None), dict(out=False), dict(cl=None), dict(table=None),
               dict(thr=float("nan")), dict(C=0), dict(C=17), dict(C=-1), dict(G=0), dict(G=137), dict(G=5), dict(table=lop),
               dict(C=2, table=np.asarray([[0, 1], [2, 0]]), G=3), dict(C=1, table=np.asarray([[1]]), G=1)):
        assert call(**kw) == -1 and b"class_auc:" in L.mcgra_last_error(), kw
    assert call(thr=float("nan")) == -1 and b"NaN" in L.mcgra_last_error()
    assert call(C=17) == -1 and b"n_class = 17" in L.mcgra_last_error()
    assert call(table=lop) == -1 and b"symmetric" in L.mcgra_last_error()
    assert call(G=5) == -1 and b"below 5" in L.mcgra_last_error()
    full = np.asarray(T.strata(16, "blocks")[0], np.uint8)
    big = CC.MAX_NIDX + 1
    assert call(n=big, lds=big, ldl=big, C=16, table=full, G=136) == -3 and b"65535" in L.mcgra_last_error()
    assert call(n=10 ** 6, lds=10 ** 6, ldl=10 ** 6, idx=p, n_idx=big) == -3
    assert call(n=big, lds=big - 1, ldl=big) == -1                            # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(call(n=big, lds=big, ldl=big))


def test_engine_entry_refuses_misuse_on_the_host(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    cl = [0, 1, 2, 0, 1]
    for real, pred in ((wide, sq), (torch.zeros(5), sq), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.class_auc.__wrapped__(real, pred, cl)
    for bad, what in ((cl[:4], "shape"), ([[0, 1, 2, 0, 1]], "shape"), ([0.0, 1, 2, 0, 1], "integers"), ([True] * 5, "integers"),
                      ([0, 1, -1, 0, 1], "class -1"), ([0, 1, 16, 0, 1], "at most 16"), (torch.tensor(cl).float(), "integers")):
        with pytest.raises(ValueError, match=what):
            E.class_auc.__wrapped__(sq, sq, bad)
    with pytest.raises(ValueError, match="how"):
        E.class_auc.__wrapped__(sq, sq, cl, None, "blocs")
    for table in (np.zeros((2, 3), np.uint8), np.zeros(4, np.uint8), np.zeros((17, 17), np.uint8)):
        with pytest.raises(ValueError, match="table"):
            E.class_auc.__wrapped__(sq, sq, cl, None, (table, ("a",)))
    with pytest.raises(ValueError, match="device tensors"):
        E.class_auc(sq, sq, cl)                                          # a host tensor: refused before anything is called


# ---------------------------------------------------------------------------------------------------- command line
FLAGS = ("by_class", "by_class_cut", "save_by_class")


def test_parser_by_class_flags_are_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in FLAGS) and "by_class" not in str(plain)
    assert "by_class" not in str(R.shown_parameters(plain))
    hidden = argparse.Namespace(**vars(plain), by_class_cut="split", save_by_class="c.npz")        # the report is off: all hidden
    assert "by_class" not in str(R.shown_parameters(hidden))
    a = p.parse_args(["--by_class", "labels", "--by_class_cut", "split", "--save_by_class", "c.npz"])
    assert (a.by_class, a.by_class_cut, a.save_by_class) == ("labels", "split", "c.npz")
    assert all(f" {k}=" in str(R.shown_parameters(a)) or f"({k}=" in str(R.shown_parameters(a)) for k in FLAGS)
    assert "hops" not in str(R.shown_parameters(a))
    assert p.parse_args(["--by_class", "degree"]).by_class == "degree" and p.parse_args(["--by_class", "x.npy", "--by_class_cut=-0.25"]).by_class_cut == "-0.25"
    for bad in ("", "Split", "nan", "inf"):
        with pytest.raises(SystemExit):
            p.parse_args(["--by_class", "labels", f"--by_class_cut={bad}"])
        assert "`split`, `edges` or a finite threshold" in capsys.readouterr().err
    for flag, value in (("--by_class_cut", "edges"), ("--save_by_class", "c.npz")):
        with pytest.raises(SystemExit):
            p.parse_args([flag, value])
        assert f"{flag} needs --by_class" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--by_class", "labels", "--save_by_class", ""])
    assert ".npz" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--by_class", ""])
    assert "`labels`, `degree`" in capsys.readouterr().err
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--by_class", "labels", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err and "--by_class" in err
    for flag in ("--by_class", "--by_class_cut", "--save_by_class"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(by_class="labels", mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --by_class"):
        M._run(argparse.Namespace(save_by_class="c.npz", mode="evaluate"), 0, 1)
    calls = []
    R.check_by_class_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_by_class_args(argparse.Namespace(by_class="degree", by_class_cut="0.5", save_by_class="c.npz", mode="evaluate"), calls.append)
    assert calls == []
    assert R.ALL_REPORTS[:len(R.EVERY_REPORT)] == R.EVERY_REPORT and [r.flags for r in R.ALL_REPORTS[len(R.EVERY_REPORT):]] == [FLAGS]
    assert R.Context._fields[-1] == "classes" and R.Context._field_defaults == {"classes": None}


def test_class_sources(pkg, tmp_path):
    import torch
    from mc_gra_amd import reports as R
    assert R.degree_classes([0, 1, 2, 3, 4, 7, 8, 2 ** 14 - 1, 2 ** 14, 2 ** 15, 2 ** 20]).tolist() == [0, 1, 2, 2, 3, 3, 4, 14, 15, 15, 15]
    n = 6
    adj = torch.zeros(n, n)
    for a, b in ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2)):
        adj[a, b] = adj[b, a] = 1
    labels = torch.tensor([2, 0, 1, 1, 0, 2])
    assert R.node_classes("labels", labels, adj).tolist() == [2, 0, 1, 1, 0, 2] and R.node_classes("labels", labels, adj).dtype == np.int64
    assert R.node_classes("degree", labels, adj).tolist() == [3, 2, 2, 1, 1, 0]
    path = str(tmp_path / "c.npy")
    np.save(path, np.asarray([0, 15, 3, 3, 1, 0], np.int32))
    assert R.node_classes(path, labels, adj).tolist() == [0, 15, 3, 3, 1, 0]
    for bad, what in ((np.asarray([0, 16, 3, 3, 1, 0]), "at most 16"), (np.asarray([0, -1, 3, 3, 1, 0]), "at most 16"),
                      (np.zeros(5, np.int64), "shape"), (np.zeros((6, 1), np.int64), "shape"), (np.zeros(6, np.float32), "dtype"),
                      (np.zeros(6, bool), "dtype")):
        np.save(path, bad)
        with pytest.raises(SystemExit, match=what):
            R.node_classes(path, labels, adj)
    with pytest.raises(SystemExit, match="not a readable .npy"):
        R.node_classes(str(tmp_path / "missing.npy"), labels, adj)
    with pytest.raises(SystemExit, match="at most 16"):
        R.node_classes("labels", torch.arange(17)[:n] + 12, adj)


def test_report_text_and_file_of_a_result(pkg, tmp_path):
    """The console line, the log lines and the .npz that reports.py makes of class_auc's dicts."""
    from mc_gra_amd import engine as E
    from mc_gra_amd import reports as R
    same = E.class_auc_stats([(10, 4, 40, 5, 3), (26, 2, 30, 1, 1)], ("same", "different"), 0.5)
    blocks = E.class_auc_stats([(4, 1, 6, 2, 1), (26, 2, 30, 1, 1), (6, 3, 9, 3, 2)], ("0-0", "0-1", "1-1"), 0.5)
    d = {"source": "labels", "classes": 2, "threshold": 0.5, "auc_pooled": 0.625, "same": same, "blocks": blocks,
         "homophily": {"true": 4 / 6, "recovered": 5 / 6, "pairs": 10 / 36}}
    res = {f"by_class_{k}": d for k in ("attack", "train", "all")}
    path = str(tmp_path / "c.npz")
    args = argparse.Namespace(by_class="labels", save_by_class=path, mode="evaluate")
    classes = np.asarray([0, 1, 1, 0, 1, 0, 1, 1, 0])
    ctx = R.Context(real=None, inference_adj=None, sets={"attack": None, "train": None, "all": None}, n=9, rank=0, other=None,
                    versus=None, args=args, classes=classes)
    rep = R.ALL_REPORTS[-1]
    assert rep.wanted(args) and not rep.wanted(argparse.Namespace(mode="evaluate"))
    text = (f"same-class AUC={40 / 48} different-class AUC={30 / 96} within blocks={45 / (6 + 96 + 18)} "
            f"adjusted={float((Fraction(6, 6) + 2 * Fraction(30, 96) + 3 * Fraction(9, 18)) / 6)} (pooled 0.625) "
            f"same-class share: true edges={4 / 6} recovered={5 / 6} pairs={10 / 36}")
    assert rep.console(res, ctx) == [f"current auc_by_class {text}"]
    log = rep.log(res, ctx)
    assert len(log) == 3 and log[2] == f"In Whole Graph: by class (labels, 2 classes) at 0.5: {text}"
    assert log[0].startswith("In attack graph: ") and log[1].startswith("In train graph: ")
    rep.save(res, ctx)
    saved = np.load(path)
    keys = ("class_i", "class_j", "count", "positives", "T", "above", "hits", "auc", "same_ints", "threshold")
    assert sorted(saved.files) == sorted([f"{k}_{s}" for k in keys for s in ("attack", "train", "all")] + ["classes"])
    assert saved["class_i_all"].tolist() == [0, 0, 1] and saved["class_j_all"].tolist() == [0, 1, 1]
    assert saved["T_all"].tolist() == [6, 30, 9] and saved["count_all"].dtype == saved["hits_all"].dtype == np.int64
    assert saved["auc_all"].dtype == np.float64 and saved["auc_all"].tolist() == list(blocks["auc"])
    assert saved["same_ints_all"].dtype == np.int64 and saved["same_ints_all"].tolist() == [[10, 4, 40, 5, 3], [26, 2, 30, 1, 1]]
    assert saved["threshold_all"].dtype == np.float32 and float(saved["threshold_all"]) == 0.5
    assert saved["classes"].dtype == np.int64 and saved["classes"].tolist() == classes.tolist()
    unsaved = argparse.Namespace(by_class="labels", mode="evaluate")
    assert rep.save(res, ctx._replace(args=unsaved)) is None
