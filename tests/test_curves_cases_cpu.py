"""CPU-side checks of the curve entry (mcgra_rank_curves, engine.roc_curve / precision_recall_curve / rank_curves, main.py
--curves): tests/curve_truth.py IS sklearn on every input tests/test_gpu_curves.py uses, those inputs have the properties the
cases are there for, the C ABI and its binding, every refusal that the arguments alone decide (the pointers here are never
followed), and the command line.  No compute: there is no GPU here."""
import ctypes
import os

import numpy as np
import pytest

from tests import curve_truth as T

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
def G():
    from tests import test_gpu_curves as G
    return G


# ------------------------------------------------------------------------------------------- the truth is sklearn
def test_curve_truth_equals_sklearn_on_every_gpu_case(G):
    """thresholds and rates by array_equal (NaN where sklearn has NaN), with drop_intermediate on and off."""
    for name in sorted(G.CASES):
        for drop in (True, False):
            t = G.truth(name, drop)
            (fpr, tpr, thr), (prec, rec, pthr) = T.sklearn_curves(*G.CASES[name], drop_intermediate=drop)
            assert t["counts"][3] == len(fpr) and t["counts"][4] == len(pthr), (name, drop)
            for got, want, what in ((t["fpr"], fpr, "fpr"), (t["tpr"], tpr, "tpr"), (t["roc"][2], thr, "roc thresholds"),
                                    (t["precision"], prec, "precision"), (t["recall"], rec, "recall"),
                                    (t["pr_thresholds"], pthr, "pr thresholds")):
                assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (name, drop, what)
            assert t["roc"][2].dtype == thr.dtype == np.float32 and t["fpr"].dtype == fpr.dtype == np.float64
            print(f"{name} drop={drop}: (P, N, levels, ROC points, PR points) = {t['counts']} best {t['best']}")


def test_truth_helper_on_a_case_worked_by_hand(G):
    """n4_f1_tie: scores 3 | 2 2 2 2 | 1 x5 | 0 x6 with positives at 3, one of the 2s and one of the 1s."""
    t = G.truth("n4_f1_tie", True)
    assert t["counts"] == (3, 13, 4, 5, 4)
    assert t["roc"][0].tolist() == [0, 1, 2, 3, 3] and t["roc"][1].tolist() == [0, 0, 3, 7, 13]
    assert t["roc"][2].tolist() == [np.inf, 3, 2, 1, 0]
    assert t["best"] == (1, 0, 0)                                 # F1 = 1/2 at level 0 and at level 1: the higher threshold
    assert T.f1_ties(*T.levels(*G.CASES["n4_f1_tie"])[:2]) == 2
    e = T.curves(*G.CASES["n4_f1_tie"], elements=True)
    assert e["counts"][2] == 16
    z = T.levels(np.array([[1, 0], [0, 1]], np.float32), np.array([[-0.0, 0.0], [1e-45, -1.0]], np.float32))
    assert z[2].tolist() == [float(np.float32(1e-45)), 0.0, -1.0] and not np.signbit(z[2][1]) and z[0].tolist() == [0, 1, 2] and z[1].tolist() == [1, 2, 2]


# --------------------------------------------------------------------------------- the inputs of the GPU test cases
def test_the_gpu_cases_cover_the_shapes_and_families(G):
    C = G.CASES
    assert set(G.TIE_FREE + G.TIED + G.QUANTISED + G.DEGENERATE) == set(C)
    lv = {k: G.truth(k, True)["counts"][2] for k in C}
    assert lv["n40_distinct"] == 1600 > 1024 and lv["n70_distinct"] == 4900 and lv["n70_distinct_subset"] == 900
    assert lv["n70_quant8"] == 8 and 3 <= lv["n70_quant8_repeats"] <= 8
    assert lv["n20_one_level"] == 1 and lv["n20_two_levels"] == 2 and lv["n4_f1_tie"] == 4
    assert 515 * 515 > 1024 * 256 and lv["n515_uniform"] > 1024 * 256 - 10000     # more tiles of levels than the scan has lanes
    assert lv["n1000_sparse"] > 900000
    for k in ("n20_no_positive", "n20_no_negative"):
        c = G.truth(k, True)["counts"]
        assert (c[0] == 0) != (c[1] == 0)
    # the zeros case: one level of more than 4000 entries holding both zeros, a subnormal level, negative levels
    real, pred, _ = C["n70_zeros"]
    bits = pred.view(np.uint32)
    assert (bits == 0x80000000).sum() > 100 and (bits == 0).sum() > 100 and (pred == 0).sum() > 4000
    assert bits[0, 0] == 0x80000000 and 0 < pred[0, 1] < 1e-38 and pred[0, 2] == -0.5 and (pred < 0).sum() > 10
    tps, fps, thr = T.levels(real, pred)
    at = int(np.flatnonzero(thr == 0)[0])
    assert (tps[at] - tps[at - 1]) + (fps[at] - fps[at - 1]) == (pred == 0).sum() and thr[at - 1] == np.float32(1e-42)
    # selections: a repeat-free subset, a shuffled permutation of all nodes, repeats
    assert len(set(C["n70_distinct_subset"][2].tolist())) == 30
    perm = C["n70_zeros_permuted"][2]
    assert sorted(perm.tolist()) == list(range(70)) and perm.tolist() != list(range(70))
    rep = C["n70_quant8_repeats"][2]
    assert len(rep) == 50 and len(set(rep.tolist())) < 50
    assert G.truth("n70_zeros_permuted", True)["counts"] == G.truth("n70_zeros", True)["counts"]


def test_each_case_tells_the_rules_apart(G):
    """A case that cannot tell a wrong reading from the right one proves nothing.  Every tie-free and every tied case: drop on
    and off give different point sets, and the ROC keep mask differs from the PR keep mask; every tied and every quantised case:
    counting entries instead of levels changes the answer.  (The quantised cases have eight levels with positives and
    negatives on each: all of them are corners of both curves, so drop_intermediate drops nothing there -- they are there
    for levels that span blocks.)"""
    for name in G.TIE_FREE + G.TIED:
        on, off = G.truth(name, True), G.truth(name, False)
        assert on["counts"][3] < off["counts"][3] and on["counts"][4] < off["counts"][4], name
        assert off["counts"][3] == off["counts"][2] + 1 and off["counts"][4] == off["counts"][2], name
        assert not np.array_equal(on["keep_roc"], on["keep_pr"]), name
    for name in G.QUANTISED:
        on = G.truth(name, True)
        assert on["keep_roc"].all() and on["keep_pr"].all(), name
    for name in G.TIED + G.QUANTISED:
        if name == "n1000_sparse":
            continue                                         # (a million entry-levels: the other tied cases tell it already)
        a, e = G.truth(name, True), T.curves(*G.CASES[name], drop_intermediate=True, elements=True)
        assert e["counts"][2] > a["counts"][2], name
        assert e["counts"][3:] != a["counts"][3:] or not np.array_equal(e["roc"][0], a["roc"][0]), name


def test_kept_and_dropped_levels_sit_on_both_sides_of_block_and_tile_edges(G):
    """Over the set of cases, for the ROC and for the PR rule: a kept and a dropped interior level at a level index that is
    the last of a 256-lane block (255 mod 256), the first of the next (0 mod 256, index >= 256), the last of a 1024-level
    stretch (1023 mod 1024) and the first of the next (0 mod 1024, index >= 1024)."""
    seen = {}
    for name in G.TIE_FREE + G.TIED:
        t = G.truth(name, True)
        L = t["counts"][2]
        l = np.arange(L)
        interior = (l > 0) & (l < L - 1)
        for rule in ("keep_roc", "keep_pr"):
            for mod, res in ((256, 255), (256, 0), (1024, 1023), (1024, 0)):
                at = interior & (l % mod == res) & (l >= mod - 1)
                for kept in (True, False):
                    if (t[rule][at] == kept).any():
                        seen.setdefault((rule, mod, res, kept), []).append(name)
    want = [(rule, mod, res, kept) for rule in ("keep_roc", "keep_pr") for mod, res in ((256, 255), (256, 0), (1024, 1023), (1024, 0))
            for kept in (True, False)]
    missing = [w for w in want if w not in seen]
    assert not missing, missing


def test_the_best_f1_tie_rule_matters_in_a_case(G):
    tied = [name for name in G.CASES if G.truth(name, True)["best"] is not None and T.f1_ties(*T.levels(*G.CASES[name])[:2]) > 1]
    print("cases with two levels of equal best F1:", tied)
    assert "n4_f1_tie" in tied
    tps, fps, _ = T.levels(*G.CASES["n4_f1_tie"])
    assert G.truth("n4_f1_tie", True)["best"][2] == 0 and 2 * tps[1] * (tps[0] + fps[0] + 3) == 2 * tps[0] * (tps[1] + fps[1] + 3)


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_rank_curves_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    lib = ctypes.CDLL(LIB)
    s = "mcgra_rank_curves"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s)
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(pkg._lib.lib.mcgra_rank_curves.argtypes) == 19
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    from mc_gra_amd import engine as E
    for f in ("roc_curve", "precision_recall_curve", "rank_curves"):
        assert callable(getattr(E, f)) and hasattr(getattr(E, f), "__wrapped__"), f      # the device guard


def test_rank_curves_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    counts = (ctypes.c_int64 * 5)()
    best = (ctypes.c_int64 * 3)()
    thr = ctypes.c_float()

    def call(n=8, ldl=8, lds=8, idx=None, n_idx=None, drop=1, cap=100, roc=(p, p, p), pr=(p, p, p), out=counts, b=best,
             t=ctypes.byref(thr), lab=p, sc=p):
        return L.mcgra_rank_curves(None, n, lab, ldl, sc, lds, idx, n if n_idx is None else n_idx, drop, cap, *roc, *pr, out, b, t)

    none = (None, None, None)
    for kw in (dict(out=None), dict(roc=none, pr=none, b=None), dict(roc=none, pr=none, b=None, t=None), dict(cap=-1),
               dict(ldl=7), dict(lds=7), dict(n=0), dict(lab=None), dict(sc=None), dict(idx=p, n_idx=0),
               dict(roc=(p, None, p)), dict(pr=(None, p, p)), dict(roc=(p, p, None), pr=none)):
        assert call(**kw) == -1 and b"rank_curves" in L.mcgra_last_error(), kw
    big = 65536
    assert call(n=big, ldl=big, lds=big) == -3 and b"65535" in L.mcgra_last_error()
    assert call(idx=p, n_idx=big) == -3
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(call(idx=p, n_idx=big, roc=none))
    assert list(counts) == [0] * 5 and list(best) == [0] * 3 and thr.value == 0.0       # nothing was written


def test_engine_entries_refuse_wrong_shapes_before_touching_a_device(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for f in (E.roc_curve, E.precision_recall_curve, E.rank_curves):
        for real, pred in ((wide, wide), (sq, other), (sq, wide), (torch.zeros(5), sq)):
            with pytest.raises(AssertionError):
                f.__wrapped__(real, pred)
        with pytest.raises(ValueError):
            f(sq, sq)                                                 # host tensors: refused by the device guard
    assert E._curve_first_cap(100, False) == 101 and E._curve_first_cap(100, True) == 101
    assert E._curve_first_cap(10 ** 8, True) == 10 ** 8 // 8 and E._curve_first_cap(4 * 10 ** 6, True) == 1 << 20 and E._curve_first_cap(10 ** 8, False) == 10 ** 8 + 1


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_curves_is_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    p = M.build_parser()
    assert p.parse_args([]).curves is None
    assert p.parse_args(["--curves", "c.npz"]).curves == "c.npz"
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--curves", "c.npz", "--mode", mode])
        assert mode in capsys.readouterr().err
    assert "--curves" in M.__doc__
    import argparse
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(curves="c.npz", mode="prepare"), 0, 1)
