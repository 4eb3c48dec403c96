"""CPU-side checks of the DeLong entries (mcgra_auc_delong, mcgra_auc_delong_paired, engine.auc_delong / auc_delong_paired,
main.py --ci / --versus / --save_scores): the truth helper against a brute-force loop of the definition, against an
independently written float64 fast-DeLong (midranks, np.cov) and against sklearn's AUC; the resolving power of the inputs
tests/test_gpu_delong.py uses; the host arithmetic and its degenerate rules; the C ABI, its binding and every refusal that the
arguments alone decide (the pointers here are never followed); the command line.  No compute: there is no GPU here."""
import argparse
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import delong_cases as D
from tests import delong_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


CASES = D.cases()


@functools.lru_cache(maxsize=None)
def truth(name):
    real, pa, pb, idx, _ = CASES[name]
    return T.paired_ints(real, pa, pb, idx)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


# ---------------------------------------------------------------------------------------------------- truth helper
def _brute(lab, s):
    """The definition, pair by pair: every positive against every negative."""
    pos, neg = s[lab], s[~lab]
    lt = (neg[None, :] < pos[:, None])
    eq = (neg[None, :] == pos[:, None])
    a = [2 * int(lt[i].sum()) + int(eq[i].sum()) for i in range(len(pos))]
    b = [2 * int(lt[:, j].sum()) + int(eq[:, j].sum()) for j in range(len(neg))]       # neg_j < pos_i: that positive is above
    return a, b


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if D.pairs_of(len(v[0]) if v[3] is None else len(v[3])) <= 20000))
def test_truth_against_a_brute_force_loop_of_the_definition(name):
    real, pa, pb, idx, _ = CASES[name]
    g = truth(name)
    lab, sa = T.candidates(real, pa, idx)
    _, sb = T.candidates(real, pb, idx)
    (aa, ba), (ab, bb) = _brute(lab, sa), _brute(lab, sb)
    assert g["pairs"] == len(lab) and g["positives"] == len(aa) and g["negatives"] == len(ba)
    assert g["T_a"] == sum(aa) == sum(ba) and g["T_b"] == sum(ab) == sum(bb)
    assert g["A2_a"] == sum(x * x for x in aa) and g["B2_a"] == sum(x * x for x in ba)
    assert g["A2_b"] == sum(x * x for x in ab) and g["B2_b"] == sum(x * x for x in bb)
    assert g["A_ab"] == sum(x * y for x, y in zip(aa, ab)) and g["B_ab"] == sum(x * y for x, y in zip(ba, bb))
    one = T.ints(real, pa, idx)
    assert one == {"pairs": g["pairs"], "positives": g["positives"], "negatives": g["negatives"], "T": g["T_a"], "A2": g["A2_a"],
                   "B2": g["B2_a"]}


def test_exact_dot_against_python_integers():
    rng = np.random.RandomState(3)
    x, y = rng.randint(0, 2 ** 32, 1000, dtype=np.int64), rng.randint(0, 2 ** 32, 1000, dtype=np.int64)
    x[:3], y[:3] = 2 ** 32 - 1, 2 ** 32 - 1
    assert T.dot(x, y) == sum(int(a) * int(b) for a, b in zip(x, y)) > 2 ** 64


def _fast_delong(lab, scorings):
    """Sun and Xu's fast DeLong in float64: midranks (scipy.stats.rankdata), np.cov.  (aucs [k], covariance [k x k])."""
    from scipy.stats import rankdata
    m, n = int(lab.sum()), int((~lab).sum())
    v01, v10, aucs = [], [], []
    for s in scorings:
        s = s.astype(np.float64)
        pos, neg = s[lab], s[~lab]
        tx, ty, tz = rankdata(pos), rankdata(neg), rankdata(np.concatenate([pos, neg]))
        aucs.append(tz[:m].sum() / m / n - (m + 1.0) / 2.0 / n)
        v01.append((tz[:m] - tx) / n)
        v10.append(1.0 - (tz[m:] - ty) / m)
    return np.array(aucs), np.atleast_2d(np.cov(np.array(v01))) / m + np.atleast_2d(np.cov(np.array(v10))) / n


@pytest.mark.parametrize("name", sorted(CASES))
def test_truth_against_an_independent_float64_fast_delong_and_sklearn(name):
    """theta, both variances and the covariance to 1e-9 relative (the two agreed to 3e-16 at 400 samples; the margin covers
    float64 np.cov over millions of samples); theta against sklearn's trapezoid AUC, a float64 sum over at most m steps, to
    1e-9 absolute (m 2^-53 = 5e-10 at the largest case)."""
    from sklearn.metrics import roc_auc_score
    real, pa, pb, idx, _ = CASES[name]
    g = truth(name)
    st = T.paired_stats(g)
    if g["positives"] < 2 or g["negatives"] < 2:                        # no variance to compare (np.cov of one sample)
        assert math.isnan(st["a"]["var"]) and math.isnan(st["cov"]) and math.isnan(st["p_value"])
        return
    lab, sa = T.candidates(real, pa, idx)
    _, sb = T.candidates(real, pb, idx)
    aucs, cov = _fast_delong(lab, [sa, sb])
    P, N = g["positives"], g["negatives"]
    var_a = T.variance(P, N, g["T_a"], g["T_a"], g["A2_a"], g["B2_a"])
    var_b = T.variance(P, N, g["T_b"], g["T_b"], g["A2_b"], g["B2_b"])
    print(name, aucs, cov.tolist(), st)
    for got, want in ((aucs[0], st["a"]["auc"]), (aucs[1], st["b"]["auc"]), (cov[0, 0], float(var_a)), (cov[1, 1], float(var_b)),
                      (cov[0, 1], st["cov"])):
        assert math.isclose(got, want, rel_tol=1e-9, abs_tol=1e-18), (name, got, want)
    assert st["a"]["var"] == float(var_a) and st["b"]["var"] == float(var_b)
    if name.startswith("carry"):                                       # (the large case: the float64 comparison above is enough)
        return
    for s, key in ((sa, "a"), (sb, "b")):
        assert abs(roc_auc_score(lab, s.astype(np.float64)) - st[key]["auc"]) <= 1e-9, (name, key)


# ------------------------------------------------------------------------------------------------ resolving power
def _variant_ints(real, pa, pb, idx, how):
    """The integers under a wrong reading of the candidates or of the ties; None where that reading meets an invalid entry."""
    real, pa, pb = np.asarray(real), np.asarray(pa), np.asarray(pb)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx, np.int64)
    if how == "ordered_entries_with_the_diagonal":
        a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(len(ix)), np.arange(len(ix)), indexing="ij"))
    else:
        a, b = np.tril_indices(len(ix), -1)
    if how == "transposed_entry":
        a, b = b, a
    lab, sa, sb = real[ix[a], ix[b]], pa[ix[a], ix[b]], pb[ix[a], ix[b]]
    if not (np.all((lab == 0) | (lab == 1)) and np.all(np.isfinite(sa)) and np.all(np.isfinite(sb))):
        return None
    lab = lab == 1
    P = int(lab.sum())

    def place(s):
        pos, neg = s[lab], s[~lab]
        sp, sn = np.sort(pos), np.sort(neg)
        lt, le = np.searchsorted(sn, pos, "left").astype(np.int64), np.searchsorted(sn, pos, "right").astype(np.int64)
        gt, ge = P - np.searchsorted(sp, neg, "right").astype(np.int64), P - np.searchsorted(sp, neg, "left").astype(np.int64)
        if how == "ties_count_0":
            return 2 * lt, 2 * gt
        if how == "ties_count_1":
            return 2 * le, 2 * ge
        return lt + le, gt + ge

    (aa, ba), (ab, bb) = place(sa), place(sb)
    g = {"pairs": len(lab), "positives": P, "negatives": len(lab) - P, "T_a": int(aa.sum()), "T_b": int(ab.sum()),
         "A2_a": T.dot(aa, aa), "B2_a": T.dot(ba, ba), "A2_b": T.dot(ab, ab), "B2_b": T.dot(bb, bb), "A_ab": T.dot(aa, ab),
         "B_ab": T.dot(ba, bb)}
    if how == "high_limb_dropped":
        g = {k: v % 2 ** 64 for k, v in g.items()}
    return g


def _variant_stats(g, how):
    """The doubles under a wrong reading of the host formulas; None where they are undefined."""
    P, N = g["positives"], g["negatives"]
    if P < 2 or N < 2:
        return None

    def var(ta, tb, A, B):
        if how == "P_in_place_of_P_minus_1":
            return Fraction(P * A - ta * tb, 4 * N ** 2 * P ** 3) + Fraction(N * B - ta * tb, 4 * P ** 2 * N ** 3)
        return T.variance(P, N, ta, tb, A, B)

    va, vb = var(g["T_a"], g["T_a"], g["A2_a"], g["B2_a"]), var(g["T_b"], g["T_b"], g["A2_b"], g["B2_b"])
    cov = 0 if how == "cov_taken_as_0" else var(g["T_a"], g["T_b"], g["A_ab"], g["B_ab"])
    return float(va), float(vb), float(va + vb - 2 * cov)


INT_READINGS = ("ties_count_0", "ties_count_1", "ordered_entries_with_the_diagonal", "transposed_entry", "high_limb_dropped")
RATE_READINGS = ("P_in_place_of_P_minus_1", "cov_taken_as_0")


@pytest.mark.parametrize("how", INT_READINGS)
def test_the_cases_tell_each_wrong_reading_of_the_integers_from_the_truth(how):
    """At least one case on which the wrong reading is defined (meets no junk) and gives other integers."""
    small = sorted(k for k in CASES if truth(k)["pairs"] <= 200000)      # the large cases add nothing to the first four
    names = small + ["carry_n3000"] if how == "high_limb_dropped" else small
    told = [k for k in names if (lambda v: v is not None and v != truth(k))(_variant_ints(*CASES[k][:4], how))]
    print(how, told)
    assert told, how
    if how == "high_limb_dropped":
        assert told == ["carry_n3000"]
    if how == "transposed_entry":
        assert "asymmetric" in told and "subset_permuted" not in told


@pytest.mark.parametrize("how", RATE_READINGS)
def test_the_cases_tell_each_wrong_reading_of_the_rates_from_the_truth(how):
    told = []
    for k in sorted(CASES):
        right, wrong = _variant_stats(truth(k), None), _variant_stats(truth(k), how)
        if right is not None and right != wrong:
            told.append(k)
    print(how, told)
    assert "two_independent_scorings" in told and len(told) >= 10, how


def test_the_carry_case_really_carries():
    g = truth("carry_n3000")
    assert g["pairs"] == D.pairs_of(3000) and abs(g["positives"] / g["pairs"] - 0.5) < 0.01
    for k in ("A2_a", "B2_a", "A2_b", "B2_b", "A_ab", "B_ab"):
        assert g[k] >= 2 ** 64, k
    st = T.paired_stats(g)
    assert 0.88 < st["a"]["auc"] < 0.92 and 0.78 < st["b"]["auc"] < 0.82 and st["z"] > 5


def test_the_cases_hold_what_they_are_named_for():
    g = {k: truth(k) for k in CASES}
    st = {k: T.paired_stats(v) for k, v in g.items()}
    assert (g["n2_one_positive"]["positives"], g["n2_one_positive"]["negatives"]) == (1, 0)
    assert (g["n2_one_negative"]["positives"], g["n2_one_negative"]["negatives"]) == (0, 1)
    assert g["n3"]["pairs"] == 3 and g["n4"]["pairs"] == 6 and g["n3_one_positive"]["positives"] == 1
    assert math.isnan(st["n2_one_positive"]["a"]["auc"]) and math.isnan(st["n3_one_positive"]["a"]["var"])
    assert st["n3_one_positive"]["a"]["auc"] == 0.5
    e = st["n64_all_equal"]
    assert e["a"]["auc"] == 0.5 and e["a"]["var"] == 0.0 and e["a"]["se"] == 0.0 and e["a"]["ci_low"] == e["a"]["ci_high"] == 0.5
    assert e["delta"] == 0.0 and e["z"] == 0.0 and e["p_value"] == 1.0
    real, pa, pb, idx, _ = CASES["five_levels"]
    assert len(np.unique(T.candidates(real, pa, idx)[1])) == 5
    for name in ("zeros_subnormals_negatives", "signed_zeros_only"):
        real, pa, pb, idx, _ = CASES[name]
        w = T.candidates(real, pa, idx)[1].view(np.uint32)
        assert (w == 0x80000000).any() and (w == 0).any(), name
        lab = T.candidates(real, pa, idx)[0]
        assert lab[w == 0x80000000].any() and (~lab[w == 0]).any()           # a -0.0 positive ties a +0.0 negative
    w = T.candidates(*CASES["zeros_subnormals_negatives"][:2])[1].view(np.uint32)
    assert (w == 1).any() and (w == 0x80000001).any() and (w == 0x007fffff).any() and (w == 0xbfc00000).any()
    assert CASES["n257_ld288"][4] == 31
    real, pa, pb, idx, _ = CASES["junk_outside_selection"]
    off = np.ones(len(real), bool); off[idx] = False
    for mtx in (real, pa, pb):
        up = np.triu(np.ones(real.shape, bool))
        assert not np.isin(mtx[up], (0.0, 1.0)).all() and np.isnan(mtx[off]).any() and np.isinf(mtx[:, off]).any()
    real, pa, pb, idx, _ = CASES["asymmetric"]
    assert not np.array_equal(pa, pa.T) and not np.array_equal(pb, pb.T)
    a, b = CASES["subset_permuted"][3], CASES["subset_reordered"][3]
    assert sorted(a.tolist()) == sorted(b.tolist()) and not np.array_equal(a, b) and not np.array_equal(a, np.sort(a))
    assert g["subset_permuted"] == g["subset_reordered"]
    # paired relations
    s = st["b_equals_a"]
    assert g["b_equals_a"]["A_ab"] == g["b_equals_a"]["A2_a"] and s["cov"] == s["a"]["var"] > 0 and s["se_delta"] == 0.0
    assert s["delta"] == 0.0 and s["z"] == 0.0 and s["p_value"] == 1.0
    same = g["b_increasing_map_of_a"]
    assert same == g["b_equals_a"] and not np.array_equal(CASES["b_increasing_map_of_a"][1], CASES["b_increasing_map_of_a"][2])
    neg = g["b_minus_a"]
    assert neg["T_b"] == 2 * neg["positives"] * neg["negatives"] - neg["T_a"] and neg["T_b"] != neg["T_a"]
    ind = st["two_independent_scorings"]
    assert 0 < ind["cov"] < min(ind["a"]["var"], ind["b"]["var"]) and ind["z"] > 2 and 0 < ind["p_value"] < 0.05


def test_the_tiling_cases_sit_on_both_sides_of_the_kernels_constants():
    rows = sorted(D.TILING)
    assert rows == [D.THREADS + 1, D.THREADS + 2, D.ROW_BLOCKS + 1, D.ROW_BLOCKS + 2, 1448, 1449]
    assert D.pairs_of(1448) < 2 ** 20 < D.pairs_of(1449)
    for r in rows:
        g = truth(f"tiling_n{r}")
        assert g["pairs"] == D.pairs_of(r) and g["positives"] >= 2 and g["negatives"] > g["positives"]
    want = {"P1023": ("positives", D.SCAN_LANES - 1), "P1024": ("positives", D.SORT_TILE), "P1025": ("positives", D.SORT_TILE + 1),
            "N1024": ("negatives", D.SORT_TILE), "N1025": ("negatives", D.SORT_TILE + 1), "P256": ("positives", D.THREADS),
            "P257": ("positives", D.THREADS + 1), "P4096_ties": ("positives", D.STAGE), "P4097_ties": ("positives", D.STAGE + 1),
            "P4097_levels": ("positives", D.STAGE + 1), "P8193": ("positives", 2 * D.STAGE + 1),
            "P524288": ("positives", D.POS_BLOCKS * D.THREADS), "P524289": ("positives", D.POS_BLOCKS * D.THREADS + 1),
            "P1048576": ("positives", D.SORT_BLOCKS * D.SORT_TILE), "P1048577": ("positives", D.SORT_BLOCKS * D.SORT_TILE + 1)}
    assert sorted(want) == sorted(D.CLASS_SIZES)
    for name, (key, count) in want.items():
        assert truth("class_" + name)[key] == count, name
    for name in ("P4096_ties", "P4097_ties"):                  # one level: every search ends at 0 or at the class size
        real, pa, pb, idx, _ = CASES["class_" + name]
        assert len(np.unique(T.candidates(real, pa, idx)[1])) == 1 and truth("class_" + name)["negatives"] > D.STAGE
    real, pa, pb, idx, _ = CASES["class_P4097_levels"]
    lab, s = T.candidates(real, pa, idx)
    assert sorted(np.unique(s).tolist()) == [0.0, 0.5, 1.0] and min(np.bincount((s[lab] * 2).astype(int))) < D.STAGE


# ------------------------------------------------------------------------------------------- the host arithmetic
@pytest.mark.parametrize("level", [0.95, 0.5])
def test_engine_stats_equal_the_truth_bit_for_bit(pkg, level):
    from mc_gra_amd import engine as E
    for name in sorted(CASES):
        g = truth(name)
        got, want = E.delong_paired_stats(g, level), T.paired_stats(g, level)
        for key in T.PAIRED_RATES:
            assert _same(got[key], want[key]), (name, key, got[key], want[key])
        for s in ("a", "b"):
            for key in T.RATES:
                assert _same(got[s][key], want[s][key]), (name, s, key)
        one = {"pairs": g["pairs"], "positives": g["positives"], "negatives": g["negatives"], "T": g["T_a"], "A2": g["A2_a"], "B2": g["B2_a"]}
        single = E.delong_stats(one, level)
        assert all(_same(single[k], want["a"][k]) for k in T.RATES) and single["ints"] == one and single["level"] == level
        assert got["ints"] == g and got["level"] == level


def test_degenerate_host_rules(pkg):
    from mc_gra_amd import engine as E
    nan = math.isnan
    none = E.delong_paired_stats({"pairs": 1, "positives": 1, "negatives": 0, "T_a": 0, "T_b": 0, "A2_a": 0, "B2_a": 0, "A2_b": 0,
                                  "B2_b": 0, "A_ab": 0, "B_ab": 0})
    assert all(nan(none[k]) for k in T.PAIRED_RATES) and all(nan(none[s][k]) for s in "ab" for k in T.RATES)
    assert all(nan(E.delong_stats({"pairs": 3, "positives": 0, "negatives": 3, "T": 0, "A2": 0, "B2": 0})[k]) for k in T.RATES)
    # P == 1: the positive beats one of two negatives under A, both under B
    lab, sa, sb = np.array([1, 0, 0], bool), np.array([0.5, 0.25, 0.75], np.float32), np.array([0.9, 0.25, 0.75], np.float32)
    real, pa, pb = D.lower(lab, 3), D.lower(sa, 3), D.lower(sb, 3)
    one = E.delong_paired_stats(T.paired_ints(real, pa, pb))
    assert one["a"]["auc"] == 0.5 and one["b"]["auc"] == 1.0 and one["delta"] == -0.5
    assert all(nan(one[k]) for k in ("cov", "se_delta", "ci_low", "ci_high", "z", "p_value"))
    assert all(nan(one["a"][k]) for k in ("var", "se", "ci_low", "ci_high"))
    # var == 0: A separates the classes perfectly, B gives every pair one score
    lab = np.array([1, 1, 0, 0, 0, 1], bool)
    real, pa, pb = D.lower(lab, 4), D.lower(np.where(lab, 2.0, 1.0), 4), D.lower(np.full(6, 0.5), 4)
    d = E.delong_paired_stats(T.paired_ints(real, pa, pb))
    assert d["a"]["auc"] == 1.0 and d["a"]["var"] == 0.0 and d["a"]["se"] == 0.0 and d["a"]["ci_low"] == d["a"]["ci_high"] == 1.0
    assert d["b"]["auc"] == 0.5 and d["b"]["var"] == 0.0 and d["delta"] == 0.5 and d["se_delta"] == 0.0
    assert d["z"] == math.inf and d["p_value"] == 0.0 and d["ci_low"] == d["ci_high"] == 0.5
    r = E.delong_paired_stats(T.paired_ints(real, pb, pa))
    assert r["z"] == -math.inf and r["p_value"] == 0.0 and r["delta"] == -0.5
    same = E.delong_paired_stats(T.paired_ints(real, pa, pa))
    assert same["z"] == 0.0 and same["p_value"] == 1.0 and same["delta"] == 0.0
    # the interval is clipped to [0, 1]
    wide = E.delong_stats(T.ints(D.lower([1, 0, 1, 0, 1, 0], 4), D.lower([6, 1, 5, 2, 3, 4], 4)))
    assert wide["ci_high"] == 1.0 and 0.0 < wide["ci_low"] < wide["auc"] < 1.0
    for level in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            E.delong_stats(T.ints(real, pa), level)


def test_the_paired_variance_is_one_rational():
    """se_delta is the root of var_a + var_b - 2 cov rounded ONCE, not of the three doubles combined."""
    g = truth("two_independent_scorings")
    P, N = g["positives"], g["negatives"]
    va = T.variance(P, N, g["T_a"], g["T_a"], g["A2_a"], g["B2_a"])
    vb = T.variance(P, N, g["T_b"], g["T_b"], g["A2_b"], g["B2_b"])
    cov = T.variance(P, N, g["T_a"], g["T_b"], g["A_ab"], g["B_ab"])
    assert T.paired_stats(g)["se_delta"] == math.sqrt(float(va + vb - 2 * cov))


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entries_are_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    lib = ctypes.CDLL(LIB)
    for s, nargs in (("mcgra_auc_delong", 9), ("mcgra_auc_delong_paired", 11)):
        assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s)
        assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == nargs
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    for f in (E.auc_delong, E.auc_delong_paired):
        assert callable(f) and hasattr(f, "__wrapped__")                                                # the device guard
        assert "DeLong" in f.__doc__ and "1988" in f.__doc__ and "not independent" in f.__doc__ and "lower bound" in f.__doc__


def test_entries_refuse_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to out."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = 2 ** 64 - 7

    def single(n=8, ldl=8, lda=8, idx=None, n_idx=None, lab=p, sa=p, out=True, **_):
        o = (ctypes.c_uint64 * 8)(*([mark] * 8))
        rc = L.mcgra_auc_delong(None, n, lab, ldl, sa, lda, idx, n if n_idx is None else n_idx, o if out else None)
        assert list(o) == [mark] * 8
        return rc

    def paired(n=8, ldl=8, lda=8, ldb=8, idx=None, n_idx=None, lab=p, sa=p, sb=p, out=True):
        o = (ctypes.c_uint64 * 17)(*([mark] * 17))
        rc = L.mcgra_auc_delong_paired(None, n, lab, ldl, sa, lda, sb, ldb, idx, n if n_idx is None else n_idx, o if out else None)
        assert list(o) == [mark] * 17
        return rc

    shared = (dict(n=0), dict(n=-3), dict(n=1), dict(ldl=7), dict(lda=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
              dict(idx=p, n_idx=-5), dict(lab=None), dict(sa=None), dict(out=False))
    for kw in shared:
        assert single(**kw) == -1 and b"auc_delong:" in L.mcgra_last_error(), kw
    for kw in shared + (dict(ldb=7), dict(sb=None)):
        assert paired(**kw) == -1 and b"auc_delong_paired:" in L.mcgra_last_error(), kw
    big = 65536
    for f in (single, paired):
        assert f(n=big, ldl=big, lda=big, ldb=big) == -3 and b"65535" in L.mcgra_last_error()
        assert f(n=10 ** 6, ldl=10 ** 6, lda=10 ** 6, ldb=10 ** 6, idx=p, n_idx=big) == -3
        assert f(n=big, ldl=big, lda=big - 1, ldb=big) == -1                  # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(single(n=big, ldl=big, lda=big))


def test_engine_entries_refuse_wrong_shapes_host_tensors_and_levels(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for real, pred in ((wide, sq), (torch.zeros(5), sq), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.auc_delong.__wrapped__(real, pred)
        with pytest.raises(AssertionError):
            E.auc_delong_paired.__wrapped__(real, pred, sq)
    with pytest.raises(AssertionError):
        E.auc_delong_paired.__wrapped__(sq, sq, other)
    with pytest.raises(ValueError, match="device tensors"):
        E.auc_delong(sq, sq)                                             # a host tensor: refused before anything is called
    with pytest.raises(ValueError, match="device tensors"):
        E.auc_delong_paired(sq, sq, sq)
    for level in (0.0, 1.0, 2.0):
        with pytest.raises(ValueError, match="level"):
            E.auc_delong.__wrapped__(sq, sq, None, level)
        with pytest.raises(ValueError, match="level"):
            E.auc_delong_paired.__wrapped__(sq, sq, sq, None, level)


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_ci_flags_are_absent_by_default_and_evaluate_only(pkg, capsys, tmp_path):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in ("ci", "versus", "save_scores"))
    assert "ci" not in str(plain) and "versus" not in str(plain) and "save_scores" not in str(plain)
    a = p.parse_args(["--ci", "--versus", "features", "--save_scores", "s.npy"])
    assert a.ci is True and a.versus == "features" and a.save_scores == "s.npy"
    assert p.parse_args(["--save_scores", "s.npy"]).save_scores == "s.npy"      # needs no --ci
    with pytest.raises(SystemExit):
        p.parse_args(["--versus", "features"])
    assert "--versus needs --ci" in capsys.readouterr().err
    for flags in (["--ci"], ["--save_scores", "s.npy"]):
        for mode in ("notrain_test", "prepare"):
            with pytest.raises(SystemExit):
                p.parse_args(flags + ["--mode", mode])
            err = capsys.readouterr().err
            assert mode in err and "--mode evaluate only, not --mode" in err and flags[0] in err
    for flag in ("--ci", "--versus", "--save_scores"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(ci=True, mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --ci"):
        M._run(argparse.Namespace(versus="features", mode="evaluate"), 0, 1)
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(save_scores="s.npy", mode="notrain_test"), 0, 1)
    calls = []
    R.check_ci_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_ci_args(argparse.Namespace(ci=True, versus="x.npy", save_scores="s.npy", mode="evaluate"), calls.append)
    R.check_ci_args(argparse.Namespace(ci=True, mode="evaluate"), calls.append)
    assert calls == []
    R.check_ci_args(argparse.Namespace(ci=True, versus="", mode="evaluate"), calls.append)
    R.check_ci_args(argparse.Namespace(save_scores="", mode="evaluate"), calls.append)
    assert len(calls) == 2 and "features" in calls[0] and ".npy" in calls[1]
    # --versus PATH: a matrix of another shape, or no .npy at all, is refused by name
    path = str(tmp_path / "other.npy")
    np.save(path, np.zeros((4, 5), np.float32))
    with pytest.raises(SystemExit, match=r"other\.npy.*\(4, 5\).*7 x 7"):
        R.load_versus(path, 7)
    with pytest.raises(SystemExit, match=r"missing\.npy"):
        R.load_versus(str(tmp_path / "missing.npy"), 7)
    np.save(path, np.arange(49, dtype=np.float64).reshape(7, 7))
    t = R.load_versus(path, 7)
    assert tuple(t.shape) == (7, 7) and str(t.dtype) == "torch.float32" and float(t[6, 6]) == 48.0
