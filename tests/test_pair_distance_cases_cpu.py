"""The truth and the cases of the link-stealing pair distances (tests/pair_distance_truth.py, tests/pair_distance_cases.py),
and everything of the feature that needs no GPU: symbols, refusals before any device call, the command line."""
import argparse
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

from tests import pair_distance_cases as Cs
from tests import pair_distance_truth as T
from tests.test_cabi_symbols import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


# ------------------------------------------------------------------------------------------------- the truth
@pytest.mark.parametrize("metric", T.METRICS)
def test_truth_is_cdist_and_the_literal_definition(metric):
    rng = np.random.RandomState(3)
    Z = (rng.randn(9, 5) * 0.8 + 0.3).astype(np.float32)
    ref = cdist(Z.astype(np.float64), Z.astype(np.float64), metric)
    assert np.allclose(T.dist64(Z, metric), ref, rtol=0, atol=1e-12)
    assert np.allclose(T.loop_dist(Z, metric), ref, rtol=0, atol=1e-12)
    for fma in (True, False):
        d32 = T.dist32(Z, metric, fma)
        assert d32.dtype == np.float32 and np.array_equal(d32, d32.T)           # the chains commute bitwise
        assert np.allclose(d32, ref, rtol=0, atol=2e-6)
    assert np.array_equal(T.scores64(Z, metric), 0.0 - T.dist64(Z, metric))


def test_truth_degenerate_rules_by_hand():
    Z = np.array([[0, 0, 0, 0], [2, 2, 2, 2], [1, 0, 0, 0], [0, 3, 0, 1]], np.float32)
    for f in (T.dist64, lambda Z, m: T.dist32(Z, m).astype(np.float64), T.loop_dist):
        cos = f(Z, "cosine")
        assert np.all(cos[0] == 1.0) and np.all(cos[:, 0] == 1.0)                # a zero row: distance 1 from everything, itself too
        assert abs(cos[1, 2] - 0.5) < 1e-6 and abs(cos[2, 3]) == 1.0             # <(1,1,1,1)/2, e_0> = 1/2; orthogonal rows
    for f in (T.dist64, lambda Z, m: T.dist32(Z, m).astype(np.float64)):
        cor = f(Z, "correlation")
        assert np.all(cor[0] == 1.0) and np.all(cor[1] == 1.0) and np.all(cor[:, 1] == 1.0)      # constant rows
        assert np.all(f(np.array([[1.5], [-2.0], [0.0]], np.float32), "correlation") == 1.0)    # d = 1: every row is constant
        can = f(Z, "canberra")
        assert can[0, 0] == 0.0 and can[0, 2] == 1.0 and can[2, 3] == 3.0        # both-zero coordinates add 0; |1-0|/1 + 3/3 + 0 + 1/1
        bc = f(Z, "braycurtis")
        assert bc[0, 0] == 0.0 and bc[0, 2] == 1.0                               # 0 / 0 -> 0
        anti = f(np.array([[1, -1], [-1, 1]], np.float32), "braycurtis")
        assert anti[0, 1] == 0.0 and anti[0, 0] == 0.0                           # |a + b| sums to zero: 4 / 0 -> 0
    # a constant row whose float32 sum does not round to d times its value is still centred to exact zeros
    odd = np.full((2, 7), np.float32(0.1))
    odd[1, 3] = 0.3
    assert np.all(T.dist32(odd, "correlation")[0] == 1.0)


def test_rank_ints_are_the_definition():
    rng = np.random.RandomState(0)
    v = rng.randint(0, 5, 60)
    l = rng.randint(0, 2, 60)
    ints = T.rank_ints(v.tolist(), l)
    t = sum(2 * int((v[l == 0] < s).sum()) + int((v[l == 0] == s).sum()) for s in v[l == 1])
    assert ints == {"pairs": 60, "positives": int(l.sum()), "negatives": int(60 - l.sum()), "T": t}
    S = rng.rand(6, 6)
    lab = (rng.rand(6, 6) < 0.5).astype(np.float32)
    vals, labs = T.lower_pairs(S, lab, [4, 1, 5])
    assert vals.tolist() == [S[1, 4], S[5, 4], S[5, 1]] and labs.tolist() == [lab[1, 4], lab[5, 4], lab[5, 1]]


# ------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("metric", T.METRICS)
@pytest.mark.parametrize("n", (65, 257))
def test_known_answer_cases_are_exact_in_any_order(metric, n):
    lab, Z, exact = Cs.known_case(metric, n)
    assert Z.shape[0] == n and np.array_equal(lab, lab.T) and not lab.diagonal().any()
    d64 = T.dist64(Z, metric)
    for fma in (True, False):                       # every partial result is a small integer (or its exact quotient / root)
        d32 = T.dist32(Z, metric, fma).astype(np.float64)
        if metric in ("cosine", "correlation"):
            assert np.array_equal(d32 * 16, exact.astype(np.float64))
        elif metric == "euclidean":
            assert np.array_equal(d32, np.sqrt(exact.astype(np.float64)).astype(np.float32))
        elif metric == "braycurtis":
            assert np.array_equal(d32, np.array([[np.float32(float(v)) for v in r] for r in exact], np.float64))
        else:
            assert np.array_equal(d32, exact.astype(np.float64))
    assert np.allclose(d64, d32, rtol=1e-6, atol=1e-7)
    if metric == "cosine":
        assert np.all((Z * Z).sum(1) == 16)
    if metric == "correlation":
        assert np.all(Z.sum(1) == 0) and np.all(np.abs(Z) == 1)
    _, _, frac, ints = Cs.known_auc(metric, n)
    assert Fraction(1, 2) < frac < 1, frac
    assert ints["pairs"] == n * (n - 1) // 2 and ints["positives"] == int(np.tril(lab, -1).sum())
    if metric == "euclidean":                       # its ranks are sqeuclidean's: sqrt is strictly monotone on these integers
        assert frac == Cs.known_auc("sqeuclidean", n)[2]
        assert len(set(np.sqrt(np.arange(0, 97, dtype=np.float32)).tolist())) == 97


def test_braycurtis_known_quotients_are_far_apart():
    """Any two distinct exact quotients of the case differ by more than 2^-18 relative: a division a few ulp off cannot
    reorder them."""
    for n in (65, 257):
        _, _, exact = Cs.known_case("braycurtis", n)
        q = sorted(set(exact.reshape(-1).tolist()))
        assert len(q) > 20
        for a, b in zip(q, q[1:]):
            assert a == 0 or (b - a) / b > Fraction(1, 2 ** 18), (a, b)


# ------------------------------------------------------------------------------------------------- accuracy cases
@pytest.fixture(scope="module")
def accuracy_aucs():
    out = {}
    for name in Cs.ACCURACY:
        lab, Z, s64 = Cs.accuracy_case(name)
        out[name] = {m: float(T.exact_auc(s64[m], lab)[0]) for m in T.METRICS}
    return out


@pytest.mark.parametrize("name", list(Cs.ACCURACY))
def test_accuracy_cases_meet_the_condition_of_the_gpu_tolerance(name, accuracy_aucs):
    """The GPU test may hold the AUC to float64 within 1e-6 only on inputs where the float32 chains and float64 agree within
    1e-7 here; the materialised float32 scores stay inside the a-priori bound of DESIGN.md."""
    lab, Z, s64 = Cs.accuracy_case(name)
    n, d = Z.shape
    assert (n, d) == tuple(int(v) for v in re.findall(r"\d+", name)) and abs(np.tril(lab, -1).sum() / (n * (n - 1) / 2) - 0.12) < 0.01
    kap = Cs.kappa(Z)
    assert kap < 5.0                                # the correlation bound stays meaningful
    for m in T.METRICS:
        s32 = 0.0 - T.dist32(Z, m).astype(np.float64)
        auc32 = float(T.exact_auc(s32, lab)[0])
        print(f"{name} {m}: auc64={accuracy_aucs[name][m]!r} |auc32 - auc64|={abs(auc32 - accuracy_aucs[name][m]):.3e}")
        assert abs(auc32 - accuracy_aucs[name][m]) <= 1e-7, (m, auc32, accuracy_aucs[name][m])
        assert 0.55 < accuracy_aucs[name][m] < 0.95
        kind, b = Cs.score_bound(m, d, kap)
        err = np.abs(s32 - s64[m])
        assert np.all(err <= b * (np.abs(s64[m]) if kind == "rel" else 1.0)), (m, kind, b, err.max())
        assert b < 1e-4


def test_resolving_power_of_the_accuracy_cases(accuracy_aucs):
    """Which metrics the AUC alone cannot tell apart (float64 AUCs closer than 1e-4): exactly euclidean / sqeuclidean (the same
    ranks) and, on softmax rows, braycurtis / cityblock (the denominator is the constant 2).  The materialised values tell
    them apart, and so does a non-normalised input."""
    for name, aucs in accuracy_aucs.items():
        close = {(a, b) for i, a in enumerate(T.METRICS) for b in T.METRICS[i + 1:] if abs(aucs[a] - aucs[b]) < 1e-4}
        want = {("euclidean", "sqeuclidean")} | ({("braycurtis", "cityblock")} if name in Cs.SOFTMAX else set())
        assert close == want, (name, close)
        _, Z, s64 = Cs.accuracy_case(name)
        assert np.abs(s64["euclidean"] - s64["sqeuclidean"]).max() > 0.1
        assert np.abs(s64["braycurtis"] - s64["cityblock"]).max() > 0.1
    assert abs(accuracy_aucs["randn_257x16"]["braycurtis"] - accuracy_aucs["randn_257x16"]["cityblock"]) > 1e-3


# ------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg._lib
    new = ["mcgra_pair_distance_rank_metrics", "mcgra_pair_distance_scores", "mcgra_pair_metric_name"]
    assert sorted(L.SYMBOLS) == header_symbols() and all(s in L.SYMBOLS and hasattr(L.lib, s) for s in new)
    assert L.lib.mcgra_pair_distance_scores.argtypes is not None and L.lib.mcgra_pair_distance_rank_metrics.restype is ctypes.c_int
    # one table: the header's ids, the library's names, _lib's and engine's tuple, the truth's
    hdr = open(os.path.join(ROOT, "include", "mcgra.h")).read()
    ids = dict(re.findall(r"#define MCGRA_PAIR_([A-Z]+) (\d+)", hdr))
    assert int(ids.pop("METRICS")) == 8 == len(L.PAIR_METRICS)
    assert tuple(k.lower() for k, _ in sorted(ids.items(), key=lambda kv: int(kv[1]))) == L.PAIR_METRICS == T.METRICS
    assert tuple(L.lib.mcgra_pair_metric_name(i).decode() for i in range(8)) == L.PAIR_METRICS
    assert L.lib.mcgra_pair_metric_name(8) is None and L.lib.mcgra_pair_metric_name(-1) is None
    from mc_gra_amd import engine as E
    assert E.PAIR_METRICS is L.PAIR_METRICS
    assert [E.pair_metric_id(m) for m in E.PAIR_METRICS] == list(range(8)) == [E.pair_metric_id(i) for i in range(8)]
    for bad in ("hamming", 8, -1, None, 1.0, True):
        with pytest.raises(ValueError, match="cosine, euclidean"):
            E.pair_metric_id(bad)


def test_pair_distance_entries_refuse_before_touching_a_device(pkg):
    """The argument checks come first: they need no GPU (the pointers here are never followed, the outputs never written)."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    auc, ap = ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    counts = (ctypes.c_int64 * 4)(-7, -7, -7, -7)

    def rank(n=8, d=4, ldz=4, metric=0, ldl=8, idx=None, n_idx=8, a=ctypes.byref(auc), b=ctypes.byref(ap), c=counts, Z=p, lab=p):
        return L.mcgra_pair_distance_rank_metrics(None, n, d, Z, ldz, metric, lab, ldl, idx, n_idx, a, b, c)

    for rc in (rank(metric=8), rank(metric=-1), rank(d=0), rank(ldz=3), rank(ldl=7), rank(idx=p, n_idx=1), rank(n=1, ldl=1),
               rank(a=None, b=None), rank(c=None), rank(n=0), rank(Z=None), rank(lab=None)):
        assert rc == -1, L.mcgra_last_error()
    assert rank(metric=9) == -1 and b"metric 9" in L.mcgra_last_error()
    assert rank(idx=p, n_idx=65536, n=70000, ldl=70000) == -3 and b"65536" in L.mcgra_last_error()
    assert rank(n=65536, ldl=65536) == -3
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(rank(n=65536, ldl=65536))
    assert (auc.value, ap.value, list(counts)) == (-7.0, -7.0, [-7] * 4)         # after a refusal nothing has been written
    scores = lambda n=8, d=4, ldz=4, metric=0, ldo=8, Z=p, out=p: L.mcgra_pair_distance_scores(None, n, d, Z, ldz, metric, out, ldo)
    for rc in (scores(metric=8), scores(metric=-1), scores(d=0), scores(ldz=3), scores(ldo=7), scores(n=0), scores(Z=None),
               scores(out=None)):
        assert rc == -1
    # a width past the decode entries' 128 columns is not an argument error (d = 1433 passes these checks; ldz < d does not)
    assert scores(d=1433, ldz=1432) == -1 and b"ldz" in L.mcgra_last_error()


def test_engine_wrappers_refuse_host_tensors_and_bad_metrics(pkg):
    from mc_gra_amd import engine as E
    Z, lab = torch.zeros(4, 3), torch.zeros(4, 4)
    with pytest.raises(ValueError, match="cpu tensor"):
        E.pair_distance_scores(Z, "cosine")
    with pytest.raises(ValueError, match="cpu tensor"):
        E.pair_distance_rank_metrics(lab, Z, "cosine")


# ------------------------------------------------------------------------------------------------- the command line
def test_parser_takes_the_mode_and_still_refuses_the_others(pkg, capsys):
    from mc_gra_amd import main as M
    p = M.build_parser()
    a = p.parse_args(["--mode", "link_stealing", "--ap"])
    assert a.mode == "link_stealing" and a.ap is True and not hasattr(a, "versus")
    for mode in ("search", "baseline", "gaussian", "gcn_attack"):
        with pytest.raises(SystemExit):
            p.parse_args(["--mode", mode])
        assert "invalid choice" in capsys.readouterr().err


@pytest.mark.parametrize("flags", (["--topk", "5"], ["--curves", "c.npz"], ["--per_node", "p.npz"], ["--binarize"], ["--ci"],
                                   ["--ci_nodes"], ["--save_scores", "s.npy"], ["--structure", "edges"], ["--hops", "3"],
                                   ["--by_class", "labels"], ["--ci", "--versus", "posteriors:cosine"]))
def test_report_flags_are_refused_under_link_stealing(pkg, capsys, flags):
    from mc_gra_amd import main as M
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["--mode", "link_stealing"] + flags)
    assert "--mode evaluate only, not --mode link_stealing" in capsys.readouterr().err
    args = argparse.ArgumentParser.parse_args(M.build_parser(), ["--mode", "link_stealing"] + flags)      # the parser without its checks
    with pytest.raises(SystemExit, match="not --mode link_stealing"):
        M._run(args, 0, 1)                                                       # run() refuses too, before it loads anything


def test_versus_baseline_shortcut_is_decided_by_name(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    a = p.parse_args(["--ci", "--versus", "posteriors:cosine"])
    assert a.versus == "posteriors:cosine" and a.mode == "evaluate"
    with pytest.raises(SystemExit):
        p.parse_args(["--versus", "posteriors:cosine"])
    assert "--versus needs --ci or --ci_nodes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--ci", "--versus", "logits:cosine"])
    assert "source `logits` is not one of posteriors, embedding, features" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--ci_nodes", "--versus", "embedding:hamming"])
    assert "metric `hamming` is not one of cosine, euclidean" in capsys.readouterr().err
    fail = []
    for s in R.LINK_SOURCES:
        for m in T.METRICS:
            assert R.versus_baseline(f"{s}:{m}", fail.append) == (s, m)
    for other in ("features", "scores.npy", "run:3/scores.npy", "", None):      # today's meanings stay
        assert R.versus_baseline(other, fail.append) is None
    assert fail == []


def test_link_stealing_lines_and_result_shape(pkg, monkeypatch):
    """main.link_stealing_metrics asks the engine for every source x metric x set and keeps auc / pairs / positives (+ ap);
    one printed line per source and metric."""
    from mc_gra_amd import main as M
    calls = []

    def fake(real, Z, metric, idx=None):
        calls.append((tuple(Z.shape), metric, None if idx is None else tuple(idx)))
        return {"pairs": 6, "positives": 2, "negatives": 4, "T": 9, "auc": 0.5625, "ap": 0.25}

    monkeypatch.setattr(M.engine, "pair_distance_rank_metrics", fake)
    src = M.link_sources(torch.log(torch.full((4, 2), 0.5)), torch.zeros(4, 3), torch.ones(4, 5), "cpu")
    assert list(src) == ["posteriors", "embedding", "features"] and torch.equal(src["posteriors"], torch.full((4, 2), 0.5))
    sets = {"attack": [0, 2, 3], "train": [1, 2], "all": None}
    res = M.link_stealing_metrics(torch.zeros(4, 4), src, sets, False)
    assert len(calls) == 72 and calls[0] == ((4, 2), "cosine", (0, 2, 3)) and calls[-1] == ((4, 5), "sqeuclidean", None)
    assert list(res) == list(src) and list(res["embedding"]) == list(T.METRICS)
    assert res["features"]["canberra"]["train"] == {"auc": 0.5625, "pairs": 6, "positives": 2}
    lines = M.link_stealing_lines(res, False)
    assert len(lines) == 24 and lines[0] == "link stealing posteriors cosine: auc_attack=0.5625 auc_train=0.5625 auc_all=0.5625"
    res = M.link_stealing_metrics(torch.zeros(4, 4), src, sets, True)
    assert res["features"]["canberra"]["all"] == {"auc": 0.5625, "pairs": 6, "positives": 2, "ap": 0.25}
    assert M.link_stealing_lines(res, True)[23] == ("link stealing features sqeuclidean: auc_attack=0.5625 auc_train=0.5625 "
                                                    "auc_all=0.5625 ap_attack=0.25 ap_train=0.25 ap_all=0.25")
