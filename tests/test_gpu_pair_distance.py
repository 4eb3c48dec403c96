"""The link-stealing pair distances on the GPU (mcgra_pair_distance_scores, mcgra_pair_distance_rank_metrics,
main.py --mode link_stealing and --versus SOURCE:METRIC) against tests/pair_distance_truth.py and the cases of
tests/pair_distance_cases.py; tests/test_pair_distance_cases_cpu.py vets those cases without a GPU."""
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import pair_distance_cases as Cs
from tests import pair_distance_truth as T

pytestmark = pytest.mark.gpu

NS = (2, 3, 63, 64, 65, 130, 257, 515)
DS = (1, 3, 16, 80, 129, 200)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _sklearn_ap(S, lab, idx):
    from sklearn.metrics import average_precision_score
    v, l = T.lower_pairs(S, lab, idx)
    P = int((l == 1).sum())
    if P == 0:
        return float("nan")
    return 1.0 if P == len(l) else float(average_precision_score(l, v))


def _rows(n, d, seed):
    """Rows with the planted groups in them, rounded to a coarse grid so that scores tie now and then."""
    lab, g = Cs.planted(n, seed)
    rng = np.random.RandomState(seed + 3)
    Z = np.round((rng.randn(n, d) + rng.randn(4, d)[g]) * 4) / 8
    return lab, Z.astype(np.float32)


# ------------------------------------------------------------------------------------------------- self-consistency
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("metric", T.METRICS)
def test_ranked_pair_by_pair_is_the_materialised_matrix(pkg, metric, n):
    """Every width: pair_distance_scores is bitwise symmetric and repeats bit for bit; the pair-by-pair entry's integers and AUC
    are auc_delong's on that matrix, for all nodes, a subset and the subset permuted; the average precision is sklearn's."""
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(n)
    sub = rng.permutation(n)[:max(2, (2 * n) // 3)]
    perm = sub[rng.permutation(len(sub))]
    for d in DS:
        lab, Z = _rows(n, d, 100 * n + d)
        dl, dz = _dev(lab), _dev(Z)
        S = E.pair_distance_scores(dz, metric)
        Sh = S.cpu().numpy()
        assert Sh.shape == (n, n) and np.array_equal(Sh.view(np.uint32), Sh.T.view(np.uint32)), (d, "symmetric bits")
        assert np.array_equal(E.pair_distance_scores(dz, E.PAIR_METRICS.index(metric)).cpu().numpy().view(np.uint32), Sh.view(np.uint32))
        assert np.all(Sh <= 0) and np.all(np.isfinite(Sh))
        ref = T.scores64(Z, metric)
        assert np.allclose(Sh, ref, rtol=1e-4, atol=1e-4), (d, np.abs(Sh - ref).max())      # (the tight bounds: the accuracy test)
        got = {}
        for name, idx in (("all", None), ("subset", sub), ("permuted", perm)):
            r = E.pair_distance_rank_metrics(dl, dz, metric, idx)
            dlg = E.auc_delong(dl, S, idx)
            assert (r["pairs"], r["positives"], r["negatives"]) == (dlg["pairs"], dlg["positives"], dlg["negatives"]), (d, name)
            assert r["T"] == dlg["ints"]["T"] and _same(r["auc"], dlg["auc"]), (d, name, r, dlg["auc"])
            again = E.pair_distance_rank_metrics(dl, dz, metric, idx)
            assert all(_same(float(r[k]), float(again[k])) for k in r), (d, name)
            want = _sklearn_ap(Sh, lab, idx)
            assert _same(r["ap"], want) or abs(r["ap"] - want) <= 1e-12, (d, name, r["ap"], want)
            got[name] = r
        assert all(got["subset"][k] == got["permuted"][k] for k in ("pairs", "positives", "negatives", "T")), d
        assert _same(got["subset"]["auc"], got["permuted"]["auc"]) and _same(got["subset"]["ap"], got["permuted"]["ap"])


@pytest.mark.parametrize("metric", ("canberra", "correlation"))
def test_past_the_grid_cap_and_in_a_wider_buffer(pkg, metric):
    """n = 2817 is 45 x 45 tiles: the 1035 tiles on or below the diagonal (and the 2025 of the materialising kernel) are more
    than the 1024 blocks of a launch, so blocks take a second tile; Z sits in a wider buffer (ldz > d)."""
    import torch
    from mc_gra_amd import engine as E
    n, d = 2817, 16
    lab, Z = _rows(n, d, 9)
    wide = torch.full((n, d + 5), float("nan"), device="cuda:0")      # what lies beside Z is never read
    wide[:, :d] = _dev(Z)
    zv = wide[:, :d]
    assert zv.stride(0) == d + 5
    dl = _dev(lab)
    S = E.pair_distance_scores(zv, metric)
    assert torch.equal(S, S.t()) and torch.equal(S, E.pair_distance_scores(_dev(Z), metric))
    rng = np.random.RandomState(1)
    for idx in (None, rng.permutation(n)[:2200]):
        r = E.pair_distance_rank_metrics(dl, zv, metric, idx)
        dlg = E.auc_delong(dl, S, idx)
        assert (r["pairs"], r["positives"], r["negatives"], r["T"]) == (dlg["pairs"], dlg["positives"], dlg["negatives"], dlg["ints"]["T"])
        assert r["auc"] == dlg["auc"] and 0.5 < r["auc"] < 1
    Sh = S.cpu().numpy()
    k = rng.permutation(n)[:40]
    assert np.allclose(Sh[np.ix_(k, k)], T.scores64(Z[k], metric), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("n", (65, 257))
@pytest.mark.parametrize("metric", T.METRICS)
def test_known_answers_are_exact(pkg, metric, n):
    from mc_gra_amd import engine as E
    lab, Z, frac, ints = Cs.known_auc(metric, n)
    r = E.pair_distance_rank_metrics(_dev(lab), _dev(Z), metric)
    assert {k: r[k] for k in ints} == ints
    assert r["auc"] == float(frac)                                    # the rational's nearest double
    sub = np.random.RandomState(n).permutation(n)[: n // 2]
    _, _, fsub, isub = Cs.known_auc(metric, n, sub)
    r = E.pair_distance_rank_metrics(_dev(lab), _dev(Z), metric, sub)
    assert {k: r[k] for k in isub} == isub and r["auc"] == float(fsub)


# ------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", list(Cs.ACCURACY))
def test_accuracy_against_float64(pkg, name):
    """On the CPU-vetted cases: the AUC within 1e-6 of float64's exact rational, every materialised score within the a-priori
    float32 bound of DESIGN.md ("Pair distances")."""
    from mc_gra_amd import engine as E
    lab, Z, s64 = Cs.accuracy_case(name)
    kap = Cs.kappa(Z)
    dl, dz = _dev(lab), _dev(Z)
    for m in T.METRICS:
        r = E.pair_distance_rank_metrics(dl, dz, m)
        want = float(T.exact_auc(s64[m], lab)[0])
        S = E.pair_distance_scores(dz, m).cpu().numpy().astype(np.float64)
        kind, b = Cs.score_bound(m, Z.shape[1], kap)
        err = np.abs(S - s64[m])
        worst = float((err / np.maximum(np.abs(s64[m]), 1e-300))[s64[m] != 0].max()) if kind == "rel" else float(err.max())
        print(f"{name} {m}: auc={r['auc']!r} float64={want!r} |diff|={abs(r['auc'] - want):.3e} {kind} error {worst:.3e} bound {b:.3e}")
        assert abs(r["auc"] - want) <= 1e-6, (m, r["auc"], want)
        assert np.all(err <= b * (np.abs(s64[m]) if kind == "rel" else 1.0)), (m, kind, b, worst)


def test_metrics_the_auc_cannot_tell_apart_differ_in_their_values(pkg):
    from mc_gra_amd import engine as E
    _, Z, _ = Cs.accuracy_case("softmax_400x4")
    S = {m: E.pair_distance_scores(_dev(Z), m).cpu().numpy() for m in ("euclidean", "sqeuclidean", "braycurtis", "cityblock")}
    assert np.abs(S["euclidean"] - S["sqeuclidean"]).max() > 0.1 and np.abs(S["braycurtis"] - S["cityblock"]).max() > 0.1
    assert np.allclose(S["braycurtis"] * 2, S["cityblock"], rtol=1e-6)       # softmax rows: the denominator is the constant 2
    lab, Z, _ = Cs.accuracy_case("randn_257x16")                             # not normalised: the two rank differently
    a = E.pair_distance_rank_metrics(_dev(lab), _dev(Z), "braycurtis")["auc"]
    b = E.pair_distance_rank_metrics(_dev(lab), _dev(Z), "cityblock")["auc"]
    assert abs(a - b) > 1e-3


def test_degenerate_rows(pkg):
    """A zero row (cosine) and a constant row (correlation) are at distance 1 from everything; d = 1 ties every pair under
    correlation; both-zero coordinates add nothing to canberra; a zero braycurtis denominator gives 0."""
    from mc_gra_amd import engine as E
    Z = np.array([[0, 0, 0, 0], [2, 2, 2, 2], [1, 0, 0, 0], [0, 3, 0, 1]], np.float32)
    cos = E.pair_distance_scores(_dev(Z), "cosine").cpu().numpy()
    assert np.all(cos[0] == -1.0) and np.all(cos[:, 0] == -1.0) and abs(cos[1, 2] + 0.5) < 1e-6
    cor = E.pair_distance_scores(_dev(Z), "correlation").cpu().numpy()
    assert np.all(cor[0] == -1.0) and np.all(cor[1] == -1.0)
    odd = np.full((3, 7), np.float32(0.1))
    odd[2, 3] = 0.3
    assert np.all(E.pair_distance_scores(_dev(odd), "correlation").cpu().numpy()[:2] == -1.0)
    one = E.pair_distance_scores(_dev(np.array([[1.5], [-2.0], [0.0]], np.float32)), "correlation").cpu().numpy()
    assert np.all(one == -1.0)
    can = E.pair_distance_scores(_dev(Z), "canberra").cpu().numpy()
    assert can[0, 0] == 0.0 and can[0, 2] == -1.0 and can[2, 3] == -3.0
    bc = E.pair_distance_scores(_dev(np.array([[1, -1], [-1, 1], [0, 0]], np.float32)), "braycurtis").cpu().numpy()
    assert bc[0, 1] == 0.0 and bc[2, 2] == 0.0 and bc[0, 2] == -1.0
    for m in T.METRICS:
        assert np.allclose(E.pair_distance_scores(_dev(Z), m).cpu().numpy(), T.scores64(Z, m), rtol=1e-6, atol=1e-6), m


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg):
    from mc_gra_amd import engine as E
    n = 70
    lab, Z = _rows(n, 8, 2)
    dl, dz = _dev(lab), _dev(Z)
    for v in (np.nan, np.inf, -np.inf):
        bad = Z.copy(); bad[69, 7] = v                                          # a row no selection names still counts
        for m in ("cosine", "cityblock", "correlation"):
            with pytest.raises(pkg._lib.McgraError, match="NaN or infinite"):
                E.pair_distance_rank_metrics(dl, _dev(bad), m, [0, 1, 2])
            with pytest.raises(pkg._lib.McgraError, match="NaN or infinite"):
                E.pair_distance_scores(_dev(bad), m)
    big = np.full((n, 8), 3e19, np.float32)
    big[::2] *= -1                                                              # finite Z, (6e19)^2 is not
    with pytest.raises(pkg._lib.McgraError, match="score is NaN or infinite"):
        E.pair_distance_rank_metrics(dl, _dev(big), "sqeuclidean")
    assert E.pair_distance_rank_metrics(dl, _dev(big), "chebyshev")["pairs"] == n * (n - 1) // 2     # 6e19 itself is a score
    two = lab.copy(); two[4, 3] = 2.0
    with pytest.raises(pkg._lib.McgraError, match="neither 0 nor 1"):
        E.pair_distance_rank_metrics(_dev(two), dz, "cosine")
    assert E.pair_distance_rank_metrics(_dev(two), dz, "cosine", [0, 1, 2, 5])["pairs"] == 6        # not selected: not looked at
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.pair_distance_rank_metrics(dl, dz, "cosine", [3, 5, 3])
    with pytest.raises(pkg._lib.McgraError, match="outside"):
        E.pair_distance_rank_metrics(dl, dz, "cosine", [0, n])
    with pytest.raises(pkg._lib.McgraError, match="outside"):
        E.pair_distance_rank_metrics(dl, dz, "cosine", [-1, 2])
    with pytest.raises(pkg._lib.McgraError):
        E.pair_distance_rank_metrics(dl, dz, "cosine", [4])
    with pytest.raises(ValueError):
        E.pair_distance_rank_metrics(dl, dz, "hamming")
    none = E.pair_distance_rank_metrics(_dev(np.zeros((n, n), np.float32)), dz, "euclidean")
    assert none["positives"] == 0 and none["T"] == 0 and math.isnan(none["auc"]) and math.isnan(none["ap"])
    full = E.pair_distance_rank_metrics(_dev(np.ones((n, n), np.float32)), dz, "euclidean")
    assert full["negatives"] == 0 and full["T"] == 0 and math.isnan(full["auc"]) and full["ap"] == 1.0


# ------------------------------------------------------------------------------------------------- the mode itself
def test_main_link_stealing_scores_the_baselines_without_an_attack(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode link_stealing on the committed brazil files (n = 131): no engine, no PGDAttack, nothing on disk; 24 lines;
    every value is a direct engine call on the source it names; the same seed gives the same bits."""
    import torch
    import mc_gra_amd.topology_attack as TA
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M

    def no_engine(*a, **k):
        raise AssertionError("--mode link_stealing built an attack engine")

    monkeypatch.setattr(M.engine, "AttackEngine", no_engine)
    monkeypatch.setattr(TA, "AttackEngine", no_engine)
    monkeypatch.setattr(M, "PGDAttack", no_engine)
    seen = []
    sources = M.link_sources
    monkeypatch.setattr(M, "link_sources", lambda *a: seen.append(sources(*a)) or seen[-1])
    monkeypatch.chdir(tmp_path)
    argv = ["--mode", "link_stealing", "--dataset", "brazil", "--dataset_root", os.path.join(H.GOLDEN, "dataset")]
    res = M.run(M.build_parser().parse_args(argv))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("link stealing ")]
    assert list(res) == ["link_stealing"] and len(lines) == 24 and not any("ap_" in l for l in lines)
    src = seen[0]
    assert [tuple(v.shape)[0] for v in src.values()] == [131] * 3 and src["posteriors"].shape[1] == 4 and src["embedding"].shape[1] == 16
    assert torch.allclose(src["posteriors"].sum(1), torch.ones(131, device=src["posteriors"].device), atol=1e-5)
    g = H.load_readme_graph("brazil")
    real = _dev(g["adj"])
    assert np.array_equal(src["features"].cpu().numpy(), np.asarray(g["features"], np.float32))
    ls = res["link_stealing"]
    assert list(ls) == ["posteriors", "embedding", "features"]
    i = 0
    for source, by_metric in ls.items():
        assert list(by_metric) == list(T.METRICS)
        for metric, by_set in by_metric.items():
            assert list(by_set) == ["attack", "train", "all"]
            assert lines[i] == f"link stealing {source} {metric}: " + " ".join(f"auc_{k}={v['auc']}" for k, v in by_set.items())
            i += 1
            d = E.pair_distance_rank_metrics(real, src[source], metric)
            assert by_set["all"] == {"auc": d["auc"], "pairs": 131 * 130 // 2, "positives": d["positives"]}
            assert sorted(by_set["train"]) == ["auc", "pairs", "positives"] and 0.0 <= by_set["train"]["auc"] <= 1.0
    assert ls["embedding"]["cosine"]["all"]["auc"] > 0.5                        # two GCN layers do leak the graph
    again = M.run(M.build_parser().parse_args(argv + ["--ap"]))
    out = [l for l in capsys.readouterr().out.splitlines() if l.startswith("link stealing ")]
    assert len(out) == 24 and all(" ap_attack=" in l and " ap_all=" in l for l in out)
    for source in ls:
        for metric in ls[source]:
            for name in ("attack", "train", "all"):
                a = dict(again["link_stealing"][source][metric][name])
                assert 0.0 < a.pop("ap") <= 1.0 and a == ls[source][metric][name]      # bit for bit
    assert not os.path.exists(tmp_path / "results") and not os.path.exists(tmp_path / "saved_data")


def test_main_evaluate_versus_a_link_stealing_baseline(pkg, tmp_path, monkeypatch, capsys):
    """--mode evaluate --ci --versus posteriors:correlation on brazil: versus_all's "b" is auc_delong on pair_distance_scores of
    exp(Y_A), the posteriors the attack itself is given."""
    import torch
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M
    seen = []
    sources = M.link_sources
    monkeypatch.setattr(M, "link_sources", lambda *a: seen.append((a[0], sources(*a))) or seen[-1][1])
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "brazil", "--dataset_root", os.path.join(H.GOLDEN, "dataset"), "--epochs", "3", "--measure", "MSELoss",
            "--w2", "100", "--w6", "100", "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A",
            "--ci", "--versus", "posteriors:correlation"]
    res = M.run(M.build_parser().parse_args(argv))
    out = capsys.readouterr().out
    (Y_A, src), = seen
    assert torch.equal(src["posteriors"], torch.exp(Y_A.to(torch.float32)))
    S = E.pair_distance_scores(src["posteriors"], "correlation")
    real = _dev(H.load_readme_graph("brazil")["adj"])
    want = E.auc_delong(real, S)
    b = res["versus_all"]["b"]
    assert b["ints"] == want["ints"] and b["auc"] == want["auc"] and b["var"] == want["var"]
    assert res["versus_all"]["a"] is res["ci_all"] and math.isfinite(res["versus_all"]["p_value"])
    assert abs(res["versus_all"]["delta"] - (res["ci_all"]["auc"] - b["auc"])) < 1e-15
    assert f"current delta={res['versus_all']['delta']}" in out
    log = open(tmp_path / "results" / "result.txt").read()
    assert "versus='posteriors:correlation'" in log and f"versus posteriors:correlation: AUC={b['auc']}" in log
