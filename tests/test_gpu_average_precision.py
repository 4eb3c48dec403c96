"""The average precision of the recovered adjacency beside its AUC (mcgra_rank_metrics, mcgra_decode_rank_metrics,
engine.rank_metrics / average_precision / decode_rank_metrics / decode_average_precision, main.py --ap): against sklearn's
average_precision_score and the closed form of tests/ap_truth.py on the committed fixtures and on ties and selections, the
walk over the positives and the fixed reduction past one term per lane, single-class answers, refusals, bit-level
determinism, n = 10 000 against the exact rational, the decode route against the materialised one, and main.py end to end.
Run with -m gpu.

The 1e-12 bar is the one tests/test_gpu_auc.py holds the AUC to against sklearn.  The kernel's own bound is (T + 32) 2^-53
relative with T = ceil(P / 2^20) terms per lane (csrc/auc.hip): below 4e-15 for every case here."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import ap_truth as T
from tests import helpers as H
from tests.test_gpu_auc import CASES, FIXTURES

pytestmark = pytest.mark.gpu

TOL = 1e-12


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
    return a == b or (math.isnan(a) and math.isnan(b))


def _check(got, real, pred, idx, what):
    ref, truth = T.sklearn_average_precision(real, pred, idx), T.average_precision(real, pred, idx)
    print(f"{what}: got {got!r} sklearn {ref!r} closed form {truth!r} diff {abs(got - ref):.3e} {abs(got - truth):.3e}")
    assert abs(got - ref) <= TOL and abs(got - truth) <= TOL, (what, got, ref, truth)


# ------------------------------------------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_average_precision_on_the_attack_fixtures(pkg, name):
    from mc_gra_amd import engine as E
    z = np.load(os.path.join(H.GOLDEN, f"{name}.npz"))
    adj, final = _dev(z["adj"]), _dev(z["final"])
    got = E.average_precision(adj, final, z["idx_attack"])
    _check(got, z["adj"], z["final"], z["idx_attack"], name)
    auc, ap = E.rank_metrics(adj, final, z["idx_attack"])
    assert auc == E.roc_auc(adj, final, z["idx_attack"]) and ap == got


# ------------------------------------------------------------------------------------------ 2. ties and selections
@pytest.mark.parametrize("name", sorted(CASES))
def test_average_precision_ties_and_selections_against_sklearn(pkg, name):
    from mc_gra_amd import engine as E
    real, pred, idx = CASES[name]
    r, p, ix = _dev(real), _dev(pred), None if idx is None else _dev(idx)
    got = E.average_precision(r, p, ix)
    _check(got, real, pred, idx, name)
    auc, ap = E.rank_metrics(r, p, ix)
    assert ap == got and auc == E.roc_auc(r, p, ix), name
    if name == "quantised":                           # counting a tie or not: 6e-2 apart (test_average_precision_cpu.py)
        assert abs(got - T.average_precision(real, pred, idx, strict=True)) > 1e-2


# ------------------------------------------------------------------------------------------- 3. walk and reduction
def _planted(seed, n, frac):
    rng = np.random.RandomState(seed)
    real = (rng.rand(n, n) < frac).astype(np.float32)
    pred = (rng.randn(n, n) + 0.7 * real).astype(np.float32)          # edges lean to the high scores
    return real, pred


def test_average_precision_more_than_one_term_per_lane(pkg):
    """n = 2048 at 30 % positives: P > 2^20 = 4096 blocks x 256 lanes, so the grid is at its cap and lanes add a second term."""
    from mc_gra_amd import engine as E
    real, pred = _planted(11, 2048, 0.3)
    assert int(real.sum()) > 1 << 20
    got = E.average_precision(_dev(real), _dev(pred))
    _check(got, real, pred, None, "n=2048")
    assert got > 0.4                                                   # the prevalence is 0.3


def test_average_precision_more_positives_than_negatives(pkg):
    """n = 700 at 70 % positives: P > N; the AUC looks the negatives up, the average precision still walks the positives."""
    from mc_gra_amd import engine as E
    real, pred = _planted(12, 700, 0.7)
    assert real.sum() > real.size - real.sum()
    auc, ap = E.rank_metrics(_dev(real), _dev(pred))
    _check(ap, real, pred, None, "n=700")
    assert auc == E.roc_auc(_dev(real), _dev(pred))


@pytest.mark.parametrize("rest", [1, 2, 3])
def test_average_precision_negatives_region_behind_padding(pkg, rest):
    """P % 4 = 1, 2, 3: the negatives' region starts 3, 2, 1 padding keys behind the last positive."""
    from mc_gra_amd import engine as E
    real, pred = _planted(13 + rest, 97, 0.25)
    pred = np.round(pred * 4).astype(np.float32) / 4                   # ties between the classes as well
    flat = real.reshape(-1)
    zeros = np.flatnonzero(flat == 0)
    k = (rest - int(flat.sum())) % 4
    flat[zeros[:k]] = 1.0
    assert int(real.sum()) % 4 == rest
    auc, ap = E.rank_metrics(_dev(real), _dev(pred))
    _check(ap, real, pred, None, f"P%4={rest}")
    assert auc == E.roc_auc(_dev(real), _dev(pred))


# ------------------------------------------------------------------------------------------------- 4. single class
def test_average_precision_single_class(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(1)
    s = _dev(rng.rand(64, 64).astype(np.float32))
    none, every = _dev(np.zeros((64, 64), np.float32)), _dev(np.ones((64, 64), np.float32))
    assert math.isnan(E.average_precision(none, s))                    # a mean over no positives
    assert E.average_precision(every, s) == 1.0                        # every term is 1 (sklearn: 1.0)
    a, p = E.rank_metrics(none, s)
    assert math.isnan(a) and math.isnan(p)
    a, p = E.rank_metrics(every, s)
    assert math.isnan(a) and p == 1.0
    lab = np.zeros((64, 64), np.float32)
    lab[5, 9] = 1.0
    assert math.isnan(E.average_precision(_dev(lab), s, [0, 1, 2, 3]))          # the positive is not selected
    lab = np.ones((64, 64), np.float32)
    lab[5, 9] = 0.0
    assert E.average_precision(_dev(lab), s, [0, 1, 2, 3]) == 1.0               # the negative is not selected
    Z = _dev(rng.randn(64, 5).astype(np.float32))
    for mode in (0, 4):
        assert math.isnan(E.decode_average_precision(none, Z, mode)) and E.decode_average_precision(every, Z, mode) == 1.0


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_rank_metrics_refuses_what_roc_auc_refuses(pkg):
    from mc_gra_amd import engine as E
    from mc_gra_amd.engine import _p, _stream
    rng = np.random.RandomState(2)
    lab = (rng.rand(80, 80) < 0.3).astype(np.float32)
    s = rng.rand(80, 80).astype(np.float32)
    sub = np.arange(60)
    want = T.average_precision(lab, s, sub)
    for f in (E.average_precision, E.rank_metrics):
        bad = lab.copy(); bad[3, 4] = 2.0
        with pytest.raises(pkg._lib.McgraError):
            f(_dev(bad), _dev(s))
        bad = lab.copy(); bad[7, 70] = 2.0                              # outside idx x idx: not looked at
        got = f(_dev(bad), _dev(s), sub)
        assert abs((got if f is E.average_precision else got[1]) - want) <= TOL
        for v in (np.nan, np.inf, -np.inf):
            t = s.copy(); t[7, 70] = v
            with pytest.raises(pkg._lib.McgraError):
                f(_dev(lab), _dev(t))
            got = f(_dev(lab), _dev(t), sub)                            # an entry outside idx x idx is not looked at
            assert abs((got if f is E.average_precision else got[1]) - want) <= TOL
        with pytest.raises(pkg._lib.McgraError):
            f(_dev(lab), _dev(s), [0, 80])                              # a node id out of range
        with pytest.raises(pkg._lib.McgraError):
            f(_dev(lab), _dev(s), [-1, 2])
        with pytest.raises(pkg._lib.McgraNotSupported):
            f(_dev(lab), _dev(s), np.arange(65536) % 80)
    L, l, t = pkg._lib.lib, _dev(lab), _dev(s)
    assert L.mcgra_rank_metrics(_stream(), 80, _p(l), 80, _p(t), 80, None, 80, None, None) == -1     # MCGRA_EINVAL
    Z = _dev(rng.randn(80, 8).astype(np.float32))
    assert L.mcgra_decode_rank_metrics(_stream(), 80, 8, _p(Z), 8, 0, _p(l), 80, None, 80, None, None) == -1
    out = ctypes.c_double()
    assert L.mcgra_rank_metrics(_stream(), 80, _p(l), 80, _p(t), 80, None, 80, None, ctypes.byref(out)) == 0
    assert out.value == E.average_precision(l, t)


# ------------------------------------------------------------------------------------------------- 6. determinism
def test_average_precision_is_deterministic(pkg):
    from mc_gra_amd import engine as E
    real, pred, _ = CASES["perm"]
    r, p = _dev(real), _dev(pred)
    n = len(real)
    a = [E.average_precision(r, p).hex() for _ in range(2)] + [E.average_precision(r, p, np.arange(n)[::-1].copy()).hex(),
                                                               E.rank_metrics(r, p)[1].hex()]
    assert len(set(a)) == 1, a
    sub = np.random.RandomState(3).choice(n, 400, replace=False)     # a repeat-free subset in two orders: the same sorted keys
    b = [E.average_precision(r, p, sub).hex(), E.average_precision(r, p, sub[::-1].copy()).hex(),
         E.average_precision(r, p, np.sort(sub)).hex()]
    assert len(set(b)) == 1 and b[0] != a[0], b


# ------------------------------------------------------------------------------------------------------- 7. scale
def test_average_precision_at_scale_against_the_exact_rational(pkg):
    """n = 10 000, the scores in a wider buffer (rows not 16-byte aligned): built as test_roc_auc_at_scale_against_the_exact_
    fraction builds it.  Scores from a few levels drawn on the device, labels leaning to the high levels; the truth is
    sum over levels of p_v TP_v / (TP_v + FP_v), over P, in Python rationals from the device histogram."""
    import torch
    from mc_gra_amd import engine as E
    n, pad = 10000, 3
    levels = torch.tensor([-3.0, -0.0, 0.0, 1e-40, 0.25, 0.5, 0.75, 1.0], device="cuda:0")
    order = [0, 1, 3, 4, 5, 6, 7]               # distinct values ascending; level 2 (+0.0) joins level 1 (-0.0)
    g = torch.Generator(device="cuda:0").manual_seed(n)
    buf = torch.empty(n, n + pad, device="cuda:0")
    scores = buf[:, :n]
    labels = torch.empty(n, n, device="cuda:0")
    hist = torch.zeros(2 * len(levels), dtype=torch.int64, device="cuda:0")
    for r0 in range(0, n, 2048):
        r1 = min(n, r0 + 2048)
        lv = torch.randint(0, len(levels), (r1 - r0, n), generator=g, device="cuda:0")
        lb = torch.rand(r1 - r0, n, generator=g, device="cuda:0") < (0.2 + 0.08 * lv.float())
        scores[r0:r1] = levels[lv]
        labels[r0:r1] = lb.float()
        hist += torch.bincount((lv * 2 + lb.long()).reshape(-1), minlength=2 * len(levels))
        del lv, lb
    h = hist.cpu().tolist()
    q = [h[2 * v] for v in range(len(levels))]
    p = [h[2 * v + 1] for v in range(len(levels))]
    q[1] += q[2]; p[1] += p[2]
    exact = T.from_counts_exact([p[v] for v in order], [q[v] for v in order])
    auc, ap = E.rank_metrics(labels, scores)
    print(f"n=10000: got {ap!r} exact {exact!r} diff {abs(ap - exact):.3e}")
    assert abs(ap - exact) <= TOL, (ap, exact)
    assert sum(p) / n ** 2 + 0.02 < exact < 1.0                       # the ranking does carry the labels
    assert auc == E.roc_auc(labels, scores) and ap == E.average_precision(labels, scores)


# ------------------------------------------------------------------------------------------------ 8. decode route
def _graph(rng, n, p=0.15):
    a = np.triu(rng.rand(n, n) < p, 1)
    a = (a | a.T).astype(np.float32)
    a[np.arange(n), np.arange(n)] = (rng.rand(n) < 0.3).astype(np.float32)
    return a


def _decode_routes_agree(E, adj, Z, mode, idx, what):
    S = E.decode_scores(Z, mode)
    got = E.decode_rank_metrics(adj, Z, mode, idx)
    want = E.rank_metrics(adj, S, idx)
    assert _same(got[0], want[0]) and _same(got[1], want[1]), (what, got, want)
    assert _same(got[0], E.decode_auc(adj, Z, mode, idx)) and _same(got[1], E.decode_average_precision(adj, Z, mode, idx)), what
    return got


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_decode_rank_metrics_is_rank_metrics_of_decode_scores_bit_for_bit(pkg, mode):
    from mc_gra_amd import engine as E
    n = 130
    rng = np.random.RandomState(500 + mode)
    adj = _dev(_graph(rng, n))
    sub = rng.choice(n, 87, replace=False)
    sels = [None, sub, np.concatenate([sub, sub[:44], sub[:1]])]      # all nodes, a subset, a subset with repeats
    for d in (7, 16, 128):
        Z = _dev((rng.randn(n, d) * (0.6 / math.sqrt(d))).astype(np.float32))
        for idx in sels:
            auc, ap = _decode_routes_agree(E, adj, Z, mode, idx, (mode, d, None if idx is None else len(idx)))
            assert 0.0 < ap < 1.0


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_decode_rank_metrics_past_the_block_cap(pkg, mode):
    """n = 2113: 34 x 34 = 1156 tiles for at most 1024 blocks, so blocks take a second tile; Z sits in a wider buffer."""
    import torch
    from mc_gra_amd import engine as E
    n, d = 2113, 16
    rng = np.random.RandomState(2113 + mode)
    adj = _dev(_graph(rng, n, 0.01))
    buf = torch.zeros(n, d + 3, device="cuda:0")
    Z = buf[:, :d]
    Z.copy_(_dev((rng.randn(n, d) * 0.3).astype(np.float32)))
    sub = rng.choice(n, 1500, replace=False)
    for idx in (None, sub):
        auc, ap = _decode_routes_agree(E, adj, Z, mode, idx, (mode, idx is None))
        assert 0.0 < auc < 1.0 and 0.0 < ap < 1.0


def test_decode_rank_metrics_refusals(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(4)
    n = 80
    lab = _dev(_graph(rng, n))
    Z = rng.randn(n, 8).astype(np.float32)
    for f in (E.decode_rank_metrics, E.decode_average_precision):
        with pytest.raises(pkg._lib.McgraNotSupported):
            f(lab, _dev(Z), 3)
        with pytest.raises(pkg._lib.McgraNotSupported):
            f(lab, _dev(rng.randn(n, 129).astype(np.float32)), 0)
        bad = Z.copy(); bad[7, 3] = np.nan
        with pytest.raises(pkg._lib.McgraError):
            f(lab, _dev(bad), 0)
        with pytest.raises(pkg._lib.McgraError):
            f(lab, _dev(Z), 0, [0, n])
    wide = _dev(rng.randn(n, 129).astype(np.float32) * 0.05)           # the wide route takes any width
    assert 0.0 < E.average_precision(lab, E.decode_scores(wide, 0)) < 1.0


# ------------------------------------------------------------------------------------------------------ 9. main.py
def test_main_notrain_test_ap(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode notrain_test --ap on the committed brazil files (n = 131): res["ap"] holds the five priors, each the
    average precision of that prior's materialised scores; the reference's four lines are still printed."""
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M
    seen = []
    orig = M.prior_rank_metrics
    monkeypatch.setattr(M, "prior_rank_metrics", lambda *a: seen.append(a) or orig(*a))
    monkeypatch.chdir(tmp_path)
    root = os.path.join(H.GOLDEN, "dataset")
    argv = ["--mode", "notrain_test", "--dataset", "brazil", "--dataset_root", root]
    res = M.run(M.build_parser().parse_args(argv + ["--ap"]))
    out = capsys.readouterr().out
    assert sorted(res) == ["ap", "feature", "label", "layer1", "layer2", "out"]
    assert sorted(res["ap"]) == ["feature", "label", "layer1", "layer2", "out"]
    adj, feature_adj, H_A1, H_A2, Y_A, label_adj, dataset = seen[0]
    scores = {"feature": feature_adj.to(adj.device), "layer1": E.decode_scores(H_A1, 4), "layer2": E.decode_scores(H_A2, 4),
              "out": E.decode_scores(Y_A, 4), "label": _dev(label_adj)}
    for k, S in scores.items():
        v = res["ap"][k]
        assert isinstance(v, float) and 0.0 < v <= 1.0 and v == E.average_precision(adj, S), (k, v)
        assert res[k] == E.roc_auc(adj, S), k
        assert f"{k} ap= {v}" in out, (k, out)
    assert abs(res["ap"]["layer2"] - T.sklearn_average_precision(adj.cpu().numpy(), scores["layer2"].cpu().numpy())) <= TOL
    for label, key in (("feautre adj=", "feature"), ("layer1 adj=", "layer1"), ("layer2 adj=", "layer2"), ("out adj=", "out")):
        assert f"{label} {res[key]}" in out, (label, out)
    assert out.index("out adj=") < out.index("feature ap=")
    plain = M.run(M.build_parser().parse_args(argv))                   # without the flag: the keys and values it had
    assert plain == {k: v for k, v in res.items() if k != "ap"}
    assert " ap=" not in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "results")


def test_main_evaluate_ap(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate --ap on brazil: the three average precisions are sklearn's on the matrices that were scored,
    the AUCs are those of the same run without --ap bit for bit, the log gains one line; without --ap it gains nothing."""
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "brazil", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    pools = []
    pool = M.metric_pool
    monkeypatch.setattr(M, "metric_pool", lambda *a: pools.append(a) or pool(*a))
    plain = M.run(M.build_parser().parse_args(argv + ["--log_name", "plain.txt"]))
    out_plain = capsys.readouterr().out
    assert len(pools) == 3 and sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.rank_metrics

    def record(real, pred, idx=None):
        v = orig(real, pred, idx)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx), v))
        return v

    monkeypatch.setattr(M.engine, "rank_metrics", record)
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "ap.txt", "--ap"]))
    out = capsys.readouterr().out
    assert len(seen) == 3 and len(pools) == 3                          # one rank_metrics call per index set, no metric_pool
    assert sorted(res) == sorted(list(plain) + ["ap_attack", "ap_train", "ap_all"])
    for (real, pred, idx, v), k in zip(seen, ("attack", "train", "all")):
        assert res[f"auc_{k}"] == v[0] and res[f"ap_{k}"] == v[1]
        ref = T.sklearn_average_precision(real, pred, idx)
        print(f"ap_{k}: {v[1]!r} sklearn {ref!r}")
        assert abs(v[1] - ref) <= TOL, (k, v, ref)
        assert res[f"auc_{k}"] == plain[f"auc_{k}"], k                  # bit for bit the run without --ap
    assert 0.0 < res["ap_all"] < 1.0
    assert f"current auc={res['auc_all']}\ncurrent ap={res['ap_all']}\n" in out
    assert "current ap=" not in out_plain
    log = open(tmp_path / "results" / "ap.txt").read().split("\n")
    assert log[1] == (f"In attack graph: AUC={res['auc_attack']}\tIn train graph: AUC={res['auc_train']}\t"
                      f"In Whole Graph: AUC={res['auc_all']}")
    assert log[2] == (f"In attack graph: AP={res['ap_attack']}\tIn train graph: AP={res['ap_train']}\t"
                      f"In Whole Graph: AP={res['ap_all']}")
    assert log[3].startswith("current density:") and "ap=True" in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "AP=" not in old and "ap=" not in old and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[3:]
