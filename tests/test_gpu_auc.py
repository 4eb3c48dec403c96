"""The recovered-adjacency AUC on the device (mcgra_roc_auc, engine.roc_auc, main.metric_pool): the reference's own AUCs on
the committed fixtures, ties and edge cases against sklearn (roc_curve + auc, as main.py:66-75 calls them) and against the
exact Mann-Whitney fraction, argument checks, more than 2^31 entries, and main.py end to end.  Run with -m gpu."""
import lzma
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

FIXTURES = [f"attack_{c}" for c in H.attack_cases()] + ["cw_s48_mse_cw"]


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


def _sklearn(real, pred, idx=None):
    from sklearn.metrics import auc, roc_curve
    if idx is not None:
        real, pred = real[idx][:, idx], pred[idx][:, idx]
    fpr, tpr, _ = roc_curve(real.reshape(-1), pred.reshape(-1))
    return auc(fpr, tpr)


def _exact(real, pred, idx=None):
    """U / (P N) as the nearest double (Fraction -> float rounds correctly), from integer counts per distinct float32 score;
    entry (i, j) weighs c_i c_j, c = how often idx names each node (the gathered matrix repeats rows and columns)."""
    n = len(real)
    c = np.ones(n) if idx is None else np.bincount(np.asarray(idx).reshape(-1), minlength=n).astype(np.float64)
    w = (c[:, None] * c[None, :]).reshape(-1)
    vals, inv = np.unique(pred.reshape(-1).astype(np.float32), return_inverse=True)    # -0.0 == +0.0: one value
    inv = inv.reshape(-1)
    lab = real.reshape(-1) == 1
    p = np.bincount(inv[lab], weights=w[lab], minlength=len(vals))
    q = np.bincount(inv[~lab], weights=w[~lab], minlength=len(vals))
    return _fraction([int(x) for x in p], [int(x) for x in q])


def _fraction(p, q):
    P, N = int(sum(p)), int(sum(q))
    if P == 0 or N == 0:
        return float("nan")
    u2, below = 0, 0
    for pv, qv in zip(p, q):
        u2 += int(pv) * (2 * below + int(qv))
        below += int(qv)
    return float(Fraction(u2, 2 * P * N))


@pytest.mark.parametrize("name", FIXTURES)
def test_roc_auc_matches_the_reference_metric_pool(pkg, name):
    """tests/golden: the reference's final inference_adj and the AUC its metric_pool computed on it (make_golden.py)."""
    from mc_gra_amd import engine as E
    z = np.load(os.path.join(H.GOLDEN, f"{name}.npz"))
    got = E.roc_auc(_dev(z["adj"]), _dev(z["final"]), z["idx_attack"])
    assert abs(got - float(z["auc"])) <= 1e-12, (got, float(z["auc"]))
    assert got == _exact(z["adj"], z["final"], z["idx_attack"])


def _labels(rng, n, p=0.3):
    return (rng.rand(n, n) < p).astype(np.float32)


def _cases():
    rng = np.random.RandomState(7)
    out = {}
    n = 1500
    out["quantised"] = (_labels(rng, n), (rng.randint(0, 5, (n, n)) * 0.25).astype(np.float32), None)
    zs = np.where(rng.rand(n, n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    zs[rng.rand(n, n) < 0.3] = 1.0
    out["signed_zeros"] = (_labels(rng, n), zs, None)
    out["all_equal"] = (_labels(rng, 700), np.full((700, 700), 0.5, np.float32), None)
    tiny = np.array([-1.5, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 3e-39, 1e-38, 2.0], np.float32)
    m = 1100
    out["negative_subnormal"] = (_labels(rng, m, 0.1), tiny[rng.randint(0, len(tiny), (m, m))], None)
    cont = rng.randn(m, m).astype(np.float32)
    out["perm"] = (_labels(rng, m, 0.05), cont, rng.permutation(m))
    out["subset"] = (_labels(rng, m, 0.05), cont, rng.choice(m, 300, replace=False))
    out["repeats"] = (_labels(rng, m, 0.2), (rng.randint(0, 9, (m, m)) * 0.5 - 2).astype(np.float32), rng.randint(0, m, 900))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_roc_auc_ties_and_selections_against_sklearn(pkg, name):
    from mc_gra_amd import engine as E
    real, pred, idx = CASES[name]
    got = E.roc_auc(_dev(real), _dev(pred), None if idx is None else _dev(idx))
    ref = _sklearn(real, pred, idx)
    assert abs(got - ref) <= 1e-12, (name, got, ref)
    assert got == _exact(real, pred, idx), name
    if name == "all_equal":
        assert got == 0.5


def test_roc_auc_single_class_is_nan(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(1)
    s = _dev(rng.rand(64, 64).astype(np.float32))
    assert math.isnan(E.roc_auc(_dev(np.zeros((64, 64), np.float32)), s))
    assert math.isnan(E.roc_auc(_dev(np.ones((64, 64), np.float32)), s))
    lab = np.zeros((64, 64), np.float32)
    lab[5, 9] = 1.0
    assert math.isnan(E.roc_auc(_dev(lab), s, [0, 1, 2, 3]))       # the positive is not selected


def test_roc_auc_refuses_what_sklearn_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(2)
    lab = _labels(rng, 80)
    s = rng.rand(80, 80).astype(np.float32)
    bad = lab.copy(); bad[3, 4] = 2.0
    with pytest.raises(pkg._lib.McgraError):
        E.roc_auc(_dev(bad), _dev(s))
    for v in (np.nan, np.inf, -np.inf):
        t = s.copy(); t[7, 70] = v
        with pytest.raises(pkg._lib.McgraError):
            E.roc_auc(_dev(lab), _dev(t))
        # an entry outside idx x idx is not looked at
        assert E.roc_auc(_dev(lab), _dev(t), np.arange(60)) == _exact(lab, s, np.arange(60))
    with pytest.raises(pkg._lib.McgraError):
        E.roc_auc(_dev(lab), _dev(s), [0, 80])                      # a node id out of range
    with pytest.raises(pkg._lib.McgraNotSupported):
        E.roc_auc(_dev(lab), _dev(s), np.arange(65536) % 80)        # 2 P N could pass 2^64
    assert E.roc_auc(_dev(lab), _dev(s), np.arange(65535) % 80) == _exact(lab, s, np.arange(65535) % 80)


def test_roc_auc_is_deterministic(pkg):
    from mc_gra_amd import engine as E
    real, pred, _ = CASES["perm"]
    r, p = _dev(real), _dev(pred)
    a = [E.roc_auc(r, p).hex() for _ in range(2)] + [E.roc_auc(r, p, np.arange(len(real))[::-1].copy()).hex()]
    assert len(set(a)) == 1, a


@pytest.mark.parametrize("n,pad", [(10000, 3), (46341, 0)])
def test_roc_auc_at_scale_against_the_exact_fraction(pkg, n, pad):
    """n = 46 341: n^2 > 2^31 entries.  Scores from a few known levels, drawn on the device with their labels, so the exact U
    comes from a device bincount of (level, label) pairs.  pad: the scores sit in a wider buffer (rows not 16-byte aligned)."""
    import torch
    from mc_gra_amd import engine as E
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
    exact = _fraction([p[v] for v in order], [q[v] for v in order])
    got = E.roc_auc(labels, scores)
    assert abs(got - exact) <= 1e-12 and got == exact, (got, exact)


def test_metric_pool_on_device_tensors(pkg):
    from mc_gra_amd import main as M
    for name in ("attack_s200_hsic", "cw_s48_mse_cw"):
        z = np.load(os.path.join(H.GOLDEN, f"{name}.npz"))
        got = M.metric_pool(_dev(z["adj"]), _dev(z["final"]), z["idx_attack"])
        assert abs(got - float(z["auc"])) <= 1e-12, (name, got, float(z["auc"]))


def test_main_run_auc_equals_sklearn_on_the_same_matrices(pkg, tmp_path, monkeypatch):
    """A Cora README line through main.run: the three AUCs it returns and logs are sklearn's on the matrices it scored."""
    from mc_gra_amd import main as M
    seen = []
    orig = M.metric_pool

    def record(ori, inf, idx):
        v = orig(ori, inf, idx)
        seen.append((ori.cpu().numpy(), inf.cpu().numpy(), None if idx is None else np.asarray(idx), v))
        return v

    monkeypatch.setattr(M, "metric_pool", record)
    monkeypatch.chdir(tmp_path)
    root = tmp_path / "dataset"                     # cora.npz is committed as an xz archive of the reference's file
    root.mkdir()
    with lzma.open(os.path.join(H.GOLDEN, "dataset", "cora.npz.xz")) as src:
        (root / "cora.npz").write_bytes(src.read())
    root = str(root)
    args = M.build_parser().parse_args(["--dataset", "cora", "--dataset_root", root, "--epochs", "6", "--w1", "0.01",
                                        "--w6", "10", "--w7", "10", "--w9", "10", "--w10", "1000", "--lr", "-2", "--useH_A",
                                        "--useY_A", "--useY", "--measure", "MSELoss"])
    res = M.run(args)
    assert len(seen) == 3
    for (ori, inf, idx, v), key in zip(seen, ("auc_attack", "auc_train", "auc_all")):
        assert res[key] == v
        assert abs(v - _sklearn(ori, inf, idx)) <= 1e-12, (key, v)
    assert 0.5 < res["auc_all"] < 1.0
    log = open(tmp_path / "results" / "result.txt").read()
    assert f"In Whole Graph: AUC={res['auc_all']}" in log
