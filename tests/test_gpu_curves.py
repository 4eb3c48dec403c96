"""The ROC and precision-recall curves on the device (mcgra_rank_curves, engine.roc_curve / precision_recall_curve /
rank_curves, main.py --curves) against tests/curve_truth.py: counts, tps, fps and thresholds element for element, the
wrapper's rates within one unit in the last place (one float64 division of exact integers on either side), the best-F1 level
exactly; the capacity rule, determinism, and the neighbouring entries' bits.  The shapes are the smallest at which a sort
tile (1024 keys), a 256-lane block and the one-lane-per-block range of the count scan (1024 blocks) are crossed.
Run with -m gpu.

tests/test_curves_cases_cpu.py checks, without a GPU, that curve_truth is sklearn on these inputs and that the inputs have
the properties the cases are there for."""
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import ap_truth as AP
from tests import curve_truth as T
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _labels(rng, n, p):
    return (rng.rand(n, n) < p).astype(np.float32)


def _distinct(rng, real):
    """n^2 distinct scores k / n^2 that lean to the edges."""
    n = len(real)
    rank = np.argsort(np.argsort((rng.rand(n, n) + 0.4 * real).reshape(-1)))
    return (rank.reshape(n, n) / np.float32(n * n)).astype(np.float32)


def _cases():
    """name -> (real, pred, idx)"""
    rng = np.random.RandomState(41)
    out = {}
    real = _labels(rng, 40, 0.2)
    out["n40_distinct"] = (real, _distinct(rng, real), None)
    real = _labels(rng, 70, 0.1)
    out["n70_distinct"] = (real, _distinct(rng, real), None)
    quant = (np.floor(8 * (rng.rand(70, 70) + 0.3 * real) / 1.3) / 8).astype(np.float32)
    out["n70_quant8"] = (real, quant, None)
    zeros = np.where(rng.rand(70, 70) < 0.9, 0.0, rng.rand(70, 70) + 0.3 * real).astype(np.float32)
    zeros[rng.rand(70, 70) < 0.2] *= np.float32(-1)          # -0.0 among the zeros, negatives among the rest
    zeros[0, 0], zeros[0, 1], zeros[0, 2] = -0.0, 1e-42, -0.5
    out["n70_zeros"] = (real, zeros, None)
    real = _labels(rng, 515, 0.01)
    out["n515_uniform"] = (real, (rng.rand(515, 515) * 0.7 + 0.3 * real).astype(np.float32), None)
    a = np.triu(rng.rand(1000, 1000) < 0.0016, 1)
    real = (a | a.T).astype(np.float32)                      # a sparse symmetric graph: about 1.6 edges per node
    out["n1000_sparse"] = (real, (rng.rand(1000, 1000).astype(np.float32) * np.float32(0.7) + np.float32(0.3) * real), None)
    # selections of the n = 70 cases: a subset, a permutation of all nodes, a subset with repeats
    out["n70_distinct_subset"] = out["n70_distinct"][:2] + (rng.permutation(70)[:30].copy(),)
    out["n70_zeros_permuted"] = out["n70_zeros"][:2] + (rng.permutation(70),)
    out["n70_quant8_repeats"] = out["n70_quant8"][:2] + (rng.randint(0, 70, 50),)
    # degenerate: one level, two levels, one class, and two levels of equal best F1 (1/2 at thresholds 3 and 2)
    real = _labels(rng, 20, 0.3)
    out["n20_one_level"] = (real, np.full((20, 20), 0.5, np.float32), None)
    out["n20_two_levels"] = (real, (rng.rand(20, 20) < 0.5).astype(np.float32), None)
    out["n20_no_positive"] = (np.zeros((20, 20), np.float32), rng.rand(20, 20).astype(np.float32), None)
    out["n20_no_negative"] = (np.ones((20, 20), np.float32), rng.rand(20, 20).astype(np.float32), None)
    lab = np.array([1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.float32).reshape(4, 4)
    sc = np.array([3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], np.float32).reshape(4, 4)
    out["n4_f1_tie"] = (lab, sc, None)
    return out


CASES = _cases()
TIE_FREE = ["n40_distinct", "n70_distinct", "n70_distinct_subset"]
TIED = ["n70_zeros", "n70_zeros_permuted", "n515_uniform", "n1000_sparse"]       # ties beside many single-entry levels
QUANTISED = ["n70_quant8", "n70_quant8_repeats"]                                 # a handful of levels, each spanning blocks
DEGENERATE = ["n20_one_level", "n20_two_levels", "n20_no_positive", "n20_no_negative", "n4_f1_tie"]


@functools.lru_cache(maxsize=None)
def truth(name, drop):
    return T.curves(*CASES[name], drop_intermediate=drop)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


@functools.lru_cache(maxsize=None)
def _dev_case(name):
    import torch
    real, pred, idx = CASES[name]
    return (torch.as_tensor(real, device="cuda:0"), torch.as_tensor(pred, device="cuda:0"),
            None if idx is None else torch.as_tensor(np.asarray(idx, np.int64), device="cuda:0"))


SENTINEL = -7


def raw(pkg, name, drop, cap, roc=True, pr=True, best=True):
    """One mcgra_rank_curves call on buffers pre-filled with a sentinel: (rc, counts, roc, pr, best, best_thr)."""
    import torch
    real, pred, ix = _dev_case(name)
    n = real.shape[0]

    def bufs(want):
        if not want:
            return None, None, None
        return (torch.full((max(cap, 1),), SENTINEL, device="cuda:0", dtype=torch.int64),
                torch.full((max(cap, 1),), SENTINEL, device="cuda:0", dtype=torch.int64),
                torch.full((max(cap, 1),), float(SENTINEL), device="cuda:0", dtype=torch.float32))

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    r, q = bufs(roc), bufs(pr)
    counts, b, thr = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 3)(*([SENTINEL] * 3)), ctypes.c_float(SENTINEL)
    rc = pkg._lib.lib.mcgra_rank_curves(None, n, p(real), real.stride(0), p(pred), pred.stride(0), p(ix),
                                        n if ix is None else ix.numel(), int(drop), cap, p(r[0]), p(r[1]), p(r[2]), p(q[0]),
                                        p(q[1]), p(q[2]), counts, b if best else None, ctypes.byref(thr) if best else None)
    torch.cuda.synchronize()
    host = lambda ts: None if ts[0] is None else tuple(t.cpu().numpy() for t in ts)
    return rc, tuple(counts), host(r), host(q), tuple(b), thr.value


def _check_points(got, want, count, what):
    for g, w, part in zip(got, want, ("tps", "fps", "thresholds")):
        assert g[:count].dtype == w.dtype and np.array_equal(g[:count], w), (what, part)
        assert (g[count:] == SENTINEL).all(), (what, part, "written past the curve")
    z = got[2][:count]
    assert not (np.signbit(z) & (z == 0)).any(), (what, "-0.0 reported")


def _within_one_ulp(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print(f"{what}: max |got - want| / |want| = {float((err / np.maximum(np.abs(want[ok]), 1e-300)).max()) if ok.any() else 0.0:.3e}")
    assert (err <= 2.0 ** -52 * np.abs(want[ok])).all(), what


# --------------------------------------------------------------------------------- 1. the integer curves and the rates
@pytest.mark.parametrize("drop", [True, False], ids=["drop", "keep"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_curves_against_the_truth(pkg, name, drop):
    from mc_gra_amd import engine as E
    want = truth(name, drop)
    cap = want["counts"][2] + 1 + 3                                  # levels + 1 always suffices; 3 spare entries stay untouched
    rc, counts, roc, pr, best, thr = raw(pkg, name, drop, cap)
    print(f"{name} drop={drop}: counts {counts} best {best} at {thr}")
    assert rc == 0, pkg._lib.lib.mcgra_last_error()
    assert counts == want["counts"], (counts, want["counts"])
    _check_points(roc, want["roc"], counts[3], (name, "roc"))
    _check_points(pr, want["pr"], counts[4], (name, "pr"))
    assert roc[2][0] == np.inf
    if want["best"] is None:
        assert best == (SENTINEL,) * 3 and thr == SENTINEL           # P == 0: not written
    else:
        assert best == want["best"], (best, want["best"])
        assert thr == T.levels(*CASES[name])[2][want["best"][2]]
    real, pred, ix = _dev_case(name)
    got = E.rank_curves(real, pred, ix, drop)
    assert (got["positives"], got["negatives"], got["levels"], got["roc_points"], got["pr_points"]) == want["counts"]
    for g, key in zip(got["roc"][:2] + got["pr"][:2], ("fpr", "tpr", "precision", "recall")):
        _within_one_ulp(g, want[key], (name, drop, key))
    for g, w in ((got["roc"][2], want["roc"][2]), (got["pr"][2], want["pr_thresholds"])):
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and np.array_equal(g, w)
    b = got["best_f1"]
    if want["best"] is None:
        assert math.isnan(b["f1"]) and math.isnan(b["threshold"])
    else:
        tp, fp, _ = want["best"]
        assert (b["tp"], b["fp"]) == (tp, fp) and b["f1"] == 2 * tp / (tp + fp + want["counts"][0])
        assert b["precision"] == tp / (tp + fp) and b["recall"] == tp / want["counts"][0] and b["threshold"] == thr
    # the single-curve wrappers: the same arrays (roc_curve drops by default, precision_recall_curve does not)
    for g, w in zip(E.roc_curve(real, pred, ix, drop), got["roc"]):
        assert np.array_equal(g.cpu().numpy(), w.cpu().numpy(), equal_nan=True)
    for g, w in zip(E.precision_recall_curve(real, pred, ix, drop), got["pr"]):
        assert np.array_equal(g.cpu().numpy(), w.cpu().numpy(), equal_nan=True)


def test_curves_of_1100_selected_nodes(pkg):
    """n_idx = 1100 of n = 1200 nodes in a shuffled order: more selected rows than the classify and emit passes have blocks
    (1024), so the first blocks take a second row.  64 score levels, about 1 % positives; both curves and the best level
    element for element."""
    import torch
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(1100)
    real = _labels(rng, 1200, 0.01)
    pred = (np.floor(64 * (rng.rand(1200, 1200) + 0.3 * real) / 1.3) / 64).astype(np.float32)
    idx = rng.permutation(1200)[:1100].copy()
    want = T.curves(real, pred, idx, drop_intermediate=True)
    assert want["counts"][0] > 0 and want["counts"][2] == 64
    dev = lambda x: torch.as_tensor(x, device="cuda:0")
    counts, roc, pr, best = E._rank_curves(dev(real), dev(pred), dev(idx), True, True, True, True)
    print("n_idx 1100: counts", counts, "best", best)
    assert counts == want["counts"]
    for got, w, what in ((roc, want["roc"], "roc"), (pr, want["pr"], "pr")):
        for g, x, part in zip(got, w, ("tps", "fps", "thresholds")):
            assert np.array_equal(g.cpu().numpy(), x), (what, part)
    assert best[:3] == want["best"] and best[3] == T.levels(real, pred, idx)[2][want["best"][2]]


def test_wrapper_defaults_are_sklearns(pkg):
    from mc_gra_amd import engine as E
    real, pred, ix = _dev_case("n70_zeros")
    assert E.roc_curve(real, pred)[0].numel() == truth("n70_zeros", True)["counts"][3]
    assert E.precision_recall_curve(real, pred)[2].numel() == truth("n70_zeros", False)["counts"][4]


# ------------------------------------------------------------------------------------------------------ 2. capacity
@pytest.mark.parametrize("name", ["n40_distinct", "n70_zeros", "n20_one_level"])
def test_capacity_one_short_is_refused_and_nothing_is_written(pkg, name):
    want = truth(name, True)
    need = max(want["counts"][3], want["counts"][4])
    rc, counts, roc, pr, _, _ = raw(pkg, name, True, need - 1)
    assert rc == -4 and str(need).encode() in pkg._lib.lib.mcgra_last_error(), pkg._lib.lib.mcgra_last_error()
    assert counts == want["counts"]
    for arr in roc + pr:
        assert (arr == SENTINEL).all()
    rc, counts, roc, pr, _, _ = raw(pkg, name, True, need)
    assert rc == 0 and counts == want["counts"]
    _check_points(roc, want["roc"], counts[3], (name, "roc"))
    _check_points(pr, want["pr"], counts[4], (name, "pr"))
    # a curve that is not asked for does not count: the PR curve alone fits its own need
    rc, counts, roc, pr, _, _ = raw(pkg, name, True, want["counts"][4], roc=False)
    assert rc == 0 and roc is None
    _check_points(pr, want["pr"], counts[4], (name, "pr alone"))


def test_wrapper_retries_once_from_the_counts(pkg, monkeypatch):
    from mc_gra_amd import engine as E
    calls = []
    orig = E.lib.mcgra_rank_curves

    class Spy:
        def __getattr__(self, k):
            return getattr(E.lib, k)

        def mcgra_rank_curves(self, *a):
            rc = orig(*a)
            calls.append((a[9], rc))
            return rc

    real, pred, ix = _dev_case("n70_zeros")
    want = truth("n70_zeros", True)
    monkeypatch.setattr(E, "lib", Spy())
    got = E.rank_curves(real, pred, ix, True, _first_cap=5)
    assert calls == [(5, -4), (max(want["counts"][3], want["counts"][4]), 0)], calls
    assert got["roc_points"] == want["counts"][3] and got["roc"][2].numel() == want["counts"][3]
    assert got["pr"][2].numel() == want["counts"][4]
    del calls[:]
    E.rank_curves(real, pred, ix, True)
    assert len(calls) == 1 and calls[0][1] == 0                                   # the default first guess fits


# ------------------------------------------------------------------------------------- 3. determinism and neighbours
@pytest.mark.parametrize("name", ["n515_uniform", "n70_quant8_repeats"])
def test_two_calls_and_single_curves_give_identical_bits(pkg, name):
    want = truth(name, True)
    cap = want["counts"][2] + 1
    a, b = raw(pkg, name, True, cap), raw(pkg, name, True, cap)
    assert a[0] == b[0] == 0 and a[1] == b[1] and a[4:] == b[4:]
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        assert x.tobytes() == y.tobytes()
    r = raw(pkg, name, True, cap, pr=False)
    q = raw(pkg, name, True, cap, roc=False, best=False)
    assert r[0] == q[0] == 0 and r[3] is None and q[2] is None and r[1] == q[1] == a[1] and r[4:] == a[4:]
    for x, y in zip(r[2] + q[3], a[2] + a[3]):
        assert x.tobytes() == y.tobytes()


def _exact_auc(name):
    tps, fps, _ = T.levels(*CASES[name])
    p, q = np.diff(np.r_[0, tps])[::-1], np.diff(np.r_[0, fps])[::-1]            # per level, ascending
    P, N = int(tps[-1]), int(fps[-1])
    if P == 0 or N == 0:
        return float("nan")
    u2, below = 0, 0
    for pv, qv in zip(p.tolist(), q.tolist()):
        u2 += pv * (2 * below + qv)
        below += qv
    return float(Fraction(u2, 2 * P * N))


@pytest.mark.parametrize("name", ["n70_zeros", "n70_quant8_repeats", "n515_uniform", "n20_no_positive", "n20_no_negative"])
def test_the_neighbouring_entries_keep_their_bits_and_the_area_agrees(pkg, name):
    """mcgra_roc_auc / mcgra_rank_metrics share classify, emit and the sorts with the curves: the AUC is still the nearest
    double of the exact fraction, the average precision still the truth of tests/ap_truth.py (and their single-class early
    return still stands), and the trapezoid area under the returned ROC curve is that AUC."""
    from mc_gra_amd import engine as E
    real, pred, ix = _dev_case(name)
    want_auc = _exact_auc(name)
    auc, ap = E.rank_metrics(real, pred, ix)
    alone = E.roc_auc(real, pred, ix)
    want_ap = AP.average_precision(*CASES[name])
    tps = T.levels(*CASES[name])[0]
    if math.isnan(want_auc):
        assert math.isnan(auc) and math.isnan(alone)
        assert (math.isnan(ap) and tps[-1] == 0) or ap == 1.0
        return
    assert auc == want_auc and alone == want_auc, (auc, alone, want_auc)
    assert abs(ap - want_ap) <= 4e-15 * want_ap, (ap, want_ap)                    # the kernel's own bound (csrc/auc.hip)
    for drop in (True, False):
        fpr, tpr, _ = (t.cpu().numpy() for t in E.roc_curve(real, pred, ix, drop))
        area = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) * 0.5))
        assert abs(area - auc) <= 1e-12, (drop, area, auc)


def test_refusals_on_the_device(pkg):
    """What roc_auc refuses, rank_curves refuses with the same codes: NaN / inf scores, labels outside {0, 1}, an id outside
    [0, n); counts stay unwritten."""
    import torch
    from mc_gra_amd import engine as E
    real, pred, _ = _dev_case("n40_distinct")
    for bad in (float("nan"), float("inf"), -float("inf")):
        p2 = pred.clone(); p2[3, 7] = bad
        with pytest.raises(pkg._lib.McgraError, match="NaN or infinite"):
            E.rank_curves(real, p2)
    r2 = real.clone(); r2[5, 5] = 0.5
    with pytest.raises(pkg._lib.McgraError, match="neither 0 nor 1"):
        E.roc_curve(r2, pred)
    with pytest.raises(pkg._lib.McgraError, match="outside"):
        E.precision_recall_curve(real, pred, [0, 40])
    p2 = pred.clone(); p2[3, 7] = float("nan")                        # outside the selection: not looked at
    E.roc_curve(real, p2, [0, 1, 2])
    with pytest.raises(ValueError):
        E.rank_curves(real.cpu(), pred)


# ------------------------------------------------------------------------------------------------------ 4. main.py
def test_main_evaluate_curves(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed brazil files (n = 131), 6 epochs: the .npz of --curves is curve_truth on the
    modified_adj that was scored, for each index set; a run without the flag returns and logs what it did before the flag
    existed."""
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "brazil", "--dataset_root", root, "--epochs", "6", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain = M.run(M.build_parser().parse_args(argv + ["--log_name", "plain.txt"]))
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.rank_curves

    def record(real, pred, idx=None, drop_intermediate=True):
        v = orig(real, pred, idx, drop_intermediate)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx)))
        return v

    monkeypatch.setattr(M.engine, "rank_curves", record)
    path = str(tmp_path / "curves.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "curves.txt", "--curves", path]))
    out = capsys.readouterr().out
    assert sorted(res) == sorted(list(plain) + ["curves_attack", "curves_train", "curves_all"]) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flag, bit for bit
    z = np.load(path)
    assert sorted(z.files) == sorted(f"{c}_{s}" for s in ("attack", "train", "all") for c in
                                     ("roc_fpr", "roc_tpr", "roc_thresholds", "pr_precision", "pr_recall", "pr_thresholds"))
    for (real, pred, idx), name in zip(seen, ("attack", "train", "all")):
        on, off = T.curves(real, pred, idx, True), T.curves(real, pred, idx, False)
        d = res[f"curves_{name}"]
        assert sorted(d) == ["best_f1", "best_threshold", "levels", "pr_points", "roc_points"]
        assert (d["levels"], d["roc_points"], d["pr_points"]) == (on["counts"][2], on["counts"][3], off["counts"][4])
        tp, fp, l = on["best"]
        assert d["best_f1"] == 2 * tp / (tp + fp + on["counts"][0]) and d["best_threshold"] == T.levels(real, pred, idx)[2][l]
        for key, w in (("roc_fpr", on["fpr"]), ("roc_tpr", on["tpr"]), ("pr_precision", off["precision"]), ("pr_recall", off["recall"])):
            g = z[f"{key}_{name}"]
            assert g.dtype == np.float64 and g.shape == w.shape and (np.abs(g - w) <= 2.0 ** -52 * np.abs(w)).all(), (key, name)
        assert np.array_equal(z[f"roc_thresholds_{name}"], on["roc"][2]) and z[f"roc_thresholds_{name}"].dtype == np.float32
        assert np.array_equal(z[f"pr_thresholds_{name}"], off["pr_thresholds"])
    assert seen[2][2] is None and res["curves_all"]["levels"] > 2
    d = res["curves_all"]
    assert f"current auc={res['auc_all']}\ncurrent best_f1={d['best_f1']} (threshold={d['best_threshold']})\n" in out
    assert "best_f1" not in out_plain
    log = open(tmp_path / "results" / "curves.txt").read().split("\n")
    assert log[2].startswith("In attack graph: ROC points=") and f"best F1={d['best_f1']} at {d['best_threshold']}" in log[2]
    assert log[3].startswith("current density:") and "curves=" in log[0] and "topk" not in log[0] and "ap=" not in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "curves" not in old and "ROC" not in old and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[3:]
