"""The recovered graph on the device (mcgra_topk_metrics, mcgra_top_pairs, engine.topk_metrics / top_pairs, main.py --topk /
--save_edges) against tests/topk_truth.py: counts, threshold bits and the edge list element for element over shapes from one
pair to 1.1e6 pairs (more than 1024 stretches of 256, so every block ranks ties behind a scan of the others' counts), score
families with the threshold inside a tie, selections, refusals, bit-level determinism and main.py end to end.  Every expected
value is exact: every comparison is equality.  Run with -m gpu.

tests/test_topk_cases_cpu.py checks, without a GPU, that these inputs have the properties the cases are there for."""
import functools
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import topk_truth as T

pytestmark = pytest.mark.gpu


def _graph(rng, n, p):
    a = np.triu(rng.rand(n, n) < p, 1)
    return (a | a.T).astype(np.float32)


def _cases():
    """name -> (real, pred, idx, pad): pad > 0 puts pred's rows into a buffer that many columns wider."""
    rng = np.random.RandomState(23)
    tiny = np.array([-1.5, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 3e-39, 1e-38, 2.0], np.float32)
    out = {}
    out["n2_one_pair"] = (np.array([[0, 1], [1, 0]], np.float32), rng.rand(2, 2).astype(np.float32), None, 0)
    out["n3_levels"] = (_graph(rng, 3, 0.6), (rng.randint(0, 2, (3, 3)) * 0.5).astype(np.float32), None, 0)
    out["n80_continuous_asym"] = ((rng.rand(80, 80) < 0.2).astype(np.float32), rng.randn(80, 80).astype(np.float32), None, 0)
    out["n80_equal_padded"] = (_graph(rng, 80, 0.2), np.full((80, 80), 0.5, np.float32), None, 3)
    out["n257_levels_asym"] = (_graph(rng, 257, 0.1), (rng.randint(0, 4, (257, 257)) * 0.25).astype(np.float32), None, 0)
    out["n257_special"] = (_graph(rng, 257, 0.1), tiny[rng.randint(0, len(tiny), (257, 257))], None, 5)
    real = _graph(rng, 1500, 0.01)
    cont = rng.randn(1500, 1500).astype(np.float32)
    out["n1500_continuous_sym"] = (real, ((cont + cont.T) * np.float32(0.5) + real).astype(np.float32), None, 0)
    out["n1500_levels"] = (real, (rng.randint(0, 5, (1500, 1500)) * 0.25).astype(np.float32), None, 0)
    out["n1500_clamped"] = (real, np.clip(rng.randn(1500, 1500) * 2 + 1.5 + real, 0, 1).astype(np.float32), None, 0)
    big = _graph(rng, 2048, 0.01)
    out["n2048_subset_levels_asym"] = (big, (rng.randint(0, 3, (2048, 2048)) * 0.5 - 0.5).astype(np.float32),
                                       rng.permutation(2048)[:1500].copy(), 0)
    return out


CASES = _cases()
# the cases whose threshold, at tie_k(), falls inside a group of equal scores that spans many 256-wide stretches (n3_levels
# ties too, but its 3 pairs cannot)
TIE_CASES = ["n80_equal_padded", "n257_levels_asym", "n257_special", "n1500_levels", "n1500_clamped",
             "n2048_subset_levels_asym"]


@functools.lru_cache(maxsize=None)
def tie_k(name):
    """A k inside a tie group: the scores' median group, half of it taken (no tie in the case: a third of the pairs)."""
    real, pred, idx, _ = CASES[name]
    s, _, _, _ = T.packed(real, pred, idx)
    m = len(s)
    if m < 3:
        return 1
    order = T.ranking(s)
    mid = s[order[m // 2]]
    group = np.flatnonzero(s[order] == mid)              # contiguous ranks
    return int(group[0] + max(1, len(group) // 2)) if len(group) > 1 else max(1, m // 3)


@functools.lru_cache(maxsize=None)
def ks_of(name):
    """k in {1, P, inside a tie group, m} and 0 (= P)."""
    real, pred, idx, _ = CASES[name]
    t = T.top_k(real, pred, None, idx)
    return tuple(sorted({1, max(1, t["positives"]), tie_k(name), t["pairs"]})) + (0,)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x, pad=0):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    if pad:
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda:0")      # the padding is never read
        buf[:, :t.shape[1]] = t
        t = buf[:, :t.shape[1]]
    return t


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_metrics(got, want, what):
    print(f"{what}: got { {k: got[k] for k in ('k', 'positives', 'hits', 'pairs', 'f1', 'threshold')} }")
    for key in ("k", "positives", "hits", "pairs"):
        assert got[key] == want[key] and isinstance(got[key], int), (what, key, got[key], want[key])
    for key in ("precision", "recall", "f1"):
        assert _same_float(got[key], want[key]), (what, key, got[key], want[key])
    if want["k"]:
        assert T.bits(got["threshold"])[0] == T.bits(want["threshold"])[0], (what, got["threshold"], want["threshold"])
    else:
        assert math.isnan(got["threshold"]), what


# ---------------------------------------------------------------------------------- 1. counts, threshold, edge list
@pytest.mark.parametrize("name", sorted(CASES))
def test_topk_against_the_truth(pkg, name):
    import torch
    from mc_gra_amd import engine as E
    real, pred, idx, pad = CASES[name]
    r, p, ix = _dev(real), _dev(pred, pad), None if idx is None else _dev(idx)
    if pad:
        assert p.stride(0) == pred.shape[1] + pad
    ks = ks_of(name)
    full = None
    for k in sorted(ks, reverse=True):                    # the largest first: the others are its prefixes
        want = T.top_k(real, pred, k, idx)
        _check_metrics(E.topk_metrics(r, p, k, ix), want, (name, k))
        if k == 0:
            _check_metrics(E.topk_metrics(r, p, None, ix), want, (name, None))
            assert want["k"] == want["positives"] and _same_float(want["precision"], want["recall"])
            continue
        pairs, scores, hits = E.top_pairs(p, k, ix, r)
        assert pairs.dtype == torch.int64 and tuple(pairs.shape) == (k, 2) and scores.dtype == torch.float32
        assert hits.dtype == torch.bool and pairs.is_cuda and scores.is_cuda and hits.is_cuda
        pairs, scores, hits = pairs.cpu().numpy(), scores.cpu().numpy(), hits.cpu().numpy()
        assert np.array_equal(pairs, want["edges"]), (name, k)
        assert np.array_equal(T.bits(scores), T.bits(want["scores"])), (name, k)
        assert np.array_equal(hits, want["edge_hits"]) and int(hits.sum()) == want["hits"], (name, k)
        if full is None:
            full = (pairs, scores, hits)
        else:                                             # the prefix property: top-k' is the first k' rows of top-k
            assert np.array_equal(pairs, full[0][:k]) and np.array_equal(T.bits(scores), T.bits(full[1][:k]))
            assert np.array_equal(hits, full[2][:k])
        bare = E.top_pairs(p, k, ix)                      # without labels: the same pairs and scores, no hits
        assert len(bare) == 2 and np.array_equal(bare[0].cpu().numpy(), pairs)
        assert np.array_equal(T.bits(bare[1].cpu().numpy()), T.bits(scores))


# ------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("name", ["n1500_levels", "n2048_subset_levels_asym"])
def test_topk_two_calls_give_identical_bits(pkg, name):
    import torch
    from mc_gra_amd import engine as E
    real, pred, idx, pad = CASES[name]
    r, p, ix = _dev(real), _dev(pred, pad), None if idx is None else _dev(idx)
    k = tie_k(name)
    a, b = E.top_pairs(p, k, ix, r), E.top_pairs(p, k, ix, r)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    ma, mb = E.topk_metrics(r, p, k, ix), E.topk_metrics(r, p, k, ix)
    assert {q: (v.hex() if isinstance(v, float) else v) for q, v in ma.items()} == \
           {q: (v.hex() if isinstance(v, float) else v) for q, v in mb.items()}


def test_topk_permuted_selection_gives_the_same_graph_without_a_threshold_tie(pkg):
    """A symmetric matrix of distinct scores: a repeat-free idx and a permutation of it name the same unordered node pairs."""
    from mc_gra_amd import engine as E
    real, pred, _, _ = CASES["n1500_continuous_sym"]
    assert np.array_equal(pred, pred.T) and np.array_equal(real, real.T)
    rng = np.random.RandomState(5)
    sub = rng.choice(1500, 400, replace=False)
    k = 3000
    s = np.sort(T.packed(real, pred, sub)[0])[::-1]
    assert s[k - 1] != s[k]                                # no tie at the threshold: the k best are one set of pairs
    r, p = _dev(real), _dev(pred)
    sets, counts = [], []
    for ix in (sub, sub[rng.permutation(400)], np.sort(sub)):
        pairs = E.top_pairs(p, k, ix)[0].cpu().numpy()
        sets.append({frozenset(e) for e in pairs.tolist()})
        m = E.topk_metrics(r, p, k, ix)
        counts.append((m["k"], m["positives"], m["hits"], m["pairs"], m["threshold"]))
        assert len(sets[-1]) == k
    assert sets[0] == sets[1] == sets[2] and counts[0] == counts[1] == counts[2], counts
    assert counts[0][2] > 0


# ---------------------------------------------------------------------------------------------------- 3. refusals
def test_topk_refusals(pkg):
    from mc_gra_amd import engine as E
    real, pred, _, _ = CASES["n80_continuous_asym"]
    r, p = _dev(real), _dev(pred)
    sub = np.arange(60)
    want_all, want_sub = T.top_k(real, pred, 100, None), T.top_k(real, pred, 100, sub)

    def both(rr, pp, k, ix):
        return E.topk_metrics(rr, pp, k, ix), E.top_pairs(pp, k, ix, rr)

    for v in (np.nan, np.inf, -np.inf):
        bad = pred.copy(); bad[7, 3] = v                                 # selected: row 7, column 3 of the lower triangle
        for f in (lambda: E.topk_metrics(r, _dev(bad), 100), lambda: E.top_pairs(_dev(bad), 100),
                  lambda: E.topk_metrics(r, _dev(bad), 100, sub)):
            with pytest.raises(pkg._lib.McgraError):
                f()
        for i, j, ix, want in ((3, 7, None, want_all), (5, 5, None, want_all), (70, 3, sub, want_sub), (3, 70, sub, want_sub)):
            ok = pred.copy(); ok[i, j] = v                               # upper triangle, diagonal, outside idx: not looked at
            m, (pairs, _, _) = both(r, _dev(ok), 100, ix)
            assert m["hits"] == want["hits"] and np.array_equal(pairs.cpu().numpy(), want["edges"]), (v, i, j)
    bad = real.copy(); bad[9, 2] = 2.0
    with pytest.raises(pkg._lib.McgraError):
        E.topk_metrics(_dev(bad), p, 100)
    with pytest.raises(pkg._lib.McgraError):
        E.top_pairs(p, 100, None, _dev(bad))
    ok = real.copy(); ok[2, 9] = 2.0                                      # its mirror is not selected
    assert E.topk_metrics(_dev(ok), p, 100)["hits"] == want_all["hits"]
    for ix in ([0, 80], [-1, 2], [4, 9, 4], [7, 7]):                      # out of range; repeated
        with pytest.raises(pkg._lib.McgraError):
            E.topk_metrics(r, p, 1, ix)
        with pytest.raises(pkg._lib.McgraError):
            E.top_pairs(p, 1, ix)
    m = 80 * 79 // 2
    assert E.topk_metrics(r, p, m)["k"] == m
    for k, ix in ((m + 1, None), (60 * 59 // 2 + 1, sub), (-1, None)):
        with pytest.raises(pkg._lib.McgraError):
            E.topk_metrics(r, p, k, ix)
        with pytest.raises(pkg._lib.McgraError):
            E.top_pairs(p, k, ix)
    with pytest.raises(pkg._lib.McgraError):
        E.top_pairs(p, 0)
    with pytest.raises(pkg._lib.McgraError):
        E.topk_metrics(r, p, 1, [5])                                     # fewer than two nodes
    none = E.topk_metrics(_dev(np.zeros((80, 80), np.float32)), p)      # k = P = 0
    assert (none["k"], none["positives"], none["hits"], none["pairs"]) == (0, 0, 0, m)
    assert all(math.isnan(none[q]) for q in ("precision", "recall", "f1", "threshold"))


# ------------------------------------------------------------------------------------------------------ 4. main.py
def test_main_evaluate_topk_and_save_edges(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed brazil files (n = 131), 3 epochs: --topk 0 gives precision = recall = F1 for
    each index set, topk_all is the truth on the modified_adj that was scored, --save_edges round-trips, and a run without
    the flags returns and logs what it did before the flags existed."""
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "brazil", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain = M.run(M.build_parser().parse_args(argv + ["--log_name", "plain.txt"]))
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.topk_metrics

    def record(real, pred, k=None, idx=None):
        v = orig(real, pred, k, idx)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), k, None if idx is None else np.asarray(idx), v))
        return v

    monkeypatch.setattr(M.engine, "topk_metrics", record)
    edges = str(tmp_path / "edges.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "topk.txt", "--topk", "0", "--save_edges", edges]))
    out = capsys.readouterr().out
    assert sorted(res) == sorted(list(plain) + ["topk_attack", "topk_train", "topk_all"]) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flag, bit for bit
    for (real, pred, k, idx, v), name in zip(seen, ("attack", "train", "all")):
        d = res[f"topk_{name}"]
        assert d is v and k == 0 and d["k"] == d["positives"] > 0
        assert d["precision"] == d["recall"] == d["f1"] == d["hits"] / d["k"], (name, d)
        _check_metrics(d, T.top_k(real, pred, 0, idx), name)
    real, pred, _, idx, d = seen[2]
    assert idx is None and d["pairs"] == 131 * 130 // 2
    want = T.top_k(real, pred, 0, None)
    z = np.load(edges)
    assert sorted(z.files) == ["hits", "pairs", "scores"]
    assert np.array_equal(z["pairs"], want["edges"]) and z["pairs"].dtype == np.int64
    assert np.array_equal(T.bits(z["scores"]), T.bits(want["scores"])) and z["scores"].dtype == np.float32
    assert np.array_equal(z["hits"], want["edge_hits"]) and z["hits"].dtype == np.bool_ and int(z["hits"].sum()) == d["hits"]
    assert f"current auc={res['auc_all']}\ncurrent f1={d['f1']} (k={d['k']})\n" in out and "current f1=" not in out_plain
    log = open(tmp_path / "results" / "topk.txt").read().split("\n")
    a, t = res["topk_attack"], res["topk_train"]
    assert log[2] == (f"In attack graph: k={a['k']} P={a['precision']} R={a['recall']} F1={a['f1']}\t"
                      f"In train graph: k={t['k']} P={t['precision']} R={t['recall']} F1={t['f1']}\t"
                      f"In Whole Graph: k={d['k']} P={d['precision']} R={d['recall']} F1={d['f1']}")
    assert log[3].startswith("current density:") and "topk=0" in log[0] and "save_edges=" in log[0] and "ap=" not in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "topk" not in old and "save_edges" not in old and "ap=" not in old and " k=" not in old and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[3:]


def test_main_topk_report_clamps_k_to_the_pair_count(pkg):
    """--topk K above a set's pair count: k = m in the returned dict (reports.topk_report), everything taken."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    real, pred, _, _ = CASES["n80_continuous_asym"]
    sub = np.arange(5, 25)
    rep = R.topk_report(_dev(real), _dev(pred), {"all": None, "sub": sub}, 10 ** 9)
    for key, idx in (("topk_all", None), ("topk_sub", sub)):
        d = rep[key]
        _check_metrics(d, T.top_k(real, pred, T.top_k(real, pred, 1, idx)["pairs"], idx), key)
        assert d["k"] == d["pairs"] and d["hits"] == d["positives"] and d["recall"] == 1.0
