"""The LinkTeller influence attack on the device (mcgra_influence_scores, engine.influence_scores, main.py --mode link_teller and
--versus linkteller:OUTPUT) against tests/influence_truth.py: every entry within its derived float32 bound of the float64 truth,
exactly +0.0 outside the reach, the three counts, the same bits on a second call and on another grid, `max` bit for bit the larger of
`directed` and its transpose, padded rows, the refusals that need the device, and the command line on the committed brazil files.
Run with -m gpu.

tests/test_influence_cases_cpu.py checks, without a GPU, that the truth is right, that the bound leaves room for a float32
evaluation and none for a wrong reading of the definition, and that the inputs (tests/influence_cases.py) have the properties they
are there for."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import influence_cases as IC
from tests import influence_truth as T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def truth(name, output):
    """(the directed truth, its bound) of one case, computed once (read-only)."""
    c = IC.case(name)
    I, B = T.truth(c, output), T.bound(c, output)
    for a in (I, B["bound"], B["excluded"], B["reach"]):
        a.setflags(write=False)
    return I, B


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda:0")


def _run(name, output="posteriors", symmetrize="directed", adj=None):
    from mc_gra_amd import engine as E
    c = IC.case(name)
    tensors = ([_dev(w) for w in c["W"]], [_dev(b) for b in c["b"]], _dev(c["Wlin"]), _dev(c["blin"]))
    out, info = E.influence_scores(tensors, _dev(c["X"]), _dev(c["A"]) if adj is None else adj, c["delta"], output, symmetrize)
    return out.cpu().numpy(), info


def _held(name, got, I, B, every_entry=False):
    """Every entry outside the reach is +0.0; every entry inside, but the excluded ones, is within its bound."""
    R = B["reach"]
    assert got.dtype == np.float32 and got.shape == I.shape
    assert not got[~R].any() and not np.signbit(got[~R]).any(), name
    check = R if every_entry else R & ~B["excluded"]
    err = np.abs(got.astype(np.float64) - I)
    worst = float((err[check] / B["bound"][check]).max()) if check.any() else 0.0
    print(f"{name}: reached {int(R.sum())}, excluded {int(B['excluded'].sum())}, k {B['k']:.0f}, worst error {worst:.3g} bounds, "
          f"{float((err[check] / (T.U * np.maximum(B['M'][check], 1e-300))).max()) if check.any() else 0.0:.3g} u M")
    assert (err[check] <= B["bound"][check]).all(), (name, worst)


@pytest.mark.parametrize("name", [n for n in IC.CASES if n not in IC.EXACT])
def test_every_entry_within_its_bound_and_zero_outside_the_reach(pkg, name):
    for output in T.OUTPUTS if name in IC.ACCURACY + ("star65_raw", "narrow64") else ("posteriors",):
        I, B = truth(name, output)
        got, info = _run(name, output)
        _held(f"{name} {output}", got, I, B)
        want = T.counts(IC.case(name))
        assert (info["nnz"], info["reached"], info["max_reach"]) == (want["nnz"], want["reached"], want["max_reach"])
        assert info["delta"] == float(np.float32(IC.case(name)["delta"])) and info["output"] == output
        if name == "zero_row130":
            assert not got[5].any()                               # a node without features moves nothing
        if name in ("star515", "complete130"):
            assert info["max_reach"] == got.shape[0]              # the dense regime: every frontier is every node


def test_the_crossing_branch(pkg):
    """Units that the perturbation switches on and off: the base pre-activations are exact in float32, so no entry is excluded."""
    for name in IC.EXACT:
        for output in T.OUTPUTS:
            I, B = truth(name, output)
            assert B["crossing"] > 0
            got, _ = _run(name, output)
            _held(f"{name} {output}", got, I, B, every_entry=True)
            wrong = T.difference(IC.case(name), output, variant="base_mask")
            assert (np.abs(wrong - I) > 10 * B["bound"]).any()   # the base relu mask alone is told apart here


@pytest.mark.parametrize("name", ["planted130", "star65_raw", "planted515", "one_node", "empty65_raw"])
def test_max_is_the_larger_of_directed_and_its_transpose_bit_for_bit(pkg, name):
    d, _ = _run(name, "posteriors", "directed")
    m, info = _run(name, "posteriors", "max")
    assert np.array_equal(m.view(np.uint32), np.maximum(d, d.T).view(np.uint32)) and np.array_equal(m.view(np.uint32), m.T.view(np.uint32))
    assert info["symmetrize"] == "max"
    if name == "planted130":                                      # the AUC the attack reports is the truth's, within the close pairs
        I, B = truth(name, "posteriors")
        labels = IC.case(name)["labels"]
        share = T.close_pair_share(T.symmetrize(I), np.maximum(B["bound"], B["bound"].T), labels)
        assert not B["excluded"].any() and share <= 1e-3
        assert abs(T.auc(m.astype(np.float64), labels) - T.auc(T.symmetrize(I), labels)) <= share


def test_the_same_bits_twice_and_on_every_grid(pkg, monkeypatch):
    for name in ("planted130", "planted515", "star65_raw"):
        a, ia = _run(name, "log_posteriors", "max")
        b, ib = _run(name, "log_posteriors", "max")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ia == ib
        for groups in ("1", "3", "130"):
            monkeypatch.setenv("MCGRA_INFLUENCE_GROUPS", groups)
            c, ic = _run(name, "log_posteriors", "max")
            monkeypatch.delenv("MCGRA_INFLUENCE_GROUPS")
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and ia == ic, (name, groups)


def _call(pkg, c, adj, lda, out, ldo, output=1, symmetrize=0, delta=None, n=None):
    """The C entry itself, on device tensors."""
    import torch
    L = pkg._lib.lib
    Ws, bs = [_dev(w) for w in c["W"]], [_dev(b) for b in c["b"]]
    X, Wlin, blin = _dev(c["X"]), _dev(c["Wlin"]), _dev(c["blin"])
    nl = len(Ws)
    dims = (ctypes.c_int32 * (nl + 1))(*([X.shape[1]] + [w.shape[1] for w in Ws]))
    Wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in Ws])
    bp = (ctypes.c_void_p * nl)(*[b.data_ptr() for b in bs])
    counts = (ctypes.c_int64 * 3)(-77, -77, -77)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.mcgra_influence_scores(None, X.shape[0] if n is None else n, X.shape[1], nl, dims, p(X), p(adj), lda, Wp, bp, p(Wlin), p(blin),
                                  Wlin.shape[0], c["delta"] if delta is None else delta, output, symmetrize, p(out), ldo, counts)
    torch.cuda.synchronize()
    return rc, list(counts)


@pytest.mark.parametrize("symmetrize", [0, 1])
def test_padded_rows_stay_untouched(pkg, symmetrize):
    import torch
    name = "planted130"
    c = IC.case(name)
    n, lda, ldo = 130, 137, 160
    adj = torch.full((n, lda), float("nan"), device="cuda:0")     # the spare columns are never read: a NaN there would be refused
    adj[:, :n] = _dev(c["A"])
    out = torch.full((n, ldo), -5.0, device="cuda:0")
    rc, counts = _call(pkg, c, adj, lda, out, ldo, 1, symmetrize)
    assert rc == 0, pkg._lib.lib.mcgra_last_error()
    got = out.cpu().numpy()
    assert (got[:, n:] == -5.0).all()
    want, _ = _run(name, "posteriors", ("directed", "max")[symmetrize])
    assert np.array_equal(got[:, :n].view(np.uint32), want.view(np.uint32))
    w = T.counts(c)
    assert counts == [w["nnz"], w["reached"], w["max_reach"]]


def test_device_side_refusals_write_no_counts(pkg):
    import torch
    L = pkg._lib.lib
    c = IC.case("cycle63")
    n = 63
    out = torch.full((n, n), -5.0, device="cuda:0")

    def refused(word, **changes):
        case = dict(c, **changes)
        rc, counts = _call(pkg, case, _dev(case["A"]), n, out, n)
        assert rc == -1 and counts == [-77] * 3 and word in L.mcgra_last_error().decode(), (changes.keys(), L.mcgra_last_error())
        assert (out == -5.0).all()

    A = c["A"].copy()
    A[3, 40] = 0.5                                                # a cell without its mirror
    refused("not symmetric", A=A)
    for bad in (np.nan, np.inf, -np.inf):
        A = c["A"].copy()
        A[7, 7] = bad
        refused("NaN or an infinity", A=A)
        X = c["X"].copy()
        X[62, 23] = bad
        refused("NaN or an infinity", X=X)
        W = [w.copy() for w in c["W"]]
        W[1][15, 15] = bad
        refused("NaN or an infinity", W=W)
        b = [x.copy() for x in c["b"]]
        b[0][0] = bad
        refused("NaN or an infinity", b=b)
        blin = c["blin"].copy()
        blin[6] = bad
        refused("NaN or an infinity", blin=blin)
    refused("NaN or an infinity", X=(c["X"] * np.float32(3e38)), W=[c["W"][0] * np.float32(1e3), c["W"][1]])   # a base output that overflows
    rc, counts = _call(pkg, c, _dev(c["A"]), n, out, n)           # and the call itself is fine
    assert rc == 0 and counts[0] == 3 * n
    from mc_gra_amd import engine as E
    with pytest.raises(pkg._lib.McgraError, match="not symmetric"):
        A = c["A"].copy()
        A[3, 40] = 0.5
        E.influence_scores(([_dev(w) for w in c["W"]], [_dev(b) for b in c["b"]], _dev(c["Wlin"]), _dev(c["blin"])), _dev(c["X"]), _dev(A))


# ------------------------------------------------------------------------------------------------------ end to end
def _brazil():
    return ["--dataset", "brazil", "--dataset_root", os.path.join(H.GOLDEN, "dataset")]


def _recomputed(M, E, R, seen, real, graph="normalised", delta=1e-4):
    """What --mode link_teller must return, from the engine's entries on a recomputed matrix."""
    model, feats, vd = seen["model"], seen["features"], seen["graph"]
    want = {}
    for output in E.INFLUENCE_OUTPUTS:
        query = vd if graph == "raw" else M.utils.normalize_adj_tensor(vd)
        S, info = E.influence_scores(model, feats, query, delta, output, "max")
        want[output] = {}
        for name, ix in seen["sets"].items():
            d = E.auc_delong(real, S, ix)
            beliefs = {}
            for belief in R.LINKTELLER_BELIEFS:
                k = min(int(math.floor(belief * d["positives"] + 0.5)), d["pairs"])
                t = E.topk_metrics(real, S, k, ix)
                beliefs[belief] = {key: t[key] for key in ("k", "hits", "precision", "recall", "f1")}
            want[output][name] = {"auc": d["auc"], "pairs": d["pairs"], "positives": d["positives"], "beliefs": beliefs}
    return want, info


def _spy(monkeypatch, M):
    import mc_gra_amd.topology_attack as TA
    seen = {}

    def no_engine(*a, **k):
        raise AssertionError("--mode link_teller built an attack engine")

    monkeypatch.setattr(M.engine, "AttackEngine", no_engine)
    monkeypatch.setattr(TA, "AttackEngine", no_engine)
    monkeypatch.setattr(M, "PGDAttack", no_engine)
    scores = M.link_teller_scores

    def link_teller_scores(model, features, graph, *a):
        seen.update(model=model, features=features, graph=graph)
        return scores(model, features, graph, *a)

    metrics = M.reports.link_teller_metrics

    def link_teller_metrics(real, S, sets):
        seen["sets"] = sets
        return metrics(real, S, sets)

    monkeypatch.setattr(M, "link_teller_scores", link_teller_scores)
    monkeypatch.setattr(M.reports, "link_teller_metrics", link_teller_metrics)
    return seen


def test_main_link_teller_on_brazil(pkg, tmp_path, monkeypatch, capsys):
    """--mode link_teller on the committed brazil files (n = 131): no attack engine, nothing on disk but --save_linkteller's file;
    every value is what the engine's entries give on a recomputed matrix; raw differs; the lines are the result's."""
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    seen = _spy(monkeypatch, M)
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / "lt.npz")
    res = M.run(M.build_parser().parse_args(_brazil() + ["--mode", "link_teller", "--save_linkteller", path]))
    out = capsys.readouterr().out
    real = _dev(H.load_readme_graph("brazil")["adj"])
    want, info = _recomputed(M, E, R, seen, real)
    assert list(res) == ["link_teller", "link_teller_info"] and res["link_teller"] == want
    assert list(res["link_teller"]) == list(E.INFLUENCE_OUTPUTS) and list(want["posteriors"]) == ["attack", "train", "all"]
    assert res["link_teller_info"] == {"delta": float(np.float32(1e-4)), "graph": "normalised", "nnz": info["nnz"],
                                       "reached": info["reached"], "max_reach": info["max_reach"]}
    assert want["posteriors"]["all"]["auc"] > 0.9 and want["posteriors"]["all"]["pairs"] == 131 * 130 // 2
    lines = [l for l in out.splitlines() if l.startswith("link teller ")]
    assert lines == R.link_teller_lines(res["link_teller"]) and len(lines) == 2 * (1 + 3)
    assert lines[0] == "link teller log_posteriors: " + " ".join(f"auc_{k}={v['auc']}" for k, v in want["log_posteriors"].items())
    z = np.load(path)
    P = want["posteriors"]["all"]["positives"]
    pairs, scores, hits = (t.cpu().numpy() for t in E.top_pairs(E.influence_scores(
        seen["model"], seen["features"], M.utils.normalize_adj_tensor(seen["graph"]))[0], P, None, real))
    assert np.array_equal(z["pairs_posteriors"], pairs) and np.array_equal(z["scores_posteriors"], scores) and np.array_equal(z["hits_posteriors"], hits)
    assert int(z["nnz"]) == info["nnz"] and str(z["graph"]) == "normalised" and float(z["auc_posteriors"]) == want["posteriors"]["all"]["auc"]
    assert os.listdir(tmp_path) == ["lt.npz"]
    raw = M.run(M.build_parser().parse_args(_brazil() + ["--mode", "link_teller", "--lt_graph", "raw", "--lt_delta", "0.001"]))
    capsys.readouterr()
    want_raw, info_raw = _recomputed(M, E, R, seen, real, "raw", 1e-3)
    assert raw["link_teller"] == want_raw and raw["link_teller_info"]["graph"] == "raw" and raw["link_teller_info"]["delta"] == float(np.float32(1e-3))
    assert raw["link_teller_info"]["nnz"] < info["nnz"] and raw["link_teller"] != res["link_teller"]


def test_main_link_teller_against_edgerand_on_brazil(pkg, tmp_path, monkeypatch, capsys):
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    seen = _spy(monkeypatch, M)
    monkeypatch.chdir(tmp_path)
    res = M.run(M.build_parser().parse_args(_brazil() + ["--mode", "link_teller", "--dp_defense", "edgerand", "--dp_eps", "8"]))
    out = capsys.readouterr().out
    A = np.asarray(H.load_readme_graph("brazil")["adj"], np.float32)
    real = _dev(A)
    perturbed, _ = E.dp_perturb_graph(real, "edgerand", 8.0, 15)
    assert bool((seen["graph"] == perturbed).all()) and not bool((perturbed == real).all())      # the victim answers from the perturbed graph
    want, info = _recomputed(M, E, R, seen, real)                                                # and is scored against the true one
    assert list(res) == ["link_teller", "link_teller_info", "defense"] and res["link_teller"] == want
    assert res["defense"]["mechanism"] == "edgerand" and res["defense"]["eps"] == 8.0 and out.count("defense edgerand eps=8.0") == 1
    assert want["posteriors"]["all"]["positives"] == int(np.tril(A, -1).sum())
    assert not os.path.exists(tmp_path / "results")


def test_main_evaluate_versus_linkteller(pkg, tmp_path, monkeypatch, capsys):
    """--mode evaluate --ci --versus linkteller:posteriors at 3 epochs: versus_all's "b" is auc_delong on the influence matrix."""
    from mc_gra_amd import engine as E
    from mc_gra_amd import main as M
    seen = {}
    scores = M.link_teller_scores

    def link_teller_scores(model, features, graph, *a):
        seen.update(model=model, features=features, graph=graph, rest=a)
        return scores(model, features, graph, *a)

    monkeypatch.setattr(M, "link_teller_scores", link_teller_scores)
    monkeypatch.chdir(tmp_path)
    argv = _brazil() + ["--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100", "--w7", "10000", "--w9", "100",
                        "--weight_sup", "0", "--lr", "-3", "--useH_A", "--ci", "--versus", "linkteller:posteriors"]
    res = M.run(M.build_parser().parse_args(argv))
    out = capsys.readouterr().out
    assert seen["rest"] == ("normalised", 1e-4, ("posteriors",))
    S, _ = E.influence_scores(seen["model"], seen["features"], M.utils.normalize_adj_tensor(seen["graph"]), 1e-4, "posteriors", "max")
    real = _dev(H.load_readme_graph("brazil")["adj"])
    want = E.auc_delong(real, S)
    b = res["versus_all"]["b"]
    assert b["ints"] == want["ints"] and b["auc"] == want["auc"] and b["var"] == want["var"]
    assert abs(res["versus_all"]["delta"] - (res["ci_all"]["auc"] - b["auc"])) < 1e-15 and math.isfinite(res["versus_all"]["p_value"])
    assert f"current delta={res['versus_all']['delta']}" in out
    log = open(tmp_path / "results" / "result.txt").read()
    assert "versus='linkteller:posteriors'" in log and f"versus linkteller:posteriors: AUC={b['auc']}" in log
