"""Without a GPU: that the truth of tests/test_gpu_influence.py (tests/influence_truth.py) is right -- the literal definition against
the difference form restated in float64, against torch.autograd's Jacobian through the repository's own victim class as Delta -> 0,
against networkx for the zero pattern; that the derived bound leaves room for a float32 evaluation of the computed form and none for
a wrong reading of the definition; that the inputs (tests/influence_cases.py) have the properties they are there for; the refusals of
the C entry and of engine.influence_scores that need no device; the command line and the printed lines."""
import argparse
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import influence_cases as IC
from tests import influence_truth as T


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


@functools.lru_cache(maxsize=None)
def truth(name, output="posteriors"):
    c = IC.case(name)
    return T.truth(c, output), T.bound(c, output)


# -------------------------------------------------------------------------------------------------- 1. the truth
@pytest.mark.parametrize("name", list(IC.CASES))
def test_the_literal_definition_is_the_difference_form(name):
    """Two float64 forwards subtracted against the differences carried in float64: the same numbers up to the cancellation of the
    first (2^-53 |O| / Delta), and exactly 0 -- in both -- outside the structural reach."""
    c = IC.case(name)
    for output in T.OUTPUTS:
        I, B = truth(name, output)
        D = T.difference(c, output)
        assert not I[~B["reach"]].any() and not D[~B["reach"]].any()
        noise = 64.0 * 2.0 ** -53 * 1e3 / abs(float(np.float32(c["delta"])))
        assert np.abs(I - D).max() <= 1e-9 * max(np.abs(I).max(), 1e-300) + noise, (name, output, np.abs(I - D).max(), np.abs(I).max())
    assert (B["reach"] == T.reach(c["A"], len(c["W"])).T).all()


def _torch_victim(c):
    """The case's victim as the repository's own class, in float64 on the host."""
    import torch
    from mc_gra_amd.models.gcn import GCN
    nfeat, nhid, nclass = c["X"].shape[1], c["W"][0].shape[1], c["Wlin"].shape[0]
    m = GCN(nfeat=nfeat, nhid=nhid, nclass=nclass, nlayer=len(c["W"]), device="cpu").double().eval()
    with torch.no_grad():
        for layer, w, b in zip(m.gc, c["W"], c["b"]):
            layer.double()
            layer.weight.copy_(torch.tensor(w, dtype=torch.float64))
            layer.bias.copy_(torch.tensor(b, dtype=torch.float64))
        m.linear1.weight.copy_(torch.tensor(c["Wlin"], dtype=torch.float64))
        m.linear1.bias.copy_(torch.tensor(c["blin"], dtype=torch.float64))
    return m


def _small(seed=3, n=20, delta=2.0 ** -20):
    rng = np.random.RandomState(seed)
    raw = IC.graph("planted", n, rng)
    W = [rng.uniform(-0.5, 0.5, (6, 5)).astype(np.float32), rng.uniform(-0.5, 0.5, (5, 5)).astype(np.float32)]
    b = [rng.uniform(-0.5, 0.5, 5).astype(np.float32) for _ in range(2)]
    return {"A": IC.normalise(raw), "A_raw": raw, "X": rng.rand(n, 6).astype(np.float32), "W": W, "b": b,
            "Wlin": rng.uniform(-0.5, 0.5, (3, 5)).astype(np.float32), "blin": rng.uniform(-0.5, 0.5, 3).astype(np.float32),
            "delta": delta, "labels": raw}


def test_the_truth_is_the_victim_class_and_its_jacobian_as_delta_vanishes(pkg):
    """forward() is models.gcn.GCN.forward; as Delta -> 0 the influence is || (dO_u / dx_v) x_v ||, torch.autograd's Jacobian."""
    import torch
    c = _small()
    m = _torch_victim(c)
    X, A = torch.tensor(c["X"], dtype=torch.float64), torch.tensor(c["A"], dtype=torch.float64)
    mm = T.Model(c)
    O, _ = T.forward(mm, mm.X @ mm.W[0])
    assert np.abs(m(X, A).detach().numpy() - O).max() < 1e-13
    for output, f in (("log_posteriors", lambda x: m(x, A)), ("posteriors", lambda x: torch.exp(m(x, A)))):
        I = T.truth(c, output)
        J = np.zeros_like(I)
        for v in range(len(X)):
            tangent = torch.zeros_like(X)
            tangent[v] = X[v]
            J[v] = torch.autograd.functional.jvp(f, X, tangent)[1].norm(dim=1).numpy()
        assert np.abs(I - J).max() <= 1e-4 * J.max() and J.max() > 0           # the second-order term is about Delta = 1e-6
        coarse = T.truth(dict(c, delta=2.0 ** -2), output)
        assert np.abs(coarse - J).max() > 1e-4 * J.max()                       # and the finite difference is not the Jacobian


@pytest.mark.parametrize("kind", ["path", "star", "cycle", "two_components"])
def test_the_zero_pattern_is_the_graphs(kind):
    """Normalised (self-loops): non-zero exactly at distance <= L.  Raw: exactly where a walk of L steps ends."""
    import networkx as nx
    n = 24
    raw = IC.graph(kind, n, None)
    G = nx.from_numpy_array(raw)
    dist = dict(nx.all_pairs_shortest_path_length(G))
    for L in (1, 2, 3):
        near = np.array([[dist[v].get(u, 10 ** 9) <= L for u in range(n)] for v in range(n)])
        walks = np.linalg.matrix_power(raw.astype(np.int64), L) > 0
        assert (T.reach(IC.normalise(raw), L) == near).all() and (T.reach(raw, L) == walks).all()
    c = _small(n=n)
    c.update(A=IC.normalise(raw), A_raw=raw, delta=1e-4, b=[np.full(5, 2.0, np.float32)] * 2)      # every unit is on: nothing dies on the way
    I = T.truth(c)
    near = np.array([[dist[v].get(u, 10 ** 9) <= 2 for u in range(n)] for v in range(n)])
    assert ((I != 0) == near).all()
    c["A"] = raw
    I = T.truth(c)
    assert ((I != 0) <= (np.linalg.matrix_power(raw.astype(np.int64), 2) > 0)).all() and (I != 0).sum() > 0
    if kind == "path":                                            # neighbours without a common neighbour score 0 on the raw graph
        assert I[3, 4] == 0 and I[3, 5] != 0 and I[3, 3] != 0


def test_one_layer_sees_the_edges_and_the_diagonal():
    c = IC.case("planted130_l1")
    I, B = truth("planted130_l1")
    assert ((I != 0) == ((c["labels"] != 0) | np.eye(130, dtype=bool))).all()
    assert T.auc(T.symmetrize(I), c["labels"]) == 1.0


# -------------------------------------------------------------------------------------------------- 2. the bound
@pytest.mark.parametrize("name", list(IC.CASES))
def test_a_float32_evaluation_of_the_computed_form_is_within_the_bound(name):
    """numpy's float32 restatement of the kernels' form stays far inside gamma(k) M: the derived bound has room."""
    c = IC.case(name)
    for output in T.OUTPUTS:
        I, B = truth(name, output)
        F = T.difference(c, output, np.float32).astype(np.float64)
        check = B["reach"] & (~B["excluded"] if name not in IC.EXACT else True)
        assert not F[~B["reach"]].any()
        assert (np.abs(F - I)[check] <= B["bound"][check]).all(), name
        assert (np.abs(F - I)[check] <= 8 * T.U * B["M"][check] + B["bound"][check] * 1e-3).all(), name   # the evidence: a few u M


def test_the_accuracy_cases_exclude_almost_nothing_and_resolve_the_auc():
    """From the truth alone: at most 1e-3 of the reached entries sit at a relu's corner, and at most 1e-3 of the (edge, non-edge)
    pairs of pairs lie closer than the sum of their bounds."""
    for name in IC.ACCURACY:
        c = IC.case(name)
        for output in T.OUTPUTS:
            I, B = truth(name, output)
            assert B["excluded"].sum() <= 1e-3 * B["reach"].sum(), (name, int(B["excluded"].sum()), int(B["reach"].sum()))
            bound = np.where(B["excluded"], np.inf, B["bound"])
            share = T.close_pair_share(T.symmetrize(I), np.maximum(bound, bound.T), c["labels"])
            assert share <= 1e-3, (name, output, share)
    for name in IC.CASES:                                         # the other cases may exclude more, never most
        if name not in IC.EXACT:
            B = truth(name)[1]
            assert B["excluded"].sum() <= 0.05 * max(B["reach"].sum(), 1), name


def test_the_planted_graph_is_attacked_well_and_the_raw_query_is_not():
    """without self-loops a 2-layer victim's influence follows walks of exactly two steps."""
    norm = T.auc(T.symmetrize(truth("planted130")[0]), IC.case("planted130")["labels"])
    raw = T.auc(T.symmetrize(truth("planted130_raw")[0]), IC.case("planted130_raw")["labels"])
    assert norm > 0.95 and raw < 0.75 and raw < norm - 0.2


def test_the_crossing_case_crosses():
    c = IC.case("crossing")
    m = T.Model(c)
    _, Ps, dPs, _, _ = T.difference(c, parts=True)
    P, dP = Ps[0][4], dPs[0][4, 4]                                # layer 0, node 4, source 4
    assert P[0] == -dP[0] / 2 < 0 < P[0] + dP[0] and P[1] == -dP[1] / 2 > 0 > P[1] + dP[1]       # one unit on, one off
    P32 = (c["A"] @ (c["X"] @ c["W"][0]) + c["b"][0]).astype(np.float32)
    assert (P32.astype(np.float64) == Ps[0]).all()                # the base pre-activations are exact in float32
    assert truth("crossing")[1]["crossing"] >= 2 and m.delta == 2.0 ** -7


def test_the_cases_tell_the_wrong_readings_from_the_truth():
    told = {}
    for variant in T.VARIANTS:
        told[variant] = []
        for name in ("planted130", "coarse130", "crossing", "softmax9", "star65_raw", "planted130_l1"):
            c = IC.case(name)
            if variant == "raw_for_normalised" and CASE_MODE(name) != "normalised":
                continue
            I, B = truth(name)
            W = T.difference(c, variant=variant)
            check = B["reach"] | (W != 0)
            if (np.abs(W - I)[check] > 10 * B["bound"][check]).any():
                told[variant].append(name)
    assert set(told) == set(T.VARIANTS)
    for variant, names in told.items():
        assert names, f"no case tells the wrong reading {variant!r} from the truth"
    assert "crossing" in told["base_mask"] and "softmax9" in told["linear_softmax"] and "coarse130" in told["jacobian"]


def CASE_MODE(name):
    return IC.CASES[name][2]


def test_belief_k_rounds_half_up_and_clamps(pkg):
    from mc_gra_amd import reports as R
    assert R.LINKTELLER_BELIEFS == (0.25, 0.5, 1.0, 2.0, 4.0)
    assert [R.belief_k(b, 10, 45) for b in R.LINKTELLER_BELIEFS] == [3, 5, 10, 20, 40]          # 2.5 -> 3
    assert [R.belief_k(b, 13, 45) for b in R.LINKTELLER_BELIEFS] == [3, 7, 13, 26, 45]          # 3.25 -> 3, 6.5 -> 7, 52 -> 45
    assert R.belief_k(0.25, 1, 45) == 0 and R.belief_k(0.5, 1, 45) == 1 and R.belief_k(4.0, 0, 45) == 0


# -------------------------------------------------------------------------------------------- 3. refusals without a device
def test_c_entry_refuses_before_any_hip_call(pkg):
    L = pkg._lib.lib
    assert "mcgra_influence_scores" in pkg._lib.SYMBOLS
    p = ctypes.c_void_p(4096)                                     # never followed: every call below is refused first
    ptrs = (ctypes.c_void_p * 8)(*([4096] * 8))
    none = (ctypes.c_void_p * 8)(*([4096, None] + [4096] * 6))

    def call(n=5, nfeat=3, nlayer=2, dims=(3, 4, 4), X=p, adj=p, lda=5, W=ptrs, b=ptrs, Wlin=p, blin=p, nclass=2, delta=1e-4, output=1,
             symmetrize=1, out=p, ldo=5, counts=True):
        c = (ctypes.c_int64 * 3)(-77, -77, -77)
        d = None if dims is None else (ctypes.c_int32 * len(dims))(*dims)
        rc = L.mcgra_influence_scores(None, n, nfeat, nlayer, d, X, adj, lda, W, b, Wlin, blin, nclass, delta, output, symmetrize, out, ldo,
                                      c if counts else None)
        assert list(c) == [-77] * 3
        return rc

    einval = (dict(n=0), dict(n=-3), dict(lda=4), dict(ldo=4), dict(nlayer=0), dict(nlayer=9, dims=(3,) + (4,) * 9), dict(dims=None), dict(X=None),
              dict(adj=None), dict(W=None), dict(b=None), dict(W=none), dict(b=none), dict(Wlin=None), dict(blin=None), dict(out=None),
              dict(counts=False), dict(delta=0.0), dict(delta=1e-50), dict(delta=math.nan), dict(delta=math.inf), dict(delta=1e39),
              dict(delta=1.0), dict(delta=-1.0), dict(delta=2.5), dict(output=2), dict(output=-1), dict(symmetrize=2), dict(symmetrize=-1),
              dict(nfeat=0, dims=(0, 4, 4)), dict(nclass=0), dict(dims=(2, 4, 4)), dict(dims=(3, 0, 4)))
    for kw in einval:
        assert call(**kw) == -1 and b"influence_scores:" in L.mcgra_last_error(), kw
    for kw in (dict(n=65536, lda=65536, ldo=65536), dict(dims=(3, 65, 4)), dict(dims=(3, 4, 65)), dict(nclass=65)):
        assert call(**kw) == -3 and b"influence_scores:" in L.mcgra_last_error(), kw
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(call(nclass=65))
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcgra.h")).read()
    assert re.search(r"#define MCGRA_INFLUENCE_MAX_WIDTH 64\b", hdr) and "#define MCGRA_INFLUENCE_POSTERIORS 1" in hdr


def test_engine_refuses_before_any_device_call(pkg, monkeypatch):
    import torch
    from mc_gra_amd import engine as E
    assert E.INFLUENCE_OUTPUTS == T.OUTPUTS == ("log_posteriors", "posteriors") and E.INFLUENCE_SYMMETRIZE == ("directed", "max")

    def never(*a, **k):
        raise AssertionError("the device entry was called")

    monkeypatch.setattr(E.lib, "mcgra_influence_scores", never)
    monkeypatch.setattr(E, "_stream", never)
    W, b, Wlin, blin = [torch.zeros(3, 4), torch.zeros(4, 4)], [torch.zeros(4), torch.zeros(4)], torch.zeros(2, 4), torch.zeros(2)
    X, A = torch.zeros(5, 3), torch.zeros(5, 5)
    good = dict(model_or_tensors=(W, b, Wlin, blin), X=X, adj=A)
    bad = [dict(output="logits"), dict(output=1), dict(symmetrize="min"), dict(symmetrize=None), dict(delta=0.0), dict(delta=1.0), dict(delta=-2.0),
           dict(delta=math.nan), dict(delta=math.inf), dict(delta=1e-50), dict(delta="1e-4"), dict(delta=True), dict(adj=torch.zeros(5, 6)),
           dict(adj=torch.zeros(4, 4)), dict(X=torch.zeros(5)), dict(X=np.zeros((5, 3))), dict(model_or_tensors=(W, b, Wlin)),
           dict(model_or_tensors=(W, b[:1], Wlin, blin)), dict(model_or_tensors=([], [], Wlin, blin)),
           dict(model_or_tensors=([torch.zeros(2, 4), W[1]], b, Wlin, blin)), dict(model_or_tensors=(W, b, torch.zeros(2, 5), blin)),
           dict(model_or_tensors=(W, b, Wlin, torch.zeros(3))), dict(model_or_tensors=([torch.zeros(3, 65), torch.zeros(65, 4)], [torch.zeros(65), b[1]], Wlin, blin)),
           dict(model_or_tensors=(W, b, torch.zeros(65, 4), torch.zeros(65))), dict(model_or_tensors=torch.nn.Linear(3, 2)),
           dict(model_or_tensors=([torch.zeros(3, 4)] * 9, [torch.zeros(4)] * 9, Wlin, blin))]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match="influence_scores"):
            E.influence_scores(**args)
    from mc_gra_amd.models.graphsage import graphsage
    with pytest.raises(ValueError, match="GraphSAGE and GAT victims are not covered"):
        E.influence_scores(graphsage(nfeat=3, nclass=2, nhid=4, device="cpu"), X, A)
    with pytest.raises(ValueError, match="65535"):
        E.influence_scores((W, b, Wlin, blin), torch.zeros(1, 3).expand(65536, 3), torch.zeros(1, 1).expand(65536, 65536))
    with pytest.raises(ValueError, match="device tensors|cpu tensor"):      # everything else in order: a host tensor is refused last
        E.influence_scores(**good)
    from mc_gra_amd.models.gcn import GCN
    got = E.victim_gcn_tensors(GCN(nfeat=3, nhid=4, nclass=2, nlayer=3, device="cpu"))
    assert [tuple(w.shape) for w in got[0]] == [(3, 4), (4, 4), (4, 4)] and tuple(got[2].shape) == (2, 4) and len(got[1]) == 3


# ------------------------------------------------------------------------------------------------ 4. the command line
def test_parser_takes_the_mode_and_its_flags(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in R.LINKTELLER_FLAGS) and "lt_" not in str(plain) and "linkteller" not in str(plain)
    a = p.parse_args(["--mode", "link_teller"])
    assert a.mode == "link_teller" == R.LINKTELLER_MODE and not any(hasattr(a, k) for k in R.LINKTELLER_FLAGS)
    a = p.parse_args(["--mode", "link_teller", "--lt_graph", "raw", "--lt_delta", "1e-3", "--save_linkteller", "lt.npz", "--dp_defense", "edgerand",
                      "--dp_eps", "8"])
    assert (a.lt_graph, a.lt_delta, a.save_linkteller, a.dp_defense) == ("raw", 1e-3, "lt.npz", "edgerand")
    for argv, message in ((["--lt_graph", "raw"], "--lt_graph needs --mode link_teller"), (["--lt_delta", "1e-3"], "--lt_delta needs --mode link_teller"),
                          (["--mode", "link_stealing", "--save_linkteller", "x.npz"], "--save_linkteller needs --mode link_teller"),
                          (["--mode", "link_teller", "--lt_graph", "weighted"], "invalid choice"),
                          (["--mode", "link_teller", "--arch", "sage"], "--arch gcn only, not --arch sage"),
                          (["--mode", "link_teller", "--arch", "gat"], "--arch gcn only, not --arch gat"),
                          (["--mode", "link_teller", "--ap"], "not --mode link_teller"),
                          (["--mode", "link_teller", "--lt_delta", "0"], "finite, not 0 and below 1"),
                          (["--mode", "link_teller", "--lt_delta", "1"], "finite, not 0 and below 1"),
                          (["--mode", "link_teller", "--lt_delta", "nan"], "finite, not 0 and below 1"),
                          (["--mode", "link_teller", "--lt_delta", "1e-60"], "finite, not 0 and below 1"),
                          (["--mode", "link_teller", "--save_linkteller", ""], ".npz"),
                          (["--ci", "--versus", "linkteller:logits"], "output `logits` is not one of log_posteriors, posteriors"),
                          (["--ci", "--versus", "linkteller:cosine"], "output `cosine` is not one of log_posteriors, posteriors"),
                          (["--versus", "linkteller:posteriors"], "--versus needs --ci or --ci_nodes"),
                          (["--ci", "--versus", "linkteller:posteriors", "--arch", "gat"], "--arch gcn only, not --arch gat")):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        assert message in capsys.readouterr().err, argv
    for out in ("posteriors", "log_posteriors"):
        a = p.parse_args(["--ci_nodes", "--versus", f"linkteller:{out}"])
        assert a.versus == f"linkteller:{out}" and R.versus_linkteller(a.versus, None) == out and R.versus_baseline(a.versus, None) is None
    fail = []
    for other in ("features", "scores.npy", "posteriors:cosine", "linkteller", "run:3/scores.npy", "", None):      # today's meanings stay
        assert R.versus_linkteller(other, fail.append) is None
    assert fail == [] and R.versus_baseline("posteriors:cosine", fail.append) == ("posteriors", "cosine")
    for flag in ("--mode link_teller", "--lt_graph", "--lt_delta", "--save_linkteller", "--versus linkteller:posteriors|log_posteriors"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="--arch gcn only"):      # a namespace built by hand is checked by the run too
        M._run(argparse.Namespace(mode="link_teller", arch="sage", seed=1), 0, 1)


@pytest.mark.parametrize("flags", (["--topk", "5"], ["--curves", "c.npz"], ["--per_node", "p.npz"], ["--binarize"], ["--ci"], ["--ci_nodes"],
                                   ["--save_scores", "s.npy"], ["--structure", "edges"], ["--hops", "3"], ["--by_class", "labels"],
                                   ["--ablate"], ["--knn", "3"], ["--exposure"], ["--ci", "--versus", "linkteller:posteriors"]))
def test_report_flags_are_refused_under_link_teller(pkg, capsys, flags):
    from mc_gra_amd import main as M
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["--mode", "link_teller"] + flags)
    assert "--mode evaluate only, not --mode link_teller" in capsys.readouterr().err
    args = argparse.ArgumentParser.parse_args(M.build_parser(), ["--mode", "link_teller"] + flags)      # the parser without its checks
    with pytest.raises(SystemExit, match="not --mode link_teller"):
        M._run(args, 0, 1)


def test_link_teller_lines_and_result_shape(pkg, monkeypatch):
    """reports.link_teller_metrics asks the engine for the AUC of every set and for the top k of every belief; the lines are the result's."""
    import torch
    from mc_gra_amd import reports as R
    calls = []

    def auc_delong(real, pred, idx=None, level=0.95):
        calls.append(("auc", None if idx is None else tuple(idx)))
        return {"auc": 0.75, "pairs": 45 if idx is None else 3, "positives": 10 if idx is None else 1, "se": 0.1}

    def topk_metrics(real, pred, k=None, idx=None):
        calls.append(("topk", k, None if idx is None else tuple(idx)))
        assert k > 0
        return {"k": k, "hits": 1, "precision": 1 / k, "recall": 0.5, "f1": 0.25, "threshold": 0.0, "pairs": 45, "positives": 10}

    monkeypatch.setattr(R.engine, "auc_delong", auc_delong)
    monkeypatch.setattr(R.engine, "topk_metrics", topk_metrics)
    S = torch.zeros(10, 10)
    res = R.link_teller_metrics(S, S, {"attack": [1, 2, 3], "all": None})
    assert list(res) == ["attack", "all"] and res["all"]["auc"] == 0.75 and sorted(res["all"]) == ["auc", "beliefs", "pairs", "positives"]
    assert [b["k"] for b in res["all"]["beliefs"].values()] == [3, 5, 10, 20, 40] and list(res["all"]["beliefs"]) == list(R.LINKTELLER_BELIEFS)
    assert [b["k"] for b in res["attack"]["beliefs"].values()] == [0, 1, 1, 2, 3]           # a set of 3 pairs with one true edge: clamped
    none = dict(res["attack"]["beliefs"][0.25])                  # k = 0: nothing is taken, and the engine is not asked
    assert math.isnan(none.pop("precision")) and none == {"k": 0, "hits": 0, "recall": 0.0, "f1": 0.0}
    assert calls.count(("auc", None)) == 1 and ("topk", 40, None) in calls and ("topk", 3, (1, 2, 3)) in calls
    lines = R.link_teller_lines({"posteriors": res})
    assert lines[0] == "link teller posteriors: auc_attack=0.75 auc_all=0.75" and len(lines) == 3
    assert lines[2].startswith("link teller posteriors all beliefs: 0.25:k=3,P=") and " 4.0:k=40,P=0.025,R=0.5,F1=0.25" in lines[2]
