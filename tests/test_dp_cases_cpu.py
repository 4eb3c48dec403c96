"""Without a GPU: that the truth of tests/test_gpu_dp_graph.py (tests/dp_truth.py) is right -- Philox4x32-10 against its known
answers, EdgeRand's threshold by hand and its flips in distribution, LapGraph's noise in distribution and its count by hand;
that the inputs of the GPU tests (tests/dp_cases.py) have the properties they are there for and tell every wrong reading of the
definition from the right one; the refusals of engine.dp_perturb_graph and of the C entry that need no device; the command line;
the console line, the log line and the file of the report."""
import argparse
import ctypes
import math

import numpy as np
import pytest

from tests import dp_cases as DC
from tests import dp_truth as T
from tests import topk_truth as TK

EDGERAND = DC.edgerand_cases()
LAPGRAPH = DC.lapgraph_cases()
SMALL_EDGERAND = [c for c in EDGERAND if c[0] <= 129]
SMALL_LAPGRAPH = [c for c in LAPGRAPH if c[0] <= 129]


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


_memo = {}


def truth(mechanism, case, variant=None):
    key = (mechanism, case, variant)
    if key not in _memo:
        n, g, eps, seed, rep = case
        _memo[key] = T.perturb(DC.graph(g, n), mechanism, eps, seed, rep, variant)
    return _memo[key]


# -------------------------------------------------------------------------------------------------- 1. the truth
def test_philox_known_answers():
    for counter, key, want in T.KNOWN_ANSWERS:
        assert tuple(int(w[0]) for w in T.philox(*counter, *key)) == want
    # vectorised: the three counters at once under one key give what each gives alone
    c = np.array([k[0] for k in T.KNOWN_ANSWERS], np.uint64).T
    together = T.philox(*c, *T.KNOWN_ANSWERS[2][1])
    for i in range(3):
        alone = T.philox(*T.KNOWN_ANSWERS[i][0], *T.KNOWN_ANSWERS[2][1])
        assert [int(w[i]) for w in together] == [int(w[0]) for w in alone]


def test_edgerand_threshold_by_hand():
    T3, q3, e3 = T.threshold(math.log(3.0))                      # 1 / (1 + 3) = 1/4 up to the rounding of T
    assert abs(T3 - 2 ** 30) <= 1 and abs(q3 - 0.25) <= 2.0 ** -32 and abs(e3 - math.log(3.0)) < 1e-8
    assert T.threshold(50.0) == (0, 0.0, math.inf)               # 2^32 / (1 + e^50) < 1/2: nothing ever flips
    assert T.threshold(800.0) == (0, 0.0, math.inf)              # e^eps overflows
    T1, q1, e1 = T.threshold(1.0)
    assert T1 == int(math.floor(2 ** 32 / (1 + math.e) + 0.5)) == 1155094609 and q1 == T1 / 2 ** 32
    assert e1 == math.log((1 - q1) / q1) and abs(e1 - 1.0) < 1e-9
    assert T.threshold(1e-12)[0] <= 2 ** 31                      # the threshold always fits 32 bits


def test_edgerand_is_linktellers_mechanism_in_distribution():
    """Flipping with probability 1 / (1 + e^eps) is "with probability s = 2 / (1 + e^eps) replace the cell by a fair coin": the
    cell changes with probability s / 2.  At n = 2 048, seed 15: the flip count within 4 sigma of m q."""
    n = 2048
    A = np.zeros((n, n), np.float32)
    m = n * (n - 1) // 2
    for eps in (1.0, 4.0, 8.0):
        r = T.edgerand(A, eps, 15)
        q = r["flip_probability"]
        assert abs(q - 0.5 * 2.0 / (1.0 + math.exp(eps))) <= 2.0 ** -32
        z = (r["flips"] - m * q) / math.sqrt(m * q * (1 - q))
        print(f"eps={eps}: flips={r['flips']} expected={m * q:.1f} z={z:+.2f}")
        assert abs(z) < 4 and r["added"] == r["flips"] and r["kept"] == r["removed"] == 0


def test_laplace_noise_in_distribution_and_in_float64():
    n = 2048
    _, _, p = T.positions(n)
    w0, w1 = T.draws(p, 15, 0)
    u = ((w0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    assert u.min() > 0 and u.max() < 1
    x = -np.log(u)                                                # Exp(1): mean 1, variance 1
    print(f"mean={x.mean():.5f} var={x.var():.5f} negative share={np.mean(w1 >> np.uint32(31)):.5f}")
    assert abs(x.mean() - 1) < 0.01 and abs(x.var() - 1) < 0.01
    assert abs(np.mean(w1 >> np.uint32(31)) - 0.5) < 4 * 0.5 / math.sqrt(len(p))
    lap = T.laplace(w0, w1, 2.5)
    assert lap.dtype == np.float64 and np.array_equal(np.abs(lap), 2.5 * x) and np.array_equal(lap < 0, (w1 >> np.uint32(31)) == 1)


def test_lapgraph_count_by_hand():
    # counter (m, 0, replicate, 0) under the seed's key; u from the top 24 bits of w0, the sign from bit 31 of w1
    E, m, eps, seed, rep = 18, 2080, 1.0, DC.SEED_HI, 1
    w = T.philox(m, 0, rep, 0, seed & 0xffffffff, seed >> 32)
    u = ((int(w[0][0]) >> 8) + 0.5) / 2 ** 24
    noise = (1.0 / (0.01 * eps)) * -math.log(u) * (-1 if int(w[1][0]) >> 31 else 1)
    got = T.count_draw(E, m, eps, seed, rep)
    assert got[0] == pytest.approx(noise, rel=1e-15) and got[2] == min(max(round(E + noise), 0), m)
    assert T.count_draw(E, m, eps, seed, rep, "count_at_0")[0] != got[0]


@pytest.mark.parametrize("case", SMALL_LAPGRAPH + [c for c in LAPGRAPH if c[0] == DC.TIE_N], ids=DC.case_id)
def test_lapgraph_truth_has_exactly_the_target_edges(case):
    r = truth("lapgraph", case)
    assert r["edges_out"] == r["target"] == int(r["bits"].sum()) and r["kept"] + r["removed"] == r["edges"]
    assert np.array_equal(r["out"], r["out"].T) and not r["out"].diagonal().any()
    order = TK.ranking(r["v"])
    assert np.array_equal(np.sort(order[:r["target"]]), np.flatnonzero(r["bits"]))
    assert r["v"].dtype == np.float32 and np.array_equal(r["v"], r["v64"].astype(np.float32))


# ------------------------------------------------------------------------------------------------- 2. the cases
def test_the_sizes_straddle_the_tiles():
    assert {63, 64, 65, 127, 128, 129} <= set(DC.SIZES) and 2 in DC.SIZES and 3 in DC.SIZES
    assert DC.BIG * (DC.BIG - 1) // 2 > 8e6 and (DC.SEED_LO ^ DC.SEED_HI) & 0xffffffff == 0 and DC.SEED_HI >> 32
    r = DC.LARGE_ROWS[1]
    assert r * (r - 1) // 2 < 2 ** 30 <= r * (r - 1) // 2 + r - 1 and DC.LARGE * (DC.LARGE - 1) // 2 < 2 ** 31
    A = DC.graph("random", 1025)
    assert np.array_equal(A, A.T) and not A.diagonal().any() and 0.008 < A.mean() < 0.012
    B = DC.graph("asymmetric", 129)
    assert np.array_equal(np.tril(B, -1), np.tril(DC.graph("random", 129), -1)) and not np.array_equal(B, B.T)


def test_every_lapgraph_count_draw_is_far_from_a_half():
    """The host's log and numpy's may differ in the last bit of the count's noise: rint(E + noise) is the same as long as
    E + noise is not within that of k + 1/2.  A condition on the inputs, not on the code."""
    for case in LAPGRAPH:
        n, g, eps, seed, rep = case
        E = int(np.tril(DC.graph(g, n), -1).sum())
        _, noisy, _ = T.count_draw(E, n * (n - 1) // 2, eps, seed, rep)
        assert abs((noisy - math.floor(noisy)) - 0.5) > 1e-6, case


def test_the_pinned_seeds_do_what_they_are_there_for():
    m = DC.CLAMP_N * (DC.CLAMP_N - 1) // 2
    zero = truth("lapgraph", (DC.CLAMP_N, "random", DC.LAP_NOISE_EPS, DC.CLAMP_ZERO_SEED, 0))
    full = truth("lapgraph", (DC.CLAMP_N, "random", DC.LAP_NOISE_EPS, DC.CLAMP_ALL_SEED, 0))
    assert zero["target"] == 0 and zero["count_noisy"] < -1 and not zero["out"].any()
    assert full["target"] == m and full["count_noisy"] > m + 1 and full["added"] == m - full["edges"]
    for g in ("random", "complete"):                              # eps = 1e4: the graph itself
        r = truth("lapgraph", (129, g, DC.LAP_EXACT_EPS, DC.SEED_LO, 0))
        assert np.array_equal(r["out"], DC.graph(g, 129)) and r["added"] == r["removed"] == 0 and abs(r["count_noise"]) < 0.5
    tie = truth("lapgraph", (DC.TIE_N, "random", 1.0, DC.TIE_SEED, 0))
    order, k = TK.ranking(tie["v"]), tie["target"]
    assert tie["v"][order[k - 1]] == tie["v"][order[k]] and order[k - 1] < order[k]      # the tie rule decides
    for eps in DC.EDGERAND_EPS:                                   # eps = 50 is the identity; the others change something
        r = truth("edgerand", (129, "random", eps, DC.SEED_LO, 0))
        assert (r["flips"] == 0) == (eps == 50.0) and (eps != 50.0 or np.array_equal(r["out"], DC.graph("random", 129)))
    a, b, c = (truth("edgerand", (129, "random", 1.0, s, r)) for s, r in ((DC.SEED_LO, 0), (DC.SEED_HI, 0), (DC.SEED_LO, 1)))
    assert not np.array_equal(a["bits"], b["bits"]) and not np.array_equal(a["bits"], c["bits"])


def test_the_cases_tell_the_wrong_readings_from_the_truth():
    told = {}
    for v in ("le", "seed_counter", "upper", "row_major"):
        told[v] = [c for c in SMALL_EDGERAND if not np.array_equal(truth("edgerand", c, v)["bits"], truth("edgerand", c)["bits"])]
    # `<=` for `<` shows only where a draw equals T: the case whose eps makes T one pair's own draw, and that pair alone
    eps, p = DC.boundary_eps()
    edge = (65, "random", eps, DC.SEED_LO, 0)
    assert told["le"] == [edge] and np.flatnonzero(truth("edgerand", edge, "le")["bits"] != truth("edgerand", edge)["bits"]).tolist() == [p]
    for v in ("sign_w0", "seed_counter", "upper", "row_major", "eps_swapped", "count_at_0", "ties_last"):
        told[v] = told.get(v, []) + [c for c in SMALL_LAPGRAPH + [LAPGRAPH[-1]] if v != "ties_last" or c[0] == DC.TIE_N
                                     if not np.array_equal(truth("lapgraph", c, v)["bits"], truth("lapgraph", c)["bits"])]
    assert set(told) == set(T.VARIANTS)
    for v, cases in told.items():
        assert cases, f"no case tells the wrong reading {v!r} from the truth"
    for mech in T.MECHANISMS:                                     # only the lower triangle is read
        assert np.array_equal(truth(mech, (129, "asymmetric", 1.0, DC.SEED_LO, 0))["bits"], truth(mech, (129, "random", 1.0, DC.SEED_LO, 0))["bits"])


def test_a_pair_draws_the_same_in_every_graph_size():
    small, big = T.draws(T.positions(65)[2], DC.SEED_HI, 1), T.draws(T.positions(129)[2], DC.SEED_HI, 1)
    assert np.array_equal(small[0], big[0][:len(small[0])]) and np.array_equal(small[1], big[1][:len(small[1])])


# -------------------------------------------------------------------------------------------- 3. refusals without a device
def test_engine_refuses_before_any_device_call(pkg, monkeypatch):
    import torch
    from mc_gra_amd import engine as E
    assert E.DP_MECHANISMS == ("edgerand", "lapgraph") == T.MECHANISMS

    def never(*a, **k):
        raise AssertionError("the device entry was called")

    monkeypatch.setattr(E.lib, "mcgra_dp_perturb_graph", never)
    monkeypatch.setattr(E, "_stream", never)
    A = torch.zeros(5, 5)
    bad = [dict(mechanism="laplace"), dict(mechanism=0), dict(mechanism=None), dict(eps=0.0), dict(eps=-1.0), dict(eps=math.nan),
           dict(eps=math.inf), dict(eps="1"), dict(eps=True), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(replicate=-1),
           dict(replicate=1 << 32), dict(want_noisy=True), dict(adj=torch.zeros(5, 6)), dict(adj=torch.zeros(5)),
           dict(adj=torch.zeros(1, 1)), dict(adj=np.zeros((5, 5))), dict(out=torch.zeros(4, 4)),
           dict(out=torch.zeros(5, 5, dtype=torch.float64)), dict(out=torch.zeros(5, 10)[:, ::2])]
    for kw in bad:
        args = dict(adj=A, mechanism="edgerand", eps=1.0, seed=15)
        args.update(kw)
        with pytest.raises(ValueError, match="dp_perturb_graph|dp mechanism"):
            E.dp_perturb_graph(**args)
    with pytest.raises(ValueError, match="65535"):
        E.dp_perturb_graph(torch.zeros(1, 1).expand(65536, 65536), "edgerand", 1.0, 0)
    with pytest.raises(ValueError, match="device tensors"):      # everything else in order: a host tensor is refused last
        E.dp_perturb_graph(A, "lapgraph", 1.0, (1 << 64) - 1, (1 << 32) - 1, want_noisy=True)


def test_c_entry_refuses_before_any_hip_call(pkg):
    L = pkg._lib.lib
    mark = -77
    p = ctypes.c_void_p(4096)                                      # never followed: every call below is refused first

    def call(n=5, adj=p, lda=5, mech=0, eps=1.0, out=p, ldo=5, noisy=None, ldn=0, counts=True):
        c, r = (ctypes.c_int64 * 6)(*([mark] * 6)), (ctypes.c_double * 2)(-7.0, -7.0)
        rc = L.mcgra_dp_perturb_graph(None, n, adj, lda, mech, eps, 15, 0, out, ldo, noisy, ldn, c if counts else None, r)
        assert list(c) == [mark] * 6 and list(r) == [-7.0, -7.0]
        return rc

    for kw in (dict(n=1), dict(n=0), dict(n=-4), dict(n=65536, lda=65536, ldo=65536), dict(eps=0.0), dict(eps=-2.0),
               dict(eps=math.nan), dict(eps=math.inf), dict(mech=2), dict(mech=-1), dict(noisy=p, ldn=5), dict(mech=1, noisy=p, ldn=4),
               dict(out=None), dict(counts=False), dict(adj=None), dict(lda=4), dict(ldo=4)):
        assert call(**kw) == -1 and b"dp_perturb_graph:" in L.mcgra_last_error(), kw


# ------------------------------------------------------------------------------------------------ 4. the command line
def test_parser_defense_flags(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    flags = ("dp_defense", "dp_eps", "dp_seed", "save_defense")
    assert not any(hasattr(plain, k) for k in flags) and "dp_" not in str(plain) and "dp_" not in str(R.shown_parameters(plain))
    assert plain.defense is False and plain.add_noise is False      # the reference's two flags stay parsed (and unused)
    a = p.parse_args(["--dp_defense", "lapgraph", "--dp_eps", "4", "--dp_seed", "7", "--save_defense", "d.npz"])
    assert (a.dp_defense, a.dp_eps, a.dp_seed, a.save_defense) == ("lapgraph", 4.0, 7, "d.npz") and R.defense_seed(a) == 7
    assert all(f"{k}=" in str(R.shown_parameters(a)) for k in flags)
    b = p.parse_args(["--dp_defense", "edgerand", "--dp_eps", "0.5", "--seed", "3"])
    assert R.defense_seed(b) == 3 and not hasattr(b, "dp_seed")
    for mode in R.DEFENSE_MODES:
        assert p.parse_args(["--dp_defense", "edgerand", "--dp_eps", "1", "--mode", mode]).mode == mode
    assert R.DEFENSE_MODES == ("evaluate", "notrain_test", "link_stealing")
    for argv, message in ((["--dp_eps", "1"], "--dp_eps needs --dp_defense"), (["--dp_seed", "1"], "--dp_seed needs --dp_defense"),
                          (["--save_defense", "x.npz"], "--save_defense needs --dp_defense"),
                          (["--dp_defense", "edgerand"], "--dp_defense needs --dp_eps"),
                          (["--dp_defense", "gauss", "--dp_eps", "1"], "invalid choice"),
                          (["--dp_defense", "edgerand", "--dp_eps", "0"], "finite privacy budget above 0"),
                          (["--dp_defense", "edgerand", "--dp_eps", "-1"], "finite privacy budget above 0"),
                          (["--dp_defense", "edgerand", "--dp_eps", "nan"], "finite privacy budget above 0"),
                          (["--dp_defense", "edgerand", "--dp_eps", "inf"], "finite privacy budget above 0"),
                          (["--dp_defense", "edgerand", "--dp_eps", "1", "--dp_seed", "-1"], "[0, 2^64)"),
                          (["--dp_defense", "edgerand", "--dp_eps", "1", "--save_defense", ""], ".npz"),
                          (["--dp_defense", "edgerand", "--dp_eps", "1", "--mode", "prepare"], "not --mode prepare")):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        assert message in capsys.readouterr().err, argv
    for flag in ("--dp_defense", "--dp_eps", "--dp_seed", "--save_defense", "--defense", "--add_noise"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="needs --dp_eps"):       # a namespace built by hand is checked by the run too
        M._run(argparse.Namespace(dp_defense="edgerand", mode="evaluate", seed=1), 0, 1)
    rep = [r for r in R.LATER_REPORTS if "dp_defense" in r.flags]
    assert len(rep) == 1 and rep[0].flags == flags and rep[0] is R.LATER_REPORTS[-1]
    assert rep[0].wanted(a) and not rep[0].wanted(plain) and not rep[0].wanted(argparse.Namespace(dp_eps=1.0))
    assert R.DefendedContext._fields == R.RunContext._fields + ("defense",) and R.DefendedContext._field_defaults["defense"] is None


# ------------------------------------------------------------------------------ 5. the report, from a fabricated info
def test_the_lines_and_the_file_from_a_fabricated_info(pkg, monkeypatch, tmp_path):
    import torch
    from mc_gra_amd import engine as E
    from mc_gra_amd import reports as R
    n = 40
    A = DC.graph("random", 129)[:n, :n] + 0
    A[5, 3] = A[3, 5] = A[9, 2] = A[2, 9] = 1.0
    r = T.edgerand(A, 2.0, 9)
    info = {"mechanism": "edgerand", "eps": 2.0, "seed": 9, "replicate": 0, "pairs": r["pairs"], "edges": r["edges"], "target": -1,
            "edges_out": r["edges_out"], "kept": r["kept"], "added": r["added"], "removed": r["removed"],
            "flip_probability": r["flip_probability"], "eps_realised": r["eps_realised"], "count_noise": math.nan,
            "test_accuracy": 0.625}
    line = R.defense_line(info)
    assert line == (f"defense edgerand eps=2.0 edges {r['edges']}->{r['edges_out']} (kept {r['kept']}, added {r['added']}, "
                    f"removed {r['removed']}) test_accuracy=0.625")

    def threshold_pairs(pred, threshold, idx=None, real=None):      # the engine's entry as its definition, on host tensors
        a, b = np.tril_indices(pred.shape[0], -1)
        keep = pred.numpy()[a, b] >= threshold
        pairs = np.stack([a[keep], b[keep]], 1).astype(np.int64)
        return torch.tensor(pairs), torch.tensor(pred.numpy()[a, b][keep]), torch.tensor(real.numpy()[a, b][keep] == 1)

    monkeypatch.setattr(E, "threshold_pairs", threshold_pairs)
    path = str(tmp_path / "d.npz")
    R.save_defense(path, torch.tensor(A), torch.tensor(r["out"]), info)
    z = np.load(path)
    assert sorted(z.files) == sorted(("edge_list", "added_list", "removed_list") + R.DEFENSE_SCALARS)
    a, b = np.tril_indices(n, -1)
    lab = A[a, b] == 1
    for key, mask in (("edge_list", r["bits"]), ("added_list", r["bits"] & ~lab), ("removed_list", lab & ~r["bits"])):
        assert z[key].dtype == np.int64 and np.array_equal(z[key], np.stack([a[mask], b[mask]], 1)), key
    assert len(z["added_list"]) == r["added"] > 0 and len(z["removed_list"]) == r["removed"] and len(z["edge_list"]) == r["edges_out"]
    assert str(z["mechanism"]) == "edgerand" and int(z["seed"]) == 9 and z["seed"].dtype == np.uint64 and int(z["target"]) == -1
    assert float(z["flip_probability"]) == r["flip_probability"] and math.isnan(float(z["count_noise"])) and float(z["test_accuracy"]) == 0.625
    # the report of --mode evaluate: auc_perturbed_* against the perturbed graph, one console line, one log line
    args = argparse.Namespace(dp_defense="edgerand", dp_eps=2.0, mode="evaluate", seed=9)
    seen = []
    monkeypatch.setattr(E, "roc_auc", lambda real, pred, idx=None: seen.append(real) or 0.25 + (0 if idx is None else len(idx)) / 1000)
    perturbed = torch.tensor(r["out"])
    ctx = R.DefendedContext(real=torch.tensor(A), inference_adj=torch.rand(n, n), sets={"attack": np.arange(30), "train": np.arange(8), "all": None},
                            n=n, rank=0, other=None, versus=None, args=args, defense={"perturbed": perturbed, "info": info})
    report = R.LATER_REPORTS[-1]
    res = report.compute(ctx)
    assert list(res) == ["defense", "auc_perturbed_attack", "auc_perturbed_train", "auc_perturbed_all"] and res["defense"] == info
    assert all(s is perturbed for s in seen) and len(seen) == 3
    assert (res["auc_perturbed_attack"], res["auc_perturbed_train"], res["auc_perturbed_all"]) == (0.28, 0.258, 0.25)
    assert report.console(res, ctx) == ["current auc_perturbed=0.25"]
    assert report.log(res, ctx) == [line + " auc_perturbed_attack=0.28 auc_perturbed_train=0.258 auc_perturbed_all=0.25"]
    assert report.save(res, ctx) is None
    # the log's parameter line shows the flags only while the defence is on
    assert "dp_defense='edgerand'" in str(R.shown_parameters(args)) and "dp_" not in str(R.shown_parameters(argparse.Namespace(seed=9, mode="evaluate")))
