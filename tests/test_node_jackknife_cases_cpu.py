"""Without a GPU: the truth of the node jackknife (tests/node_jackknife_truth.py) against a literal delete-a-node-and-recount,
against DeLong's truth and against its own identities; that the inputs of tests/test_gpu_node_jackknife.py
(tests/node_jackknife_cases.py) have the properties they are named for and tell each wrong reading of the definition from the
right one; the host arithmetic of engine.node_jackknife_stats / node_jackknife_paired_stats; a seeded simulation of the order
DeLong < truth < jackknife; the refusals that need no device and main.py's argument checks."""
import argparse
import ctypes
import math

import numpy as np
import pytest

from tests import delong_truth as DT
from tests import node_jackknife_cases as NC
from tests import node_jackknife_truth as T

CASES = NC.cases()
SMALL = [k for k, v in CASES.items() if (len(v[0]) if v[3] is None else len(v[3])) <= 12]
UP_TO_400 = [k for k, v in CASES.items() if (len(v[0]) if v[3] is None else len(v[3])) <= 400]


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


def _rows(name):
    real, _, _, idx, _ = CASES[name]
    return len(real) if idx is None else len(idx)


def _heavy(rng, n, asym):
    """n <= 12 nodes, scores from five values with both zeros, asymmetric on demand."""
    vals = np.array([-0.0, 0.0, 0.5, -1.5, 2.0], np.float32)
    real = (rng.rand(n, n) < 0.4).astype(np.float32)
    pred = vals[rng.randint(0, len(vals), (n, n))]
    if not asym:
        real, pred = np.tril(real, -1) + np.tril(real, -1).T, np.tril(pred, -1) + np.tril(pred, -1).T
    return real, pred


# ------------------------------------------------------------------------------------------------ 1. the truth
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 12])
@pytest.mark.parametrize("asym", [False, True])
def test_truth_against_a_literal_delete_and_recount(n, asym):
    """T - A_v - B_v + C_v, P - P_v and N - N_v are what is counted when position v is really deleted: ties, signed zeros,
    asymmetric matrices, a permuted subset."""
    rng = np.random.RandomState(100 * n + asym)
    real, pred = _heavy(rng, n + 3, asym)
    for idx in (None, rng.permutation(n + 3)[:n]):
        g = T.ints(real, pred, idx)
        want = T.recount(real, pred, idx)
        got = [(g["T"] - a - b + c, g["positives"] - pv, g["negatives"] - nv)
               for pv, nv, a, b, c in zip(*(g[k] for k in T.COLUMNS))]
        if (n if idx is not None else n + 3) > 2:
            assert got == want, (n, asym, idx)
        d = DT.ints(real, pred, idx)
        assert (g["pairs"], g["positives"], g["negatives"], g["T"]) == (d["pairs"], d["positives"], d["negatives"], d["T"])


@pytest.mark.parametrize("name", SMALL)
def test_small_cases_against_the_recount(name):
    real, pa, pb, idx, _ = CASES[name]
    for pred in (pa, pb):
        g = T.ints(real, pred, idx)
        got = [(g["T"] - a - b + c, g["positives"] - pv, g["negatives"] - nv) for pv, nv, a, b, c in zip(*(g[k] for k in T.COLUMNS))]
        if _rows(name) > 2:
            assert got == T.recount(real, pred, idx), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_truth_against_delongs_header_and_the_identities(name):
    """sum P_v = 2 P, sum N_v = 2 N, sum A_v = sum B_v = 2 T, C_v <= min(A_v, B_v, 2 P_v N_v), P_v + N_v = m - 1."""
    real, pa, _, idx, _ = CASES[name]
    g = T.ints(real, pa, idx)
    m = _rows(name)
    if m <= 1100:
        d = DT.ints(real, pa, idx)
        assert (g["pairs"], g["positives"], g["negatives"], g["T"]) == (d["pairs"], d["positives"], d["negatives"], d["T"])
    assert g["pairs"] == m * (m - 1) // 2 == g["positives"] + g["negatives"]
    assert sum(g["P_v"]) == 2 * g["positives"] and sum(g["N_v"]) == 2 * g["negatives"]
    assert sum(g["A_v"]) == sum(g["B_v"]) == 2 * g["T"]
    for pv, nv, a, b, c in zip(*(g[k] for k in T.COLUMNS)):
        assert pv + nv == m - 1 and 0 <= c <= min(a, b, 2 * pv * nv)
    assert max(g["A_v"] + g["B_v"]) < 2 ** 48 and g["T"] < 2 ** 61


def test_the_closed_form_of_the_capacity_case():
    for n in (2, 3, 4, 5, 6, 7, 9, 50, 51):
        real, pred = NC.path_scores(n)
        assert NC.path_truth(n) == T.ints(real, pred), n
    g = NC.path_truth(NC.MAX_NIDX)
    assert 2 ** 31 - 2 ** 17 < g["pairs"] < 2 ** 31 and sum(g["A_v"]) == sum(g["B_v"]) == 2 * g["T"] and sum(g["N_v"]) == 2 * g["negatives"]
    assert max(g["C_v"]) > 0 and min(g["C_v"]) >= 0 and len(set(g["A_v"])) > 2 and T.stats(g)["undefined_nodes"] == 0


# ---------------------------------------------------------------------------------------- 2. the wrong readings
def _wrong(how, real, pred, idx):
    g = T.ints(real, pred, idx)
    if how == "c_dropped":
        return dict(g, C_v=[0] * len(g["C_v"]))
    if how == "c_subtracted":
        return dict(g, C_v=[-c for c in g["C_v"]])
    if how == "ties_count_0":
        return T.ints(real, pred, idx, tie=0)
    if how == "ties_count_1":
        return T.ints(real, pred, idx, tie=2)
    if how == "rows_not_the_lower_triangle":       # pair (a, b), a > b, read at [idx[b]][idx[a]]
        return T.ints(np.asarray(real).T, np.asarray(pred).T, idx)
    if how == "node_id_for_position":              # row v of the answer given to the v-th smallest node id
        order = np.argsort(np.arange(len(real)) if idx is None else idx)
        return dict(g, **{k: [g[k][i] for i in order] for k in T.COLUMNS})
    if how == "ordered_pairs":                     # every pair twice
        return dict({k: [2 * x for x in g[k]] for k in T.COLUMNS}, pairs=2 * g["pairs"], positives=2 * g["positives"],
                    negatives=2 * g["negatives"], T=4 * g["T"])
    raise KeyError(how)


TELLS = {
    "c_dropped": ["n4", "five_levels", "hub_degree_299", "path_n50"],
    "c_subtracted": ["n4", "five_levels", "hub_degree_299", "path_n50"],
    "ties_count_0": ["n4_ties", "n64_all_equal", "five_levels", "signed_zeros_only", "class_P4096_ties", "path_n50"],
    "ties_count_1": ["n4_ties", "n64_all_equal", "five_levels", "signed_zeros_only", "class_P4096_ties", "path_n50"],
    "rows_not_the_lower_triangle": ["asymmetric", "asymmetric_labels", "idx_descending"],
    "node_id_for_position": ["subset_permuted", "subset_reordered", "idx_descending"],
    "ordered_pairs": ["n3", "five_levels", "asymmetric"],
}


@pytest.mark.parametrize("how", sorted(TELLS))
def test_the_cases_tell_each_wrong_reading_from_the_truth(how):
    """Each family differs from the reading it is there for in the integers, and where deletions are defined in the jackknife's
    doubles too."""
    for name in TELLS[how]:
        real, pa, _, idx, _ = CASES[name]
        g, w = T.ints(real, pa, idx), _wrong(how, real, pa, idx)
        assert g != w, (how, name)
        if how in ("c_dropped", "c_subtracted"):
            gv, wv = T.influences(g)[1], T.influences(w)[1]
            assert any(x is not None and x != y for x, y in zip(gv, wv)), (how, name)
    # junk outside the selected lower triangle cannot even be read the wrong way round
    real, pa, _, idx, _ = CASES["junk_outside_selection"]
    with pytest.raises(AssertionError):
        _wrong("rows_not_the_lower_triangle", real, pa, idx)


def test_the_cases_hold_what_they_are_named_for():
    for rows, why in NC.TILING.items():
        assert _rows(f"tiling_n{rows}") == rows and why
        g = T.ints(*CASES[f"tiling_n{rows}"][:2])
        assert g["positives"] > 0 and T.stats(g)["var"] > 0
    for c in (NC.THREADS, NC.ROW_BLOCKS, NC.COLS):
        assert c + 1 in NC.TILING and c + 2 in NC.TILING                 # c columns / rows with candidates, and c + 1
    assert NC.SCAN_LANES - 1 in NC.TILING and NC.SCAN_LANES in NC.TILING      # n_idx + 1 degrees are scanned
    for name, (n, P, kind, why) in NC.CLASS_SIZES.items():
        real = CASES[f"class_{name}"][0]
        a, b = np.tril_indices(n, -1)
        assert len(real) == n and int((real[a, b] == 1).sum()) == P and why
    sizes = {v[1] for v in NC.CLASS_SIZES.values()}
    for c in (NC.THREADS, NC.SORT_TILE // 2, NC.SORT_TILE, NC.POS_BLOCKS * NC.THREADS, NC.SORT_BLOCKS * NC.SORT_TILE // 2):
        assert c in sizes and c + 1 in sizes, c
    assert NC.STAGE in sizes and NC.STAGE + 1 in sizes and 2 * NC.STAGE + 1 in sizes
    # node kinds
    g = T.ints(*CASES["star"][:2])
    s = T.stats(g)
    assert g["P_v"][17] == g["positives"] == 49 and s["undefined_nodes"] == 1 and math.isnan(s["var"]) and not math.isnan(s["auc"])
    assert math.isnan(s["influence"][17]) and not math.isnan(s["influence"][16])
    g = T.ints(*CASES["isolated_node"][:2])
    assert g["P_v"][23] == 0 and g["A_v"][23] == 0 and g["C_v"][23] == 0 and g["B_v"][23] > 0 and T.stats(g)["var"] > 0
    g = T.ints(*CASES["hub_degree_299"][:2])
    assert g["P_v"][5] >= 299 > NC.THREADS and T.stats(g)["undefined_nodes"] == 0
    for name, key in (("n64_no_positive", "positives"), ("n64_no_negative", "negatives")):
        g = T.ints(*CASES[name][:2])
        assert g[key] == 0 and g["T"] == 0 and not any(g["A_v"] + g["B_v"] + g["C_v"]) and T.stats(g)["undefined_nodes"] == 64
    # asymmetric and junk: nothing outside the selected lower triangle is valid
    real, pa, pb, idx, _ = CASES["junk_outside_selection"]
    assert np.isnan(pa[np.triu_indices(len(pa))]).any() and not np.array_equal(CASES["asymmetric"][1], CASES["asymmetric"][1].T)
    idx = CASES["idx_descending"][3]
    assert (np.diff(idx) < 0).all()
    assert CASES["n257_ld288"][4] == 31
    # the reordered subset: the same nodes, every node's five integers the same
    a, b = CASES["subset_permuted"][3], CASES["subset_reordered"][3]
    ga, gb = T.ints(*CASES["subset_permuted"][:2], a), T.ints(*CASES["subset_reordered"][:2], b)
    assert sorted(a) == sorted(b) and list(a) != list(b)
    where = {int(v): i for i, v in enumerate(a)}
    assert all(gb[k] == [ga[k][where[int(v)]] for v in b] for k in T.COLUMNS) and ga["P_v"] != gb["P_v"]
    # the paired relations
    real, a, same, _, _ = CASES["b_equals_a"]
    assert np.array_equal(a[np.tril_indices(len(a), -1)], same[np.tril_indices(len(a), -1)])
    p = T.paired_stats(T.ints(real, a), T.ints(real, same))
    assert p["delta"] == 0.0 and p["se_delta"] == 0.0 and p["z"] == 0.0 and p["p_value"] == 1.0 and not any(p["influence"])
    p = T.paired_stats(T.ints(real, a), T.ints(real, CASES["b_minus_a"][2]))
    assert p["a"]["auc"] + p["b"]["auc"] == 1.0 and p["se_delta"] > 0


# ---------------------------------------------------------------------------------------- 3. the host arithmetic
@pytest.mark.parametrize("level", [0.95, 0.5])
def test_engine_stats_equal_the_truth_bit_for_bit(pkg, level):
    from mc_gra_amd import engine as E
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or a == b
    for name in UP_TO_400:
        real, pa, pb, idx, _ = CASES[name]
        ga, gb = T.ints(real, pa, idx), T.ints(real, pb, idx)
        got, want = E.node_jackknife_stats(ga, level), T.stats(ga, level)
        for k in T.RATES:
            assert isinstance(got[k], float) and same(got[k], want[k]), (name, k, got[k], want[k])
        assert got["ints"] == ga and got["undefined_nodes"] == want["undefined_nodes"] and got["nodes"] == _rows(name)
        assert all(same(x, y) for x, y in zip(got["influence"].tolist(), want["influence"])) and got["level"] == level
        got, want = E.node_jackknife_paired_stats(ga, gb, level), T.paired_stats(ga, gb, level)
        for k in T.PAIRED_RATES:
            assert isinstance(got[k], float) and same(got[k], want[k]), (name, k, got[k], want[k])
        assert all(same(x, y) for x, y in zip(got["influence"].tolist(), want["influence"]))
    # the sequences may be tensors
    import torch
    g = T.ints(*CASES["five_levels"][:2])
    as_t = dict(g, **{k: torch.tensor(g[k]) for k in T.COLUMNS})
    assert E.node_jackknife_stats(as_t)["var"] == T.stats(g)["var"] and E.node_jackknife_stats(as_t)["ints"] == g


def test_host_stats_against_a_full_fraction_evaluation(pkg):
    """At m <= 60 the same formulas with nothing rounded until the end: var within 4 ulp."""
    from mc_gra_amd import engine as E
    checked = 0
    for name in sorted(CASES):
        if not 3 <= _rows(name) <= 60:
            continue
        real, pa, pb, idx, _ = CASES[name]
        for pred in (pa, pb):
            g = T.ints(real, pred, idx)
            auc, d = T.influences(g)
            if auc is None or any(x is None for x in d):
                continue
            exact = float(T.exact_variance(d))
            got = E.node_jackknife_stats(g)["var"]
            print(name, got, exact)
            assert abs(got - exact) <= 4 * math.ulp(exact), (name, got, exact)
            m = len(d)
            assert abs(E.node_jackknife_stats(g)["auc_jackknife"] - float(auc + (m - 1) * sum(d) / m)) <= 4 * math.ulp(float(auc))
            checked += 1
    assert checked >= 8


def test_degenerate_host_rules(pkg):
    from mc_gra_amd import engine as E
    nan = math.isnan
    # P or N = 0, also m = 2: everything NaN
    for name in ("n64_no_positive", "n64_no_negative", "n2_one_positive", "n2_one_negative"):
        s = E.node_jackknife_stats(T.ints(*CASES[name][:2]))
        assert all(nan(s[k]) for k in T.RATES) and s["influence"].isnan().all() and s["undefined_nodes"] == s["nodes"]
    # a node whose deletion leaves no AUC: the AUC alone
    s = E.node_jackknife_stats(T.ints(*CASES["star"][:2]))
    assert not nan(s["auc"]) and all(nan(s[k]) for k in T.RATES[1:]) and s["undefined_nodes"] == 1
    assert int(s["influence"].isnan().sum()) == 1
    s = E.node_jackknife_stats(T.ints(*CASES["n3_one_positive"][:2]))
    assert not nan(s["auc"]) and nan(s["var"]) and s["undefined_nodes"] == 3     # the third node holds both negatives
    p = E.node_jackknife_paired_stats(T.ints(*CASES["star"][:2]), T.ints(CASES["star"][0], CASES["star"][2]))
    assert not nan(p["delta"]) and all(nan(p[k]) for k in T.PAIRED_RATES[1:]) and p["undefined_nodes"] == 1
    # var == 0: the interval is [auc, auc]
    s = E.node_jackknife_stats(T.ints(*CASES["n64_all_equal"][:2]))
    assert s["auc"] == 0.5 and s["var"] == 0.0 and s["se"] == 0.0 and s["ci_low"] == s["ci_high"] == 0.5 and not s["influence"].any()
    assert s["auc_jackknife"] == 0.5
    # paired, var == 0 with delta == 0: a scoring against itself
    ga = T.ints(*CASES["n64_all_equal"][:2])
    p = E.node_jackknife_paired_stats(ga, ga)
    assert p["delta"] == 0.0 and p["z"] == 0.0 and p["p_value"] == 1.0 and p["ci_low"] == p["ci_high"] == 0.0
    # paired, var == 0 with delta != 0: a perfect matching of 4 nodes, every positive above every negative against every one below
    real = np.zeros((4, 4), np.float32)
    real[1, 0] = real[3, 2] = 1
    up, down = T.ints(real, real), T.ints(real, -real)
    assert up["P_v"] == [1] * 4 and up["T"] == 16 and down["T"] == 0
    for a, b, sign in ((up, down, 1.0), (down, up, -1.0)):
        p = E.node_jackknife_paired_stats(a, b)
        assert p["delta"] == sign and p["var_delta"] == 0.0 and p["z"] == sign * math.inf and p["p_value"] == 0.0
        assert p["ci_low"] == p["ci_high"] == sign and T.paired_stats(a, b)["z"] == p["z"]


def test_level_validation_and_the_paired_disagreement_check(pkg):
    from mc_gra_amd import engine as E
    g = T.ints(*CASES["n4"][:2])
    for level in (0.0, 1.0, 2.0, -0.5):
        with pytest.raises(ValueError, match="level"):
            E.node_jackknife_stats(g, level)
        with pytest.raises(ValueError, match="level"):
            E.node_jackknife_paired_stats(g, g, level)
    other = T.ints(CASES["n4_ties"][0], CASES["n4"][1])
    assert other["P_v"] == g["P_v"]
    E.node_jackknife_paired_stats(g, other)                                 # the same labels: fine
    flipped = CASES["n4"][0].copy()
    flipped[1, 0], flipped[2, 0] = flipped[2, 0], flipped[1, 0]              # the same P and N, other nodes
    with pytest.raises(ValueError, match="P_v"):
        E.node_jackknife_paired_stats(g, T.ints(flipped, CASES["n4"][1]))
    with pytest.raises(ValueError, match="positives"):
        E.node_jackknife_paired_stats(g, T.ints(*CASES["n3"][:2]) | {"pairs": g["pairs"]})
    with pytest.raises(ValueError, match="pairs"):
        E.node_jackknife_paired_stats(g, T.ints(*CASES["n3"][:2]))
    with pytest.raises(ValueError, match="length"):
        E.node_jackknife_stats(dict(g, C_v=g["C_v"][:-1]))


# ------------------------------------------------------------------------------------------------ 4. simulation
def simulate(reps=300, n=40, seed=7):
    """(empirical variance of the AUC over the replicates, mean DeLong variance, mean node-jackknife variance): graphs of a 2-d
    latent-position model, scores = latent product + an additive per-node effect + pair noise."""
    rng = np.random.RandomState(seed)
    a, b = np.tril_indices(n, -1)
    aucs, delong, jack = [], [], []
    for _ in range(reps):
        z, u = rng.randn(n, 2), 0.7 * rng.randn(n)
        g = (z @ z.T)[a, b]
        real, pred = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
        real[a, b] = rng.rand(len(a)) < 1 / (1 + np.exp(-(g - 1.5)))
        pred[a, b] = g + u[a] + u[b] + 0.5 * rng.randn(len(a))
        s, d = T.stats(T.ints(real, pred)), DT.stats(DT.ints(real, pred))
        if s["undefined_nodes"] or math.isnan(d["var"]):
            continue
        aucs.append(s["auc"]); delong.append(d["var"]); jack.append(s["var"])
    return float(np.var(aucs, ddof=1)), float(np.mean(delong)), float(np.mean(jack)), len(aucs)


def test_simulation_delong_below_the_truth_below_the_jackknife():
    """Only the order is asserted: DeLong's variance treats pairs that share a node as independent (optimistic), the node
    jackknife is biased upward (Efron and Stein 1981).  On this model the room is wide: about 0.26 : 1 : 1.18."""
    emp, dl, jk, used = simulate()
    print(f"empirical var {emp:.6f} (sd {math.sqrt(emp):.4f}); DeLong {dl:.6f} ({dl / emp:.2f} x, se {math.sqrt(dl):.4f}); "
          f"jackknife {jk:.6f} ({jk / emp:.2f} x, se {math.sqrt(jk):.4f}); {used} replicates")
    assert used >= 290 and dl < emp < jk


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    s = "mcgra_auc_node_jackknife"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 10
    for f in (E.auc_node_jackknife, E.auc_node_jackknife_paired):
        assert callable(f) and hasattr(f, "__wrapped__")                                                # the device guard
        assert "conservative where DeLong's" in f.__doc__ and "optimistic" in f.__doc__
    assert "Efron and Stein" in E.auc_node_jackknife.__doc__ and "1981" in E.auc_node_jackknife.__doc__
    assert E.NODE_JACKKNIFE_COLUMNS == T.COLUMNS


def test_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to the header."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = 2 ** 64 - 7

    def call(n=8, ldl=8, lds=8, idx=None, n_idx=None, lab=p, s=p, header=True, out=p):
        h = (ctypes.c_uint64 * 4)(*([mark] * 4))
        rc = L.mcgra_auc_node_jackknife(None, n, lab, ldl, s, lds, idx, n if n_idx is None else n_idx, h if header else None, out)
        assert list(h) == [mark] * 4
        return rc

    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(ldl=7), dict(lds=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(lab=None), dict(s=None), dict(out=None), dict(header=False)):
        assert call(**kw) == -1 and b"auc_node_jackknife:" in L.mcgra_last_error(), kw
    big = NC.MAX_NIDX + 1
    assert call(n=big, ldl=big, lds=big) == -3 and b"65535" in L.mcgra_last_error()
    assert call(n=10 ** 6, ldl=10 ** 6, lds=10 ** 6, idx=p, n_idx=big) == -3
    assert call(n=big, ldl=big, lds=big - 1) == -1                            # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(call(n=big, ldl=big, lds=big))


def test_engine_entries_refuse_wrong_shapes_host_tensors_and_levels(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for real, pred in ((wide, sq), (torch.zeros(5), sq), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.auc_node_jackknife.__wrapped__(real, pred)
        with pytest.raises(AssertionError):
            E.auc_node_jackknife_paired.__wrapped__(real, pred, sq)
    with pytest.raises(ValueError, match="device tensors"):
        E.auc_node_jackknife(sq, sq)                                     # a host tensor: refused before anything is called
    with pytest.raises(ValueError, match="device tensors"):
        E.auc_node_jackknife_paired(sq, sq, sq)
    for level in (0.0, 1.0, 2.0):
        with pytest.raises(ValueError, match="level"):
            E.auc_node_jackknife.__wrapped__(sq, sq, None, level)
        with pytest.raises(ValueError, match="level"):
            E.auc_node_jackknife_paired.__wrapped__(sq, sq, sq, None, level)


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_ci_nodes_flags_are_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in ("ci_nodes", "save_influence"))
    assert "ci_nodes" not in str(plain) and "save_influence" not in str(plain)
    a = p.parse_args(["--ci_nodes", "--versus", "features", "--save_influence", "i.npz"])
    assert a.ci_nodes is True and a.versus == "features" and a.save_influence == "i.npz" and not hasattr(a, "ci")
    a = p.parse_args(["--ci", "--ci_nodes", "--versus", "s.npy"])
    assert a.ci is True and a.ci_nodes is True
    with pytest.raises(SystemExit):
        p.parse_args(["--versus", "features"])
    assert "--versus needs --ci or --ci_nodes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--save_influence", "i.npz"])
    assert "--save_influence needs --ci_nodes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--ci", "--save_influence", "i.npz"])
    assert "--save_influence needs --ci_nodes" in capsys.readouterr().err
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ci_nodes", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err and "--ci_nodes" in err
    for flag in ("--ci_nodes", "--save_influence"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(ci_nodes=True, mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --ci_nodes"):
        M._run(argparse.Namespace(save_influence="i.npz", mode="evaluate"), 0, 1)
    calls = []
    R.check_ci_nodes_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_ci_nodes_args(argparse.Namespace(ci_nodes=True, save_influence="i.npz", mode="evaluate"), calls.append)
    R.check_ci_args(argparse.Namespace(ci_nodes=True, versus="x.npy", mode="evaluate"), calls.append)
    assert calls == []
    R.check_ci_nodes_args(argparse.Namespace(ci_nodes=True, save_influence="", mode="evaluate"), calls.append)
    assert len(calls) == 1 and ".npz" in calls[0]
