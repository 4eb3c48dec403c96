"""Without a GPU: the truth of the graph-structure entry (tests/graph_structure_truth.py) against a literal triple loop, against
networkx where it is installed and against its own identities; that the inputs of tests/test_gpu_graph_structure.py
(tests/graph_structure_cases.py) have the properties they are named for and tell each wrong reading of the definition from the
right one; the host arithmetic of engine.graph_structure_stats and its degenerate rules; the entry's device-free refusals;
main.py's --structure / --save_structure checks."""
import argparse
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import graph_structure_cases as GC
from tests import graph_structure_truth as T
from tests.delong_cases import graph, lower, pairs_of

CASES = GC.cases()


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


def each_run(names=None):
    for name in sorted(CASES) if names is None else names:
        real, pred, idx, thrs = CASES[name]
        for thr in thrs:
            yield name, real, pred, idx, thr


def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


def same_stats(a, b):
    """Two stats dicts hold the same keys, the same integers and the same bits."""
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], dict):
            assert sorted(a[k]) == sorted(b[k]), k
            assert all(_same(a[k][q], b[k][q]) for q in a[k]), (k, a[k], b[k])
        else:
            assert _same(a[k], b[k]), (k, a[k], b[k])
    return True


# ------------------------------------------------------------------------------------------------ 1. the definition
def loop_ints(real, pred, thr, idx=None):
    """The definition, literally: a set of edges per graph, and for every position the pairs of its neighbours that are joined."""
    ix = list(range(len(pred))) if idx is None else [int(v) for v in idx]
    m = len(ix)
    thr = np.float32(thr)
    edges = {"R": set(), "G": set(), "C": set()}
    for a in range(m):
        for b in range(a):
            r = bool(np.float32(pred[ix[a], ix[b]]) >= thr)
            g = real is not None and real[ix[a], ix[b]] == 1
            for name, hit in (("R", r), ("G", g), ("C", r and g)):
                if hit:
                    edges[name].add((a, b))
    out = {"pairs": m * (m - 1) // 2}
    for name in "RGC":
        e = edges[name]
        has = lambda u, w: (max(u, w), min(u, w)) in e
        d, t = [0] * m, [0] * m
        for v in range(m):
            nb = [u for u in range(m) if u != v and has(u, v)]
            d[v] = len(nb)
            for i in range(len(nb)):
                for j in range(i):
                    t[v] += has(nb[i], nb[j])
        tri = sum(1 for a in range(m) for b in range(a) for c in range(b) if has(a, b) and has(a, c) and has(b, c))
        if real is None and name != "R":
            d, t, E, tri, W = [-1] * m, [-1] * m, -1, -1, -1
        else:
            E, W = len(e), sum(x * (x - 1) // 2 for x in d)
        out[f"d_{name}"], out[f"t_{name}"], out[f"E_{name}"], out[f"T_{name}"] = d, t, E, tri
        if name != "C":
            out[f"W_{name}"] = W
    return out


def small_inputs():
    rng = np.random.RandomState(3)
    for m in (2, 3, 5, 8, 12):
        real = graph(rng, m, 0.5)
        levels = lower(rng.randint(0, 4, pairs_of(m)) / 4, m)                 # ties at the thresholds
        for thr in (0.25, 0.5, 0.0, -float("inf"), float("inf")):
            yield real, levels, None, thr
        zeros = lower(np.array([0x80000000, 0, 1, 0x80000001], np.uint32).view(np.float32)[rng.randint(0, 4, pairs_of(m))], m)
        for thr in (-0.0, 0.0, 1e-45):
            yield real, zeros, None, thr
        asym = rng.randint(0, 4, (m, m)).astype(np.float32) / 4
        up = np.triu(np.ones((m, m), bool), 1)
        asym[up] = (0.75 - asym.T)[up]                                       # the opposite values above the diagonal
        asym[up & (rng.rand(m, m) < 0.3)] = np.nan
        lab = real.copy()
        lab[up] = 1 - lab[up]
        yield lab, asym, None, 0.5
    n = 12
    real, pred = graph(rng, n, 0.5), rng.randint(0, 8, (n, n)).astype(np.float32) / 8
    for k in (2, 5, 9, 12):
        yield real, pred, rng.permutation(n)[:k].copy(), 0.5


def test_truth_is_the_literal_definition():
    runs = 0
    for real, pred, idx, thr in small_inputs():
        for r in (real, None):
            assert T.ints(r, pred, thr, idx) == loop_ints(r, pred, thr, idx), (pred.shape, idx, thr)
            runs += 1
    assert runs >= 90
    # the sparse path of the truth is the dense one
    rng = np.random.RandomState(4)
    real = graph(rng, 200, 0.1)
    pred = GC.noisy_copy(rng, real, 0.1)
    dense = T.ints(real, pred, 0.5)
    old, T.DENSE_MAX = T.DENSE_MAX, 10
    try:
        assert T.ints(real, pred, 0.5) == dense
    finally:
        T.DENSE_MAX = old


def test_truth_against_networkx():
    nx = pytest.importorskip("networkx")
    for name, real, pred, idx, thr in each_run(["m63", "m65", "m129", "subset_permuted", "hub_and_isolated", "asymmetric",
                                                "circulant_n70", "m3_path"]):
        g = T.ints(real, pred, thr, idx)
        s = T.stats(g)
        Rm, Gm, _ = T.graphs(real, pred, thr, idx)
        for X, key, which in ((Rm, "R", "recovered"), (Gm, "G", "true")):
            G = nx.from_numpy_array(X.astype(np.int64))
            m = X.shape[0]
            assert [G.degree(v) for v in range(m)] == g[f"d_{key}"]
            tri = nx.triangles(G)
            assert [tri[v] for v in range(m)] == g[f"t_{key}"]
            assert G.number_of_edges() == g[f"E_{key}"] and sum(tri.values()) == 3 * g[f"T_{key}"]
            for got, want in ((s[which]["transitivity"], nx.transitivity(G)), (s[which]["avg_clustering"], nx.average_clustering(G))):
                assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300) or got == want, (name, thr, which, got, want)


def test_identities_hold_on_every_case():
    for name, real, pred, idx, thr in each_run():
        g = T.ints(real, pred, thr, idx)
        m = len(g["d_R"])
        assert g["pairs"] == pairs_of(m)
        for k in "RGC":
            assert sum(g[f"d_{k}"]) == 2 * g[f"E_{k}"] and sum(g[f"t_{k}"]) == 3 * g[f"T_{k}"], (name, k)
            assert all(t <= d * (d - 1) // 2 for d, t in zip(g[f"d_{k}"], g[f"t_{k}"]))
        for k in "RG":
            assert g[f"W_{k}"] == sum(d * (d - 1) // 2 for d in g[f"d_{k}"]) and 3 * g[f"T_{k}"] <= g[f"W_{k}"]
        assert all(c <= min(r, q) for c, r, q in zip(g["d_C"], g["d_R"], g["d_G"]))
        assert all(c <= min(r, q) for c, r, q in zip(g["t_C"], g["t_R"], g["t_G"]))
        bare = T.ints(None, pred, thr, idx)
        assert all(bare[k] == g[k] for k in ("pairs", "E_R", "T_R", "W_R", "d_R", "t_R"))
        assert all(bare[k] == -1 for k in T.HEADER[4:]) and all(bare[k] == [-1] * m for k in T.COLUMNS[2:])
    g = T.ints(*CASES["g_equals_r"][:2], 0.5)
    assert g["d_R"] == g["d_G"] == g["d_C"] and g["t_R"] == g["t_G"] == g["t_C"] and g["T_R"] > 0
    assert (g["E_R"], g["T_R"], g["W_R"]) == (g["E_G"], g["T_G"], g["W_G"]) and (g["E_C"], g["T_C"]) == (g["E_R"], g["T_R"])


# ------------------------------------------------------------------------------------------------ 2. the cases
def test_cases_have_the_properties_they_are_named_for():
    inf = float("inf")
    for m in list(GC.SIZES) + list(GC.COMPLETE):
        real, pred, idx, thrs = CASES[f"m{m}"]
        assert pred.shape == (m, m) and idx is None and -inf in thrs
        g = T.ints(real, pred, -inf)
        assert g["d_R"] == [m - 1] * m and g["t_R"] == [(m - 1) * (m - 2) // 2] * m          # complete: t_v = C(m - 1, 2)
        assert g["E_R"] == pairs_of(m) and g["T_R"] == m * (m - 1) * (m - 2) // 6
        assert (g["d_C"], g["t_C"]) == (g["d_G"], g["t_G"])
        s = np.tril(pred, -1)[np.tril_indices(m, -1)]
        assert any((s == np.float32(t)).any() for t in thrs if abs(t) != inf)                  # a threshold that is a stored score
    assert T.ints(None, CASES["m130"][1], -inf)["t_R"] == [129 * 128 // 2] * 130
    for m in GC.SIZES:
        e = T.ints(*CASES[f"m{m}"][:2], inf)
        assert e["E_R"] == e["T_R"] == e["W_R"] == e["E_C"] == 0 and e["E_G"] > 0               # the empty graph
    assert [GC.words(m) for m in sorted(GC.SIZES)] == [1, 1, 2, 2, 2, 3]
    assert [GC.words(m) for m in sorted(GC.SPARSE_SIZES)] == [64, 64, 65, 65] and GC.words(GC.MAX_NIDX) == 1024
    for m in GC.SPARSE_SIZES:
        real, pred, _, _ = CASES[f"sparse_m{m}"]
        g = T.ints(real, pred, 0.5)
        assert pred.shape == (m, m) and g["T_R"] > 20 and g["T_G"] > 20 and 0 < g["T_C"] < g["T_G"] and max(g["d_R"]) < 64
        assert max(np.nonzero(np.asarray(g["d_R"]))[0]) >= m - 64                               # the last word of a row is used
    g = T.ints(*CASES["hub_and_isolated"][:2], 0.5)
    assert g["d_R"][5] == g["d_G"][5] == 398 and g["d_R"][23] == g["d_G"][23] == 0 and g["t_R"][5] == g["E_R"] - 398 > 0
    real, pred, idx, _ = CASES["subset_permuted"]
    assert len(idx) == 100 < len(pred) and sorted(idx.tolist()) != idx.tolist()
    off = np.ones(len(pred), bool); off[idx] = False
    assert not np.isfinite(pred[off]).any() and not np.isfinite(pred[:, off]).any() and not np.isfinite(real[off]).any()
    real, pred, _, thrs = CASES["signed_zeros"]
    neg0, pos0, sub, nsub = thrs
    assert math.copysign(1, neg0) == -1 and neg0 == 0 and pos0 == 0 and sub == 2.0 ** -149 and nsub == -2.0 ** -149
    a, b, c, d = (T.ints(real, pred, t) for t in thrs)
    assert a == b and 0 < c["E_R"] < a["E_R"] < d["E_R"] == pairs_of(40)                        # -0.0 >= +0.0 holds
    # the capacity's closed form is the truth at n = 70, and at the smallest n it is claimed for
    for n in (7, 8, 70, 129):
        assert T.ints(GC.circulant(n), GC.circulant(n), 0.5) == GC.circulant_truth(n), n


WRONG = {"transposed": ("asymmetric", 0.5), "strict": ("m63", 0.5), "node_id": ("subset_permuted", 0.5), "ordered2": ("m3_triangle", 0.5),
         "ordered6": ("m3_triangle", 0.5), "diagonal": ("asymmetric", 0.5), "union": ("m4_missing_triangle", 0.5),
         "pad_bits": ("m65", -float("inf"))}


def test_each_wrong_reading_is_told_apart_by_a_named_case():
    assert sorted(WRONG) == sorted(T.VARIANTS)
    for variant, (name, thr) in WRONG.items():
        real, pred, idx, thrs = CASES[name]
        assert thr in thrs
        right, wrong = T.ints(real, pred, thr, idx), T.ints(real, pred, thr, idx, variant)
        differ = [k for k in T.HEADER + T.COLUMNS if right[k] != wrong[k]]
        assert differ, variant
    # the pad bits of every complete graph from 65 to 127 positions would be counted
    rng = np.random.RandomState(8)
    for m in range(65, 128):
        pred = rng.rand(m, m).astype(np.float32)
        right, wrong = T.ints(None, pred, -float("inf")), T.ints(None, pred, -float("inf"), None, "pad_bits")
        assert right["d_R"] == [m - 1] * m and wrong["d_R"] == [127] * m and wrong["T_R"] > right["T_R"]
    # the union reading turns the missing triangle into a found one
    g = T.ints(*CASES["m4_missing_triangle"][:2], 0.5)
    u = T.ints(*CASES["m4_missing_triangle"][:2], 0.5, None, "union")
    assert (g["T_R"], g["T_G"], g["T_C"]) == (0, 1, 0) and u["T_C"] == 1


# ------------------------------------------------------------------------------------------------ 3. the host arithmetic
def test_engine_stats_are_the_truth_bit_for_bit(pkg):
    from mc_gra_amd import engine as E
    assert E.GRAPH_STRUCTURE_HEADER == T.HEADER and E.GRAPH_STRUCTURE_COLUMNS == T.COLUMNS
    runs = 0
    for name, real, pred, idx, thr in each_run([n for n in sorted(CASES) if not n.startswith("sparse_m4")] + ["sparse_m4097"]):
        for r in (real, None):
            g = T.ints(r, pred, thr, idx)
            got = E.graph_structure_stats({k: g[k] for k in T.HEADER}, {k: g[k] for k in T.COLUMNS})
            assert same_stats(got, T.stats(g)), (name, thr)
            assert (got["true"] is None) == (r is None) and (("f1" in got) == (r is not None))
            runs += 1
    assert runs >= 60
    import torch
    g = T.ints(*CASES["m65"][:2], 0.5)
    as_t = E.graph_structure_stats({k: g[k] for k in T.HEADER}, {k: torch.tensor(g[k]) for k in T.COLUMNS})
    assert same_stats(as_t, T.stats(g))


def test_stats_by_hand_and_degenerate_rules(pkg):
    from mc_gra_amd import engine as E
    nan = float("nan")
    stats = lambda g: E.graph_structure_stats({k: g[k] for k in T.HEADER}, {k: g[k] for k in T.COLUMNS})
    # a triangle with a tail 0-1-2-0, 2-3 against the path 0-1-2-3
    real = lower([1, 0, 1, 0, 0, 1], 4)
    pred = lower([1, 1, 1, 0, 0, 1], 4)
    g = T.ints(real, pred, 0.5)
    assert (g["d_R"], g["t_R"], g["d_G"], g["t_G"]) == ([2, 2, 3, 1], [1, 1, 1, 0], [1, 2, 2, 1], [0, 0, 0, 0])
    assert [g[k] for k in T.HEADER] == [6, 4, 1, 5, 3, 0, 2, 3, 0]
    s = stats(g)
    r, t = s["recovered"], s["true"]
    assert (r["edges"], r["triangles"], r["wedges"], r["max_degree"], r["degree_hist"]) == (4, 1, 5, 3, [0, 1, 2, 1])
    assert r["density"] == 4 / 6 and r["mean_degree"] == 2.0 and r["transitivity"] == 3 / 5
    assert r["avg_clustering"] == math.fsum([1.0, 1.0, float(Fraction(1, 3)), 0.0]) / 4
    assert t["transitivity"] == 0.0 and t["avg_clustering"] == 0.0 and t["degree_hist"] == [0, 2, 2]
    assert s["precision"] == 0.75 and s["recall"] == 1.0 and s["f1"] == float(Fraction(6, 7))
    assert s["triangle_hits"] == 0 and s["triangle_precision"] == 0.0 and math.isnan(s["triangle_recall"])       # T_G = 0
    assert s["degree_l1"] == 0.5 and s["degree_ks"] == 0.25
    # Pearson's r of (2, 2, 3, 1) and (1, 2, 2, 1): c = 4 * 13 - 8 * 6 = 4, v_R = 4 * 18 - 64 = 8, v_G = 4 * 10 - 36 = 4
    assert s["degree_corr"] == math.sqrt(float(Fraction(16, 32))) and abs(s["degree_corr"] - np.corrcoef(g["d_R"], g["d_G"])[0, 1]) < 1e-15
    assert s["clustering_l1"] == math.fsum([1.0, 1.0, float(Fraction(1, 3)), 0.0]) / 4
    # W = 0: transitivity 0.0 as networkx; no edge at all: every ratio NaN
    e = stats(T.ints(real, pred, float("inf")))
    assert e["recovered"]["transitivity"] == 0.0 and e["recovered"]["avg_clustering"] == 0.0 and e["recovered"]["degree_hist"] == [4]
    assert math.isnan(e["precision"]) and e["recall"] == 0.0 and math.isnan(e["triangle_precision"]) and math.isnan(e["triangle_recall"])
    assert math.isnan(e["degree_corr"]) and e["degree_ks"] == 1.0 and e["degree_l1"] == 1.5             # zero variance of d_R; every d_R is 0, no d_G is
    one = stats(T.ints(*CASES["m2_edge"][:2], 0.5))
    assert one["recovered"]["transitivity"] == 0.0 and one["f1"] == 1.0 and math.isnan(one["degree_corr"])
    # a negative correlation keeps its sign; a perfect one is exactly 1
    star_in, star_out = lower([1, 1, 0, 1, 0, 0], 4), lower([0, 0, 1, 0, 1, 1], 4)      # the star at 0 and its complement
    s = stats(T.ints(star_in, star_out, 0.5))
    assert s["degree_corr"] == -1.0 and s["f1"] == 0.0
    assert stats(T.ints(*CASES["g_equals_r"][:2], 0.5))["degree_corr"] == 1.0
    for bad in (dict(g, pairs=7), dict(g, t_R=[0, 0, 0]), dict(g, d_G=[1, 2])):
        with pytest.raises(ValueError):
            stats(bad)
    assert nan != nan


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    s = "mcgra_graph_structure"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 11
    assert callable(E.graph_structure) and hasattr(E.graph_structure, "__wrapped__")                  # the device guard
    assert "mcgra_graph_structure" in E.graph_structure.__doc__ and "No device" in E.graph_structure_stats.__doc__


def test_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to the header."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = -7

    def call(n=8, lds=8, ldl=8, idx=None, n_idx=None, s=p, lab=p, thr=0.5, header=True, out=p):
        h = (ctypes.c_int64 * 9)(*([mark] * 9))
        rc = L.mcgra_graph_structure(None, n, s, lds, lab, ldl, idx, n if n_idx is None else n_idx, thr, h if header else None, out)
        assert list(h) == [mark] * 9
        return rc

    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(lds=7), dict(ldl=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(s=None), dict(out=None), dict(header=False), dict(thr=float("nan")),
               dict(lab=None, thr=float("nan"))):
        assert call(**kw) == -1 and b"graph_structure:" in L.mcgra_last_error(), kw
    assert call(thr=float("nan")) == -1 and b"NaN" in L.mcgra_last_error()
    big = GC.MAX_NIDX + 1
    assert call(n=big, lds=big, ldl=big) == -3 and b"65535" in L.mcgra_last_error()
    assert call(n=10 ** 6, lds=10 ** 6, ldl=10 ** 6, idx=p, n_idx=big) == -3
    assert call(n=big, lds=big - 1, ldl=big) == -1                            # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(call(n=big, lds=big, ldl=big))


def test_engine_entry_refuses_wrong_shapes_and_host_tensors(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for pred, real in ((wide, sq), (torch.zeros(5), sq), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.graph_structure.__wrapped__(pred, 0.5, None, real)
    with pytest.raises(ValueError, match="device tensors"):
        E.graph_structure(sq, 0.5)                                       # a host tensor: refused before anything is called


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_structure_flags_are_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in ("structure", "save_structure"))
    assert "structure" not in str(plain)
    a = p.parse_args(["--structure", "split", "--save_structure", "s.npz"])
    assert a.structure == "split" and a.save_structure == "s.npz"
    assert p.parse_args(["--structure", "edges"]).structure == "edges" and p.parse_args(["--structure", "0.9"]).structure == "0.9"
    assert p.parse_args(["--structure=-0.25"]).structure == "-0.25"
    assert (R.structure_source("split"), R.structure_source("edges"), R.structure_source("0.9"), R.structure_source("-1e-3")) == \
        ("split", "edges", 0.9, -0.001)
    for bad in ("", "Split", "kmeans", "nan", "inf", "-inf", "0.5x"):
        assert R.structure_source(bad) is None
        with pytest.raises(SystemExit):
            p.parse_args([f"--structure={bad}"])
        assert "`split`, `edges` or a finite threshold" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--save_structure", "s.npz"])
    assert "--save_structure needs --structure" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--structure", "split", "--save_structure", ""])
    assert ".npz" in capsys.readouterr().err
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--structure", "split", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err and "--structure" in err
    for flag in ("--structure", "--save_structure"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(structure="split", mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --structure"):
        M._run(argparse.Namespace(save_structure="s.npz", mode="evaluate"), 0, 1)
    calls = []
    R.check_structure_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_structure_args(argparse.Namespace(structure="0.5", save_structure="s.npz", mode="evaluate"), calls.append)
    assert calls == []
