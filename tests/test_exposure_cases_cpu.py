"""Without a GPU: that the truth of tests/test_gpu_exposure.py (tests/exposure_truth.py) is right -- against literal loops,
against networkx, against DeLong's, the graph-structure and the threshold truths and against its closed form; that the inputs of
the GPU tests (tests/exposure_cases.py) have the properties they are named for and tell every wrong reading of the definition
from the right one; the host arithmetic of engine.edge_exposure_stats; the refusals that need no device; the command line and
the report."""
import argparse
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import delong_truth as DT
from tests import exposure_cases as XC
from tests import exposure_truth as T
from tests import graph_structure_truth as GT
from tests import two_means_truth as TM
from tests.hop_truth import adjacency

CASES = XC.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcgra.h")
SMALL = [k for k, v in CASES.items() if (len(v[0]) if v[2] is None else len(v[2])) <= 70]


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


_memo = {}


def ints(name, thr="first", wrong=None):
    real, pred, idx, _, thresholds = CASES[name]
    thr = thresholds[0] if thr == "first" else thr
    key = (name, thr, wrong)
    if key not in _memo:
        _memo[key] = T.ints(real, pred, idx, thr, wrong)
    return _memo[key]


# -------------------------------------------------------------------------------------------------- 1. the truth
@pytest.mark.parametrize("name", SMALL)
def test_truth_against_the_literal_loops(name):
    real, pred, idx, _, thresholds = CASES[name]
    for thr in thresholds:
        g = T.ints(real, pred, idx, thr)
        header, table, rows = T.loop_ints(real, pred, idx, thr)
        assert g["header"] == header and g["table"] == table, (name, thr)
        assert [tuple(r) for r in g["pairs_list"].tolist()] == [r[:2] for r in rows]
        assert g["scores"].tolist() == [float(r[2]) for r in rows] and g["placement"].tolist() == [r[3] for r in rows]
        assert g["common"].tolist() == [r[4] for r in rows] and [tuple(r) for r in g["deg"].tolist()] == [r[5:] for r in rows]
        assert g["pairs_list"].dtype == g["placement"].dtype == np.int64 and g["common"].dtype == g["deg"].dtype == np.int32


@pytest.mark.parametrize("name", ["m65", "sub129", "two_cliques_bridge", "through_unselected", "dense_n200", "star_n70"])
def test_common_neighbours_and_degrees_are_those_of_networkx(name):
    import networkx as nx
    real, pred, idx, _, _ = CASES[name]
    ix = np.arange(len(real)) if idx is None else idx
    a, b = np.tril_indices(len(ix), -1)
    on = real[ix[a], ix[b]] == 1
    G = nx.Graph()
    G.add_nodes_from(int(v) for v in ix)
    G.add_edges_from((int(u), int(v)) for u, v in zip(ix[a[on]], ix[b[on]]))             # the induced subgraph, by node id
    g = ints(name)
    assert len(g["pairs_list"]) == G.number_of_edges() > 0
    for (u, v), c, (du, dv) in zip(g["pairs_list"].tolist(), g["common"].tolist(), g["deg"].tolist()):
        assert G.has_edge(u, v) and c == len(list(nx.common_neighbors(G, u, v))) and (du, dv) == (G.degree(u), G.degree(v))


@pytest.mark.parametrize("name", sorted(CASES))
def test_truth_against_delongs_the_structure_and_the_threshold_truths(name):
    real, pred, idx, _, thresholds = CASES[name]
    dl = DT.ints(real, pred, idx)
    gs = GT.ints(real, pred, 0.0, idx)
    m = len(gs["d_G"])
    ix = np.arange(len(real)) if idx is None else idx
    for thr in thresholds:
        g = ints(name, thr)
        hd, tb = g["header"], g["table"]
        assert hd[:4] == [dl["pairs"], dl["positives"], dl["negatives"], dl["T"]]
        assert [sum(c[q] for row in tb for c in row) for q in range(3)] == [hd[1], hd[3], hd[4]]
        assert all(c == [0, 0, 0] for row in tb for c in row[:1])                            # dc >= 1 for every edge
        st = T.stats(hd, tb)
        if hd[1] and hd[2]:
            assert st["auc_pooled"] == float(Fraction(dl["T"], 2 * dl["positives"] * dl["negatives"]))
        # every edge lies in c_e triangles: sum c_e = 3 T_G, and over the edges at v it is 2 t_G(v)
        assert int(g["common"].sum()) == 3 * gs["T_G"] and len(g["common"]) == gs["E_G"]
        at = np.zeros(m, np.int64)
        pos = {int(v): k for k, v in enumerate(ix)}
        for (u, v), c, (du, dv) in zip(g["pairs_list"].tolist(), g["common"].tolist(), g["deg"].tolist()):
            at[pos[u]] += c
            at[pos[v]] += c
            assert (du, dv) == (gs["d_G"][pos[u]], gs["d_G"][pos[v]])
        assert at.tolist() == [2 * t for t in gs["t_G"]]
        if thr is not None:
            _, _, hits = TM.threshold_pairs(real, pred, thr, idx)
            assert (hd[4], hd[5]) == (int(hits.sum()), int((~hits).sum()))
        else:
            assert (hd[4], hd[5]) == (0, 0)


def test_closed_form_of_the_capacity_case_is_the_truth_at_small_n():
    for n in (9, 10, 17, 64, 65, 130):
        both = XC.circulant(n)
        g = T.ints(both, both, None, 0.5)
        header, table = T.circulant_ints(n)
        assert g["header"] == header and g["table"] == table, n
        assert set(g["placement"].tolist()) == {2 * header[2]} and set(g["deg"].reshape(-1).tolist()) == {4}
        assert sorted(set(g["common"].tolist())) == [1, 2]


# ------------------------------------------------------------------------------------------------- 2. the cases
def test_cases_have_the_properties_they_are_named_for():
    size = lambda v: len(v[0]) if v[2] is None else len(v[2])
    for m in XC.SIZES:
        assert size(CASES[f"m{m}"]) == size(CASES[f"sub{m}"]) == m and CASES[f"sub{m}"][3] > 0
        assert CASES[f"sub{m}"][2] is not None and (np.diff(CASES[f"sub{m}"][2]) < 0).any()
    assert size(CASES["sparse_n1025"]) == size(CASES["sparse_sub1025"]) == XC.ROW_BLOCKS + 1
    P = lambda name: ints(name)["header"][1]
    assert P("dense_n200") > max(XC.EDGE_WAVES, XC.STAGE) and 0 < P("sparse_n1025") < XC.EDGE_WAVES
    assert ints("empty_n66")["header"][1] == 0 and ints("complete_n66")["header"][2] == 0
    assert ints("complete_n66")["header"][3] == 0 and ints("complete_n66")["table"][15][7][0] == 66 * 65 // 2     # c = 64, d = 65
    assert ints("one_edge")["header"][1] == 1 and ints("one_edge")["table"][0][1][0] == 1
    g = ints("star_n70")
    assert g["table"][0][1][0] == 69 == g["header"][1] and set(g["deg"].min(1).tolist()) == {1} and set(g["deg"].max(1).tolist()) == {69}
    for name, c in (("clique17", 15), ("clique18", 16)):
        g = ints(name)
        assert set(g["common"].tolist()) == {c} and g["table"][15][5][0] == g["header"][1] == (c + 2) * (c + 1) // 2
    g = ints("two_cliques_bridge")
    bridge = [k for k, r in enumerate(g["pairs_list"].tolist()) if sorted(r) == [19, 50]]
    assert len(bridge) == 1 and g["common"][bridge[0]] == 0 and sorted(g["deg"][bridge[0]].tolist()) == [18, 20]
    assert g["table"][0][5][0] == 1
    g = ints("path_n11")
    assert set(g["common"].tolist()) == {0} and g["table"][0][1][0] == 2 and g["table"][0][2][0] == 8
    g = ints("all_equal")
    assert set(g["placement"].tolist()) == {g["header"][2]}
    assert len(np.unique(DT.candidates(*CASES["two_valued"][:3])[1])) == 2
    s = DT.candidates(*CASES["signed_zeros"][:3])[1]
    assert np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any() and (np.abs(s[s != 0]) < 1e-40).all()
    assert (DT.candidates(*CASES["negative"][:3])[1] < 0).all()
    # every class of the table's two axes that small graphs can reach is reached somewhere
    reached = {(e, c) for name in CASES for e in range(16) for c in range(16) if ints(name)["table"][e][c][0]}
    assert {e for e, _ in reached} == set(range(16)) and {c for _, c in reached} >= set(range(1, 8))
    # masked: nothing but the selected strict lower triangle is valid
    for name, (real, pred, idx, _, _) in CASES.items():
        if name != "through_unselected":
            assert np.isnan(real).sum() == np.isnan(pred).sum() == real.size - size(CASES[name]) * (size(CASES[name]) - 1) // 2


WRONG_SHOWS = {
    "whole_graph": "through_unselected",      # node 1, not selected, is a common neighbour of two selected edges
    "max_degree": "star_n70",
    "cap16": "clique18",
    "bit_length_off": "path_n11",
    "ties2": "m63",
    "ties0": "m63",
    "all_candidates": "sub65",
    "strict_cut": "m63",                      # the cut is a stored score
    "row_major": "m65",
}


@pytest.mark.parametrize("wrong", T.WRONG)
def test_cases_tell_the_wrong_readings_apart(wrong):
    assert sorted(WRONG_SHOWS) == sorted(T.WRONG)
    name = WRONG_SHOWS[wrong]
    right, other = ints(name), ints(name, "first", wrong)
    if wrong == "row_major":
        assert right["table"] == other["table"] and right["header"] == other["header"]
        assert not np.array_equal(right["pairs_list"], other["pairs_list"])
        assert sorted(map(tuple, right["pairs_list"].tolist())) == sorted(map(tuple, other["pairs_list"].tolist()))
        pos = {int(v): k for k, v in enumerate(np.arange(len(CASES[name][0])))}
        packed = [pos[u] * (pos[u] - 1) // 2 + pos[v] for u, v in right["pairs_list"].tolist()]
        assert packed == sorted(packed)
    else:
        assert right["table"] != other["table"][:16] or right["header"] != other["header"], wrong
    differ = [k for k in CASES if ints(k)["table"] != ints(k, "first", wrong)["table"][:16] or ints(k)["header"] != ints(k, "first", wrong)["header"]
              or not np.array_equal(ints(k)["pairs_list"], ints(k, "first", wrong)["pairs_list"])]
    assert name in differ


# ---------------------------------------------------------------------------------------- 3. the host arithmetic
def _table(cells):
    tb = [[[0, 0, 0] for _ in range(16)] for _ in range(16)]
    for (e, c), v in cells.items():
        tb[e][c] = list(v)
    return tb


def test_edge_exposure_stats_by_hand_and_its_nan_rules(pkg):
    from mc_gra_amd import engine as E
    isnan = math.isnan
    assert E.EXPOSURE_COMMON_NAMES == T.COMMON_NAMES and E.EXPOSURE_DEGREE_NAMES == T.DEGREE_NAMES and E.EXPOSURE_HEADER == T.HEADER
    assert T.DEGREE_NAMES[1:4] == ("1", "2-3", "4-7") and T.COMMON_NAMES[14:] == ("14", "15+")
    # 6 edges, 10 non-edges: cells (0, 1) = 2 edges, (0, 2) = 1 edge, (3, 2) = 3 edges
    tb = _table({(0, 1): (2, 12, 0), (0, 2): (1, 15, 1), (3, 2): (3, 57, 3)})
    hd = [16, 6, 10, 84, 4, 2]
    s = E.edge_exposure_stats(hd, tb)
    assert (s["pairs"], s["positives"], s["negatives"], s["T"], s["above_pos"], s["above_neg"]) == tuple(hd)
    assert s["auc_pooled"] == 84 / 120 == float(Fraction(84, 120)) and s["recall"] == 4 / 6 and s["precision"] == 4 / 6
    e, d = s["by_embeddedness"], s["by_degree"]
    assert e["names"] == T.COMMON_NAMES and e["count"][:4] == (3, 0, 0, 3) and e["T"][:4] == (27, 0, 0, 57) and e["above"][:4] == (1, 0, 0, 3)
    assert e["auc"][0] == 27 / 60 and isnan(e["auc"][1]) and e["auc"][3] == 57 / 60 and e["recall"][0] == 1 / 3 and isnan(e["recall"][2])
    assert e["share"][0] == 0.5 and e["share"][1] == 0.0 and e["lift"][3] == float(Fraction(57, 60) - Fraction(84, 120)) and isnan(e["lift"][1])
    assert d["names"] == T.DEGREE_NAMES and d["count"][:3] == (0, 2, 4) and d["T"][:3] == (0, 12, 72) and d["above"][:3] == (0, 0, 4)
    assert d["auc"][1] == 12 / 40 and d["auc"][2] == 72 / 80 and d["recall"][1] == 0.0 and d["share"][2] == 4 / 6
    assert [(c["ec"], c["dc"], c["common"], c["degree"], c["count"]) for c in s["cells"]] == [(0, 1, "0", "1", 2), (0, 2, "0", "2-3", 1),
                                                                                           (3, 2, "3", "2-3", 3)]
    assert s["cells"][2]["auc"] == 57 / 60 and s["cells"][0]["recall"] == 0.0 and s["cells"][1]["share"] == 1 / 6
    # the pooled AUC is the share-weighted mean of the class AUCs
    assert abs(sum(a * w for a, w in zip(e["auc"], e["share"]) if w) - s["auc_pooled"]) < 1e-15
    assert T.same(s, T.stats(hd, tb))
    p0 = E.edge_exposure_stats([6, 0, 6, 0, 0, 2], _table({}))                              # P = 0
    assert isnan(p0["auc_pooled"]) and isnan(p0["recall"]) and p0["precision"] == 0.0 and p0["cells"] == []
    assert all(isnan(v) for v in p0["by_degree"]["auc"] + p0["by_degree"]["share"] + p0["by_degree"]["lift"])
    n0 = E.edge_exposure_stats([3, 3, 0, 0, 0, 0], _table({(1, 2): (3, 0, 0)}))             # N = 0
    assert isnan(n0["auc_pooled"]) and isnan(n0["precision"]) and n0["recall"] == 0.0
    assert isnan(n0["by_embeddedness"]["auc"][1]) and isnan(n0["by_embeddedness"]["lift"][1]) and n0["by_embeddedness"]["share"][1] == 1.0
    for name, (_, _, _, _, thresholds) in CASES.items():
        for thr in thresholds[:2]:
            g = ints(name, thr)
            assert T.same(E.edge_exposure_stats(g["header"], g["table"]), T.stats(g["header"], g["table"])), (name, thr)
    for bad_hd, bad_tb in ((hd[:5], tb), ([16, 6, 10, 85, 4, 2], tb), ([16, 6, 10, 84, 3, 2], tb), ([17, 6, 10, 84, 4, 2], tb),
                           (hd, tb[:15]), (hd, _table({(0, 1): (2, 12, 0), (0, 2): (1, 15, 1), (3, 2): (3, 57, 2)})),
                           ([16, 6, 10, 84, 4, -2], tb), (hd, [row[:15] for row in tb])):
        with pytest.raises(ValueError, match="edge_exposure_stats"):
            E.edge_exposure_stats(bad_hd, bad_tb)


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    s = "mcgra_edge_exposure"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 17
    assert "#define MCGRA_EXPOSURE_CLASSES 16" in open(HEADER).read() and E.EXPOSURE_CLASSES == T.CLASSES == 16
    assert callable(E.edge_exposure) and hasattr(E.edge_exposure, "__wrapped__")                      # the device guard
    assert "mcgra_edge_exposure" in E.edge_exposure.__doc__ and "No device" in E.edge_exposure_stats.__doc__


def test_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to header or table."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = -7

    def call(n=8, ldl=8, lds=8, idx=None, n_idx=None, lab=p, s=p, thr=0.5, cap=0, pairs=None, other=None, header=True, table=True):
        hd, tb = (ctypes.c_int64 * 6)(*([mark] * 6)), (ctypes.c_int64 * 768)(*([mark] * 768))
        rc = L.mcgra_edge_exposure(None, n, lab, ldl, s, lds, idx, n if n_idx is None else n_idx, thr, cap, pairs, other, other,
                                   other, other, hd if header else None, tb if table else None)
        assert list(hd) == [mark] * 6 and list(tb) == [mark] * 768
        return rc

    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(lds=7), dict(ldl=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(s=None), dict(lab=None), dict(header=False), dict(table=False), dict(thr=float("nan")),
               dict(cap=-1), dict(cap=5), dict(cap=5, other=p), dict(cap=0, pairs=p), dict(cap=0, other=p)):
        assert call(**kw) == -1 and b"edge_exposure:" in L.mcgra_last_error(), kw
    assert call(thr=float("nan")) == -1 and b"NaN" in L.mcgra_last_error()
    assert call(cap=5) == -1 and b"cap = 5 with pairs NULL" in L.mcgra_last_error()
    assert call(cap=-2) == -1 and b"cap = -2" in L.mcgra_last_error()
    big = XC.MAX_NIDX + 1
    assert call(n=big, lds=big, ldl=big) == -3 and b"65535" in L.mcgra_last_error()
    assert call(n=10 ** 6, lds=10 ** 6, ldl=10 ** 6, idx=p, n_idx=big) == -3
    assert call(n=big, lds=big - 1, ldl=big) == -1                            # a bad argument is named before the capacity
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        pkg._lib.check(call(n=big, lds=big, ldl=big))


def test_engine_entry_refuses_wrong_shapes_and_host_tensors(pkg, monkeypatch):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for real, pred in ((wide, sq), (torch.zeros(5), sq), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.edge_exposure.__wrapped__(real, pred)
    with pytest.raises(ValueError, match="device tensors"):
        E.edge_exposure(sq, sq)                                          # a host tensor: refused before anything is called
    # the refusals of the C entry reach the caller as exceptions that name the cause (no stream is needed to be refused)
    monkeypatch.setattr(E, "_stream", lambda: None)
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.edge_exposure.__wrapped__(sq, sq, None, float("nan"))
    with pytest.raises(pkg._lib.McgraError, match="at least 2"):
        E.edge_exposure.__wrapped__(sq, sq, [3], 0.5, edges=True)
    with pytest.raises(pkg._lib.McgraNotSupported, match="65535"):
        E.edge_exposure.__wrapped__(sq, sq, list(range(XC.MAX_NIDX + 1)))      # the count is refused before an id is read


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_exposure_flags_are_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not any(hasattr(plain, k) for k in ("exposure", "exposure_cut", "save_exposure")) and "exposure" not in str(plain)
    assert "exposure" not in str(R.shown_parameters(plain))
    a = p.parse_args(["--exposure", "--exposure_cut", "split", "--save_exposure", "x.npz"])
    assert (a.exposure, a.exposure_cut, a.save_exposure) == (True, "split", "x.npz")
    assert all(f" {k}=" in " " + str(R.shown_parameters(a)).replace("(", " ") for k in ("exposure", "exposure_cut", "save_exposure"))
    assert p.parse_args(["--exposure", "--exposure_cut=-0.25"]).exposure_cut == "-0.25"
    only = str(R.shown_parameters(p.parse_args(["--exposure"])))
    assert "exposure=True" in only and "exposure_cut" not in only and "save_exposure" not in only
    for bad in ("", "Split", "nan", "inf"):
        with pytest.raises(SystemExit):
            p.parse_args(["--exposure", f"--exposure_cut={bad}"])
        assert "`split`, `edges` or a finite threshold" in capsys.readouterr().err
    for flag, value in (("--exposure_cut", "edges"), ("--save_exposure", "x.npz")):
        with pytest.raises(SystemExit):
            p.parse_args([flag, value])
        assert f"{flag} needs --exposure" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["--exposure", "--save_exposure", ""])
    assert ".npz" in capsys.readouterr().err
    for mode in ("notrain_test", "prepare", "link_stealing"):
        with pytest.raises(SystemExit):
            p.parse_args(["--exposure", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err and "--exposure" in err
    for flag in ("--exposure", "--exposure_cut", "--save_exposure"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(exposure=True, mode="link_stealing"), 0, 1)
    with pytest.raises(SystemExit, match="needs --exposure"):
        M._run(argparse.Namespace(save_exposure="x.npz", mode="evaluate"), 0, 1)
    calls = []
    R.check_exposure_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_exposure_args(argparse.Namespace(exposure=True, exposure_cut="0.5", save_exposure="x.npz", mode="evaluate"), calls.append)
    assert calls == []


def test_the_later_reports_follow_the_table_without_touching_it(pkg):
    from mc_gra_amd import reports as R
    later = [f for r in R.LATER_REPORTS for f in r.flags]
    before = [f for r in R.EVALUATE_REPORTS for f in r.flags]
    assert len(later) == len(set(later)) and not set(later) & set(before)
    rep = [r for r in R.LATER_REPORTS if "exposure" in r.flags]
    assert len(rep) == 1 and rep[0].flags == ("exposure", "exposure_cut", "save_exposure")
    assert rep[0].wanted(argparse.Namespace(exposure=True)) and not rep[0].wanted(argparse.Namespace())
    assert not rep[0].wanted(argparse.Namespace(exposure_cut="edges", save_exposure="x.npz"))
    assert not any(r.wanted(argparse.Namespace(exposure=True)) for r in R.EVALUATE_REPORTS)
    assert "LATER_REPORTS" in R.__doc__


# ----------------------------------------------------------------------------------- the report, from the truth
def _fake_engine(monkeypatch, E):
    """engine.edge_exposure, engine.topk_metrics and engine.two_means_split as the truths, on host tensors."""
    import torch
    from tests import topk_truth as TK
    seen = []

    def edge_exposure(real, pred, idx=None, threshold=None, edges=False):
        g = T.ints(real.numpy(), pred.numpy(), idx, threshold)
        seen.append((idx, threshold, edges))
        res = dict(zip(T.HEADER, g["header"]))
        res.update({"threshold": None if threshold is None else float(threshold), "table": T.as_tuples(g["table"]), "ints": g["header"],
                    "stats": T.stats(g["header"], g["table"])})
        if edges:
            res.update({q: torch.tensor(g[q]) for q in T.COLUMNS})
        return res

    monkeypatch.setattr(E, "edge_exposure", edge_exposure)
    monkeypatch.setattr(E, "topk_metrics", lambda real, pred, k=None, idx=None: TK.top_k(real.numpy(), pred.numpy(), k, idx))
    return seen


def test_the_report_text_and_file_from_the_truth(pkg, monkeypatch, tmp_path):
    import torch
    from mc_gra_amd import engine as E
    from mc_gra_amd import reports as R
    from tests import topk_truth as TK
    seen = _fake_engine(monkeypatch, E)
    rng = np.random.RandomState(4)
    n = 40
    real = XC.graph(rng, n, 0.2)
    pred = (0.5 * real + XC.scores(rng, real, "random")).astype(np.float32)
    sets = {"attack": rng.permutation(n)[:30], "train": np.arange(5, 17), "all": None}
    path = str(tmp_path / "x.npz")
    args = argparse.Namespace(exposure=True, save_exposure=path, mode="evaluate")
    ctx = R.RunContext(real=torch.tensor(real), inference_adj=torch.tensor(pred), sets=sets, n=n, rank=0, other=None, versus=None, args=args)
    report = R.LATER_REPORTS[0]
    res = report.compute(ctx)
    assert sorted(res) == ["exposure_all", "exposure_attack", "exposure_train"]
    for name, ix in sets.items():
        d = res[f"exposure_{name}"]
        thr = TK.top_k(real, pred, 0, ix)["threshold"]                        # --exposure_cut defaults to `edges`
        g = T.ints(real, pred, ix, thr)
        assert d["threshold"] == float(thr) and d["ints"] == g["header"] and d["table"] == T.as_tuples(g["table"])
        assert T.same(d["stats"], T.stats(g["header"], g["table"]))
    d = res["exposure_all"]
    q = d["stats"]
    e, dg = q["by_embeddedness"], q["by_degree"]
    by = lambda mg: " ".join(f"{k}:{a}" for k, c, a in zip(mg["names"], mg["count"], mg["auc"]) if c)
    line = f"current exposure by common neighbours {by(e)} (pooled {q['auc_pooled']}) | by min degree {by(dg)}"
    assert report.console(res, ctx) == [line] and line.startswith("current exposure by common neighbours 0:") and " 1:" in line
    log = report.log(res, ctx)
    assert len(log) == 3 and [l.split(":")[0] for l in log] == ["In attack graph", "In train graph", "In Whole Graph"]
    assert log[2].startswith(f"In Whole Graph: exposure at {d['threshold']}: edges={d['positives']} recall={q['recall']} "
                             f"precision={q['precision']} by common neighbours 0: count={e['count'][0]} AUC={e['auc'][0]} recall={e['recall'][0]}")
    assert f"(pooled {q['auc_pooled']}) | by min degree " in log[2]
    calls = len(seen)
    report.save(res, ctx)
    assert len(seen) == calls + 1 and seen[-1] == (None, d["threshold"], True)
    saved = np.load(path)
    assert sorted(saved.files) == sorted([f"{k}_{s}" for k in ("nodes", "table", "threshold") for s in sets] +
                                         ["pairs", "scores", "placement", "common", "deg"])
    g = T.ints(real, pred, None, d["threshold"])
    for k, col in (("pairs", "pairs_list"), ("scores", "scores"), ("placement", "placement"), ("common", "common"), ("deg", "deg")):
        assert saved[k].dtype == g[col].dtype and np.array_equal(saved[k], g[col]), k
    for name, ix in sets.items():
        assert saved[f"table_{name}"].dtype == np.int64 and saved[f"table_{name}"].shape == (16, 16, 3)
        assert saved[f"table_{name}"].tolist() == [[list(c) for c in row] for row in res[f"exposure_{name}"]["table"]]
        assert saved[f"threshold_{name}"].dtype == np.float32 and float(saved[f"threshold_{name}"]) == res[f"exposure_{name}"]["threshold"]
    assert np.array_equal(saved["nodes_attack"], sets["attack"]) and np.array_equal(saved["nodes_all"], np.arange(n))
    # --exposure_cut: a float is itself; without --save_exposure nothing is written
    seen.clear()
    cut = ctx._replace(args=argparse.Namespace(exposure=True, exposure_cut="0.25", mode="evaluate"))
    report.compute(cut)
    assert [s[1:] for s in seen] == [(0.25, False)] * 3
    assert report.save(res, cut) is None and len(seen) == 3
