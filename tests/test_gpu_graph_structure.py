"""Degree, triangle and clustering statistics of the recovered graph on the device (mcgra_graph_structure,
engine.graph_structure, main.py --structure / --save_structure) against tests/graph_structure_truth.py: every integer of the
header and of the six columns compared for equality, every double of `stats` bit for bit -- at the smallest selections where
the kernels change behaviour (one word, two words, the diagonal tile's mask, the pad bits, W on both sides of one 64-lane
stride), thresholds that are a stored score, signed zeros, +-inf, layouts (n > m with a permuted idx, junk outside the
selection, an asymmetric matrix), node kinds (a hub, an isolated node), labels given and NULL, and the capacity.  Run with -m gpu.

tests/test_graph_structure_cases_cpu.py checks, without a GPU, that these inputs (tests/graph_structure_cases.py) have the
properties the cases are there for and that they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import graph_structure_cases as GC
from tests import graph_structure_truth as T
from tests import helpers as H
from tests import two_means_truth as TM

pytestmark = pytest.mark.gpu

CASES = GC.cases()


@functools.lru_cache(maxsize=None)
def truth(name, thr, labelled=True):
    """The truth of a case at one threshold, computed once and shared (read-only)."""
    real, pred, idx, _ = CASES[name]
    return T.ints(real if labelled else None, pred, thr, idx)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda:0")                    # a copy: the cases are read-only


def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


def _check(got, ints, thr, what):
    """Every integer and every double of one engine.graph_structure result."""
    want = T.stats(ints)
    print(f"{what}: header {[got[k] for k in T.HEADER]} transitivity={got['stats']['recovered']['transitivity']} "
          f"clustering={got['stats']['recovered']['avg_clustering']} degree_corr={got['stats'].get('degree_corr')}")
    assert got["nodes"] == len(ints["d_R"]) and _same(got["threshold"], float(thr))
    for k in T.HEADER:
        assert isinstance(got[k], int) and got[k] == ints[k], (what, k, got[k], ints[k])
    for k in T.COLUMNS:
        assert str(got[k].dtype) == "torch.int64" and got[k].is_cuda and got[k].tolist() == ints[k], (what, k)
    s = got["stats"]
    assert sorted(s) == sorted(want), what
    for k, v in want.items():
        if isinstance(v, dict):
            assert sorted(s[k]) == sorted(v) and all(_same(s[k][q], v[q]) for q in v), (what, k, s[k], v)
            assert all(isinstance(s[k][q], float) for q in T.GRAPH_DOUBLES)
        else:
            assert _same(s[k], v), (what, k, s[k], v)
    if want["true"] is not None:
        assert all(isinstance(s[k], float) for k in T.VERSUS_DOUBLES)


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_graph_structure_against_the_truth(pkg, name):
    """Every integer of the entry and every double the engine forms from them, at each threshold, with labels and without."""
    from mc_gra_amd import engine as E
    real, pred, idx, thrs = CASES[name]
    r, p, ix = _dev(real), _dev(pred), None if idx is None else _dev(idx)
    for thr in thrs:
        _check(E.graph_structure(p, thr, ix, r), truth(name, thr), thr, (name, thr))
        _check(E.graph_structure(p, thr, ix), truth(name, thr, False), thr, (name, thr, "bare"))


def test_closed_forms_of_the_extremes(pkg):
    """-inf is the complete graph, t_v = C(m - 1, 2) (at m = 130, C(129, 2)); +inf the empty one; one triangle at m = 3."""
    from mc_gra_amd import engine as E
    real, pred, _, _ = CASES["m130"]
    g = E.graph_structure(_dev(pred), -float("inf"), None, _dev(real))
    assert g["d_R"].tolist() == [129] * 130 and g["t_R"].tolist() == [129 * 128 // 2] * 130
    assert (g["E_R"], g["T_R"], g["W_R"]) == (130 * 129 // 2, 130 * 129 * 128 // 6, 130 * (129 * 128 // 2))
    assert g["t_C"].tolist() == g["t_G"].tolist() and g["stats"]["recovered"]["transitivity"] == 1.0 and g["stats"]["recall"] == 1.0
    e = E.graph_structure(_dev(pred), float("inf"), None, _dev(real))
    assert (e["E_R"], e["T_R"], e["W_R"], e["E_C"], e["T_C"]) == (0, 0, 0, 0, 0) and not e["d_R"].any() and e["E_G"] > 0
    real, pred, _, _ = CASES["m3_triangle"]
    t = E.graph_structure(_dev(pred), 0.5, None, _dev(real))
    assert [t[k] for k in T.HEADER] == [3, 3, 1, 3, 3, 1, 3, 3, 1] and t["t_R"].tolist() == [1, 1, 1]
    real, pred, _, _ = CASES["signed_zeros"]
    a, b = (E.graph_structure(_dev(pred), thr) for thr in (-0.0, 0.0))
    assert a["E_R"] == b["E_R"] > 0 and a["d_R"].tolist() == b["d_R"].tolist()                    # -0.0 >= +0.0 holds


@pytest.mark.parametrize("name", ["m65", "subset_permuted", "asymmetric", "hub_and_isolated", "sparse_m4097", "signed_zeros"])
def test_edge_counts_are_those_of_threshold_pairs(pkg, name):
    """E_R and E_C are mcgra_threshold_pairs' counts on the same input, and its edge list is R."""
    from mc_gra_amd import engine as E
    real, pred, idx, thrs = CASES[name]
    r, p, ix = _dev(real), _dev(pred), None if idx is None else _dev(idx)
    for thr in thrs:
        g = E.graph_structure(p, thr, ix, r)
        pairs, _, hits = E.threshold_pairs(p, thr, ix, r)
        assert (g["E_R"], g["E_C"]) == (len(pairs), int(hits.sum())), (name, thr)
        want = TM.threshold_pairs(real, pred, thr, idx)
        assert g["E_R"] == len(want[0]) and g["E_C"] == int(want[2].sum())
        nodes = np.arange(len(pred)) if idx is None else np.asarray(idx)
        deg = np.bincount(np.searchsorted(np.sort(nodes), pairs.cpu().numpy().reshape(-1)), minlength=len(nodes))
        assert deg[np.argsort(np.argsort(nodes))].tolist() == g["d_R"].tolist()


@pytest.mark.parametrize("name", ["m129", "subset_permuted", "hub_and_isolated", "sparse_m4160"])
def test_two_calls_give_identical_bits(pkg, name):
    from mc_gra_amd import engine as E
    real, pred, idx, thrs = CASES[name]
    r, p, ix = _dev(real), _dev(pred), None if idx is None else _dev(idx)
    one, two = E.graph_structure(p, thrs[0], ix, r), E.graph_structure(p, thrs[0], ix, r)
    assert all(one[k] == two[k] for k in T.HEADER) and all(one[k].tolist() == two[k].tolist() for k in T.COLUMNS)
    for k, v in one["stats"].items():
        assert all(_same(v[q], two["stats"][k][q]) for q in v) if isinstance(v, dict) else _same(v, two["stats"][k]), k


def test_other_dtypes_devices_and_padded_rows(pkg):
    """float64 / bool operands and host node ids are converted as the neighbours convert them; a padded leading dimension is kept."""
    import torch
    from mc_gra_amd import engine as E
    real, pred, idx, _ = CASES["subset_permuted"]
    got = E.graph_structure(_dev(pred).double(), 0.5, idx.tolist(), _dev(np.nan_to_num(real, nan=0, posinf=0)).bool())
    want = truth("subset_permuted", 0.5)
    assert all(got[k] == want[k] for k in T.HEADER) and all(got[k].tolist() == want[k] for k in T.COLUMNS)
    real, pred, _, _ = CASES["m129"]
    buf = torch.full((129, 160), float("nan"), device="cuda:0")             # the padding is never read
    buf[:, :129] = _dev(pred)
    p = buf[:, :129]
    assert p.stride(0) == 160
    _check(E.graph_structure(p, 0.5, None, _dev(real)), truth("m129", 0.5), 0.5, "ld 160")


def test_graph_structure_capacity(pkg):
    """n_idx = 65 535, every node selected, built on the device in row blocks: the circulant graph of offsets +-1, +-2 as scores
    and labels at once, threshold 0.5.  Closed form (held to the numpy truth at small n by the CPU tests): d = 4, t = 3, T = m.
    1024 words per row, 524 800 tiles, matrix offsets up to 2^32."""
    import torch
    from mc_gra_amd import engine as E
    n = GC.MAX_NIDX
    need = 4 * n * n + 3 * 8 * n * GC.words(n) + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the capacity case needs {need / 2 ** 30:.1f} GiB of device memory (a 17 GB matrix and 1.6 GB of bit "
                    f"matrices); {free / 2 ** 30:.1f} GiB are free")
    both = torch.empty(n, n, device="cuda:0", dtype=torch.float32)
    cols = torch.arange(n, device="cuda:0", dtype=torch.int32)[None, :]
    for r0 in range(0, n, 4096):
        rows = torch.arange(r0, min(n, r0 + 4096), device="cuda:0", dtype=torch.int32)[:, None]
        d = (rows - cols) % n
        both[r0:r0 + 4096] = ((d == 1) | (d == 2) | (d == n - 1) | (d == n - 2)).to(torch.float32)
    del d
    got = E.graph_structure(both, 0.5, None, both)
    assert n * n > 2 ** 31 and got["pairs"] == n * (n - 1) // 2
    _check(got, GC.circulant_truth(n), 0.5, "capacity")
    assert (got["E_R"], got["T_R"], got["W_R"], got["T_C"]) == (2 * n, n, 6 * n, n) and got["stats"]["recovered"]["transitivity"] == 0.5


# ------------------------------------------------------------------------------------------------ 2. the refusals
def test_device_refusals_leave_the_outputs_untouched(pkg):
    """A NaN or infinite score, a label of 0.5, a repeated id, an id out of range: MCGRA_EINVAL, the cause named, and not one
    word of the header or of out written; the same entries outside the selected triangle are not looked at."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n = 70
    real, pa = GC.graph(rng, n, 0.2), rng.rand(n, n).astype(np.float32)
    mark = -7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(real, pa, idx=None, thr=0.5):
        r, a = None if real is None else _dev(real), _dev(pa)
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        rows = n if idx is None else len(idx)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        hd = (ctypes.c_int64 * 9)(*([mark] * 9))
        out = torch.full((rows, 6), mark, device="cuda:0", dtype=torch.int64)
        rc = L.mcgra_graph_structure(stream, n, p(a), n, p(r), n, p(ix), rows, thr, hd, p(out))
        return rc, L.mcgra_last_error().decode(), list(hd), bool((out == mark).all()), bool((out == mark).any())

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    rc, _, hd, untouched, any_left = run(real, pa)
    assert rc == 0 and hd[0] == GC.pairs_of(n) and mark not in hd and not any_left
    for value in (np.nan, np.inf, -np.inf):
        for thr in (0.5, float("inf"), -float("inf")):                       # whatever the threshold decides about the entry
            rc, e, hd, untouched, _ = run(real, bad(pa, value), None, thr)
            assert rc == -1 and "NaN or infinite" in e and "graph_structure" in e and hd == [mark] * 9 and untouched
        rc, e, hd, untouched, _ = run(None, bad(pa, value))
        assert rc == -1 and "NaN or infinite" in e and hd == [mark] * 9 and untouched
    for value in (0.5, np.nan, 2.0):
        rc, e, hd, untouched, _ = run(bad(real, value), pa)
        assert rc == -1 and "label" in e and hd == [mark] * 9 and untouched
    # the same invalid entries above the diagonal, on it, and in unselected rows and columns are not looked at
    rc, _, _, _, any_left = run(bad(real, 0.5, (7, 40)), bad(pa, np.nan, (7, 40)))
    assert rc == 0 and not any_left
    rc, _, _, _, any_left = run(bad(real, 0.5, (9, 9)), bad(pa, np.inf, (9, 9)))
    assert rc == 0 and not any_left
    rc, _, hd, _, any_left = run(bad(real, 0.5), bad(pa, np.nan), [3, 41, 7, 12, 60])
    assert rc == 0 and not any_left and hd[0] == 10
    rc, e, hd, untouched, _ = run(real, bad(pa, np.nan), [3, 7, 40, 12, 60])          # node 40 at position 2, node 7 at 1: [40][7] is read
    assert rc == -1 and "NaN or infinite" in e and hd == [mark] * 9 and untouched
    rc, _, _, _, any_left = run(real, bad(pa, np.nan), [3, 40, 7, 12, 60])            # node 7 at position 2, node 40 at 1: [7][40] is read
    assert rc == 0 and not any_left
    rc, _, hd, untouched, _ = run(real, bad(pa, np.nan, (7, 40)), [3, 40, 7, 12, 60])
    assert rc == -1 and hd == [mark] * 9 and untouched
    rc, e, hd, untouched, _ = run(real, pa, [3, 9, 4, 9, 12])
    assert rc == -1 and "twice" in e and hd == [mark] * 9 and untouched
    for ids in ([3, 9, n], [3, -1, 5]):
        rc, e, hd, untouched, _ = run(real, pa, ids)
        assert rc == -1 and "outside" in e and hd == [mark] * 9 and untouched
    rc, e, hd, untouched, _ = run(real, pa, None, float("nan"))
    assert rc == -1 and "NaN" in e and hd == [mark] * 9 and untouched


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = GC.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.graph_structure(_dev(nan), 0.5, None, _dev(real))
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.graph_structure(_dev(pa), float("nan"))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.graph_structure(_dev(pa), 0.5, [1, 2, 1])
    with pytest.raises(pkg._lib.McgraError):
        E.graph_structure(_dev(pa), 0.5, [4])                                 # fewer than two nodes


# ------------------------------------------------------------------------------------------------------ 3. main.py
def test_main_evaluate_structure_and_save_structure(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --structure split adds the
    structure_* dicts, each the truth on the matrices that were scored at the threshold of the set's own 2-means split;
    --save_structure writes the six columns of each set; --structure edges cuts at the P-th best score; a run without the flags
    returns and logs what it did before the flags existed."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt"])
    assert not any(hasattr(plain_args, k) for k in ("structure", "save_structure"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.graph_structure

    def record(pred, threshold, idx=None, real=None):
        v = orig(pred, threshold, idx, real)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx), threshold, v))
        return v

    monkeypatch.setattr(M.engine, "graph_structure", record)
    path = str(tmp_path / "structure.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "split.txt", "--structure", "split", "--save_structure", path]))
    out = capsys.readouterr().out
    new = [f"structure_{s}" for s in ("attack", "train", "all")]
    assert sorted(res) == sorted(list(plain) + new) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    saved = np.load(path)
    assert sorted(saved.files) == sorted(f"{k}_{s}" for k in ("nodes", "threshold") + T.COLUMNS for s in ("attack", "train", "all"))
    for (real, pred, idx, thr, v), name in zip(seen, ("attack", "train", "all")):
        assert res[f"structure_{name}"] is v
        split = TM.split(real, pred, idx)
        assert not split["degenerate"] and thr == float(split["threshold"]) and v["E_R"] == split["edges"] and v["E_C"] == split["hits"]
        ints = T.ints(real, pred, thr, idx)
        _check(v, ints, thr, name)
        again = orig(_dev(pred), thr, idx, _dev(real))                   # the engine's own call on the matrices that were scored
        assert np.array_equal(saved[f"nodes_{name}"], np.arange(1190) if idx is None else idx)
        for k in T.COLUMNS:
            assert saved[f"{k}_{name}"].dtype == np.int64 and saved[f"{k}_{name}"].tolist() == again[k].tolist() == ints[k], (k, name)
        assert saved[f"threshold_{name}"].dtype == np.float32 and float(saved[f"threshold_{name}"]) == thr
    d = res["structure_all"]
    q = d["stats"]
    assert d["nodes"] == 1190 and d["pairs"] == GC.pairs_of(1190) and d["E_G"] > 0
    assert (f"current auc={res['auc_all']}\ncurrent transitivity={q['recovered']['transitivity']} (true {q['true']['transitivity']}) "
            f"triangles={d['T_C']}/{d['T_G']} degree_corr={q['degree_corr']} degree_ks={q['degree_ks']}\n" in out)
    assert "transitivity" not in out_plain
    log = open(tmp_path / "results" / "split.txt").read().split("\n")
    for i, (name, key) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        d = res[f"structure_{key}"]
        q = d["stats"]
        assert log[2 + i] == (f"In {name}: structure at {d['threshold']}: edges={d['E_R']} (true {d['E_G']}, shared {d['E_C']}) "
                              f"triangles={d['T_R']} (true {d['T_G']}, shared {d['T_C']}) "
                              f"transitivity={q['recovered']['transitivity']} (true {q['true']['transitivity']}) "
                              f"clustering={q['recovered']['avg_clustering']} (true {q['true']['avg_clustering']}) "
                              f"degree_corr={q['degree_corr']} degree_ks={q['degree_ks']} degree_l1={q['degree_l1']}")
    assert log[5].startswith("current density:") and "structure='split'" in log[0] and "save_structure=" in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "structure" not in old and old.count("\n") == 3 and old.split("\n")[1:] == log[1:2] + log[5:]
    # --structure edges: at least as many edges as the truth (ties may add some), the real count reported; a float: itself
    seen.clear()
    edges = M.run(M.build_parser().parse_args(argv + ["--log_name", "edges.txt", "--structure", "edges"]))
    capsys.readouterr()
    for (real, pred, idx, thr, v), name in zip(seen, ("attack", "train", "all")):
        assert v["E_R"] >= v["E_G"] > 0 and all(v[k] == T.ints(real, pred, thr, idx)[k] for k in T.HEADER)
        s = np.sort(TM.K.packed(real, pred, idx)[0])[::-1]
        assert thr == float(s[v["E_G"] - 1]) and v["E_R"] == int((s >= np.float32(thr)).sum())
    real, pred, idx, _, _ = seen[0]
    assert R.structure_threshold(R.structure_source("0.25"), _dev(real), _dev(pred), idx) == 0.25
    assert R.structure_threshold("edges", _dev(np.zeros_like(real)), _dev(pred), idx) == float("inf")      # P = 0: the empty graph
    assert R.structure_threshold("split", None, _dev(np.full_like(pred, 0.5)), idx) == float("inf")        # a degenerate split
