"""The AUC within node classes on the device (mcgra_class_auc, engine.class_auc, main.py --by_class / --by_class_cut /
--save_by_class) against tests/class_truth.py: every integer and every double compared for equality, twice with the same bits
-- at the smallest selections where the kernels change behaviour (a row shorter than, as long as and longer than a wave and a
block, more rows than the grid of the row passes, more edges than one sort tile and than the staged samples), tables (one, same,
own, blocks for 1, 2, 3, 7 and 16 classes: 1 to 136 strata), class layouts (a class of one node, strata without edges and
without non-edges, the complete and the empty graph, segments of one edge), scores (four levels, negative, signed zeros,
subnormals), thresholds -inf, +inf, a stored score, -0.0 against +0.0 and None, layouts (n > m with a permuted idx, padded
rows and classes out of range on the unselected nodes), the identities on the device, the refusals, and the capacity.  Run
with -m gpu.

tests/test_class_cases_cpu.py checks, without a GPU, that these inputs (tests/class_cases.py) have the properties the cases
are there for and that they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import class_cases as CC
from tests import class_truth as T
from tests import helpers as H
from tests import two_means_truth as TM
from tests.test_gpu_hops import _circulant_on_device, _dev

pytestmark = pytest.mark.gpu

CASES = CC.cases()


@functools.lru_cache(maxsize=None)
def prep(name):
    """What the truth of a case shares over its runs, computed once (read-only)."""
    real, pred, classes, idx, _, _, _ = CASES[name]
    return T.prepare(real, pred, classes, idx)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_class_auc_against_the_truth(pkg, name):
    """Every integer of the entry and every double the engine forms from them, at each (C, table, threshold) of the case, on
    two calls."""
    from mc_gra_amd import engine as E
    real, pred, classes, idx, pad, runs, brute = CASES[name]
    r, p, ix = _dev(real, pad), _dev(pred, pad), None if idx is None else _dev(idx)
    for C, how, thr in runs:
        table, names = T.strata(C, how)
        want = T.stats(T.rows_of(prep(name), table, len(names), thr, brute), names, thr)
        mine = E.class_strata(C, how)
        assert mine[0].tolist() == table and mine[1] == names
        one, two = E.class_auc(r, p, classes, ix, mine, thr), E.class_auc(r, p, classes, ix, mine, thr)
        print(f"{name} C={C} {how} threshold={thr}: {one['ints']} within={one['auc_within']} adjusted={one['auc_adjusted']}")
        assert T.same(one, want) and T.same(two, one), (name, C, how, thr)


@pytest.mark.parametrize("name", ["m257_c7", "sub65_c3", "dense_n200_c3", "sparse_sub1054"])
def test_identities_on_the_device(pkg, name):
    """`one` is {m, P, T} of mcgra_auc_delong and the counts of mcgra_threshold_pairs; stratum c of `own` is mcgra_auc_delong on
    the selected nodes of class c alone; a how string takes C from the selected nodes."""
    from mc_gra_amd import engine as E
    real, pred, classes, idx, pad, runs, _ = CASES[name]
    C = runs[0][0]
    r, p, ix = _dev(real, pad), _dev(pred, pad), None if idx is None else _dev(idx)
    dl = E.auc_delong(r, p, ix)
    one = E.class_auc(r, p, classes, ix, "one", 0.5)
    assert one["ints"] == [(dl["pairs"], dl["positives"], dl["ints"]["T"], one["above"][0], one["hits"][0])]
    assert one["auc"][0] == dl["auc"] == one["auc_within"] == one["auc_adjusted"] or dl["positives"] * dl["negatives"] == 0
    _, _, hits = E.threshold_pairs(p, 0.5, ix, r)
    assert (one["above"][0], one["hits"][0]) == (int(hits.numel()), int(hits.sum()))
    sel = np.arange(len(real)) if idx is None else idx
    own = E.class_auc(r, p, classes, ix, "own")
    assert len(own["names"]) == int(classes[sel].max()) + 2 == C + 1 and "above" not in own
    for c in range(C):
        nodes = sel[classes[sel] == c]
        if len(nodes) >= 2:
            d = E.auc_delong(r, p, _dev(nodes))
            assert (own["count"][c], own["positives"][c], own["T"][c]) == (d["pairs"], d["positives"], d["ints"]["T"]), c
        else:
            assert own["ints"][c] == (0, 0, 0, 0, 0)
    assert sum(own["count"]) == dl["pairs"] and sum(own["positives"]) == dl["positives"]


def test_any_permutation_of_idx_and_any_renaming_of_the_classes(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(3)
    n, C = 150, 5
    g = CC.graph(rng, n, 0.05)
    s = CC.scores(rng, g, "levels4")                                     # symmetric: a permutation keeps every candidate's score
    cl = CC.spread(rng, n, C)
    sel = rng.permutation(n)[:101]
    table, names = T.strata(C, "blocks")
    want = T.ints(g, s, cl, sel, table, len(names), 0.5)
    tab = np.asarray(table, np.uint8)
    for _ in range(3):
        got = E.class_auc(_dev(g), _dev(s), cl, _dev(rng.permutation(sel)), (tab, names), 0.5)
        assert got["ints"] == [tuple(c) for c in want]
        perm = rng.permutation(C)                                         # class c is renamed perm[c]; the table goes with it
        renamed = np.empty_like(tab)
        renamed[np.ix_(perm, perm)] = tab
        got = E.class_auc(_dev(g), _dev(s), perm[cl], _dev(sel), (renamed, names), 0.5)
        assert got["ints"] == [tuple(c) for c in want]


def test_other_dtypes_host_node_ids_and_class_containers(pkg):
    """float64 / bool operands and a list of node ids are converted as the neighbours convert them; the classes may be a list,
    an int32 array or a device tensor."""
    import torch
    from mc_gra_amd import engine as E
    real, pred, classes, idx, _, _, _ = CASES["sub65_c3"]
    table, names = T.strata(3, "blocks")
    want = T.stats(T.rows_of(prep("sub65_c3"), table, 6, THR), names, THR)
    r, p = _dev(np.nan_to_num(real, nan=0)).bool(), _dev(np.nan_to_num(pred, nan=0)).double()
    for cl in (classes.tolist(), classes.astype(np.int32), torch.as_tensor(classes.copy(), device="cuda:0")):
        assert T.same(E.class_auc(r, p, cl, idx.tolist(), "blocks", THR), want)


THR = CC.THR_OF[CC.KINDS[(list(CC.SIZES).index(65) + 1) % 4]]


def test_class_auc_capacity(pkg):
    """n_idx = 65 535, every node selected, built on the device in row blocks: the circulant graph of offsets +-1, +-2 as scores
    and labels at once, the classes v mod 16, all 136 blocks, threshold 0.5.  Matrix offsets up to 2^32, 64 rows per block of the
    stream, T_g up to 2^41; the expected counts in O(n) from the class sizes and the 2 n edges."""
    import torch
    from mc_gra_amd import engine as E
    n = CC.MAX_NIDX
    need = 4 * n * n + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the capacity case needs {need / 2 ** 30:.1f} GiB of device memory (a 17 GB matrix); "
                    f"{free / 2 ** 30:.1f} GiB are free")
    assert n * n > 2 ** 31
    both = _circulant_on_device(n)
    cl = np.arange(n) % 16
    one, two = E.class_auc(both, both, cl, None, "blocks", 0.5), E.class_auc(both, both, cl, None, "blocks", 0.5)
    want = T.stats(T.circulant_rows(n, 16), T.strata(16, "blocks")[1], 0.5)
    print(f"capacity: {one['ints'][:3]} ...")
    assert T.same(one, want) and T.same(two, one)
    assert sum(one["positives"]) == 2 * n and one["auc_within"] == 1.0 and one["auc_adjusted"] == 1.0


# ------------------------------------------------------------------------------------------------ 2. the refusals
def test_device_refusals_leave_out_untouched(pkg):
    """A NaN or infinite score, a label of 0.5, a repeated id, an id out of range, a selected node of a class the table does not
    hold: MCGRA_EINVAL, the cause named, and not one word of out written; the same entries outside the selected triangle, and
    such classes on unselected nodes, are not looked at."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n, C = 70, 3
    real, pa = CC.graph(rng, n, 0.05), rng.rand(n, n).astype(np.float32)
    cl = CC.spread(rng, n, C)
    table = np.asarray(T.strata(C, "blocks")[0], np.uint8)
    mark, words = -7, 5 * 6 + 10
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(real, pa, idx=None, thr=0.5, cl=cl):
        r, a = _dev(real), _dev(pa)
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        c = _dev(np.asarray(cl, np.int32))
        rows = n if idx is None else len(idx)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        out = (ctypes.c_int64 * words)(*([mark] * words))
        rc = L.mcgra_class_auc(stream, n, p(r), n, p(a), n, p(ix), rows, p(c), C, table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                               6, thr, out)
        return rc, L.mcgra_last_error().decode(), list(out)

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    untouched = [mark] * words
    rc, _, out = run(real, pa)
    assert rc == 0 and mark not in out[:30] and out[30:] == [mark] * 10 and sum(out[0:30:5]) == n * (n - 1) // 2
    for value in (np.nan, np.inf, -np.inf):
        for thr in (0.5, float("inf"), -float("inf")):                       # whatever the threshold decides about the entry
            rc, e, out = run(real, bad(pa, value), None, thr)
            assert rc == -1 and "NaN or infinite" in e and "class_auc" in e and out == untouched
    for value in (0.5, np.nan, 2.0):
        rc, e, out = run(bad(real, value), pa)
        assert rc == -1 and "label" in e and out == untouched
    # the same invalid entries above the diagonal, on it, and in unselected rows and columns are not looked at
    assert run(bad(real, 0.5, (7, 40)), bad(pa, np.nan, (7, 40)))[0] == 0
    assert run(bad(real, 0.5, (9, 9)), bad(pa, np.inf, (9, 9)))[0] == 0
    rc, _, out = run(bad(real, 0.5), bad(pa, np.nan), [3, 41, 7, 12, 60])
    assert rc == 0 and sum(out[0:30:5]) == 10
    rc, e, out = run(real, bad(pa, np.nan), [3, 7, 40, 12, 60])               # node 40 at position 2, node 7 at 1: [40][7] is read
    assert rc == -1 and "NaN or infinite" in e and out == untouched
    assert run(real, bad(pa, np.nan), [3, 40, 7, 12, 60])[0] == 0             # node 7 at position 2, node 40 at 1: [7][40] is read
    rc, e, out = run(real, pa, [3, 9, 4, 9, 12])
    assert rc == -1 and "twice" in e and out == untouched
    for ids in ([3, 9, n], [3, -1, 5]):
        rc, e, out = run(real, pa, ids)
        assert rc == -1 and "outside" in e and out == untouched
    for value in (C, -1, 255, 256, -2 ** 31):
        wrong = cl.copy()
        wrong[12] = value
        rc, e, out = run(real, pa, None, 0.5, wrong)
        assert rc == -1 and "class" in e and "outside [0, 3)" in e and out == untouched, value
        rc, e, out = run(real, pa, [3, 41, 12, 7, 60], 0.5, wrong)           # by node id: node 12 is selected
        assert rc == -1 and "outside [0, 3)" in e and out == untouched
        assert run(real, pa, [3, 41, 7, 13, 60], 0.5, wrong)[0] == 0          # node 12 is not selected, position 12 does not exist
    rc, e, out = run(real, pa, None, float("nan"))
    assert rc == -1 and "NaN" in e and out == untouched


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = CC.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    cl = CC.spread(rng, n, 3)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.class_auc(_dev(real), _dev(nan), cl)
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.class_auc(_dev(real), _dev(pa), cl, None, "same", float("nan"))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.class_auc(_dev(real), _dev(pa), cl, [1, 2, 1])
    with pytest.raises(pkg._lib.McgraError):
        E.class_auc(_dev(real), _dev(pa), cl, [4])                            # fewer than two nodes
    with pytest.raises(pkg._lib.McgraError, match=r"outside \[0, 2\)"):
        E.class_auc(_dev(real), _dev(pa), cl, None, E.class_strata(2, "blocks"))      # class 2 is not in the table
    lop = (np.asarray([[0, 1], [0, 0]], np.uint8), ("a", "b"))
    with pytest.raises(pkg._lib.McgraError, match="symmetric"):
        E.class_auc(_dev(real), _dev(pa), cl % 2, None, lop)
    with pytest.raises(ValueError, match="at most 16"):
        E.class_auc(_dev(real), _dev(pa), cl + 14)
    with pytest.raises(ValueError, match="class -1"):
        E.class_auc(_dev(real), _dev(pa), cl - 1)
    with pytest.raises(ValueError, match="shape"):
        E.class_auc(_dev(real), _dev(pa), cl[:-1])
    with pytest.raises(ValueError, match="integers"):
        E.class_auc(_dev(real), _dev(pa), cl.astype(np.float32))
    big = cl.copy()
    big[[0, 19]] = (99, -4)                                               # unselected: never looked at
    assert E.class_auc(_dev(real), _dev(pa), big, list(range(1, 19)))["pairs"] == 18 * 17 // 2


# ------------------------------------------------------------------------------------------------------ 3. main.py
def test_main_evaluate_by_class_and_save_by_class(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --by_class labels adds the
    by_class_* dicts, each the truth on the matrices that were scored with the run's labels as classes, its pairs counted at
    the score of the set's P-th best pair; --save_by_class writes the blocks of each set; --by_class degree takes the classes
    from the true graph's degrees; a run without the flags returns and logs what it did before the flags existed."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt"])
    assert not any(hasattr(plain_args, k) for k in ("by_class", "by_class_cut", "save_by_class"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.class_auc

    def record(real, pred, classes, idx=None, strata="blocks", threshold=None):
        v = orig(real, pred, classes, idx, strata, threshold)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), np.asarray(classes), None if idx is None else np.asarray(idx),
                     strata, threshold, v))
        return v

    monkeypatch.setattr(M.engine, "class_auc", record)
    path = str(tmp_path / "classes.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "cls.txt", "--by_class", "labels", "--save_by_class", path, "--ci"]))
    out = capsys.readouterr().out
    new = [f"{k}_{s}" for k in ("by_class", "ci") for s in ("attack", "train", "all")]
    assert sorted(res) == sorted(list(plain) + new) and len(seen) == 6
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    saved = np.load(path)
    keys = ("class_i", "class_j", "count", "positives", "T", "above", "hits", "auc", "same_ints", "threshold")
    assert sorted(saved.files) == sorted([f"{k}_{s}" for k in keys for s in ("attack", "train", "all")] + ["classes"])
    classes = saved["classes"]
    C = int(classes.max()) + 1
    assert classes.dtype == np.int64 and classes.shape == (1190,) and 2 <= C <= 16
    for k, name in enumerate(("attack", "train", "all")):
        d = res[f"by_class_{name}"]
        (real, pred, cl, idx, st_same, thr, v_same), (_, _, _, _, st_blocks, thr2, v_blocks) = seen[2 * k], seen[2 * k + 1]
        assert d["same"] is v_same and d["blocks"] is v_blocks and thr == thr2 == d["threshold"] and np.array_equal(cl, classes)
        assert (d["source"], d["classes"]) == ("labels", C) and st_same[1] == ("same", "different") and len(st_blocks[1]) == C * (C + 1) // 2
        s = np.sort(TM.K.packed(real, pred, idx)[0])[::-1]
        P = sum(v_same["positives"])
        assert P > 0 and thr == float(s[P - 1])                                          # --by_class_cut defaults to `edges`
        pr = T.prepare(real, pred, cl, idx)
        for how, v in (("same", v_same), ("blocks", v_blocks)):
            table, names = T.strata(C, how)
            assert T.same(v, T.stats(T.rows_of(pr, table, len(names), thr, False), names, thr)), (name, how)
        assert d["auc_pooled"] == res[f"ci_{name}"]["auc"]                               # auc_pairs of --ci
        h = d["homophily"]
        assert h == {"true": v_same["positives"][0] / P, "recovered": v_same["above"][0] / sum(v_same["above"]),
                     "pairs": v_same["count"][0] / v_same["pairs"]}
        assert saved[f"class_i_{name}"].tolist() == [i for i in range(C) for _ in range(i, C)]
        assert saved[f"class_j_{name}"].tolist() == [j for i in range(C) for j in range(i, C)]
        for key in ("count", "positives", "T", "above", "hits"):
            assert saved[f"{key}_{name}"].dtype == np.int64 and saved[f"{key}_{name}"].tolist() == list(v_blocks[key]), (key, name)
        assert saved[f"auc_{name}"].dtype == np.float64 and np.array_equal(saved[f"auc_{name}"], np.asarray(v_blocks["auc"]), equal_nan=True)
        assert saved[f"same_ints_{name}"].dtype == np.int64 and saved[f"same_ints_{name}"].tolist() == [list(r) for r in v_same["ints"]]
        assert saved[f"threshold_{name}"].dtype == np.float32 and float(saved[f"threshold_{name}"]) == thr
    line = f"current auc_by_class {R._by_class_text(res['by_class_all'])}\n"
    assert line in out and out.index("current auc_pairs=") < out.index(line) and "auc_by_class" not in out_plain
    log = open(tmp_path / "results" / "cls.txt").read().split("\n")
    for i, (title, key) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        d = res[f"by_class_{key}"]
        assert log[5 + i] == f"In {title}: by class (labels, {C} classes) at {d['threshold']}: {R._by_class_text(d)}"
    assert log[8].startswith("current density:") and "by_class='labels'" in log[0] and "save_by_class=" in log[0] and "by_class_cut" not in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "by_class" not in old and old.count("\n") == 3 and old.split("\n")[1:] == log[1:2] + log[8:]
    # --by_class degree, --by_class_cut: a float is itself
    seen.clear()
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "deg.txt", "--by_class", "degree", "--by_class_cut", "0.25"]))
    capsys.readouterr()
    real = seen[0][0]
    degree = (np.nan_to_num(real) != 0).sum(1)
    assert np.array_equal(seen[0][2], [min(15, int(d).bit_length()) for d in degree]) and [s[5] for s in seen] == [0.25] * 6
    assert res["by_class_all"]["source"] == "degree" and res["by_class_all"]["classes"] == int(seen[0][2].max()) + 1
