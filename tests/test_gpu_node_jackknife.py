"""The node jackknife of the AUC on the device (mcgra_auc_node_jackknife, engine.auc_node_jackknife / auc_node_jackknife_paired,
main.py --ci_nodes / --save_influence) against tests/node_jackknife_truth.py: every integer of the header and of the five
columns compared for equality, every double of the engine's dicts and every influence bit for bit -- over the smallest
selections, ties, signed zeros, subnormals and negative scores, layouts (padding, NaN junk outside the selected lower triangle,
asymmetric matrices, permuted subsets), node kinds (a hub that holds every positive, an isolated node, a long list), selections
and class sizes on both sides of every constant the kernels' grids, chunks and sorts use, the capacity, and the paired
relations B = A and B = -A.  Run with -m gpu.

tests/test_node_jackknife_cases_cpu.py checks, without a GPU, that these inputs (tests/node_jackknife_cases.py) have the
properties the cases are there for and that they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import delong_truth as DT
from tests import helpers as H
from tests import node_jackknife_cases as NC
from tests import node_jackknife_truth as T

pytestmark = pytest.mark.gpu

CASES = NC.cases()


@functools.lru_cache(maxsize=None)
def truth(name, which="a"):
    """The truth of a case's scoring, computed once and shared (read-only)."""
    real, pa, pb, idx, _ = CASES[name]
    return T.ints(real, pa if which == "a" else pb, idx)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x, pad=0):
    import torch
    t = torch.as_tensor(np.array(x), device="cuda:0")                    # a copy: the cases are read-only
    if pad:
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda:0")      # the padding is never read
        buf[:, :t.shape[1]] = t
        t = buf[:, :t.shape[1]]
    return t


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _same_list(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _check_single(got, ints, level, what):
    want = T.stats(ints, level)
    print(f"{what}: header {[got['ints'][k] for k in ('pairs', 'positives', 'negatives', 'T')]} auc={got['auc']} "
          f"var={got['var']} want var={want['var']} ci=[{got['ci_low']}, {got['ci_high']}] undefined={got['undefined_nodes']}")
    for k in ("pairs", "positives", "negatives", "T") + T.COLUMNS:
        assert got["ints"][k] == ints[k], (what, k, got["ints"][k], ints[k])
    assert got["ints"] == ints
    assert (got["pairs"], got["nodes"], got["positives"], got["negatives"], got["level"]) == \
        (ints["pairs"], len(ints["P_v"]), ints["positives"], ints["negatives"], level)
    assert got["undefined_nodes"] == want["undefined_nodes"]
    for key in T.RATES:
        assert isinstance(got[key], float) and _same(got[key], want[key]), (what, key, got[key], want[key])
    assert str(got["influence"].dtype) == "torch.float64" and _same_list(got["influence"].tolist(), want["influence"]), what


def _check_paired(got, ia, ib, level, what):
    want = T.paired_stats(ia, ib, level)
    print(f"{what}: delta={got['delta']} se={got['se_delta']} z={got['z']} p={got['p_value']}")
    _check_single(got["a"], ia, level, (what, "a"))
    _check_single(got["b"], ib, level, (what, "b"))
    assert got["undefined_nodes"] == want["undefined_nodes"] and got["level"] == level
    for key in T.PAIRED_RATES:
        assert isinstance(got[key], float) and _same(got[key], want[key]), (what, key, got[key], want[key])
    assert _same_list(got["influence"].tolist(), want["influence"]), what


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_node_jackknife_against_the_truth(pkg, name):
    """Every integer of the entry and every double the engine forms from them, for both scorings and the pair."""
    from mc_gra_amd import engine as E
    real, pa, pb, idx, pad = CASES[name]
    r, a, b, ix = _dev(real, pad), _dev(pa, pad), _dev(pb, pad), None if idx is None else _dev(idx)
    if pad:
        assert a.stride(0) == b.stride(0) == r.stride(0) == pa.shape[1] + pad
    _check_single(E.auc_node_jackknife(r, a, ix), truth(name, "a"), 0.95, name)
    _check_single(E.auc_node_jackknife(r, b, ix, level=0.9), truth(name, "b"), 0.9, name)
    _check_paired(E.auc_node_jackknife_paired(r, a, b, ix), truth(name, "a"), truth(name, "b"), 0.95, name)


@pytest.mark.parametrize("name", ["five_levels", "junk_outside_selection", "tiling_n2050", "class_P4097_levels", "star",
                                  "n64_no_positive", "n2_one_positive"])
def test_the_header_is_the_one_of_auc_delong(pkg, name):
    from mc_gra_amd import engine as E
    real, pa, _, idx, pad = CASES[name]
    r, a, ix = _dev(real, pad), _dev(pa, pad), None if idx is None else _dev(idx)
    nj, dl = E.auc_node_jackknife(r, a, ix)["ints"], E.auc_delong(r, a, ix)["ints"]
    assert all(nj[k] == dl[k] for k in ("pairs", "positives", "negatives", "T")), (nj, dl)
    assert dl == DT.ints(real, pa, idx)


def test_reordered_selection_permutes_the_nodes(pkg):
    """The same node set in another order names the same pairs of a symmetric matrix: the same header, and every node keeps its
    five integers and its influence, found at its new position; var is a sum over the nodes in another order, an fsum."""
    from mc_gra_amd import engine as E
    real, pa, _, a, _ = CASES["subset_permuted"]
    b = CASES["subset_reordered"][3]
    r, d = _dev(real), _dev(pa)
    ga, gb = E.auc_node_jackknife(r, d, a), E.auc_node_jackknife(r, d, _dev(b))
    gl = E.auc_node_jackknife(r, d, b.tolist())
    assert gl["ints"] == gb["ints"] == truth("subset_reordered") and ga["ints"] == truth("subset_permuted")
    where = {int(v): i for i, v in enumerate(a)}
    at = [where[int(v)] for v in b]
    for k in T.COLUMNS:
        assert gb["ints"][k] == [ga["ints"][k][i] for i in at], k
    assert all(ga["ints"][k] == gb["ints"][k] for k in ("pairs", "positives", "negatives", "T"))
    assert gb["influence"].tolist() == [ga["influence"].tolist()[i] for i in at]
    assert ga["auc"] == gb["auc"] and ga["var"] == gb["var"] and ga["auc_jackknife"] == gb["auc_jackknife"]


@pytest.mark.parametrize("name", ["tiling_n2050", "class_P4097_levels", "subset_permuted", "hub_degree_299"])
def test_two_calls_give_identical_bits(pkg, name):
    from mc_gra_amd import engine as E
    real, pa, pb, idx, pad = CASES[name]
    r, a, ix = _dev(real, pad), _dev(pa, pad), None if idx is None else _dev(idx)
    one, two = E.auc_node_jackknife(r, a, ix), E.auc_node_jackknife(r, a, ix)
    assert one["ints"] == two["ints"] and all(_same(one[k], two[k]) for k in T.RATES)
    assert _same_list(one["influence"].tolist(), two["influence"].tolist())


def test_paired_relations(pkg):
    """B = A: every d_v is exactly 0, so delta, se and z are 0 and p is 1; B = -A: T_b = 2 P N - T_a, the AUCs add to 1."""
    from mc_gra_amd import engine as E
    real, a, _, _, _ = CASES["b_equals_a"]
    r, da = _dev(real), _dev(a)
    same = E.auc_node_jackknife_paired(r, da, da)                           # one buffer as both matrices
    assert same["a"]["ints"] == same["b"]["ints"] == truth("b_equals_a") and same["a"]["se"] > 0
    assert same["delta"] == 0.0 and same["se_delta"] == 0.0 and same["z"] == 0.0 and same["p_value"] == 1.0
    assert same["ci_low"] == 0.0 and same["ci_high"] == 0.0 and not same["influence"].any()
    neg = E.auc_node_jackknife_paired(r, da, _dev(CASES["b_minus_a"][2]))
    ga, gb = neg["a"]["ints"], neg["b"]["ints"]
    P, N = ga["positives"], ga["negatives"]
    assert gb["T"] == 2 * P * N - ga["T"] and neg["b"]["auc"] == float(1 - Fraction(ga["T"], 2 * P * N))
    for pv, nv, aa, ba, ca, ab, bb, cb in zip(ga["P_v"], ga["N_v"], ga["A_v"], ga["B_v"], ga["C_v"], gb["A_v"], gb["B_v"], gb["C_v"]):
        assert (ab, bb, cb) == (2 * pv * N - aa, 2 * nv * P - ba, 2 * pv * nv - ca)
    assert neg["delta"] == float(Fraction(ga["T"] - gb["T"], 2 * P * N)) and neg["se_delta"] > 0


def test_other_dtypes_and_devices_of_the_operands(pkg):
    """float64 / bool operands and host node ids are converted as auc_delong converts them."""
    import torch
    from mc_gra_amd import engine as E
    real, pa, _, _, _ = CASES["asymmetric"]
    got = E.auc_node_jackknife(_dev(real).bool(), _dev(pa).double(), torch.arange(len(real)))
    assert got["ints"] == truth("asymmetric")


def test_node_jackknife_capacity(pkg):
    """n_idx = 65 535, every node selected, built on the device in row blocks: the path graph of node_jackknife_cases.path_scores,
    whose integers have a closed form (held to the numpy truth at n = 50 by the CPU tests).  2.1e9 pairs, matrix offsets up to 2^32: the index arithmetic past 2^31."""
    import torch
    from mc_gra_amd import engine as E
    n = NC.MAX_NIDX
    real = torch.empty(n, n, device="cuda:0", dtype=torch.float32)
    pred = torch.empty(n, n, device="cuda:0", dtype=torch.float32)
    cols = torch.arange(n, device="cuda:0", dtype=torch.int32)[None, :]
    for r0 in range(0, n, 4096):
        rows = torch.arange(r0, min(n, r0 + 4096), device="cuda:0", dtype=torch.int32)[:, None]
        d = rows - cols
        real[r0:r0 + 4096] = (d == 1).to(torch.float32)
        pred[r0:r0 + 4096] = torch.where(d == 1, torch.where(rows % 3 == 0, 1.0, 2.0), torch.where(d % 2 == 0, 1.0, 0.0))
    del d
    got = E.auc_node_jackknife(real, pred)
    want = NC.path_truth(n)
    assert got["ints"]["pairs"] == n * (n - 1) // 2 and n * n > 2 ** 31
    _check_single(got, want, 0.95, "capacity")
    assert got["undefined_nodes"] == 0 and got["se"] > 0


# ------------------------------------------------------------------------------------------------ 2. the refusals
def test_device_refusals_leave_the_outputs_untouched(pkg):
    """A NaN or infinite score, a label of 0.5, a repeated id, an id out of range: MCGRA_EINVAL, the cause named, and not one
    word of the header or of out written."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n = 70
    real, pa = NC.graph(rng, n, 0.2), rng.rand(n, n).astype(np.float32)
    mark = 2 ** 64 - 7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(real, pa, idx=None):
        r, a = _dev(real), _dev(pa)
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        rows = n if idx is None else len(idx)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        hd = (ctypes.c_uint64 * 4)(*([mark] * 4))
        out = torch.full((rows, 5), -7, device="cuda:0", dtype=torch.int64)
        rc = L.mcgra_auc_node_jackknife(stream, n, p(r), n, p(a), n, p(ix), rows, hd, p(out))
        return rc, L.mcgra_last_error().decode(), list(hd), bool((out == -7).all()), bool((out == -7).any())

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    rc, _, hd, untouched, any_left = run(real, pa)
    assert rc == 0 and hd[0] == NC.pairs_of(n) and mark not in hd and not any_left
    for value in (np.nan, np.inf, -np.inf):
        rc, e, hd, untouched, _ = run(real, bad(pa, value))
        assert rc == -1 and "NaN or infinite" in e and "auc_node_jackknife" in e and hd == [mark] * 4 and untouched
    rc, e, hd, untouched, _ = run(bad(real, 0.5), pa)
    assert rc == -1 and "label" in e and hd == [mark] * 4 and untouched
    # the same invalid entries above the diagonal are not looked at
    rc, _, _, _, any_left = run(bad(real, 0.5, (7, 40)), bad(pa, np.nan, (7, 40)))
    assert rc == 0 and not any_left
    rc, e, hd, untouched, _ = run(real, pa, [3, 9, 4, 9, 12])
    assert rc == -1 and "twice" in e and hd == [mark] * 4 and untouched
    for ids in ([3, 9, n], [3, -1, 5]):
        rc, e, hd, untouched, _ = run(real, pa, ids)
        assert rc == -1 and "outside" in e and hd == [mark] * 4 and untouched


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = NC.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.auc_node_jackknife(_dev(real), _dev(nan))
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.auc_node_jackknife_paired(_dev(real), _dev(pa), _dev(nan))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.auc_node_jackknife(_dev(real), _dev(pa), [1, 2, 1])
    with pytest.raises(pkg._lib.McgraError):
        E.auc_node_jackknife(_dev(real), _dev(pa), [4])                        # fewer than two nodes
    with pytest.raises(ValueError, match="level"):
        E.auc_node_jackknife(_dev(real), _dev(pa), None, 1.0)


# ------------------------------------------------------------------------------------------------------ 3. main.py
def test_main_evaluate_ci_nodes_versus_and_save_influence(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --ci_nodes --versus features
    adds the ci_nodes_* and versus_nodes_* dicts, each the truth on the matrices that were scored; --save_influence writes the
    five columns and d_v of each set; with --ci the ratio se_nodes / se is reported; a run without the flags returns and logs
    what it did before the flags existed."""
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt"])
    assert not any(hasattr(plain_args, k) for k in ("ci_nodes", "save_influence"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.auc_node_jackknife_paired

    def record(real, pred_a, pred_b, idx=None, level=0.95):
        v = orig(real, pred_a, pred_b, idx, level)
        seen.append((real.cpu().numpy(), pred_a.cpu().numpy(), pred_b.cpu().numpy(), None if idx is None else np.asarray(idx), v))
        return v

    monkeypatch.setattr(M.engine, "auc_node_jackknife_paired", record)
    path = str(tmp_path / "influence.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "nodes.txt", "--ci_nodes", "--versus", "features",
                                                    "--save_influence", path]))
    out = capsys.readouterr().out
    new = [f"{f}_{s}" for f in ("ci_nodes", "versus_nodes") for s in ("attack", "train", "all")]
    assert sorted(res) == sorted(list(plain) + new) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    saved = np.load(path)
    for (real, pa, pb, idx, v), name in zip(seen, ("attack", "train", "all")):
        assert res[f"versus_nodes_{name}"] is v and res[f"ci_nodes_{name}"] is v["a"]
        ia, ib = T.ints(real, pa, idx), T.ints(real, pb, idx)
        _check_paired(v, ia, ib, 0.95, name)
        assert np.array_equal(saved[f"nodes_{name}"], np.arange(1190) if idx is None else idx)
        for k in T.COLUMNS:
            assert saved[f"{k}_{name}"].dtype == np.int64 and saved[f"{k}_{name}"].tolist() == ia[k], (k, name)
        assert saved[f"influence_{name}"].dtype == np.float64
        assert _same_list(saved[f"influence_{name}"].tolist(), v["a"]["influence"].tolist())
    c, d = res["ci_nodes_all"], res["versus_nodes_all"]
    assert c["nodes"] == 1190 and c["pairs"] == NC.pairs_of(1190) and c["se"] > 0
    assert (f"current auc={res['auc_all']}\ncurrent auc_pairs={c['auc']} se_nodes={c['se']} ci_nodes=[{c['ci_low']}, {c['ci_high']}]\n"
            f"current delta={d['delta']} se_nodes={d['se_delta']} z={d['z']} p={d['p_value']}\n" in out) and "se_nodes" not in out_plain
    log = open(tmp_path / "results" / "nodes.txt").read().split("\n")
    for i, (name, key) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        c, v = res[f"ci_nodes_{key}"], res[f"versus_nodes_{key}"]
        assert log[2 + 2 * i] == (f"In {name}: nodes={c['nodes']} pairs={c['pairs']} AUC of pairs={c['auc']} "
                                  f"jackknife AUC={c['auc_jackknife']} se_nodes={c['se']} 95% CI_nodes=[{c['ci_low']}, {c['ci_high']}] "
                                  f"undefined_nodes={c['undefined_nodes']}")
        assert log[3 + 2 * i] == (f"In {name}: versus features (nodes): AUC={v['b']['auc']} delta={v['delta']} se_nodes={v['se_delta']} "
                                  f"z={v['z']} p={v['p_value']}")
    assert log[8].startswith("current density:") and "ci_nodes=True" in log[0] and "save_influence=" in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert all(w not in old for w in ("ci_nodes", "save_influence", "se_nodes")) and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[8:]
    # with --ci as well: DeLong's dicts beside the jackknife's, and the ratio of the two standard errors
    both = M.run(M.build_parser().parse_args(argv + ["--log_name", "both.txt", "--ci", "--ci_nodes"]))
    out = capsys.readouterr().out
    assert sorted(both) == sorted(list(plain) + [f"{f}_{s}" for f in ("ci", "ci_nodes") for s in ("attack", "train", "all")])
    for name in ("attack", "train", "all"):
        cn, cd = both[f"ci_nodes_{name}"], both[f"ci_{name}"]
        assert cn["ints"] == res[f"ci_nodes_{name}"]["ints"] and cn["se"] == res[f"ci_nodes_{name}"]["se"]
        assert cn["auc"] == cd["auc"] and all(cn["ints"][k] == cd["ints"][k] for k in ("pairs", "positives", "negatives", "T"))
    cn, cd = both["ci_nodes_all"], both["ci_all"]
    assert f"se_nodes={cn['se']} ci_nodes=[{cn['ci_low']}, {cn['ci_high']}] se_nodes/se={cn['se'] / cd['se']}\n" in out
    assert "se_nodes/se=" in open(tmp_path / "results" / "both.txt").read()
