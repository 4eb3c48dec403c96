"""DeLong's variance and paired test on the device (mcgra_auc_delong, mcgra_auc_delong_paired, engine.auc_delong /
auc_delong_paired, main.py --ci / --versus / --save_scores) against tests/delong_truth.py: every integer of `out` compared for
equality, for both entries, and every double of the engine's dicts bit for bit (one correctly rounded rational each defines
them) -- over the smallest selections, ties, signed zeros, subnormals and negative scores, layouts (padding, NaN junk outside
the selected lower triangle, asymmetric matrices, permuted subsets), selections and class sizes on both sides of every
constant the kernels' grids and steps use, the case whose sums carry into the high limb, and the paired relations B = A,
B an increasing map of A, B = -A and two independent scorings.  Run with -m gpu.

tests/test_delong_cases_cpu.py checks, without a GPU, that these inputs (tests/delong_cases.py) have the properties the cases
are there for and that they tell seven wrong readings of the definition from the right one."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import delong_cases as D
from tests import delong_truth as T
from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = D.cases()
TILING = D.TILING


@functools.lru_cache(maxsize=None)
def truth(name):
    """The truth of a case, computed once and shared (read-only)."""
    real, pa, pb, idx, _ = CASES[name]
    return T.paired_ints(real, pa, pb, idx)


def single_of(g, s="a"):
    return {"pairs": g["pairs"], "positives": g["positives"], "negatives": g["negatives"], "T": g["T_" + s], "A2": g["A2_" + s],
            "B2": g["B2_" + s]}


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


def _check_single(got, ints, level, what):
    want = T.stats(ints, level)
    print(f"{what}: got {got['ints']} auc={got['auc']} var={got['var']} ci=[{got['ci_low']}, {got['ci_high']}]")
    assert got["ints"] == ints, (what, got["ints"], ints)
    assert (got["pairs"], got["positives"], got["negatives"], got["level"]) == (ints["pairs"], ints["positives"], ints["negatives"], level)
    for key in T.RATES:
        assert isinstance(got[key], float) and _same(got[key], want[key]), (what, key, got[key], want[key])


def _check_paired(got, ints, level, what):
    want = T.paired_stats(ints, level)
    print(f"{what}: got {got['ints']} delta={got['delta']} cov={got['cov']} z={got['z']} p={got['p_value']}")
    assert got["ints"] == ints, (what, got["ints"], ints)
    for s in ("a", "b"):
        _check_single(got[s], single_of(ints, s), level, (what, s))
    for key in T.PAIRED_RATES:
        assert isinstance(got[key], float) and _same(got[key], want[key]), (what, key, got[key], want[key])


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_delong_against_the_truth(pkg, name):
    """Every integer of both entries and every double the engine forms from them."""
    from mc_gra_amd import engine as E
    real, pa, pb, idx, pad = CASES[name]
    r, a, b, ix = _dev(real, pad), _dev(pa, pad), _dev(pb, pad), None if idx is None else _dev(idx)
    if pad:
        assert a.stride(0) == b.stride(0) == r.stride(0) == pa.shape[1] + pad
    g = truth(name)
    _check_single(E.auc_delong(r, a, ix), single_of(g, "a"), 0.95, name)
    _check_single(E.auc_delong(r, b, ix, level=0.9), single_of(g, "b"), 0.9, name)
    _check_paired(E.auc_delong_paired(r, a, b, ix), g, 0.95, name)


def test_paired_relations(pkg):
    """B = A: cov = var and var_delta = 0; B an increasing map of A: the same integers; B = -A: T_b = 2 P N - T_a."""
    from mc_gra_amd import engine as E
    real, a, _, _, _ = CASES["b_equals_a"]
    r, da = _dev(real), _dev(a)
    same = E.auc_delong_paired(r, da, da)                                   # one buffer as both matrices
    assert same["ints"] == truth("b_equals_a") and same["cov"] == same["a"]["var"] == same["b"]["var"] > 0
    assert same["se_delta"] == 0.0 and same["delta"] == 0.0 and same["z"] == 0.0 and same["p_value"] == 1.0
    up = E.auc_delong_paired(r, da, _dev(CASES["b_increasing_map_of_a"][2]))
    assert up["ints"] == same["ints"]
    neg = E.auc_delong_paired(r, da, _dev(CASES["b_minus_a"][2]))
    g = neg["ints"]
    assert g["T_b"] == 2 * g["positives"] * g["negatives"] - g["T_a"] and neg["b"]["auc"] == 1.0 - neg["a"]["auc"]
    swapped = E.auc_delong_paired(r, _dev(CASES["b_minus_a"][2]), da)["ints"]
    assert (swapped["T_a"], swapped["A2_a"], swapped["B2_a"], swapped["A_ab"], swapped["B_ab"]) == \
        (g["T_b"], g["A2_b"], g["B2_b"], g["A_ab"], g["B_ab"])


def test_reordered_selection_gives_the_same_integers(pkg):
    """The same node set in another order names the same pairs of a symmetric matrix: the same integers, the same doubles."""
    from mc_gra_amd import engine as E
    real, pa, pb, a, _ = CASES["subset_permuted"]
    b = CASES["subset_reordered"][3]
    r, da, db = _dev(real), _dev(pa), _dev(pb)
    ga, gb = E.auc_delong_paired(r, da, db, a), E.auc_delong_paired(r, da, db, b)
    gs = E.auc_delong_paired(r, da, db, np.sort(a))
    assert ga["ints"] == gb["ints"] == gs["ints"] == truth("subset_permuted")
    assert ga["z"] == gb["z"] and ga["a"]["var"] == gb["a"]["var"]
    assert E.auc_delong(r, da, a.tolist())["ints"] == E.auc_delong(r, da, _dev(b))["ints"]      # list or device tensor


@pytest.mark.parametrize("name", ["tiling_n1449", "class_P4097_levels", "subset_permuted"])
def test_two_calls_give_identical_bits(pkg, name):
    from mc_gra_amd import engine as E
    real, pa, pb, idx, pad = CASES[name]
    r, a, b, ix = _dev(real, pad), _dev(pa, pad), _dev(pb, pad), None if idx is None else _dev(idx)
    one, two = E.auc_delong_paired(r, a, b, ix), E.auc_delong_paired(r, a, b, ix)
    assert one["ints"] == two["ints"] and all(_same(one[k], two[k]) for k in T.PAIRED_RATES)
    s1, s2 = E.auc_delong(r, a, ix), E.auc_delong(r, a, ix)
    assert s1["ints"] == s2["ints"] and all(_same(s1[k], s2[k]) for k in T.RATES)


def test_other_dtypes_and_devices_of_the_operands(pkg):
    """float64 / bool operands and host node ids are converted as topk_metrics converts them."""
    import torch
    from mc_gra_amd import engine as E
    real, pa, pb, idx, _ = CASES["asymmetric"]
    g = truth("asymmetric")
    got = E.auc_delong_paired(_dev(real).bool(), _dev(pa).double(), _dev(pb), torch.arange(len(real)))
    assert got["ints"] == g


# ------------------------------------------------------------------------------------------------ 2. the refusals
def test_device_refusals_leave_out_untouched(pkg):
    """A NaN score in A only, in B only, an infinite score, a label of 0.5, a repeated id, an id out of range: MCGRA_EINVAL,
    the cause named, and not one word of out written."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n = 70
    real, pa, pb = D.graph(rng, n, 0.2), rng.rand(n, n).astype(np.float32), rng.rand(n, n).astype(np.float32)
    mark = 2 ** 64 - 7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(real, pa, pb, idx=None):
        r, a, b = _dev(real), _dev(pa), _dev(pb)
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        rows = n if idx is None else len(idx)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        o1, o2 = (ctypes.c_uint64 * 8)(*([mark] * 8)), (ctypes.c_uint64 * 17)(*([mark] * 17))
        rc1 = L.mcgra_auc_delong(stream, n, p(r), n, p(a), n, p(ix), rows, o1)
        e1 = L.mcgra_last_error().decode()
        rc2 = L.mcgra_auc_delong_paired(stream, n, p(r), n, p(a), n, p(b), n, p(ix), rows, o2)
        e2 = L.mcgra_last_error().decode()
        return rc1, e1, list(o1), rc2, e2, list(o2)

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    rc1, _, o1, rc2, _, o2 = run(real, pa, pb)
    assert rc1 == 0 and rc2 == 0 and o1[0] == o2[0] == D.pairs_of(n) and mark not in o1 and mark not in o2
    # a NaN in A: both entries refuse; the paired one names scores_a
    rc1, e1, o1, rc2, e2, o2 = run(real, bad(pa, np.nan), pb)
    assert rc1 == -1 and rc2 == -1 and "NaN" in e1 and "scores_a" in e2 and "scores_b" not in e2
    assert o1 == [mark] * 8 and o2 == [mark] * 17
    # a NaN in B only: the single entry on A passes, the paired one names scores_b
    rc1, e1, o1, rc2, e2, o2 = run(real, pa, bad(pb, np.nan))
    assert rc1 == 0 and rc2 == -1 and "scores_b" in e2 and "scores_a" not in e2 and o2 == [mark] * 17
    rc1, e1, o1, rc2, e2, o2 = run(real, bad(pa, -np.inf), bad(pb, np.inf))
    assert rc1 == -1 and rc2 == -1 and "scores_a" in e2 and "scores_b" in e2 and o1 == [mark] * 8 and o2 == [mark] * 17
    rc1, e1, o1, rc2, e2, o2 = run(bad(real, 0.5), pa, pb)
    assert rc1 == -1 and rc2 == -1 and "label" in e1 and "label" in e2 and o1 == [mark] * 8 and o2 == [mark] * 17
    # the same invalid entries above the diagonal are not looked at
    rc1, _, _, rc2, _, _ = run(bad(real, 0.5, (7, 40)), bad(pa, np.nan, (7, 40)), bad(pb, np.nan, (3, 3)))
    assert rc1 == 0 and rc2 == 0
    rc1, e1, o1, rc2, e2, o2 = run(real, pa, pb, [3, 9, 4, 9, 12])
    assert rc1 == -1 and rc2 == -1 and "twice" in e1 and "twice" in e2 and o1 == [mark] * 8 and o2 == [mark] * 17
    for ids in ([3, 9, n], [3, -1, 5]):
        rc1, e1, o1, rc2, e2, o2 = run(real, pa, pb, ids)
        assert rc1 == -1 and rc2 == -1 and "outside" in e1 and "outside" in e2 and o1 == [mark] * 8 and o2 == [mark] * 17


def test_engine_raises_what_the_entries_refuse(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = D.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.auc_delong(_dev(real), _dev(nan))
    with pytest.raises(pkg._lib.McgraError, match="scores_b"):
        E.auc_delong_paired(_dev(real), _dev(pa), _dev(nan))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.auc_delong(_dev(real), _dev(pa), [1, 2, 1])
    with pytest.raises(pkg._lib.McgraError):
        E.auc_delong(_dev(real), _dev(pa), [4])                                # fewer than two nodes
    with pytest.raises(ValueError, match="level"):
        E.auc_delong(_dev(real), _dev(pa), None, 1.0)


# ------------------------------------------------------------------------------------------------------ 3. main.py
def test_main_evaluate_ci_versus_and_save_scores(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --ci --versus features adds
    the ci_* and versus_* dicts, each the truth on the matrices that were scored; --save_scores writes modified_adj, which
    round-trips through --versus PATH to delta = 0, z = 0, p = 1; a run without the flags returns and logs what it did before
    the flags existed."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt"])
    assert not any(hasattr(plain_args, k) for k in ("ci", "versus", "save_scores"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.auc_delong_paired

    def record(real, pred_a, pred_b, idx=None, level=0.95):
        v = orig(real, pred_a, pred_b, idx, level)
        seen.append((real.cpu().numpy(), pred_a.cpu().numpy(), pred_b.cpu().numpy(), None if idx is None else np.asarray(idx), v))
        return v

    monkeypatch.setattr(M.engine, "auc_delong_paired", record)
    path = str(tmp_path / "scores.npy")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "ci.txt", "--ci", "--versus", "features", "--save_scores", path]))
    out = capsys.readouterr().out
    new = [f"{f}_{s}" for f in ("ci", "versus") for s in ("attack", "train", "all")]
    assert sorted(res) == sorted(list(plain) + new) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    for (real, pa, pb, idx, v), name in zip(seen, ("attack", "train", "all")):
        assert res[f"versus_{name}"] is v and res[f"ci_{name}"] is v["a"]
        g = T.paired_ints(real, pa, pb, idx)
        _check_paired(v, g, 0.95, name)
    real, pa, pb, idx, d = seen[2]
    assert idx is None and d["ints"]["pairs"] == D.pairs_of(1190) and d["a"]["positives"] >= 2 and d["a"]["se"] > 0
    assert 0.0 <= d["a"]["ci_low"] < d["a"]["auc"] < d["a"]["ci_high"] <= 1.0 and 0.0 <= d["p_value"] <= 1.0
    saved = np.load(path)
    assert saved.dtype == np.float32 and saved.shape == (1190, 1190) and np.array_equal(saved.view(np.uint32), pa.view(np.uint32))
    c = res["ci_all"]
    assert (f"current auc={res['auc_all']}\ncurrent auc_pairs={c['auc']} se={c['se']} ci=[{c['ci_low']}, {c['ci_high']}]\n"
            f"current delta={d['delta']} z={d['z']} p={d['p_value']}\n" in out) and "auc_pairs" not in out_plain
    log = open(tmp_path / "results" / "ci.txt").read().split("\n")
    for i, (name, key) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        c, v = res[f"ci_{key}"], res[f"versus_{key}"]
        assert log[2 + 2 * i] == (f"In {name}: pairs={c['pairs']} positives={c['positives']} AUC of pairs={c['auc']} se={c['se']} "
                                  f"95% CI=[{c['ci_low']}, {c['ci_high']}]")
        assert log[3 + 2 * i] == (f"In {name}: versus features: AUC={v['b']['auc']} delta={v['delta']} se={v['se_delta']} "
                                  f"z={v['z']} p={v['p_value']}")
    assert log[8].startswith("current density:") and "ci=True" in log[0] and "versus='features'" in log[0] and "save_scores=" in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert all(w not in old for w in ("ci=", "versus", "save_scores", "AUC of pairs")) and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[8:]
    # the saved scores against the same run: the paired test of a matrix with itself
    seen.clear()
    again = M.run(M.build_parser().parse_args(argv + ["--log_name", "again.txt", "--ci", "--versus", path]))
    capsys.readouterr()
    assert len(seen) == 3 and np.array_equal(seen[2][1].view(np.uint32), seen[2][2].view(np.uint32))
    for name in ("attack", "train", "all"):
        v = again[f"versus_{name}"]
        assert v["delta"] == 0.0 and v["z"] == 0.0 and v["p_value"] == 1.0 and v["se_delta"] == 0.0, name
        assert v["a"] == res[f"ci_{name}"]
    # --ci alone is the single entry: the same dicts, no versus_* keys
    sets = {"attack": seen[0][3], "train": seen[1][3], "all": None}
    alone = R.ci_report(_dev(real), _dev(pa), sets)
    assert sorted(alone) == ["ci_all", "ci_attack", "ci_train"]
    for name in sets:
        assert alone[f"ci_{name}"] == res[f"ci_{name}"], name
