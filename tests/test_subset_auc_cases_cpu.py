"""Without a GPU: the truth of the subset AUCs (tests/subset_auc_truth.py) against a literal double loop and against sklearn;
that the cases of tests/subset_auc_cases.py tell the definition apart from its wrong readings and have the properties they are
there for; the known answers; engine.ablation_masks and engine.shapley_shares (pure host); every refusal that needs the
arguments alone, of the two entries, of the wrappers and of main.py's parser."""
import argparse
import ctypes
import functools
import itertools
from fractions import Fraction

import numpy as np
import pytest

from tests import subset_auc_cases as SC
from tests import subset_auc_truth as T

CASES = SC.cases()


@functools.lru_cache(maxsize=None)
def truth(name, which):
    real, comps, idx, _, lists = CASES[name]
    return T.ints(real, comps, lists[which], idx)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    return mcgra_loader.load()


def selected(name):
    real, comps, idx, _, _ = CASES[name]
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx)
    a, b = np.tril_indices(len(ix), -1)
    return real[ix[a], ix[b]] == 1, [c[ix[a], ix[b]] for c in comps]


# ------------------------------------------------------------------------------------------------- 1. the truth itself
@pytest.mark.parametrize("name", ["all2_k1", "all3_k3", "all63_k8", "ints64_k3", "sub63_k3", "one_edge", "no_edge", "complete",
                                  "cancellation"])
def test_truth_against_the_double_loop(name):
    lab, sel = selected(name)
    real, comps, idx, _, lists = CASES[name]
    masks = lists[0][-3:]
    want = [T.brute_T(lab, T.subset_sum(sel, q)) for q in masks]
    assert want == [T.T_with_ties(lab, T.subset_sum(sel, q), 1) for q in masks]
    got = T.ints(real, comps, masks, idx)
    assert got["T"] == want and got["pairs"] == len(lab) and got["positives"] == int(lab.sum())
    assert got["negatives"] == got["pairs"] - got["positives"] and all(0 <= t <= 2 * got["positives"] * got["negatives"] for t in want)


@pytest.mark.parametrize("name", ["all63_k8", "all65_k3", "one_edge", "floats65_k1"])
def test_truth_against_sklearn_where_nothing_ties(name):
    from sklearn.metrics import roc_auc_score
    lab, sel = selected(name)
    real, comps, idx, _, lists = CASES[name]
    masks = lists[0][:16]
    g = T.stats(T.ints(real, comps, masks, idx), masks)
    held = 0
    for q, auc in zip(masks, g["auc"]):
        s = T.subset_sum(sel, q)
        if len(np.unique(s)) == len(s):                                  # (two of a few thousand floats may coincide)
            held += 1
            assert abs(auc - roc_auc_score(lab, s.astype(np.float64))) <= 1e-12
    assert held >= (len(masks) + 1) // 2


# --------------------------------------------------------------------------------------------- 2. the resolving power
def wrong_readings(name, which):
    real, comps, idx, _, lists = CASES[name]
    masks = lists[which]
    K = len(comps)
    lab, sel = selected(name)
    flip = lambda q: sum(1 << (K - 1 - k) for k in range(K) if q >> k & 1)
    ix = np.arange(real.shape[0]) if idx is None else np.asarray(idx)
    full_lab = real[np.ix_(ix, ix)].reshape(-1) == 1
    full_sel = [c[np.ix_(ix, ix)].reshape(-1) for c in comps]
    right = truth(name, which)["T"]
    return {
        "descending-k sum": T.ints(real, comps, masks, idx, order=-1)["T"],
        "float64 sum": T.ints(real, comps, masks, idx, dtype=np.float64)["T"],
        "reversed bit order": T.ints(real, comps, [flip(q) for q in masks], idx)["T"],
        "ties counted 0": [T.T_with_ties(lab, T.subset_sum(sel, q), 0) for q in masks],
        "ties counted 2": [T.T_with_ties(lab, T.subset_sum(sel, q), 2) for q in masks],
        "ordered pairs with the diagonal": [T.T_of(full_lab, T.subset_sum(full_sel, q)) for q in masks],
        "T shifted by one mask": right[1:] + right[:1],
        "transposed read": T.ints(real, [c.T for c in comps], masks, idx)["T"],
    }


def test_the_cases_tell_the_wrong_readings_apart():
    """Over the case set the GPU tests run, each wrong reading of the definition changes some T."""
    names = ("all63_k8", "ints64_k3", "all65_k3", "sub63_k3", "cancellation", "cancellation_descending", "ints129_k8")
    caught = {}
    for name in names:
        for reading, T_wrong in wrong_readings(name, 0).items():
            if T_wrong != truth(name, 0)["T"]:
                caught.setdefault(reading, []).append(name)
    assert sorted(caught) == sorted(wrong_readings("all3_k3", 0)), caught
    assert "cancellation" in caught["float64 sum"] and "cancellation_descending" in caught["descending-k sum"]
    assert "ints64_k3" in caught["ties counted 0"] and "ints64_k3" in caught["ties counted 2"]
    assert "sub63_k3" in caught["transposed read"]


def test_the_cases_have_what_they_are_there_for():
    assert sorted({(c[0].shape[0] if c[2] is None else len(c[2])) for c in CASES.values()}) == sorted(set(SC.SIZES) | {63})
    assert {len(c[1]) for c in CASES.values()} == set(SC.KS)
    lists = [q for c in CASES.values() for q in c[4]]
    assert any(len(q) == 1 for q in lists) and any(len(q) == 255 for q in lists) and any(len(set(q)) < len(q) for q in lists)
    assert SC.table_masks() in lists and len(SC.table_masks()) <= 25
    assert any(c[3] > 0 for c in CASES.values()) and any(c[2] is not None and c[0].shape[0] > len(c[2]) for c in CASES.values())
    P = lambda name: truth(name, 0)["positives"]
    N = lambda name: truth(name, 0)["negatives"]
    assert P("one_edge") == 1 and P("no_edge") == 0 and N("complete") == 0 and P("complete") == 63 * 31
    assert P("dense257_k8") > 100 * SC.SAMPLES_AT_255 and len(CASES["dense257_k8"][4][0]) == 255     # strides far above one
    assert P("all3_k3") <= SC.SAMPLES_AT_255 and P("sub63_k3") > 0
    # a permutation of idx changes nothing
    for a, b in (("sub257_k8", "sub257_k8_permuted"), ("sym63_k3", "sym63_k3_permuted")):
        assert sorted(CASES[a][2]) == sorted(CASES[b][2]) and list(CASES[a][2]) != list(CASES[b][2])
        assert truth(a, 0) == truth(b, 0)
    # repeats give equal T; ties and signed zeros exist in the integer cases
    rep = truth("ints64_k3", 1)["T"]
    assert rep[0] == rep[2] == rep[5] and rep[1] == rep[4]
    lab, sel = selected("ints64_k3")
    assert len(np.unique(T.subset_sum(sel, 7))) < 20 and np.any(np.signbit(sel[0]) & (sel[0] == 0))
    assert set(np.unique(sel[2])) == {0.0, 1.0}


def test_known_answers():
    real, comps, idx, _, _ = CASES["cancellation"]
    g = T.ints(real, comps, [7, 5, 2], idx)
    P, N = g["positives"], g["negatives"]
    assert P > 0 and N > 0 and g["T"] == [0, P * N, 2 * P * N]           # 0.0f < 0.5 ; 0 == 0: all ties; 1 > 0.5
    assert T.ints(real, comps, [7], idx, dtype=np.float64)["T"] == [2 * P * N]
    assert T.ints(real, [(comps[0] + comps[2]).astype(np.float32), comps[1]], [3], idx)["T"] == [2 * P * N]      # (c0 + c2) + c1
    real, comps, idx, _, _ = CASES["cancellation_descending"]
    assert T.ints(real, comps, [7], idx)["T"] == [0] and T.ints(real, comps, [7], idx, order=-1)["T"] == [2 * P * N]
    # small integers, by hand: positions 0 .. 3, edges (1, 0) and (3, 2)
    real = np.zeros((4, 4), np.float32)
    real[1, 0] = real[0, 1] = real[3, 2] = real[2, 3] = 1
    c0 = np.asarray([[0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 0, 0], [0, 2, 1, 0]], np.float32)
    c1 = np.asarray([[0, 9, 9, 9], [0, 0, 9, 9], [1, 0, 0, 9], [2, -1, 0, 0]], np.float32)
    # pairs (a, b): (1,0)+ (2,0) (2,1) (3,0) (3,1) (3,2)+ ; c0: 2 | 1 1 0 2 | 1 ; c1: 0 | 1 0 2 -1 | 0 ; sum: 2 | 2 1 2 1 | 1
    g = T.ints(real, [c0, c1], [1, 2, 3])
    assert (g["pairs"], g["positives"], g["negatives"]) == (6, 2, 4)
    assert g["T"] == [(2 + 2 + 2 + 1) + (1 + 1 + 2 + 0), 2 * (0 + 1 + 0 + 2), (1 + 2 + 1 + 2) + (0 + 1 + 0 + 1)] == [11, 6, 8]
    assert all(type(t) is int for t in g["T"])


# ------------------------------------------------------------------------------------------ 3. the mask table (host)
def test_ablation_masks(pkg):
    from mc_gra_amd import engine as E
    assert E.ENSEMBLE_COMPONENTS == T.NAMES and len(E.ENSEMBLE_COMPONENTS) == 8
    for extra_p, extra_u in itertools.product(range(8), range(8)):
        present, used = 0x1f | extra_p << 5, 0x1f | extra_u << 5
        if used & ~present:
            with pytest.raises(ValueError):
                E.ablation_masks(present, used)
            continue
        table = E.ablation_masks(present, used)
        assert table == T.ablation_masks(present, used)
        assert 1 <= len(table) <= 25 and len(set(table)) == len(table) and table[0] == used
        assert all(1 <= q <= present and q & ~present == 0 for q in table)
        k = bin(present).count("1")
        assert table[1:1 + k] == [1 << b for b in range(8) if present >> b & 1]
        flags = [q for q in table if q & 0x1f == 0x1f]
        assert set(flags) >= {0x1f | s << 5 for s in range(8) if (s << 5) & ~present == 0}
    assert E.ablation_masks(0xff, 0xff) == [0xff] + [1 << k for k in range(8)] + [0xff ^ 1 << k for k in range(8)] + \
        [0x1f, 0x3f, 0x5f, 0x9f]                 # (0x7f, 0xbf, 0xdf and 0xff are there already)
    assert E.ablation_masks(0xff, 0x1f)[-7:] == [0x3f, 0x5f, 0x7f, 0x9f, 0xbf, 0xdf, 0xff]
    assert E.ablation_masks(0x1f, 0x1f) == [0x1f, 1, 2, 4, 8, 16, 0x1e, 0x1d, 0x1b, 0x17, 0x0f]
    assert E.ablation_masks(0x1f, 1) == [1, 2, 4, 8, 16, 0x1f]                # used alone: `without` would be the empty set
    for bad in ((0x0f, 0x0f), (0x1f, 0), (0x1f, 0x3f), (0x1ff, 0x1f), (-1, 1), (True, 1), (0x1f, 1.0)):
        with pytest.raises(ValueError):
            E.ablation_masks(*bad)


# ------------------------------------------------------------------------------------------ 4. Shapley shares (host)
def test_shapley_shares(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(3)
    for K in (1, 2, 4, 5):
        value = {q: Fraction(int(rng.randint(0, 1001)), 1000) for q in range(1, 1 << K)}
        got = E.shapley_shares(K, value)
        assert got == T.shapley_by_permutations(K, value) and all(isinstance(s, Fraction) for s in got)
        assert sum(got) == value[(1 << K) - 1] - Fraction(1, 2)                          # efficiency, exactly
    # players 1 and 2 are duplicates (v depends on them symmetrically); player 3 adds nothing (a component of zeros)
    K = 4
    base = {q: Fraction(int(rng.randint(0, 1001)), 1000) for q in range(1, 1 << K)}
    value = {}
    for q in range(1, 1 << K):
        core = q & ~8                                                     # without player 3
        sym = (core & ~6) | (6 if core & 6 == 6 else (2 if core & 6 else 0))      # players 1, 2: only how many of them
        value[q] = base[sym] if sym else Fraction(1, 2)
    got = E.shapley_shares(K, value)
    assert got[1] == got[2] and got[3] == 0 and sum(got) == value[15] - Fraction(1, 2)
    for bad in ((0, {}), (9, {}), (2, {1: Fraction(1), 2: Fraction(1)}), (2, {1: 0.5, 2: 0.5, 3: 0.5}), (True, {1: Fraction(1)})):
        with pytest.raises(ValueError):
            E.shapley_shares(*bad)


def test_ablation_stats_from_integers(pkg):
    """reports.ablation_stats (no device): the dict of one index set from subset_auc's dict, with the shares of the game on
    the present components."""
    from mc_gra_amd import reports as R
    present, used = 0x7f, 0x3f                            # no label adjacency; Y_A held but not used
    masks = R.ablation_masks(present, used, "shapley")
    assert len(masks) == 127 and sorted(masks) == [q for q in range(1, 256) if q & ~present == 0]
    assert set(R.ablation_masks(present, used, "table")) <= set(masks)
    rng = np.random.RandomState(8)
    P, N = 30, 70
    d = {"pairs": 100, "positives": P, "negatives": N, "masks": masks, "T": [int(t) for t in rng.randint(0, 2 * P * N + 1, len(masks))]}
    d["auc"] = [float(Fraction(t, 2 * P * N)) for t in d["T"]]
    res = R.ablation_stats(d, present, used, 0, "shapley")
    auc = dict(zip(masks, d["auc"]))
    assert res["auc_used"] == auc[used] and res["alone"] == {T.NAMES[k]: auc[1 << k] for k in range(7)}
    assert res["without"] == {T.NAMES[k]: auc[used ^ 1 << k] for k in range(6)}
    assert [(r["useH_A"], r["useY_A"], r["useY"], r["mask"]) for r in res["flag_table"]] == \
        [(False, False, False, 0x1f), (True, False, False, 0x3f), (False, True, False, 0x5f), (True, True, False, 0x7f)]
    assert [r["mask"] for r in res["subsets"]] == masks and res["subsets"][2]["names"] == ("learned", "feature")
    value = {q: Fraction(d["T"][q - 1], 2 * P * N) for q in range(1, 128)}          # present = the low seven bits: player = bit
    want = R.engine.shapley_shares(7, value)
    assert res["shapley"] == {T.NAMES[k]: float(s) for k, s in enumerate(want)} and "label" not in res["shapley"]
    assert res["shapley_sum"] == float(Fraction(d["T"][masks.index(present)], 2 * P * N) - Fraction(1, 2))
    plain = R.ablation_stats({**d, "masks": masks, "T": d["T"], "auc": d["auc"]}, present, used, 3, "table")
    assert "shapley" not in plain and plain["decode_mode"] == 3 and plain["components"] == T.NAMES


# ------------------------------------------------------------------------------------------------- 5. the refusals
def test_entries_refuse_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine; nothing is written to out."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    mark = 2 ** 64 - 7

    def run(n=8, ldl=8, ldc=8, idx=None, n_idx=None, lab=p, K=3, comps=True, masks=(1, 7, 5), n_masks=None, out=True, hole=None,
            no_masks=False):
        ptrs = (ctypes.c_void_p * 8)(*([64] * 8))
        if hole is not None:
            ptrs[hole] = None
        ms = (ctypes.c_uint32 * max(1, len(masks)))(*masks)
        o = (ctypes.c_uint64 * 12)(*([mark] * 12))
        rc = L.mcgra_subset_auc(None, n, lab, ldl, ptrs if comps else None, K, ldc, idx, n if n_idx is None else n_idx,
                                None if no_masks else ms, len(masks) if n_masks is None else n_masks, o if out else None)
        assert list(o) == [mark] * 12
        return rc, L.mcgra_last_error().decode()

    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(ldl=7), dict(ldc=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(lab=None), dict(comps=False), dict(out=False), dict(no_masks=True), dict(K=0),
               dict(K=9), dict(K=-1), dict(hole=0), dict(hole=2), dict(n_masks=0), dict(n_masks=256), dict(n_masks=-1),
               dict(masks=(0,)), dict(masks=(1, 8)), dict(masks=(1, 2 ** 32 - 1)), dict(K=1, masks=(2,))):
        rc, e = run(**kw)
        assert rc == -1 and "subset_auc" in e, kw
    rc, e = run(idx=p, n_idx=SC.MAX_NIDX + 1, n=10 ** 6, ldl=10 ** 6, ldc=10 ** 6)
    assert rc == -3 and "65535" in e
    assert run(n=SC.MAX_NIDX + 1, ldl=SC.MAX_NIDX + 1, ldc=SC.MAX_NIDX + 1)[0] == -3
    # mcgra_attack_finalize_components without an engine
    present = ctypes.c_uint(77)
    rc = L.mcgra_attack_finalize_components(None, None, 0, None, None, None, 0x1f, p, p, ctypes.byref(present))
    assert rc == -1 and present.value == 77


def test_wrappers_refuse_wrong_arguments(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, other = torch.zeros(5, 5), torch.zeros(4, 4)
    run = E.subset_auc.__wrapped__
    with pytest.raises(ValueError, match="device tensors"):
        E.subset_auc(sq, [sq], [1])                                      # a host tensor: refused before anything is called
    for comps in ([], [sq] * 9, torch.zeros(5, 5), torch.zeros(9, 5, 5), torch.zeros(0, 5, 5)):
        with pytest.raises(ValueError, match="comps"):
            run(sq, comps, [1])
    for comps in ([other], [sq, other], torch.zeros(2, 5, 4), [sq, np.zeros((5, 5))]):
        with pytest.raises(ValueError, match="5 x 5"):
            run(sq, comps, [1])
    for masks in ([], [0], [4], [1, -1], [1.0], [True], list(range(1, 4)) * 100):
        with pytest.raises(ValueError, match="mask"):
            run(sq, [sq, sq], masks)


def test_parser_ablate_flags_are_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    plain = p.parse_args([])
    assert not hasattr(plain, "ablate") and not hasattr(plain, "save_ablation")
    assert "ablate" not in str(R.shown_parameters(plain))
    assert p.parse_args(["--ablate"]).ablate == "table" and p.parse_args(["--ablate", "shapley"]).ablate == "shapley"
    a = p.parse_args(["--ablate", "table", "--save_ablation", "a.npz"])
    assert (a.ablate, a.save_ablation) == ("table", "a.npz") and "save_ablation='a.npz'" in str(R.shown_parameters(a))
    for argv, word in ((["--save_ablation", "a.npz"], "needs --ablate"), (["--ablate", "--save_ablation", ""], ".npz"),
                       (["--ablate", "all"], "table or shapley")):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        assert word in capsys.readouterr().err
    for mode in ("notrain_test", "prepare", "link_stealing"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ablate", "--mode", mode])
        err = capsys.readouterr().err
        assert mode in err and "--mode evaluate only, not --mode" in err and "--ablate" in err
    for flag in ("--ablate", "--save_ablation", "polblogs / usair"):
        assert flag in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(ablate="table", mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --ablate"):
        M._run(argparse.Namespace(save_ablation="a.npz", mode="evaluate"), 0, 1)
    assert R.REPORT_TABLE[:len(R.ALL_REPORTS)] == R.ALL_REPORTS and R.REPORT_TABLE[-1].flags == ("ablate", "save_ablation")
    assert R.RunContext._fields == R.Context._fields + ("components",) and R.RunContext._field_defaults == {"classes": None, "components": None}
