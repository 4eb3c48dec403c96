"""CPU-side checks of the top-k entries (mcgra_topk_metrics, mcgra_top_pairs, main.py --topk / --save_edges): the C ABI and its
binding, every refusal that the arguments alone decide (before a device is touched: the pointers here are never followed),
the command line, the truth helper, and the resolving power of the inputs tests/test_gpu_topk.py uses (no compute: there is
no GPU here)."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import topk_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


@pytest.fixture(scope="module")
def gpu_cases():
    from tests import test_gpu_topk as G
    return G


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_topk_entries_are_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    lib = ctypes.CDLL(LIB)
    for s in ("mcgra_topk_metrics", "mcgra_top_pairs"):
        assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(pkg._lib.lib, s).restype is ctypes.c_int
    assert len(pkg._lib.lib.mcgra_topk_metrics.argtypes) == 11 and len(pkg._lib.lib.mcgra_top_pairs.argtypes) == 12
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    from mc_gra_amd import engine as E
    for f in ("topk_metrics", "top_pairs"):
        assert callable(getattr(E, f)) and hasattr(getattr(E, f), "__wrapped__"), f      # the device guard


def test_topk_entries_refuse_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    counts = (ctypes.c_int64 * 4)()
    thr = ctypes.c_float()

    def met(n=8, ldl=8, lds=8, idx=None, n_idx=None, k=0, lab=p, sc=p, out=counts, t=ctypes.byref(thr)):
        return L.mcgra_topk_metrics(None, n, lab, ldl, sc, lds, idx, n if n_idx is None else n_idx, k, out, t)

    def top(n=8, lds=8, idx=None, n_idx=None, k=1, lab=None, ldl=0, pairs=p, ps=None, hits=None, sc=p):
        return L.mcgra_top_pairs(None, n, sc, lds, idx, n if n_idx is None else n_idx, k, lab, ldl, pairs, ps, hits)

    m = 8 * 7 // 2
    for kw in (dict(n=0), dict(n=1), dict(ldl=7), dict(lds=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0), dict(lab=None),
               dict(sc=None), dict(out=None), dict(k=-1), dict(k=m + 1), dict(idx=p, n_idx=4, k=7)):
        assert met(**kw) == -1 and b"topk_metrics" in L.mcgra_last_error(), kw
    for kw in (dict(n=0), dict(n=1), dict(lds=7), dict(idx=p, n_idx=1), dict(sc=None), dict(pairs=None), dict(k=0), dict(k=-3),
               dict(k=m + 1), dict(idx=p, n_idx=4, k=7), dict(hits=p), dict(lab=p, ldl=7), dict(lab=p, ldl=7, hits=p)):
        assert top(**kw) == -1 and b"top_pairs" in L.mcgra_last_error(), kw
    big = 65536
    assert met(n=big, ldl=big, lds=big) == -3 and b"65535" in L.mcgra_last_error()
    assert met(idx=p, n_idx=big) == -3 and top(n=big, lds=big) == -3 and top(idx=p, n_idx=big) == -3
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(top(idx=p, n_idx=big))
    assert list(counts) == [0, 0, 0, 0] and thr.value == 0.0              # nothing was written


def test_engine_entries_refuse_wrong_shapes_before_touching_a_device(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for real, pred in ((wide, wide), (sq, other), (sq, wide), (torch.zeros(5), sq)):
        with pytest.raises(AssertionError):
            E.topk_metrics.__wrapped__(real, pred)
    for pred, real in ((wide, None), (torch.zeros(5), None), (sq, other), (sq, wide)):
        with pytest.raises(AssertionError):
            E.top_pairs.__wrapped__(pred, 1, None, real)


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_topk_is_absent_by_default_and_save_edges_needs_it(pkg, capsys):
    from mc_gra_amd import main as M
    p = M.build_parser()
    a = p.parse_args([])
    assert a.topk is None and a.save_edges is None
    assert p.parse_args(["--topk", "0"]).topk == 0 and p.parse_args(["--topk", "250"]).topk == 250
    a = p.parse_args(["--topk", "7", "--save_edges", "e.npz"])
    assert a.topk == 7 and a.save_edges == "e.npz"
    for argv, word in ((["--save_edges", "e.npz"], "--topk"), (["--topk", "-1"], ">= 0"),
                       (["--topk", "5", "--mode", "notrain_test"], "notrain_test"), (["--topk", "5", "--mode", "prepare"], "prepare")):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    assert "--topk" in M.__doc__ and "--save_edges" in M.__doc__
    # a namespace that did not come through the parser is checked by run() as well, before anything is loaded
    import argparse
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(topk=3, save_edges=None, mode="prepare"), 0, 1)
    with pytest.raises(SystemExit, match="needs --topk"):
        M._run(argparse.Namespace(save_edges="e.npz", mode="evaluate"), 0, 1)


# ---------------------------------------------------------------------------------------------------- truth helper
def test_truth_helper_on_a_case_worked_by_hand():
    """n = 4: packed order (1,0) (2,0) (2,1) (3,0) (3,1) (3,2)."""
    pred = np.array([[9, 9, 9, 9], [.5, 9, 9, 9], [.75, .5, 9, 9], [-0.0, .5, 0.0, 9]], np.float32)
    real = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 1, 0]], np.float32)
    s, lab, u, v = T.packed(real, pred)
    assert s.tolist() == [.5, .75, .5, 0, .5, 0] and lab.tolist() == [True, False, True, True, False, True]
    assert list(zip(u.tolist(), v.tolist())) == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    t = T.top_k(real, pred, 3)
    assert t["order"].tolist() == [1, 0, 2] and t["edges"].tolist() == [[2, 0], [1, 0], [2, 1]]
    assert (t["k"], t["positives"], t["hits"], t["pairs"]) == (3, 4, 2, 6) and t["threshold"] == np.float32(.5)
    assert t["precision"] == 2 / 3 and t["recall"] == 2 / 4 and t["f1"] == 4 / 7
    assert T.top_k(real, pred, 3, variant="ties_last")["order"].tolist() == [1, 4, 2]
    t = T.top_k(real, pred, 5)                               # -0.0 == +0.0: position 3 before position 5; its bits are kept
    assert t["order"].tolist() == [1, 0, 2, 4, 3] and T.bits(t["threshold"])[0] == 0x80000000
    t = T.top_k(real, pred, 0)
    assert t["k"] == 4 and t["precision"] == t["recall"] == t["f1"] == 2 / 4
    t = T.top_k(real, pred, 2, idx=[3, 1, 2])                # pairs (1,3) (2,3) (2,1): scores pred[1,3], pred[2,3], pred[2,1]
    assert t["scores"].tolist() == [9, 9] and t["edges"].tolist() == [[1, 3], [2, 3]] and t["pairs"] == 3
    assert T.top_k(real, pred, 2, idx=[3, 1, 2], variant="upper")["scores"].tolist() == [9, .5]
    assert T.top_k(real, pred, 1, variant="ordered")["pairs"] == 16
    z = T.top_k(np.zeros((4, 4), np.float32), pred, 0)
    assert z["k"] == 0 and all(math.isnan(z[q]) for q in ("precision", "recall", "f1")) and math.isnan(z["threshold"])


# --------------------------------------------------------------------------------- the inputs of the GPU test cases
def test_the_gpu_cases_cover_the_shapes_and_families(gpu_cases):
    C = gpu_cases.CASES
    rows = {k: (len(v[2]) if v[2] is not None else len(v[0])) for k, v in C.items()}
    assert {2, 3, 80, 257, 1500} <= set(rows.values())
    assert any(len(v[0]) == 2048 and v[2] is not None and len(v[2]) == 1500 and len(set(v[2].tolist())) == 1500
               and not np.array_equal(v[2], np.sort(v[2])) for v in C.values())          # a shuffled 1500-node subset of 2048
    assert 1500 * 1499 // 2 > 1024 * 256
    assert any(v[3] > 0 for v in C.values())                                             # a padded leading dimension
    assert any(not np.array_equal(v[1], v[1].T) for v in C.values())                     # asymmetric scores
    assert any(len(np.unique(v[1])) == 1 for v in C.values())                            # all equal
    sp = C["n257_special"][1]
    b = T.bits(sp)
    assert (b == 0x80000000).any() and (b == 0).any() and (sp < 0).any()
    assert ((b & 0x7f800000) == 0).sum() > ((b & 0x7fffffff) == 0).sum()                # subnormals beside the zeros
    for name in C:
        ks = gpu_cases.ks_of(name)
        real, pred, idx, _ = C[name]
        t = T.top_k(real, pred, None, idx)
        assert ks[-1] == 0 and 1 in ks and t["pairs"] in ks and max(1, t["positives"]) in ks and gpu_cases.tie_k(name) in ks, name


def test_each_tie_case_cuts_a_tie_group_spread_over_many_stretches(gpu_cases):
    """At tie_k the threshold's tie group has more members than are taken, and the members lie in at least three different
    256-wide stretches of packed order: the rank of a tie crosses blocks."""
    for name in gpu_cases.TIE_CASES:
        real, pred, idx, _ = gpu_cases.CASES[name]
        members, taken = T.tie_group(real, pred, gpu_cases.tie_k(name), idx)
        stretches = len(set((members // 256).tolist()))
        print(f"{name}: k {gpu_cases.tie_k(name)} group {len(members)} taken {taken} stretches {stretches}")
        assert 1 <= taken < len(members) and stretches >= 3, (name, taken, len(members), stretches)
    # the signed zeros of n257_special tie with each other: the group at a zero threshold holds both bit patterns
    real, pred, idx, _ = gpu_cases.CASES["n257_special"]
    s = T.packed(real, pred, idx)[0]
    k0 = int((s > 0).sum()) + 5
    members, taken = T.tie_group(real, pred, k0, idx)
    assert taken == 5 and len(set(T.bits(s[members]).tolist())) == 2


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_the_gpu_cases_tell_each_wrong_reading_from_the_truth(gpu_cases, variant):
    """A case that cannot tell a wrong reading from the right one proves nothing: each of the three differs from the truth,
    in the counts or in the edge list, on at least one (case, k) the GPU test runs."""
    told = []
    for name in sorted(gpu_cases.CASES):
        real, pred, idx, _ = gpu_cases.CASES[name]
        if len(real) > 300 and told:
            continue                                         # one telling case is enough; the large ones cost seconds
        for k in gpu_cases.ks_of(name):
            a = T.top_k(real, pred, k, idx)
            if variant == "ordered" and k > a["pairs"]:
                continue
            b = T.top_k(real, pred, k, idx, variant)
            if (a["hits"], a["pairs"], a["positives"]) != (b["hits"], b["pairs"], b["positives"]) or \
                    not np.array_equal(a["edges"], b["edges"]):
                told.append((name, k))
    print(variant, told)
    assert told, variant
    if variant == "ties_last":                               # and it changes a COUNT, not only the order of the list
        real, pred, idx, _ = gpu_cases.CASES["n257_levels_asym"]
        k = gpu_cases.tie_k("n257_levels_asym")
        assert T.top_k(real, pred, k, idx)["hits"] != T.top_k(real, pred, k, idx, variant)["hits"]
