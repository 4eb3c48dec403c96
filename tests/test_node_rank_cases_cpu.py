"""CPU-side checks of the per-node ranking entry (mcgra_node_rank_metrics, engine.node_rank_metrics, main.py --per_node): the
truth helper against an independent brute-force definition, sklearn and the reference's loop; the C ABI, its binding and every
refusal that the arguments alone decide (the pointers here are never followed); the wrapper's refusals; the command line; and
the resolving power of the inputs tests/test_gpu_node_rank.py uses (no compute: there is no GPU here)."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from tests import node_rank_truth as T

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
    from tests import test_gpu_node_rank as G
    return G


# ---------------------------------------------------------------------------------------------------- truth helper
def _value(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def brute_row(real, pred, a, idx=None):
    """The definitions, literally, in O(c^2): float32 comparisons (-0.0 == +0.0 and distinct subnormals are what IEEE
    comparison gives when nothing flushes), the rank of each candidate by counting who is ahead of it."""
    ids = np.arange(len(pred)) if idx is None else np.asarray(idx)
    cand = [b for b in range(len(ids)) if b != a]
    s = [np.float32(pred[ids[a], ids[b]]) for b in cand]
    lab = [real[ids[a], ids[b]] == 1 for b in cand]
    c = len(cand)
    P = sum(lab)
    wins = sum(1 for i in range(c) for j in range(c) if lab[i] and not lab[j] and s[i] > s[j])
    ties = sum(1 for i in range(c) for j in range(c) if lab[i] and not lab[j] and s[i] == s[j])
    ahead = [sum(1 for j in range(c) if s[j] > s[i] or (s[j] == s[i] and cand[j] < cand[i])) for i in range(c)]
    hits = sum(1 for i in range(c) if lab[i] and ahead[i] < P)
    first = 1 + min(sum(1 for j in range(c) if s[j] > s[i]) for i in range(c) if lab[i]) if P else 0
    return P, wins, ties, hits, first


def _small_graphs():
    rng = np.random.RandomState(3)
    special = np.array([-2.0, -1e-45, -0.0, 0.0, 1e-45, 2e-45, 1e-38, 0.5], np.float32)
    for n in (2, 3, 5, 8, 12):
        for fam in range(4):
            real = (rng.rand(n, n) < (0.5 if fam == 3 else 0.3)).astype(np.float32)
            pred = (rng.randn(n, n).astype(np.float32), (rng.randint(0, 3, (n, n)) * 0.5).astype(np.float32),
                    special[rng.randint(0, len(special), (n, n))], np.zeros((n, n), np.float32))[fam]
            idx = None if fam % 2 == 0 or n < 4 else rng.permutation(n)[:max(2, n - 2)]
            yield real, pred, idx


def test_truth_agrees_with_the_brute_force_definition():
    seen_ties = seen_cut = 0
    for real, pred, idx in _small_graphs():
        n_idx = len(pred) if idx is None else len(idx)
        got = T.per_node(real, pred, idx)
        for a in range(n_idx):
            want = brute_row(real, pred, a, idx)
            assert tuple(got[a]) == want, (a, idx, got[a], want)
            seen_ties += want[2] > 0
            seen_cut += 0 < want[3] < want[0]
    assert seen_ties > 10 and seen_cut > 10


def test_truth_key_orders_like_float32_and_keeps_subnormals_apart():
    v = np.array([-np.float32(3e38), -1.0, -1e-38, -3e-45, -1e-45, -0.0, 0.0, 1e-45, 3e-45, 1e-38, 1.0, 3e38], np.float32)
    k = T.key(v)
    assert k[5] == k[6] and np.array_equal(np.sign(np.diff(k)), [1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1])
    assert _value(0x00000001) > 0 and T.key(_value(0x00000001)) > T.key(np.float32(0.0))


def test_truth_auc_is_sklearns_per_row():
    from sklearn import metrics
    rng = np.random.RandomState(11)
    n = 60
    real = (rng.rand(n, n) < 0.2).astype(np.float32)
    checked = 0
    for pred in (rng.randn(n, n).astype(np.float32), (rng.randint(0, 4, (n, n)) * 0.25).astype(np.float32)):
        cols = T.per_node(real, pred)
        auc = T.rates(cols, n)["auc"]
        for a in range(n):
            y, s = np.delete(real[a], a), np.delete(pred[a], a)
            if 0 < y.sum() < len(y):
                assert abs(auc[a] - metrics.roc_auc_score(y, s)) <= 1e-12, a
                checked += 1
            else:
                assert np.isnan(auc[a])
    assert checked > 100


def test_truth_mean_rank_is_the_reference_loop():
    """calc_mrr, the direct loop of the formula: the mean over the true samples of (false samples above it + 1) / #false."""
    rng = np.random.RandomState(12)
    n = 40
    real = (rng.rand(n, n) < 0.25).astype(np.float32)
    pred = (rng.randint(0, 5, (n, n)) * 0.2).astype(np.float32)
    got = T.rates(T.per_node(real, pred), n)["mean_rank"]
    for a in range(n):
        y, s = np.delete(real[a], a), np.delete(pred[a], a)
        false, true = s[y == 0], s[y == 1]
        if len(false) == 0 or len(true) == 0:
            assert np.isnan(got[a])
            continue
        total = 0
        for x in true:
            total += (int((false > x).sum()) + 1) / len(false)
        assert abs(got[a] - total / len(true)) <= 1e-12, a


def test_truth_on_a_row_worked_by_hand():
    """Row 0 of 6 nodes: candidates 1..5 with scores .5 .5 .9 .5 .1 and labels 1 0 0 1 0: best first 3 | 1 2 4 | 5."""
    pred = np.zeros((6, 6), np.float32); pred[0] = [7, .5, .5, .9, .5, .1]
    real = np.zeros((6, 6), np.float32); real[0] = [1, 1, 0, 0, 1, 0]
    assert T.row(real, pred, 0) == (2, 2, 2, 1, 2)          # P, wins (each beats 5), ties (each ties 2), hits (3, 1), first
    r = T.rates([T.row(real, pred, 0)], 6)
    assert r["auc"][0] == 6 / 12 and r["r_precision"][0] == .5 and r["reciprocal_rank"][0] == .5 and r["mean_rank"][0] == 4 / 6
    assert T.row(real, pred, 0, idx=[0, 4, 2, 1]) == (2, 0, 2, 1, 1)   # nodes 4 2 1 by position: all .5, labels 1 0 1
    assert T.row(real, pred, 1) == (0, 0, 0, 0, 0)


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_node_rank_entry_is_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    from mc_gra_amd import engine as E
    lib = ctypes.CDLL(LIB)
    s = "mcgra_node_rank_metrics"
    assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s)
    assert getattr(pkg._lib.lib, s).restype is ctypes.c_int and len(getattr(pkg._lib.lib, s).argtypes) == 9
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    assert callable(E.node_rank_metrics) and hasattr(E.node_rank_metrics, "__wrapped__")      # the device guard
    assert "gcn_parameterized.py:18-26" in E.node_rank_metrics.__doc__


def test_constants_agree_between_header_kernel_engine_and_tests(pkg, gpu_cases):
    from mc_gra_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "mcgra.h")).read()
    src = open(os.path.join(ROOT, "mc-gra_amd", "csrc", "node_rank.hip")).read()
    bound = int(re.search(r"#define MCGRA_NODE_RANK_MAX_NIDX (\d+)", hdr).group(1))
    threads = int(re.search(r"constexpr int NODE_RANK_THREADS = (\d+);", src).group(1))
    smallest = int(re.search(r"constexpr int NODE_RANK_MIN_CLASS = (\d+);", src).group(1))
    launched = [bound if c == "MCGRA_NODE_RANK_MAX_NIDX" else int(c) for c in re.findall(r"node_rank_launch<(\w+)>\(st", src)]
    assert bound >= 16384 and E.NODE_RANK_MAX_NIDX == bound == gpu_cases.MAX_NIDX
    assert E.NODE_RANK_THREADS == threads == gpu_cases.THREADS
    assert list(E.NODE_RANK_CLASSES) == launched == list(gpu_cases.CLASSES) and launched[0] == smallest and launched[-1] == bound
    assert all(b == 2 * a for a, b in zip(launched, launched[1:]))
    assert tuple(E.NODE_RANK_DEGREE_BINS) == T.DEGREE_BINS


def test_node_rank_entry_refuses_before_touching_a_device(pkg):
    """Every check that needs only the arguments: MCGRA_EINVAL (-1) / MCGRA_ENOSUP (-3) with pointers that are never followed
    and no GPU in the machine."""
    from mc_gra_amd import engine as E
    L, p = pkg._lib.lib, ctypes.c_void_p(64)

    def call(n=8, ldl=8, lds=8, idx=None, n_idx=None, lab=p, sc=p, out=p):
        return L.mcgra_node_rank_metrics(None, n, lab, ldl, sc, lds, idx, n if n_idx is None else n_idx, out)

    for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(ldl=7), dict(lds=7), dict(idx=p, n_idx=1), dict(idx=p, n_idx=0),
               dict(idx=p, n_idx=-5), dict(lab=None), dict(sc=None), dict(out=None)):
        assert call(**kw) == -1 and b"node_rank_metrics" in L.mcgra_last_error(), kw
    big = E.NODE_RANK_MAX_NIDX + 1
    assert call(n=big, ldl=big, lds=big) == -3 and str(E.NODE_RANK_MAX_NIDX).encode() in L.mcgra_last_error()
    assert call(n=10 ** 6, ldl=10 ** 6, lds=10 ** 6, idx=p, n_idx=big) == -3
    assert b"node_rank_metrics" in L.mcgra_last_error()
    with pytest.raises(pkg._lib.McgraNotSupported, match=str(E.NODE_RANK_MAX_NIDX)):
        pkg._lib.check(call(idx=p, n_idx=big, n=big, ldl=big, lds=big))
    assert call(n=big, ldl=big - 1, lds=big) == -1                     # a bad argument is named before the capacity


def test_engine_entry_refuses_wrong_shapes_and_host_tensors(pkg):
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for real, pred in ((wide, wide), (sq, other), (sq, wide), (torch.zeros(5), sq)):
        with pytest.raises(AssertionError):
            E.node_rank_metrics.__wrapped__(real, pred)
    with pytest.raises(ValueError, match="device tensors"):
        E.node_rank_metrics(sq, sq)                                       # a host tensor: refused before anything is called


def test_node_rates_of_the_wrapper_are_the_truths(pkg):
    """The host half of the wrapper (the rates and the summary from the integer columns) needs no device."""
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(8)
    n = 70
    real = np.zeros((n, n), np.float32)
    for a in range(n):                                                  # degrees 0 .. 44: every bin of by_degree is filled
        real[a, np.delete(np.arange(n), a)[rng.permutation(n - 1)[:a % 45]]] = 1
    real[4] = 0; real[9] = 1
    pred = (rng.randint(0, 4, (n, n)) * 0.25 + real * 0.25).astype(np.float32)
    cols = T.per_node(real, pred)
    rates, summary = E._node_rates(cols, n)
    want = T.rates(cols, n)
    for r in T.RATES:
        assert rates[r].dtype == np.float64 and np.array_equal(np.isnan(rates[r]), np.isnan(want[r]))
        assert np.array_equal(rates[r][~np.isnan(want[r])], want[r][~np.isnan(want[r])]), r
    assert np.isnan(rates["auc"][4]) and np.isnan(rates["auc"][9]) and rates["r_precision"][9] == 1.0
    assert np.isnan(rates["reciprocal_rank"][4]) and rates["reciprocal_rank"][9] == 1.0
    ws = T.summary(cols, n)
    assert repr(summary) == repr(ws)
    assert sum(b[2] for b in summary["by_degree"]) == int((cols[:, 0] > 0).sum()) and all(b[2] > 0 for b in summary["by_degree"])


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_per_node_is_absent_by_default_and_evaluate_only(pkg, capsys):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    p = M.build_parser()
    assert p.parse_args([]).per_node is None
    assert p.parse_args(["--per_node", "n.npz"]).per_node == "n.npz"
    for mode in ("notrain_test", "prepare"):
        with pytest.raises(SystemExit):
            p.parse_args(["--per_node", "n.npz", "--mode", mode])
        assert mode in capsys.readouterr().err
    assert "--per_node" in M.__doc__
    with pytest.raises(SystemExit, match="evaluate only"):
        M._run(argparse.Namespace(per_node="n.npz", mode="prepare"), 0, 1)
    calls = []
    R.check_per_node_args(argparse.Namespace(per_node=None, mode="prepare"), calls.append)
    R.check_per_node_args(argparse.Namespace(mode="prepare"), calls.append)
    R.check_per_node_args(argparse.Namespace(per_node="x", mode="evaluate"), calls.append)
    assert calls == []


def test_per_node_is_hidden_from_the_parameter_line_when_unset(pkg):
    """The log's parameter line prints reports.shown_parameters(args): per_node is in it exactly when --per_node is set, and each
    of the flags that are hidden while unset brings exactly its own names."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    older = ("ap", "topk", "save_edges", "curves", "per_node", "binarize", "save_graph")
    args = M.build_parser().parse_args([])
    assert all(f" {k}=" in str(args) for k in older)
    assert not any(f" {k}=" in str(R.shown_parameters(args)) for k in older)
    for argv, own in ((["--per_node", "n.npz"], ("per_node",)), (["--ap"], ("ap",)), (["--topk", "0"], ("topk", "save_edges")),
                      (["--topk", "5", "--save_edges", "e.npz"], ("topk", "save_edges")), (["--curves", "c.npz"], ("curves",)),
                      (["--binarize"], ("binarize", "save_graph"))):
        args = M.build_parser().parse_args(argv)
        text = str(R.shown_parameters(args))
        assert [k for k in older if f" {k}=" in text] == list(own), (argv, text)
        assert all(f" {k}={getattr(args, k)!r}" in text for k in own)


# --------------------------------------------------------------------------------- the inputs of the GPU test cases
def test_the_gpu_lengths_cover_every_path_of_the_launcher(gpu_cases):
    L, C, t = gpu_cases.LENGTHS, gpu_cases.CLASSES, gpu_cases.THREADS
    assert {1, 2, 63, 64, 65, t - 1, t, t + 1} <= set(L)
    for c in C[:-1]:
        assert c in L and c + 1 in L                                   # the last length of a class, the first of the next
    assert C[-1] == gpu_cases.MAX_NIDX                                 # the last class ends at the capacity case: c = MAX_NIDX - 1
    assert max(L) + 1 <= gpu_cases.MAX_NIDX


def test_the_gpu_cases_hold_what_they_are_named_for(gpu_cases):
    C = gpu_cases.CASES
    b = {k: T.key(v[1]) for k, v in C.items()}
    assert len(np.unique(C["equal"][1])) == 1 and len(np.unique(C["levels4_ties"][1])) == 4
    z = C["signed_zeros"][1].view(np.uint32)
    assert (z == 0x80000000).any() and (z == 0).any() and len(np.unique(b["signed_zeros"])) == 1
    s = C["subnormals"][1].view(np.uint32)
    assert ((s & 0x7f800000) == 0).sum() > ((s & 0x7fffffff) == 0).sum() > 0 and len(np.unique(b["subnormals"])) >= 5
    assert (C["negative"][1] < 0).all()
    d = C["distinct_asym"][1]
    assert len(np.unique(d)) == d.size and (d < 0).any() and (d > 0).any()
    real, pred, _, _ = C["row_kinds_dense"]
    n = len(real)
    cols = T.per_node(real, pred)
    assert cols[3, 0] == 0 and cols[5, 0] == n - 1 and abs(np.median(cols[:, 0]) - n / 2) < n / 8
    assert (cols[:, 2] > 0).sum() > n / 2                              # and its rows tie
    real, pred, idx, pad = C["padded_rows"]
    assert pad == 3 and idx is None
    real, pred, idx, _ = C["subset_idx"]
    assert len(idx) < len(real) and len(set(idx.tolist())) == len(idx) and not np.array_equal(idx, np.sort(idx))
    real, pred, idx, _ = C["junk_outside_selection"]
    off = np.ones(len(real), bool); off[idx] = False
    sel = real[np.ix_(idx, idx)][~np.eye(len(idx), dtype=bool)]
    assert set(np.unique(sel).tolist()) <= {0.0, 1.0} and off.sum() > 50
    for block in (real[:, off], real[off]):                            # nothing outside the selection is a valid label
        assert not np.isin(block, (0.0, 1.0)).any() and np.isnan(block).any() and (block == 2.0).any()
    diag = np.diagonal(real)[idx]
    assert (diag == 2.0).any() and np.isnan(diag).any()


def test_the_tie_case_has_a_tie_group_across_the_cut_of_hits(gpu_cases):
    """Guard: a row whose P-th and (P + 1)-th ranked candidates share one key, so that `hits` depends on the tie rule."""
    real, pred, idx, _ = gpu_cases.CASES["levels4_ties"]
    rows = gpu_cases.tie_rows(real, pred, idx)
    assert len(rows) >= 10
    told = 0
    for a in rows:
        k, lab, b = T.candidates(real, pred, a, idx)
        told += T.counts(k, lab, b)[3] != T.counts(k, lab, -b)[3]      # ties taken from the other end: other hits
    assert told >= 5, told


def test_the_permuted_case_tells_position_order_from_node_order(gpu_cases):
    """Guard: a row where breaking ties by node id and by position in idx give different hits."""
    real, pred, idx, _ = gpu_cases.CASES["permuted_idx"]
    assert idx is not None and sorted(idx.tolist()) == list(range(len(real))) and not np.array_equal(idx, np.sort(idx))
    by_pos, by_node = T.per_node(real, pred, idx), T.per_node(real, pred, idx, by="node")
    assert np.array_equal(by_pos[:, :3], by_node[:, :3]) and (by_pos[:, 3] != by_node[:, 3]).sum() >= 5


def test_the_asymmetric_case_tells_rows_from_columns(gpu_cases):
    """Guard: a row whose counts differ from its column's (the transposed matrices' row)."""
    real, pred, idx, _ = gpu_cases.CASES["distinct_asym"]
    assert not np.array_equal(pred, pred.T) and not np.array_equal(real, real.T)
    rows, cols = T.per_node(real, pred, idx), T.per_node(real.T, pred.T, idx)
    assert (rows != cols).any(1).sum() >= len(real) // 2
    real, pred, idx, _ = gpu_cases.CASES["levels4_ties"]
    assert np.array_equal(real, real.T) and (T.per_node(real, pred, idx) != T.per_node(real, pred.T, idx)).any()
