"""The selection checks the ranking entries share (rank_common.hip: rank_check_args, rank_check_idx, rank_flag_error),
pinned across all of them at once, at n = 9 with an idx of 5 nodes.  Run with -m gpu.

Two populations.  The ORDERED entries of auc.hip (roc_auc, rank_metrics, rank_curves, decode_auc, decode_rank_metrics) range
over every ordered entry of the gathered submatrix: a repeated id is accepted and a permutation of all nodes is the whole
matrix.  The PAIR entries (topk_metrics, top_pairs, node_rank_metrics, two_means_split, threshold_pairs, auc_delong,
auc_delong_paired, auc_node_jackknife, graph_structure, hop_auc, class_auc) range over the pairs of positions a > b of a repeat-free idx of at least two nodes,
and their answer depends on the order of idx.  (mcgra_decode_scores takes neither idx nor labels: nothing of this applies.)

Every entry is called through its engine wrapper and reduced to plain Python values; the expected values are those of the
truth helpers of tests/ on the same selection.  The decode entries rank decode_scores(Z, mode); their Z is checked in every
row, so the "NaN outside the selection" case is run for the entries that read a score matrix only."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import ap_truth as AP
from tests import class_truth as CL
from tests import curve_truth as CT
from tests import delong_truth as DT
from tests import graph_structure_truth as GS
from tests import hop_truth as HT
from tests import node_jackknife_truth as NJ
from tests import node_rank_truth as NR
from tests import topk_truth as TK
from tests import two_means_truth as TM

pytestmark = pytest.mark.gpu

N = 9
IDX = [7, 2, 5, 0, 3]                       # 5 of the 9 nodes, not in order
OUTSIDE = (8, 6)                            # an entry whose row and column are both outside IDX
INSIDE = (5, 2)                             # positions a = 2 > b = 1 of IDX: an entry both populations read
PERM = [4, 8, 1, 6, 0, 3, 7, 2, 5]          # all nodes in another order
MODE = 0                                    # decode mode of the decode entries: sigmoid(relu(<z_i, z_j> - [i == j]))
THR = 0.5
HOPS = 2                                    # hop_auc: distances 1, 2 and beyond
CLASSES = (np.arange(N) % 3).tolist()       # class_auc: three node classes, strata "same" (same class, different classes)
AP_TOL = 34 * 2.0 ** -53                    # k_ap_terms: (T + 32) 2^-53 with T = 1 term per lane, + the truth's own rounding


def _inputs():
    rng = np.random.RandomState(20260)
    real = (rng.rand(N, N) < 0.4).astype(np.float32)
    real = np.maximum(real, real.T)
    pred = (rng.randint(0, 8, (N, N)) / 8.0).astype(np.float32)          # 8 levels in [0, 1): ties, and in range for 2-means
    pred_b = (rng.randint(0, 8, (N, N)) / 8.0).astype(np.float32)
    Z = rng.randn(N, 3).astype(np.float32)
    for m in (real, pred, pred_b, Z):
        m.setflags(write=False)
    return real, pred, pred_b, Z


REAL, PRED, PRED_B, Z = _inputs()


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


@pytest.fixture(scope="module")
def decoded(pkg):
    """decode_scores(Z, MODE) on the host: the matrix the decode entries rank (computed once, read-only)."""
    from mc_gra_amd import engine as E
    s = E.decode_scores(_dev(Z), MODE).cpu().numpy()
    s.setflags(write=False)
    return s


def _dev(x, pad=3):
    import torch
    t = torch.as_tensor(np.array(x), device="cuda:0")
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda:0")      # the padding is never read
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _bits(x):
    return None if x is None else int(np.float32(x).view(np.uint32))


def _auc_exact(p, q):
    """The AUC of per-level counts (levels ascending) as the nearest double of the exact rational."""
    P, Q = int(p.sum()), int(q.sum())
    if P == 0 or Q == 0:
        return float("nan")
    below = np.cumsum(q) - q
    return float(Fraction(sum(int(pi) * (2 * int(b) + int(qi)) for pi, b, qi in zip(p, below, q)), 2 * P * Q))


# ---- each entry: got(E, real, pred, idx) from the device, want(real, pred, idx) from the truth helpers; both plain values
def _got_curves(E, real, pred, idx):
    counts, roc, pr, best = E._rank_curves(real, pred, idx, True, True, True, True)
    pts = lambda c: tuple(tuple(t.cpu().numpy().tolist()) for t in c[:2]) + (tuple(_bits(v) for v in c[2].cpu().numpy()),)
    return counts, pts(roc), pts(pr), None if best is None else (best[0], best[1], best[2])


def _want_curves(real, pred, idx):
    w = CT.curves(real, pred, idx, True)
    pts = lambda c: tuple(tuple(np.asarray(t).tolist()) for t in c[:2]) + (tuple(_bits(v) for v in c[2]),)
    return tuple(w["counts"]), pts(w["roc"]), pts(w["pr"]), w["best"]


TOPK_KEYS = ("k", "positives", "hits", "pairs")
TM_KEYS = ("pairs", "iterations", "converged", "degenerate", "edges", "t", "c0", "c1", "positives", "hits")


def _got_top_pairs(E, real, pred, idx):
    pairs, scores, hits = E.top_pairs(pred, 3, idx, real)
    return pairs.cpu().numpy().tolist(), [_bits(s) for s in scores.cpu().numpy()], hits.cpu().numpy().tolist()


def _want_top_pairs(real, pred, idx):
    w = TK.top_k(real, pred, 3, idx)
    return w["edges"].tolist(), [_bits(s) for s in w["scores"]], w["edge_hits"].tolist()


def _got_two_means(E, real, pred, idx):
    g = E.two_means_split(pred, idx, real)
    return tuple(int(g[k]) for k in TM_KEYS) + (_bits(g["threshold"]), _bits(g["threshold_low"]))


def _want_two_means(real, pred, idx):
    w = TM.split(real, pred, idx)
    return tuple(int(w[k]) for k in TM_KEYS) + (_bits(w["threshold"]), _bits(w["threshold_low"]))


def _got_threshold_pairs(E, real, pred, idx):
    pairs, scores, hits = E.threshold_pairs(pred, THR, idx, real)
    return pairs.cpu().numpy().tolist(), [_bits(s) for s in scores.cpu().numpy()], hits.cpu().numpy().tolist()


def _want_threshold_pairs(real, pred, idx):
    pairs, scores, hits = TM.threshold_pairs(real, pred, THR, idx)
    return pairs.tolist(), [_bits(s) for s in scores], hits.tolist()


def _got_topk(E, real, pred, idx):
    g = E.topk_metrics(real, pred, None, idx)
    return tuple(g[k] for k in TOPK_KEYS) + (_bits(g["threshold"]),)


def _want_topk(real, pred, idx):
    w = TK.top_k(real, pred, None, idx)
    return tuple(w[k] for k in TOPK_KEYS) + (_bits(w["threshold"]),)


def _got_node_rank(E, real, pred, idx):
    g = E.node_rank_metrics(real, pred, idx)
    return np.stack([g[k].cpu().numpy() for k in ("positives", "wins", "ties", "hits", "first_rank")], 1).tolist()


def _got_graph_structure(E, real, pred, idx):
    g = E.graph_structure(pred, THR, idx, real)
    return [g[k] for k in GS.HEADER], [g[k].tolist() for k in GS.COLUMNS]


def _want_graph_structure(real, pred, idx):
    w = GS.ints(real, pred, THR, idx)
    return [w[k] for k in GS.HEADER], [w[k] for k in GS.COLUMNS]


def _want_class_auc(real, pred, idx):
    table, names = CL.strata(3, "same")
    return CL.ints(real, pred, CLASSES, idx, table, len(names), THR)


# name -> (population, reads a factor Z instead of a score matrix, got, want)
ENTRIES = {
    "roc_auc": ("ordered", False, lambda E, r, p, i: E.roc_auc(r, p, i), lambda r, p, i: _auc_exact(*AP.level_counts(r, p, i))),
    "rank_metrics": ("ordered", False, lambda E, r, p, i: E.rank_metrics(r, p, i),
                     lambda r, p, i: (_auc_exact(*AP.level_counts(r, p, i)), AP.from_counts_exact(*AP.level_counts(r, p, i)))),
    "rank_curves": ("ordered", False, _got_curves, _want_curves),
    "decode_auc": ("ordered", True, lambda E, r, z, i: E.decode_auc(r, z, MODE, i),
                   lambda r, s, i: _auc_exact(*AP.level_counts(r, s, i))),
    "decode_rank_metrics": ("ordered", True, lambda E, r, z, i: E.decode_rank_metrics(r, z, MODE, i),
                            lambda r, s, i: (_auc_exact(*AP.level_counts(r, s, i)), AP.from_counts_exact(*AP.level_counts(r, s, i)))),
    "topk_metrics": ("pairs", False, _got_topk, _want_topk),
    "top_pairs": ("pairs", False, _got_top_pairs, _want_top_pairs),
    "node_rank_metrics": ("pairs", False, _got_node_rank, lambda r, p, i: NR.per_node(r, p, i).tolist()),
    "two_means_split": ("pairs", False, _got_two_means, _want_two_means),
    "threshold_pairs": ("pairs", False, _got_threshold_pairs, _want_threshold_pairs),
    "auc_delong": ("pairs", False, lambda E, r, p, i: E.auc_delong(r, p, i)["ints"], lambda r, p, i: DT.ints(r, p, i)),
    "auc_delong_paired": ("pairs", False, lambda E, r, p, i: E.auc_delong_paired(r, p, _dev(PRED_B), i)["ints"],
                          lambda r, p, i: DT.paired_ints(r, p, PRED_B, i)),
    "auc_node_jackknife": ("pairs", False, lambda E, r, p, i: E.auc_node_jackknife(r, p, i)["ints"],
                           lambda r, p, i: NJ.ints(r, p, i)),
    "graph_structure": ("pairs", False, _got_graph_structure, _want_graph_structure),
    "hop_auc": ("pairs", False, lambda E, r, p, i: [list(c) for c in E.hop_auc(r, p, i, HOPS, THR)["ints"]],
                lambda r, p, i: HT.ints(r, p, i, HOPS, THR)),
    "class_auc": ("pairs", False, lambda E, r, p, i: [list(c) for c in E.class_auc(r, p, CLASSES, i, "same", THR)["ints"]],
                  _want_class_auc),
}
ALL = sorted(ENTRIES)
ORDERED = [e for e in ALL if ENTRIES[e][0] == "ordered"]
PAIRS = [e for e in ALL if ENTRIES[e][0] == "pairs"]
MATRIX = [e for e in ALL if not ENTRIES[e][1]]


def _same(got, want, what):
    """Equal values; a float pair within AP_TOL in its second value (rank_metrics: the AUC exactly, the AP to its bound)."""
    if isinstance(want, float):
        want, got = (want,), (got,)
    if isinstance(want, tuple) and all(isinstance(w, float) for w in want):
        assert len(got) == len(want), (what, got, want)
        for q, (g, w) in enumerate(zip(got, want)):
            tol = AP_TOL * abs(w) if q == 1 and not math.isnan(w) else 0.0
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= tol, (what, q, g, w)
        return
    assert got == want, (what, got, want)


def _call(pkg, entry, idx, real=REAL, pred=PRED, z=Z):
    from mc_gra_amd import engine as E
    _, factor, got, _ = ENTRIES[entry]
    return got(E, _dev(real), _dev(z if factor else pred), idx)


def _truth(entry, idx, decoded, real=REAL, pred=PRED):
    _, factor, _, want = ENTRIES[entry]
    return want(real, decoded if factor else pred, idx)


def _refused(pkg, entry, word, idx=IDX, **kw):
    """MCGRA_EINVAL with `word` in the reason."""
    with pytest.raises(pkg._lib.McgraError, match="mcgra error -1: .*" + word) as e:
        _call(pkg, entry, idx, **kw)
    print(entry, "->", e.value)


@pytest.mark.parametrize("entry", ALL)
def test_the_selection_against_the_truth(pkg, decoded, entry):
    got, want = _call(pkg, entry, IDX), _truth(entry, IDX, decoded)
    print(entry, got)
    _same(got, want, entry)


@pytest.mark.parametrize("bad", [N, -1])
@pytest.mark.parametrize("entry", ALL)
def test_an_id_outside_the_graph_is_refused(pkg, entry, bad):
    """k_auc_index reads idx alone, so nothing is dereferenced out of range before the refusal."""
    _refused(pkg, entry, "outside", idx=[7, 2, bad, 0, 3])


@pytest.mark.parametrize("entry", PAIRS)
def test_a_repeated_id_is_refused_by_the_pair_entries(pkg, entry):
    _refused(pkg, entry, "twice", idx=[7, 2, 5, 2, 3])


@pytest.mark.parametrize("entry", ORDERED)
def test_a_repeated_id_is_the_gathered_submatrix_for_the_ordered_entries(pkg, decoded, entry):
    idx = [7, 2, 5, 2, 3]
    _same(_call(pkg, entry, idx), _truth(entry, idx, decoded), entry)


@pytest.mark.parametrize("entry", ORDERED)
def test_a_permutation_of_all_nodes_has_the_bits_of_no_idx(pkg, entry):
    got, whole = _call(pkg, entry, PERM), _call(pkg, entry, None)
    assert got == whole or (got != got and whole != whole), (entry, got, whole)


@pytest.mark.parametrize("entry", PAIRS)
def test_a_permutation_of_all_nodes_is_that_order_for_the_pair_entries(pkg, decoded, entry):
    _same(_call(pkg, entry, PERM), _truth(entry, PERM, decoded), entry)


def _with(m, at, value):
    m = np.array(m)
    m[at] = value
    return m


@pytest.mark.parametrize("entry", MATRIX)
def test_a_nan_score_counts_only_inside_the_selection(pkg, decoded, entry):
    _refused(pkg, entry, "NaN or infinite", pred=_with(PRED, INSIDE, np.nan))
    _same(_call(pkg, entry, IDX, pred=_with(PRED, OUTSIDE, np.nan)), _truth(entry, IDX, decoded), entry)


@pytest.mark.parametrize("entry", ALL)
def test_a_label_of_one_half_counts_only_inside_the_selection(pkg, decoded, entry):
    _refused(pkg, entry, "neither 0 nor 1", real=_with(REAL, INSIDE, 0.5))
    _same(_call(pkg, entry, IDX, real=_with(REAL, OUTSIDE, 0.5)), _truth(entry, IDX, decoded), entry)


@pytest.mark.parametrize("entry", PAIRS)
def test_one_selected_node_is_refused_by_the_pair_entries(pkg, entry):
    _refused(pkg, entry, "bad argument", idx=[4])
