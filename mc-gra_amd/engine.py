"""Thin host wrapper over the C-ABI attack engine and standalone ops.

PyTorch is used only as plumbing: it owns the caller-side device buffers and
the HIP stream.  All arithmetic happens in libmcgra_hip.so.
"""
import ctypes as C
import math
import statistics
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from ._lib import AttackConfig, check, lib


import functools


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tensors(args):
    for a in args:
        if isinstance(a, torch.Tensor):
            yield a
        elif isinstance(a, (list, tuple)):
            yield from _tensors(a)


def _need_device(op, *args):
    """ValueError for a tensor that is not in device memory: the C ABI would follow its data_ptr() on the GPU."""
    for t in _tensors(args):
        if not t.is_cuda:
            raise ValueError(f"{op}: a {t.device.type} tensor of shape {tuple(t.shape)}; the standalone ops take device tensors")


def _on_operand_device(fn, every=False):
    """Standalone ops launch on the device (and its current stream) of their first tensor argument, not on
    whatever device happens to be current.  A first argument that is not on a device is refused before anything is called."""
    @functools.wraps(fn)
    def run(first, *a, **k):
        _need_device(fn.__name__, first, *((*a, *k.values()) if every else ()))
        with torch.cuda.device(first.device):
            return fn(first, *a, **k)
    return run


def _device_operands(fn):
    """_on_operand_device for the wrappers that hand data_ptr() of EVERY tensor argument to the C ABI (the metrics move theirs
    to the first operand's device instead): any of them on the host is refused."""
    return _on_operand_device(fn, every=True)


def _f32(x):
    """An operand as the C ABI reads it: float32, contiguous, no autograd history (the reference's functions take any float
    tensor).  A float32 contiguous tensor is passed through as it is."""
    return None if x is None else x.detach().to(dtype=torch.float32).contiguous()


def _strided_f32(op, *ts):
    """The GEMM family passes strides on and may write into `out`: nothing is converted (a copy would break out= aliasing),
    so anything the kernels cannot read as float32 rows is refused."""
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise ValueError(f"{op}: {t.dtype} operand; the GEMM family takes float32")
        if t.stride(-1) != 1:
            raise ValueError(f"{op}: operand of shape {tuple(t.shape)} with strides {tuple(t.stride())}; the inner stride must be 1")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev_f32(x, device):
    if isinstance(x, torch.Tensor):
        if x.is_sparse:
            x = x.to_dense()
        return x.detach().to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)), device=device)


def _dev_i32(x, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.int32)), device=device)


# ------------------------------------------------------------- standalone ops
@_device_operands
def sgemm(A, B, ta=False, tb=False, alpha=1.0, beta=0.0, out=None):
    """torch.mm on the fp32 MFMA kernel (mcgra_sgemm)."""
    _strided_f32("sgemm", A, B, out)
    m = A.shape[1] if ta else A.shape[0]
    k = A.shape[0] if ta else A.shape[1]
    n = B.shape[0] if tb else B.shape[1]
    assert (B.shape[1] if tb else B.shape[0]) == k
    if out is None:
        out = torch.zeros(m, n, device=A.device, dtype=torch.float32)
    check(lib.mcgra_sgemm(_stream(), int(ta), int(tb), m, n, k, float(alpha), _p(A), A.stride(0), _p(B),
                          B.stride(0), float(beta), _p(out), out.stride(0)))
    return out


@_device_operands
def ssyrk_lower(A, out=None):
    """C = A A^T on the lower tile storage (128 x 128 tiles on or below the diagonal); the rest of
    `out` is left untouched (mcgra_ssyrk_lower)."""
    _strided_f32("ssyrk_lower", A, out)
    n, k = A.shape
    if out is None:
        out = torch.zeros(n, n, device=A.device, dtype=torch.float32)
    check(lib.mcgra_ssyrk_lower(_stream(), n, k, 1.0, _p(A), A.stride(0), 0.0, _p(out), out.stride(0)))
    return out


@_device_operands
def ssymm_lower(S, B, beta=0.0, out=None):
    """C = S B with symmetric S read from its lower tile storage only (mcgra_ssymm_lower)."""
    _strided_f32("ssymm_lower", S, B, out)
    n, m = S.shape[0], B.shape[1]
    if out is None:
        out = torch.zeros(n, m, device=S.device, dtype=torch.float32)
    check(lib.mcgra_ssymm_lower(_stream(), n, m, 1.0, _p(S), S.stride(0), _p(B), B.stride(0), float(beta), _p(out),
                                out.stride(0)))
    return out


@_device_operands
def ssymm_split_bf16(S, X, rowsub=None, out=None):
    """C = S (X - rowsub 1^T)^T through the 3-plane bf16 split kernel (mcgra_ssymm_split_bf16); S symmetric."""
    _strided_f32("ssymm_split_bf16", S, X, rowsub, out)
    n = S.shape[0]
    if out is None:
        out = torch.empty(n, n, device=S.device, dtype=torch.float32)
    check(lib.mcgra_ssymm_split_bf16(_stream(), n, _p(S), S.stride(0), _p(X), X.stride(0), _p(rowsub), _p(out), out.stride(0)))
    return out


@_device_operands
def sgemm_skinny_x3(M, V, out=None):
    """M @ V (M [n x n], V [n x nc], nc <= 48) on the three-plane bf16 kernel of the fused step's forward
    (mcgra_sgemm_skinny_x3); M's rows must be 16-byte aligned (stride a multiple of 4)."""
    _strided_f32("sgemm_skinny_x3", M, V, out)
    n, nc = M.shape[0], V.shape[1]
    assert M.shape[1] == n and V.shape[0] == n
    if out is None:
        out = torch.empty(n, nc, device=M.device, dtype=torch.float32)
    check(lib.mcgra_sgemm_skinny_x3(_stream(), n, _p(M), M.stride(0), _p(V), V.stride(0), nc, _p(out), out.stride(0)))
    return out


@_device_operands
def ssymm_split_f16(S, X, rowsub=None, out=None):
    """The same product through the 2-plane fp16 split kernel (mcgra_ssymm_split_f16); S symmetric."""
    _strided_f32("ssymm_split_f16", S, X, rowsub, out)
    n = S.shape[0]
    if out is None:
        out = torch.empty(n, n, device=S.device, dtype=torch.float32)
    check(lib.mcgra_ssymm_split_f16(_stream(), n, _p(S), S.stride(0), _p(X), X.stride(0), _p(rowsub), _p(out), out.stride(0)))
    return out


@_device_operands
def normalize_adj_tensor(adj):
    """utils.normalize_adj_tensor, dense branch (utils.py:211-230)."""
    adj = _f32(adj)
    out = torch.empty_like(adj)
    check(lib.mcgra_normalize_adj(_stream(), adj.shape[0], _p(adj), _p(out)))
    return out


@_device_operands
def get_modified_adj(adj_changes, ori_adj, n):
    adj_changes, ori_adj = _f32(adj_changes), _f32(ori_adj)
    out = torch.empty(n, n, device=adj_changes.device, dtype=torch.float32)
    check(lib.mcgra_get_modified_adj(_stream(), n, _p(adj_changes), _p(ori_adj), _p(out)))
    return out


@_device_operands
def pack_tril(M):
    """M[tril_indices(n, n, -1)]: the inverse data movement of get_modified_adj (mcgra_pack_tril)."""
    M = _f32(M)
    n = M.shape[0]
    out = torch.empty(n * (n - 1) // 2, device=M.device, dtype=torch.float32)
    check(lib.mcgra_pack_tril(_stream(), n, _p(M), M.stride(0), _p(out)))
    return out


@_device_operands
def info_entropy(prob):
    prob = _f32(prob)
    out = torch.zeros(1, device=prob.device, dtype=torch.float32)
    check(lib.mcgra_info_entropy(_stream(), prob.shape[0], _p(prob), _p(out)))
    return out[0]


@_device_operands
def dot_product_decode(Z):
    Z = _f32(Z)
    n, d = Z.shape
    out = torch.empty(n * (n - 1) // 2, device=Z.device, dtype=torch.float32)
    check(lib.mcgra_dot_product_decode(_stream(), n, d, _p(Z), _p(out)))
    return out


@_device_operands
def dot_product_decode2(Z, mode):
    """PGDAttack.dot_product_decode2 (topology_attack.py:421-467); `mode` as topology_attack._decode_mode gives it."""
    Z = _f32(Z)
    n, d = Z.shape
    out = torch.empty(n, n, device=Z.device, dtype=torch.float32)
    check(lib.mcgra_dot_product_decode2(_stream(), n, d, _p(Z), int(mode), _p(out)))
    return out


@_device_operands
def linear_hsic(X, Y):
    X, Y = _f32(X), _f32(Y)
    out = torch.zeros(1, device=X.device, dtype=torch.float32)
    check(lib.mcgra_linear_hsic(_stream(), X.shape[0], X.shape[1], Y.shape[1], _p(X), _p(Y), _p(out)))
    return out[0]


@_device_operands
def mutual_information(X, Y, want_grad=False):
    """utils.MutualInformation(sigma=0.4, num_bins=X.shape[1], normalize=True)(X, Y)[0] (utils.py:980-1049); want_grad: also
    its gradients w.r.t. X and Y (mcgra_mutual_information)."""
    m, c = X.shape
    assert Y.shape == X.shape
    X, Y = _f32(X), _f32(Y)
    out = torch.zeros(1, device=X.device, dtype=torch.float32)
    gX = torch.empty(m, c, device=X.device, dtype=torch.float32) if want_grad else None
    gY = torch.empty(m, c, device=X.device, dtype=torch.float32) if want_grad else None
    check(lib.mcgra_mutual_information(_stream(), m, c, _p(X), _p(Y), _p(out), _p(gX), _p(gY)))
    return (out[0], gX, gY) if want_grad else out[0]


@_device_operands
def hsic_regular(x, y, sigma):
    """hsic.hsic_regular (hsic.py:117-124) with a given sigma."""
    x, y = _f32(x), _f32(y)
    out = torch.zeros(1, device=x.device, dtype=torch.float32)
    check(lib.mcgra_hsic_regular(_stream(), x.shape[0], x.shape[1], y.shape[1], _p(x), _p(y), float(sigma), _p(out)))
    return out[0]


@_device_operands
def hsic_normalized(x, y, sigma):
    """hsic.hsic_normalized (hsic.py:127-135) with a given sigma."""
    x, y = _f32(x), _f32(y)
    out = torch.zeros(1, device=x.device, dtype=torch.float32)
    check(lib.mcgra_hsic_normalized(_stream(), x.shape[0], x.shape[1], y.shape[1], _p(x), _p(y), float(sigma), _p(out)))
    return out[0]


@_device_operands
def hsic_regular2(x, y, sigma_x, sigma_y, normalized=False):
    """hsic.hsic_regular / hsic_normalized with one bandwidth per operand, as kernelmat takes them for sigma=None
    (hsic.py:39-41; mcgra_hsic_regular2)."""
    x, y = _f32(x), _f32(y)
    out = torch.zeros(1, device=x.device, dtype=torch.float32)
    check(lib.mcgra_hsic_regular2(_stream(), x.shape[0], x.shape[1], y.shape[1], _p(x), _p(y), float(sigma_x), float(sigma_y),
                                  int(bool(normalized)), _p(out)))
    return out[0]


@_device_operands
def mmd(x, y, sigma_x, sigma_y, sigma_xy):
    """hsic.mmd (hsic.py:68-89) with its three bandwidths given (mcgra_mmd); x [mx x d], y [my x d]."""
    x, y = _f32(x), _f32(y)
    out = torch.zeros(1, device=x.device, dtype=torch.float32)
    check(lib.mcgra_mmd(_stream(), x.shape[0], y.shape[0], x.shape[1], _p(x), _p(y), float(sigma_x), float(sigma_y),
                        float(sigma_xy), _p(out)))
    return out[0]


@_device_operands
def mmd_pxpy_pxy(x, y, sigma_x, sigma_y):
    """hsic.mmd_pxpy_pxy (hsic.py:92-114) with its two bandwidths given (mcgra_mmd_pxpy_pxy)."""
    x, y = _f32(x), _f32(y)
    out = torch.zeros(1, device=x.device, dtype=torch.float32)
    check(lib.mcgra_mmd_pxpy_pxy(_stream(), x.shape[0], x.shape[1], y.shape[1], _p(x), _p(y), float(sigma_x), float(sigma_y),
                                 _p(out)))
    return out[0]


@_device_operands
def mse(X, Y):
    X, Y = _f32(X), _f32(Y)
    out = torch.zeros(1, device=X.device, dtype=torch.float32)
    check(lib.mcgra_mse(_stream(), X.numel(), _p(X), _p(Y), _p(out)))
    return out[0]


def _rows_f32(t, dev):
    """t as float32 rows on dev (unit stride inside a row; a padded leading dimension is kept)."""
    t = t.detach()
    if t.device != dev or t.dtype != torch.float32 or t.stride(1) != 1:
        t = t.to(device=dev, dtype=torch.float32).contiguous()
    return t


def _node_ids(idx, dev):
    if idx is None:
        return None
    ix = idx.detach() if isinstance(idx, torch.Tensor) else torch.as_tensor(np.asarray(idx, dtype=np.int64))
    return ix.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()


def _ranked(idx, first, *more, factor=None):
    """What every ranking wrapper starts with.  first and more: the n x n matrices of the call (an entry of more may be None,
    e.g. an optional real); factor: a thin n x d factor instead of a score matrix.  Returns them as float32 rows on first's
    device, in that order (factor last), then the node ids on that device (or None), n and the number of selected nodes."""
    dev, n = first.device, first.shape[0]
    mats = (first,) + more
    assert first.dim() == 2 and all(m is None or tuple(m.shape) == (n, n) for m in mats) and \
        (factor is None or (factor.dim() == 2 and factor.shape[0] == n)), \
        [None if m is None else tuple(m.shape) for m in mats + (factor,)]
    ix = _node_ids(idx, dev)
    mats = [None if m is None else _rows_f32(m, dev) for m in mats + (() if factor is None else (factor,))]
    return (*mats, ix, n, ix.numel() if ix is not None else n)


@_on_operand_device
def roc_auc(real, pred, idx=None):
    """main.metric_pool (main.py:66-75): roc_curve + auc of real[idx][:, idx] against pred[idx][:, idx], exactly, without
    gathering the submatrix (mcgra_roc_auc).  real, pred: n x n on the device; idx: node ids (tensor, array or list,
    repeats allowed) or None for all nodes.  NaN when one class is absent; McgraError for a NaN / inf score or a label
    other than 0 / 1."""
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    out = C.c_double()
    check(lib.mcgra_roc_auc(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, C.byref(out)))
    return out.value


@_on_operand_device
def decode_auc(real, Z, mode, idx=None):
    """roc_auc(real, decode_scores(Z, mode), idx), bit for bit, without the n x n score matrix (mcgra_decode_auc): the AUC
    of a prior's decode, main.py:412-437.  Z: n x d, d <= 128; mode 0, 1, 2 or 4 (McgraNotSupported otherwise)."""
    real, Z, ix, n, rows = _ranked(idx, real, factor=Z)
    out = C.c_double()
    check(lib.mcgra_decode_auc(_stream(), n, Z.shape[1], _p(Z), Z.stride(0), int(mode), _p(real), real.stride(0), _p(ix), rows,
                               C.byref(out)))
    return out.value


def _rank_metrics(real, pred, idx, want_auc, want_ap):
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    auc, ap = C.c_double(), C.c_double()
    check(lib.mcgra_rank_metrics(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows,
                                 C.byref(auc) if want_auc else None, C.byref(ap) if want_ap else None))
    return auc.value, ap.value


@_on_operand_device
def rank_metrics(real, pred, idx=None):
    """(roc_auc(real, pred, idx), average precision of the same ranking) from one sort of the selected entries
    (mcgra_rank_metrics).  The AUC is bit for bit roc_auc's; the average precision is
    sklearn.metrics.average_precision_score(real[idx][:, idx].reshape(-1), pred[idx][:, idx].reshape(-1)): ties share one
    term, summed in a fixed order (the same bits on every call).  Arguments and refusals as roc_auc.  No selected
    positive: (NaN, NaN); no selected negative: (NaN, 1.0)."""
    return _rank_metrics(real, pred, idx, True, True)


@_on_operand_device
def average_precision(real, pred, idx=None):
    """The second value of rank_metrics alone (the pair count of the AUC is not run)."""
    return _rank_metrics(real, pred, idx, False, True)[1]


def _ratio(num, den):
    return num / den if den else float("nan")


@_on_operand_device
def topk_metrics(real, pred, k=None, idx=None):
    """The recovered graph in numbers (mcgra_topk_metrics): of the k best-scored unordered node pairs of pred within idx, how
    many are edges of real.  The candidates are the pairs of positions a > b of idx (REPEAT-FREE node ids; None: all nodes in
    order) with score pred[idx[a], idx[b]] and label real[idx[a], idx[b]] -- the strict lower triangle of the gathered
    submatrix, also for an asymmetric pred -- ranked by score descending (float32 values, -0.0 == +0.0), ties by ascending
    packed position a (a - 1) / 2 + b.  k None or 0: the true edge count among the candidates (then precision = recall = f1).
    Returns {"k", "positives" (P), "hits" (TP), "pairs" (m), "precision" TP / k, "recall" TP / P, "f1" 2 TP / (k + P),
    "threshold" (the k-th pair's score)}: exact integers, one float64 division each, NaN for a zero denominator (and for
    the threshold when k = 0).  McgraError for k > m, a repeated or out-of-range id, a selected NaN / inf score or a selected
    label other than 0 / 1."""
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    counts, thr = (C.c_int64 * 4)(), C.c_float(float("nan"))
    check(lib.mcgra_topk_metrics(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, int(k or 0),
                                 counts, C.byref(thr)))
    kk, P, tp, m = (int(c) for c in counts)
    return {"k": kk, "positives": P, "hits": tp, "pairs": m, "precision": _ratio(tp, kk), "recall": _ratio(tp, P),
            "f1": _ratio(2 * tp, kk + P), "threshold": thr.value}


@_on_operand_device
def top_pairs(pred, k, idx=None, real=None):
    """The recovered graph as an edge list (mcgra_top_pairs): (pairs [k, 2] int64, scores [k] float32), and hits [k] bool when
    real is given -- the k best pairs of topk_metrics' ranking, best first (ties by ascending packed position), so the first
    k' rows are the answer for k'.  pairs[i] = (idx[a], idx[b]), a > b; scores[i] = pred[pairs[i, 0], pairs[i, 1]], the bits as
    stored; hits[i] = (real[pairs[i, 0], pairs[i, 1]] == 1).  Device tensors.  1 <= k <= m; refusals as topk_metrics."""
    pred, real, ix, n, rows = _ranked(idx, pred, real)
    k = int(k)
    pairs = torch.empty(max(k, 0), 2, device=pred.device, dtype=torch.int64)
    scores = torch.empty(max(k, 0), device=pred.device, dtype=torch.float32)
    hits = None if real is None else torch.empty(max(k, 0), device=pred.device, dtype=torch.uint8)
    check(lib.mcgra_top_pairs(_stream(), n, _p(pred), pred.stride(0), _p(ix), rows, k,
                              _p(real), real.stride(0) if real is not None else 0, _p(pairs), _p(scores), _p(hits)))
    return (pairs, scores) if real is None else (pairs, scores, hits.view(torch.bool))


TWO_MEANS_SCALE = 2.0 ** -28      # one unit of the quantised scores of mcgra_two_means_split


@_on_operand_device
def two_means_split(pred, idx=None, real=None, max_iter=256):
    """Which candidates are edges, decided from the scores alone (mcgra_two_means_split; the reference's PGDAttack.kmeans,
    baseline.py:88-109, exact and repeatable): Lloyd's 2-means on q = rint(s 2^28) of the candidates of topk_metrics (the pairs
    of positions a > b of a REPEAT-FREE idx; None: all nodes), in integers, from t_0 = floor((min + max) / 2) + 1, a value
    equidistant from the two centres going low.  Scores must lie in [0, 16).  Returns {"pairs" (m), "iterations", "converged",
    "degenerate", "edges" (the size of the high cluster), "threshold" (its smallest score: the high cluster is exactly
    pred >= threshold, what threshold_pairs returns), "threshold_low" (the largest score of the low cluster), "center_low",
    "center_high" (c 2^-28 as Python floats), "t", "c0", "c1" (the integers)}; with real also "positives", "hits",
    "precision" hits / edges, "recall" hits / positives, "f1" 2 hits / (edges + positives).  One distinct value among the
    candidates is the degenerate case: no edges, iterations 0, thresholds None.  McgraError for a selected NaN / inf score, a
    label other than 0 / 1 or a repeated id; McgraNotSupported for a finite score outside [0, 16)."""
    pred, real, ix, n, rows = _ranked(idx, pred, real)
    out, hi, lo = (C.c_int64 * 10)(), C.c_float(float("nan")), C.c_float(float("nan"))
    check(lib.mcgra_two_means_split(_stream(), n, _p(pred), pred.stride(0), _p(real), real.stride(0) if real is not None else 0,
                                    _p(ix), rows, int(max_iter), out, C.byref(hi), C.byref(lo)))
    m, it, conv, t, n_high, c0, c1, P, tp, degenerate = (int(v) for v in out)
    res = {"pairs": m, "iterations": it, "converged": bool(conv), "degenerate": bool(degenerate), "edges": n_high,
           "threshold": None if degenerate else hi.value, "threshold_low": None if degenerate else lo.value,
           "center_low": c0 * TWO_MEANS_SCALE, "center_high": c1 * TWO_MEANS_SCALE, "t": t, "c0": c0, "c1": c1}
    if real is not None:
        res.update({"positives": P, "hits": tp, "precision": _ratio(tp, n_high), "recall": _ratio(tp, P),
                    "f1": _ratio(2 * tp, n_high + P)})
    return res


@_on_operand_device
def threshold_pairs(pred, threshold, idx=None, real=None):
    """Every candidate of topk_metrics' selection with pred[idx[a], idx[b]] >= threshold (float32 comparison), in ascending
    packed position (mcgra_threshold_pairs): (pairs [k, 2] int64, scores [k] float32, hits [k] bool or None without real),
    device tensors.  The counts are asked for first, then exactly k rows are allocated.  With the threshold of
    two_means_split this is its high cluster; with 0.9 the reference's filter() (baseline.py:106-109)."""
    pred, real, ix, n, rows = _ranked(idx, pred, real)
    ldl = real.stride(0) if real is not None else 0
    counts = (C.c_int64 * 3)()
    check(lib.mcgra_threshold_pairs(_stream(), n, _p(pred), pred.stride(0), _p(real), ldl, _p(ix), rows, float(threshold), 0,
                                    None, None, None, counts))
    k = int(counts[1])
    pairs = torch.empty(k, 2, device=pred.device, dtype=torch.int64)
    scores = torch.empty(k, device=pred.device, dtype=torch.float32)
    hits = None if real is None else torch.empty(k, device=pred.device, dtype=torch.uint8)
    if k:
        check(lib.mcgra_threshold_pairs(_stream(), n, _p(pred), pred.stride(0), _p(real), ldl, _p(ix), rows, float(threshold), k,
                                        _p(pairs), _p(scores), _p(hits), counts))
    return pairs, scores, None if hits is None else hits.view(torch.bool)


def _limbs(lo, hi):
    return int(lo) + (int(hi) << 64)


def _norm_quantile(level):
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"auc_delong: level = {level!r}; a confidence level lies strictly between 0 and 1")
    return statistics.NormalDist().inv_cdf((1.0 + level) / 2.0)


def _delong_parts(P, N, T_a, T_b, A, B):
    """(P A - T_a T_b) / (4 N^2 P^2 (P - 1)) + (N B - T_a T_b) / (4 P^2 N^2 (N - 1)) as one exact rational: DeLong's variance
    (T_a = T_b = T, A = A2, B = B2) or covariance (A = A_ab, B = B_ab).  Needs P, N >= 2."""
    return (Fraction(P * A - T_a * T_b, 4 * N * N * P * P * (P - 1)) + Fraction(N * B - T_a * T_b, 4 * P * P * N * N * (N - 1)))


def delong_stats(ints, level=0.95):
    """The dict of auc_delong from its integers {"pairs", "positives", "negatives", "T", "A2", "B2"} (Python ints): exact
    rationals, each rounded to a double once.  No device is involved."""
    nan = float("nan")
    zq = _norm_quantile(level)
    m, P, N, T, A2, B2 = (int(ints[k]) for k in ("pairs", "positives", "negatives", "T", "A2", "B2"))
    res = {"pairs": m, "positives": P, "negatives": N, "auc": nan, "var": nan, "se": nan, "ci_low": nan, "ci_high": nan,
           "level": float(level), "ints": dict(ints)}
    if P == 0 or N == 0:
        return res
    res["auc"] = float(Fraction(T, 2 * P * N))
    if P == 1 or N == 1:
        return res
    res["var"] = float(_delong_parts(P, N, T, T, A2, B2))
    res["se"] = math.sqrt(res["var"])
    res["ci_low"] = max(0.0, res["auc"] - zq * res["se"])
    res["ci_high"] = min(1.0, res["auc"] + zq * res["se"])
    return res


def delong_paired_stats(ints, level=0.95):
    """The dict of auc_delong_paired from its integers {"pairs", "positives", "negatives", "T_a", "T_b", "A2_a", "B2_a", "A2_b",
    "B2_b", "A_ab", "B_ab"}.  var_delta = var_a + var_b - 2 cov is formed as ONE rational before it is rounded, so the
    cancellation between two nearly equal scorings is exact."""
    nan = float("nan")
    zq = _norm_quantile(level)
    g = {k: int(v) for k, v in ints.items()}
    m, P, N = g["pairs"], g["positives"], g["negatives"]
    res = {"a": delong_stats({"pairs": m, "positives": P, "negatives": N, "T": g["T_a"], "A2": g["A2_a"], "B2": g["B2_a"]}, level),
           "b": delong_stats({"pairs": m, "positives": P, "negatives": N, "T": g["T_b"], "A2": g["A2_b"], "B2": g["B2_b"]}, level),
           "cov": nan, "delta": nan, "se_delta": nan, "ci_low": nan, "ci_high": nan, "z": nan, "p_value": nan,
           "level": float(level), "ints": dict(g)}
    if P == 0 or N == 0:
        return res
    delta = Fraction(g["T_a"] - g["T_b"], 2 * P * N)
    res["delta"] = float(delta)
    if P == 1 or N == 1:
        return res
    var_a = _delong_parts(P, N, g["T_a"], g["T_a"], g["A2_a"], g["B2_a"])
    var_b = _delong_parts(P, N, g["T_b"], g["T_b"], g["A2_b"], g["B2_b"])
    cov = _delong_parts(P, N, g["T_a"], g["T_b"], g["A_ab"], g["B_ab"])
    var_d = var_a + var_b - 2 * cov
    res["cov"] = float(cov)
    res["se_delta"] = math.sqrt(float(var_d))
    res["ci_low"] = max(-1.0, res["delta"] - zq * res["se_delta"])
    res["ci_high"] = min(1.0, res["delta"] + zq * res["se_delta"])
    if var_d == 0:
        res["z"] = 0.0 if delta == 0 else math.copysign(float("inf"), delta)
    else:
        res["z"] = res["delta"] / res["se_delta"]
    res["p_value"] = math.erfc(abs(res["z"]) / math.sqrt(2.0))
    return res


@_on_operand_device
def auc_delong(real, pred, idx=None, level=0.95):
    """How far the AUC of the recovered graph can be trusted (mcgra_auc_delong): DeLong's variance of the AUC (DeLong, DeLong
    and Clarke-Pearson, Biometrics 44, 1988) over the candidates of topk_metrics -- the m unordered pairs of positions a > b of
    a REPEAT-FREE idx (None: all nodes), score pred[idx[a], idx[b]], label real[idx[a], idx[b]], float32 comparison with ties
    counted 1/2.  NOT the population of roc_auc, which counts every pair twice and the diagonal; "auc" here is the AUC of the
    unordered pairs.  Returns {"pairs" (m), "positives" (P), "negatives" (N), "auc" T / (2 P N), "var", "se" sqrt(var),
    "ci_low", "ci_high" (auc -+ z se clipped to [0, 1], z the normal quantile of (1 + level) / 2), "level", "ints" (the exact
    integers T, A2, B2 of the header)}: integer counts from the device, exact rationals on the host, one rounding each, the same
    bits on every call.  P or N == 0: everything NaN; P or N == 1: the AUC alone; var == 0: the interval is [auc, auc].
    Caveat: two pairs that share a node are not independent samples, so the interval is a lower bound on the real uncertainty.
    McgraError for a repeated or out-of-range id, a selected NaN / inf score or a selected label other than 0 / 1."""
    _norm_quantile(level)
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    out = (C.c_uint64 * 8)()
    check(lib.mcgra_auc_delong(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, out))
    m, P, N, T = (int(v) for v in out[:4])
    return delong_stats({"pairs": m, "positives": P, "negatives": N, "T": T, "A2": _limbs(out[4], out[5]),
                         "B2": _limbs(out[6], out[7])}, level)


@_on_operand_device
def auc_delong_paired(real, pred_a, pred_b, idx=None, level=0.95):
    """Whether two scorings of the same pairs differ (mcgra_auc_delong_paired): DeLong's test for two correlated AUCs (DeLong
    et al. 1988) over the candidates of auc_delong.  Returns {"a", "b" (each the dict of auc_delong for that scoring), "cov"
    (DeLong's covariance of the two AUCs), "delta" auc_a - auc_b, "se_delta" sqrt(var_a + var_b - 2 cov), "ci_low", "ci_high"
    (delta -+ z se_delta clipped to [-1, 1]), "z" delta / se_delta, "p_value" erfc(|z| / sqrt 2) (two-sided), "level", "ints"}.
    var_delta == 0: z = 0, p = 1 when delta == 0, else z = +-inf, p = 0.  P or N == 0: everything NaN; P or N == 1: the AUCs
    and delta alone.  The caveat of auc_delong holds: pairs that share a node are not independent, so se_delta is a
    lower bound on the real one and the p-value is optimistic.  Refusals as auc_delong, for either matrix."""
    _norm_quantile(level)
    real, pred_a, pred_b, ix, n, rows = _ranked(idx, real, pred_a, pred_b)
    out = (C.c_uint64 * 17)()
    check(lib.mcgra_auc_delong_paired(_stream(), n, _p(real), real.stride(0), _p(pred_a), pred_a.stride(0), _p(pred_b),
                                      pred_b.stride(0), _p(ix), rows, out))
    ints = {"pairs": int(out[0]), "positives": int(out[1]), "negatives": int(out[2]), "T_a": int(out[3]), "T_b": int(out[4])}
    for i, k in enumerate(("A2_a", "B2_a", "A2_b", "B2_b", "A_ab", "B_ab")):
        ints[k] = _limbs(out[5 + 2 * i], out[6 + 2 * i])
    return delong_paired_stats(ints, level)


NODE_JACKKNIFE_COLUMNS = ("P_v", "N_v", "A_v", "B_v", "C_v")


def _jackknife_influences(ints):
    """(m, P, N, auc as a Fraction or None, [(numerator, denominator) of d_v or None]) from the integers of
    auc_node_jackknife: d_v = AUC - AUC_-v = (T D_v - T_-v D) / (D D_v), D = 2 P N, D_v = 2 (P - P_v) (N - N_v); None where
    deleting v leaves no positive or no negative.  The denominator depends on the labels alone."""
    P, N, T = (int(ints[k]) for k in ("positives", "negatives", "T"))
    cols = [[int(x) for x in ints[k]] for k in NODE_JACKKNIFE_COLUMNS]
    m = len(cols[0])
    if any(len(c) != m for c in cols):
        raise ValueError("node_jackknife_stats: the five columns differ in length")
    if P == 0 or N == 0:
        return m, P, N, None, [None] * m
    D = 2 * P * N
    d = []
    for pv, nv, av, bv, cv in zip(*cols):
        Dv = 2 * (P - pv) * (N - nv)
        d.append(None if Dv == 0 else (T * Dv - (T - av - bv + cv) * D, D * Dv))
    return m, P, N, Fraction(T, D), d


def _influence_doubles(d):
    """The exact influences d = (numerator, denominator) or None, each ONE Fraction rounded to a double once; NaN for None."""
    return [float("nan") if x is None else float(Fraction(*x)) for x in d]


def _jackknife(dv, m):
    """(mean, var) of the delete-one jackknife over the m doubles dv, by math.fsum."""
    mean = math.fsum(dv) / m
    return mean, (m - 1) / m * math.fsum((x - mean) ** 2 for x in dv)


def node_jackknife_stats(ints, level=0.95):
    """The dict of auc_node_jackknife from its integers {"pairs", "positives", "negatives", "T" and the per-node sequences "P_v",
    "N_v", "A_v", "B_v", "C_v"}: the influence d_v = AUC - AUC_-v, AUC_-v = (T - A_v - B_v + C_v) / (2 (P - P_v) (N - N_v)), is
    ONE exact rational per node, rounded to a double once; the mean and var = (m - 1) / m sum (d_v - mean)^2 over the m nodes
    are math.fsum of those doubles, so they are the same on every call.  No device is involved."""
    nan = float("nan")
    zq = _norm_quantile(level)
    m, P, N, auc, d = _jackknife_influences(ints)
    undefined = sum(x is None for x in d)
    dv = _influence_doubles(d)
    res = {"pairs": int(ints["pairs"]), "nodes": m, "positives": P, "negatives": N, "auc": nan, "auc_jackknife": nan, "var": nan,
           "se": nan, "ci_low": nan, "ci_high": nan, "level": float(level), "undefined_nodes": undefined,
           "influence": torch.tensor(dv, dtype=torch.float64),
           "ints": {k: (list(int(x) for x in v) if k in NODE_JACKKNIFE_COLUMNS else int(v)) for k, v in ints.items()}}
    if auc is None:
        return res
    res["auc"] = float(auc)
    if undefined or m < 3:
        return res
    mean, var = _jackknife(dv, m)
    res["auc_jackknife"] = res["auc"] + (m - 1) * mean
    res["var"] = var
    res["se"] = math.sqrt(var)
    res["ci_low"] = max(0.0, res["auc"] - zq * res["se"])
    res["ci_high"] = min(1.0, res["auc"] + zq * res["se"])
    return res


def node_jackknife_paired_stats(ints_a, ints_b, level=0.95):
    """The node jackknife of the difference of two scorings' AUCs over the same pairs, from the integers of two
    auc_node_jackknife calls: d_v = d_v^A - d_v^B is ONE exact rational per node before it is rounded, then the jackknife of
    node_jackknife_stats.  Returns {"a", "b" (each scoring's dict), "delta" auc_a - auc_b, "delta_jackknife", "var_delta",
    "se_delta", "ci_low", "ci_high" (delta -+ z se_delta clipped to [-1, 1]), "z", "p_value", "influence", "undefined_nodes",
    "nodes", "pairs", "positives", "negatives", "level"}; var_delta == 0: z = 0, p = 1 when delta == 0, else z = +-inf, p = 0.
    ValueError when "pairs", "positives", "negatives", "P_v" or "N_v" differ: the two runs did not see the same pairs."""
    nan = float("nan")
    zq = _norm_quantile(level)
    a, b = node_jackknife_stats(ints_a, level), node_jackknife_stats(ints_b, level)
    for k in ("pairs", "positives", "negatives", "P_v", "N_v"):
        if a["ints"][k] != b["ints"][k]:
            raise ValueError(f"node_jackknife_paired_stats: the two runs disagree in {k}: not two scorings of the same pairs")
    m, P, N, auc_a, da = _jackknife_influences(ints_a)
    _, _, _, auc_b, db = _jackknife_influences(ints_b)
    dv = _influence_doubles([None if x is None else (x[0] - y[0], x[1]) for x, y in zip(da, db)])   # P_v, N_v agree: one denominator
    res = {"a": a, "b": b, "pairs": a["pairs"], "nodes": m, "positives": P, "negatives": N, "delta": nan, "delta_jackknife": nan,
           "var_delta": nan, "se_delta": nan, "ci_low": nan, "ci_high": nan, "z": nan, "p_value": nan, "level": float(level),
           "undefined_nodes": a["undefined_nodes"],
           "influence": torch.tensor(dv, dtype=torch.float64)}
    if auc_a is None:
        return res
    delta = auc_a - auc_b
    res["delta"] = float(delta)
    if a["undefined_nodes"] or m < 3:
        return res
    mean, var = _jackknife(dv, m)
    res["delta_jackknife"] = res["delta"] + (m - 1) * mean
    res["var_delta"] = var
    res["se_delta"] = math.sqrt(var)
    res["ci_low"] = max(-1.0, res["delta"] - zq * res["se_delta"])
    res["ci_high"] = min(1.0, res["delta"] + zq * res["se_delta"])
    if var == 0:
        res["z"] = 0.0 if delta == 0 else math.copysign(float("inf"), delta)
    else:
        res["z"] = res["delta"] / res["se_delta"]
    res["p_value"] = math.erfc(abs(res["z"]) / math.sqrt(2.0))
    return res


def _node_jackknife_ints(real, pred, idx):
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    header = (C.c_uint64 * 4)()
    out = torch.empty(max(rows, 0), 5, device=pred.device, dtype=torch.int64)        # every value is below 2^61
    check(lib.mcgra_auc_node_jackknife(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, header,
                                       _p(out)))
    ints = {"pairs": int(header[0]), "positives": int(header[1]), "negatives": int(header[2]), "T": int(header[3])}
    ints.update(zip(NODE_JACKKNIFE_COLUMNS, out.t().tolist()))
    return ints


@_on_operand_device
def auc_node_jackknife(real, pred, idx=None, level=0.95):
    """How far the AUC of the recovered graph can be trusted when NODES are the independent units, and which nodes carry it
    (mcgra_auc_node_jackknife): the delete-one-node jackknife of the AUC of auc_delong (Efron and Stein, Ann. Statist. 9, 1981)
    over the same candidates -- the m_pairs unordered pairs of positions a > b of a REPEAT-FREE idx (None: all nodes), score
    pred[idx[a], idx[b]], label real[idx[a], idx[b]], float32 comparison with ties counted 1/2.  Per position v of idx the
    device returns five exact integers over the pairs that contain v (P_v, N_v, the placement sums A_v, B_v and their overlap
    C_v); deleting v leaves AUC_-v = (T - A_v - B_v + C_v) / (2 (P - P_v) (N - N_v)).  Returns {"pairs", "nodes" (m),
    "positives", "negatives", "auc" T / (2 P N) (auc_delong's), "auc_jackknife" auc + (m - 1) mean(d) (bias-corrected), "var"
    (m - 1) / m sum (d_v - mean)^2, "se", "ci_low", "ci_high" (auc -+ z se clipped to [0, 1]), "level", "undefined_nodes",
    "influence" (float64 [m]: d_v = auc - AUC_-v, positive where the node helps the attack), "ints" (the header and the five
    columns)}: integer counts from the device, one exact rational per node on the host, the same bits on every call.
    This se is conservative where DeLong's is optimistic: the node jackknife is biased upward, never downward, when nodes are
    the exchangeable units, while DeLong's treats pairs that share a node as independent; reporting both brackets the truth.
    P or N == 0: everything NaN; a node that holds every positive or every negative (its deletion leaves no AUC; counted in
    "undefined_nodes", its influence NaN) or m == 2: the AUC alone; var == 0: the interval is [auc, auc].  Refusals as
    auc_delong."""
    _norm_quantile(level)
    return node_jackknife_stats(_node_jackknife_ints(real, pred, idx), level)


@_on_operand_device
def auc_node_jackknife_paired(real, pred_a, pred_b, idx=None, level=0.95):
    """Whether two scorings of the same pairs differ when NODES are the independent units: mcgra_auc_node_jackknife once per
    scoring, then node_jackknife_paired_stats -- the jackknife of d_v^A - d_v^B, delta, se_delta, the interval clipped to
    [-1, 1], z and the two-sided p_value.  This se is conservative where DeLong's (auc_delong_paired) is optimistic.  Refusals
    as auc_delong, for either matrix."""
    _norm_quantile(level)
    return node_jackknife_paired_stats(_node_jackknife_ints(real, pred_a, idx), _node_jackknife_ints(real, pred_b, idx), level)


GRAPH_STRUCTURE_HEADER = ("pairs", "E_R", "T_R", "W_R", "E_G", "T_G", "W_G", "E_C", "T_C")
GRAPH_STRUCTURE_COLUMNS = ("d_R", "t_R", "d_G", "t_G", "d_C", "t_C")


def _clustering(d, t):
    """The local clustering coefficients 2 t_v / (d_v (d_v - 1)) as exact rationals (numerator, denominator); 0 / 1 where
    d_v < 2."""
    return [(2 * tv, dv * (dv - 1)) if dv >= 2 else (0, 1) for dv, tv in zip(d, t)]


def _one_graph_stats(pairs, E, T, W, d, c):
    # a / b of two Python integers is the correctly rounded quotient: float(Fraction(a, b)) without the gcd
    m = len(d)
    hist = [0] * (max(d) + 1)
    for dv in d:
        hist[dv] += 1
    return {"edges": E, "density": E / pairs, "mean_degree": 2 * E / m, "max_degree": max(d),
            "triangles": T, "wedges": W, "transitivity": 3 * T / W if W else 0.0,
            "avg_clustering": math.fsum(a / b for a, b in c) / m, "degree_hist": hist}


def graph_structure_stats(header, cols):
    """The doubles of graph_structure from its integers: header = {"pairs", "E_R", "T_R", "W_R", "E_G", "T_G", "W_G", "E_C",
    "T_C"} and cols = {"d_R", "t_R", "d_G", "t_G", "d_C", "t_C"} (sequences over the m positions; the G and C entries -1 or
    None without the truth).  Every double is ONE rounding of an exact rational (the correctly rounded quotient of two Python
    integers), or a math.fsum of such.  No device is involved.
    Returns {"nodes", "recovered": g(R), "true": g(G) or None, ...}, g(X) = {"edges", "density" E / pairs, "mean_degree"
    2 E / m, "max_degree", "triangles", "wedges", "transitivity" 3 T / W (0.0 when W == 0, as networkx), "avg_clustering"
    fsum(c_v) / m with c_v = 2 t_v / (d_v (d_v - 1)) and 0 where d_v < 2 (nx.average_clustering's default), "degree_hist"
    (nodes per degree 0 .. max_degree)}.  With the truth also: "precision" E_C / E_R, "recall" E_C / E_G, "f1"
    2 E_C / (E_R + E_G), "triangle_hits" T_C, "triangle_recall" T_C / T_G, "triangle_precision" T_C / T_R (each NaN on a zero
    denominator), "degree_l1" sum |d_R - d_G| / m, "degree_ks" max_k |#{d_R <= k} - #{d_G <= k}| / m, "degree_corr" Pearson's
    r of the two degree sequences, sign(c) sqrt(c^2 / (v_R v_G)) from the integer moments c = m sum d_R d_G - sum d_R sum d_G,
    v_X = m sum d_X^2 - (sum d_X)^2: one rational, one rounding, one square root; NaN when either variance is 0, and
    "clustering_l1" fsum(|c_R(v) - c_G(v)|) / m."""
    nan = float("nan")
    h = {k: int(header[k]) for k in GRAPH_STRUCTURE_HEADER}
    dR, tR = ([int(x) for x in cols[k]] for k in ("d_R", "t_R"))
    m = len(dR)
    have = h["E_G"] >= 0
    if m < 2 or len(tR) != m or h["pairs"] != m * (m - 1) // 2:
        raise ValueError("graph_structure_stats: the columns do not belong to the header")
    cR = _clustering(dR, tR)
    res = {"nodes": m, "recovered": _one_graph_stats(h["pairs"], h["E_R"], h["T_R"], h["W_R"], dR, cR), "true": None}
    if not have:
        return res
    dG, tG = ([int(x) for x in cols[k]] for k in ("d_G", "t_G"))
    if len(dG) != m or len(tG) != m:
        raise ValueError("graph_structure_stats: the columns differ in length")
    cG = _clustering(dG, tG)
    res["true"] = _one_graph_stats(h["pairs"], h["E_G"], h["T_G"], h["W_G"], dG, cG)
    ratio = lambda a, b: a / b if b else nan
    res.update({"precision": ratio(h["E_C"], h["E_R"]), "recall": ratio(h["E_C"], h["E_G"]),
                "f1": ratio(2 * h["E_C"], h["E_R"] + h["E_G"]), "triangle_hits": h["T_C"],
                "triangle_recall": ratio(h["T_C"], h["T_G"]), "triangle_precision": ratio(h["T_C"], h["T_R"]),
                "degree_l1": sum(abs(a - b) for a, b in zip(dR, dG)) / m})
    hr, hg = res["recovered"]["degree_hist"], res["true"]["degree_hist"]
    run = worst = 0
    for k in range(max(len(hr), len(hg))):
        run += (hr[k] if k < len(hr) else 0) - (hg[k] if k < len(hg) else 0)
        worst = max(worst, abs(run))
    res["degree_ks"] = worst / m
    sr, sg = sum(dR), sum(dG)
    cov = m * sum(a * b for a, b in zip(dR, dG)) - sr * sg
    vr, vg = m * sum(a * a for a in dR) - sr * sr, m * sum(b * b for b in dG) - sg * sg
    res["degree_corr"] = math.copysign(math.sqrt(cov * cov / (vr * vg)), cov) if vr and vg else nan
    res["clustering_l1"] = math.fsum(abs(a * q - p * b) / (b * q) for (a, b), (p, q) in zip(cR, cG)) / m
    return res


@_on_operand_device
def graph_structure(pred, threshold, idx=None, real=None):
    """Whether the recovered graph looks like the real one (mcgra_graph_structure): degrees, triangles and wedges of R, the
    graph on the positions of a REPEAT-FREE idx (None: all nodes) with the edge {a, b}, a > b, iff pred[idx[a], idx[b]] >=
    threshold (threshold_pairs' float32 comparison: its edge list is R); with real also of G (real[idx[a], idx[b]] == 1) and of
    C = R & G.  Returns {"threshold", "nodes" (m), the header integers "pairs", "E_R", "T_R", "W_R", "E_G", "T_G", "W_G", "E_C",
    "T_C" (edges, triangles, wedges; -1 for G and C without real), the columns "d_R", "t_R", "d_G", "t_G", "d_C", "t_C" (device
    int64 [m], row = position in idx: degree and triangles through the node; -1 for G and C without real), "stats"
    (graph_structure_stats of them)}.  Exact integers from the device (bit matrices, AND + popcount), exact rationals on the
    host, the same bits on every call.  McgraError for a NaN threshold, a repeated or out-of-range id, a selected NaN / inf
    score or a selected label other than 0 / 1."""
    header, cols = _graph_structure_ints(pred, threshold, idx, real)
    res = {"threshold": float(threshold), "nodes": cols.shape[1]}
    res.update(zip(GRAPH_STRUCTURE_HEADER, header))
    res.update(zip(GRAPH_STRUCTURE_COLUMNS, cols))
    res["stats"] = graph_structure_stats(res, dict(zip(GRAPH_STRUCTURE_COLUMNS, cols.tolist())))
    return res


def _graph_structure_ints(pred, threshold, idx, real):
    """The device entry alone: (the nine header integers, the six columns as one device int64 tensor [6, m])."""
    pred, real, ix, n, rows = _ranked(idx, pred, real)
    header = (C.c_int64 * 9)()
    out = torch.empty(max(rows, 0), 6, device=pred.device, dtype=torch.int64)
    check(lib.mcgra_graph_structure(_stream(), n, _p(pred), pred.stride(0), _p(real), real.stride(0) if real is not None else 0,
                                    _p(ix), rows, float(threshold), header, _p(out)))
    return [int(v) for v in header], out.t().contiguous()


HOP_MAX = 8        # MCGRA_HOP_MAX (include/mcgra.h)


def _hops(hops):
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= hops <= HOP_MAX:
        raise ValueError(f"hop_auc: hops = {hops!r}; distances are told apart up to an integer hops in [1, {HOP_MAX}]")
    return int(hops)


def hop_auc_stats(ints, hops, threshold=None):
    """The dict of hop_auc from its integers: ints = the hops + 1 rows (pairs_c, T_c, above_c) of mcgra_hop_auc, row c - 1 the
    candidates at distance c of the true graph, the last row those beyond hops.  Every double is the correctly rounded
    quotient of two Python integers.  No device is involved.
    Returns {"hops", "threshold", "pairs" (m), "positives" (P = pairs_1), "negatives" (N), "distance" (1, ..., hops, "beyond"),
    and per class as tuples of length hops + 1: "count", "T", "above", "auc" T_c / (2 P pairs_c) (NaN for class 1 and where P
    or pairs_c is 0), "share" pairs_c / N (NaN for class 1, and where N is 0), "fp_share" above_c / the false positives (NaN
    for class 1 and when there are none); "auc_pooled" T_1 / (2 P N), auc_delong's "auc" bit for bit (NaN when P or N is 0);
    "ints" (the rows)}.  threshold None: no "above" and no "fp_share"."""
    nan = float("nan")
    H = _hops(hops)
    rows = [tuple(int(v) for v in r) for r in ints]
    if len(rows) != H + 1 or any(len(r) != 3 or min(r) < 0 for r in rows):
        raise ValueError(f"hop_auc_stats: {len(rows)} rows for hops = {H}; the entry returns hops + 1 rows of three counts")
    count, T, above = (tuple(r[q] for r in rows) for q in range(3))
    P, N, fp = count[0], sum(count[1:]), sum(above[1:])
    if T[0] != sum(T[1:]):
        raise ValueError("hop_auc_stats: T_1 is not the sum of the other classes' T")
    res = {"hops": H, "threshold": None if threshold is None else float(threshold), "pairs": P + N, "positives": P,
           "negatives": N, "distance": tuple(range(1, H + 1)) + ("beyond",), "count": count, "T": T, "above": above,
           "auc": (nan,) + tuple(t / (2 * P * c) if P and c else nan for t, c in zip(T[1:], count[1:])),
           "share": (nan,) + tuple(c / N if N else nan for c in count[1:]),
           "fp_share": (nan,) + tuple(a / fp if fp else nan for a in above[1:]),
           "auc_pooled": T[0] / (2 * P * N) if P and N else nan, "ints": rows}
    if threshold is None:
        del res["above"], res["fp_share"]
    return res


@_on_operand_device
def hop_auc(real, pred, idx=None, hops=3, threshold=None):
    """Where the attack's errors sit (mcgra_hop_auc): the candidates of auc_delong -- the unordered pairs of positions a > b of a
    REPEAT-FREE idx (None: all nodes), score pred[idx[a], idx[b]], label real[idx[a], idx[b]] -- classed by their distance in
    the TRUE graph on the selected nodes (the induced subgraph: no path runs through an unselected node): 1 (the edges), 2,
    ..., hops, and "beyond" (farther, or no path).  Per class the count, the AUC of the edges against that class alone and,
    with a threshold, the candidates at or above it (threshold_pairs' float32 comparison): the false positives by where they
    sit.  Returns hop_auc_stats' dict; "auc_pooled" is auc_delong's "auc" and the share-weighted mean of the class AUCs.
    Exact integers from the device (bit matrices of the reach, a search among the sorted edges), correctly rounded quotients
    on the host, the same bits on every call.  ValueError for hops outside [1, 8]; McgraError for a NaN threshold, a repeated
    or out-of-range id, a selected NaN / inf score or a selected label other than 0 / 1."""
    H = _hops(hops)
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    out = (C.c_int64 * (3 * (H + 1)))()
    check(lib.mcgra_hop_auc(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, H,
                            float("inf") if threshold is None else float(threshold), out))
    return hop_auc_stats([out[3 * c:3 * c + 3] for c in range(H + 1)], H, threshold)


EXPOSURE_CLASSES = 16                              # MCGRA_EXPOSURE_CLASSES (include/mcgra.h)
EXPOSURE_MAX_NIDX = 65535                          # the capacity of the placement entries
EXPOSURE_FIRST_CAP = 8                             # edge_exposure(edges=True) first allocates this many rows per selected node
EXPOSURE_HEADER = ("pairs", "positives", "negatives", "T", "above_pos", "above_neg")
# the classes of an edge: ec = min(common neighbours, 15); dc = min(15, bit_length(min degree))
EXPOSURE_COMMON_NAMES = tuple(str(c) for c in range(EXPOSURE_CLASSES - 1)) + (f"{EXPOSURE_CLASSES - 1}+",)
EXPOSURE_DEGREE_NAMES = ("0", "1") + tuple(f"{1 << (c - 1)}-{(1 << c) - 1}" for c in range(2, EXPOSURE_CLASSES - 1)) + \
    (f"{1 << (EXPOSURE_CLASSES - 2)}+",)


def edge_exposure_stats(header, table):
    """The doubles of edge_exposure from its integers: header = mcgra_edge_exposure's six (m, P, N, T, above_pos, above_neg),
    table its 16 x 16 x 3 cells (ec, dc) -> (count, T, above) over the true edges with ec = min(common neighbours, 15) and
    dc = min(15, bit_length(min degree)).  No device is involved; every double is the correctly rounded quotient of two Python
    integers, NaN on a zero denominator.  Returns {"pairs", "positives" (P), "negatives" (N), "T", "above_pos", "above_neg",
    "auc_pooled" T / (2 P N) (auc_delong's "auc" bit for bit), "recall" above_pos / P, "precision" above_pos / (above_pos +
    above_neg), the marginals "by_embeddedness" and "by_degree", each {"names" (EXPOSURE_COMMON_NAMES: "0" ... "14", "15+";
    EXPOSURE_DEGREE_NAMES: "0", "1", "2-3", "4-7", ..., "16384+") and as tuples over the 16 classes "count", "T", "above", "auc"
    T_c / (2 count_c N): the class's edges against ALL non-edges, "recall" above_c / count_c, "share" count_c / P, "lift" auc_c -
    auc_pooled = (T_c P - T count_c) / (2 count_c P N)}, and "cells", the non-empty cells of the joint table in (ec, dc) order:
    {"ec", "dc", "common", "degree" (the two names), "count", "T", "above", "auc", "recall", "share"}}."""
    nan = float("nan")
    K = EXPOSURE_CLASSES
    hd = tuple(int(v) for v in header)
    tb = tuple(tuple(tuple(int(v) for v in cell) for cell in row) for row in table)
    if len(hd) != 6 or min(hd) < 0 or len(tb) != K or any(len(row) != K or any(len(cell) != 3 or min(cell) < 0 for cell in row)
                                                          for row in tb):
        raise ValueError(f"edge_exposure_stats: six header integers and {K} x {K} x 3 table integers, none negative")
    m, P, N, T, above_pos, above_neg = hd
    sums = tuple(sum(cell[q] for row in tb for cell in row) for q in range(3))
    if m != P + N or sums != (P, T, above_pos):
        raise ValueError(f"edge_exposure_stats: the cells sum to {sums}; the header says {(P, T, above_pos)} of {m} = {P} + {N}")

    def doubles(count, t, above):
        return {"auc": t / (2 * count * N) if count and N else nan, "recall": _ratio(above, count), "share": _ratio(count, P)}

    def marginal(names, cells_of):
        rows = [tuple(sum(cell[q] for cell in cells_of(c)) for q in range(3)) for c in range(K)]
        d = [doubles(*r) for r in rows]
        res = {"names": names, "count": tuple(r[0] for r in rows), "T": tuple(r[1] for r in rows), "above": tuple(r[2] for r in rows)}
        res.update({q: tuple(x[q] for x in d) for q in ("auc", "recall", "share")})
        res["lift"] = tuple((t * P - T * c) / (2 * c * P * N) if c and N else nan for c, t, _ in rows)
        return res

    res = dict(zip(EXPOSURE_HEADER, hd))
    res.update({"auc_pooled": T / (2 * P * N) if P and N else nan, "recall": _ratio(above_pos, P),
                "precision": _ratio(above_pos, above_pos + above_neg),
                "by_embeddedness": marginal(EXPOSURE_COMMON_NAMES, lambda c: tb[c]),
                "by_degree": marginal(EXPOSURE_DEGREE_NAMES, lambda c: [tb[e][c] for e in range(K)]),
                "cells": [{"ec": e, "dc": c, "common": EXPOSURE_COMMON_NAMES[e], "degree": EXPOSURE_DEGREE_NAMES[c],
                           "count": tb[e][c][0], "T": tb[e][c][1], "above": tb[e][c][2], **doubles(*tb[e][c])}
                          for e in range(K) for c in range(K) if tb[e][c][0]]})
    return res


@_on_operand_device
def edge_exposure(real, pred, idx=None, threshold=None, edges=False):
    """Which edges leak (mcgra_edge_exposure): every true edge's own placement among the non-edges, by where the edge sits in
    the TRUE graph.  The candidates are auc_delong's -- the unordered pairs of positions a > b of a REPEAT-FREE idx (None: all
    nodes), score pred[idx[a], idx[b]], label real[idx[a], idx[b]] -- and G is the true graph on the selected nodes (the induced
    subgraph: an unselected neighbour does not exist).  Every edge of G has its placement a_e = 2 #{non-edges scoring lower} +
    #{non-edges scoring the same}, its embeddedness c_e = the common neighbours of its ends in G (the triangles through it) and
    d_e = the smaller of their degrees in G; the edges are classed by ec = min(c_e, 15) and dc = min(15, bit_length(d_e)).
    threshold (None: +inf, nothing is above): where "above" is counted, threshold_pairs' float32 comparison.
    Returns {"pairs" (m), "positives" (P), "negatives" (N), "T" (auc_delong's), "above_pos", "above_neg", "threshold", "table"
    (16 x 16 x 3 nested tuples of Python ints, cell (ec, dc) = (count, T, above)), "ints" (the six header integers), "stats"
    (edge_exposure_stats of them)}; with edges also the edge list in ascending packed position a (a - 1) / 2 + b as device
    tensors: "pairs_list" [P, 2] int64 = (idx[a], idx[b]), "scores" [P] float32 (the bits as stored), "placement" [P] int64,
    "common" [P] int32 (c_e, uncapped) and "deg" [P, 2] int32 (the degrees of a and of b); the columns are first allocated for
    EXPOSURE_FIRST_CAP edges per selected node, and the entry runs a second time only when the graph has more.
    Exact integers from the device (a bit matrix, AND + popcount, a search among the sorted edges), correctly rounded quotients
    on the host, the same bits on every call.  McgraError for a NaN threshold, a repeated or out-of-range id, a selected NaN /
    inf score or a selected label other than 0 / 1."""
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    dev, K = pred.device, EXPOSURE_CLASSES
    thr = float("inf") if threshold is None else float(threshold)
    header, table = (C.c_int64 * 6)(), (C.c_int64 * (K * K * 3))()
    cap = EXPOSURE_FIRST_CAP * rows if edges and 2 <= rows <= EXPOSURE_MAX_NIDX else 0
    for attempt in range(2):
        cols = (torch.empty(cap, 2, device=dev, dtype=torch.int64), torch.empty(cap, device=dev, dtype=torch.float32),
                torch.empty(cap, device=dev, dtype=torch.int64), torch.empty(cap, device=dev, dtype=torch.int32),
                torch.empty(cap, 2, device=dev, dtype=torch.int32)) if cap else (None,) * 5
        header[1] = -1
        rc = lib.mcgra_edge_exposure(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, thr, cap,
                                     *(_p(t) for t in cols), header, table)
        if rc == -4 and header[1] > cap and attempt == 0:     # MCGRA_ENOMEM with the header written: more edges than cap
            cap = int(header[1])
            continue
        check(rc)
        break
    P = int(header[1])
    hd = [int(v) for v in header]
    tb = tuple(tuple(tuple(int(table[(e * K + c) * 3 + q]) for q in range(3)) for c in range(K)) for e in range(K))
    res = dict(zip(EXPOSURE_HEADER, hd))
    res.update({"threshold": None if threshold is None else thr, "table": tb, "ints": hd, "stats": edge_exposure_stats(hd, tb)})
    if edges:
        res.update(zip(("pairs_list", "scores", "placement", "common", "deg"), (t[:P] for t in cols)))       # (cap > 0 here)
    return res


CLASS_MAX = 16                                     # MCGRA_CLASS_MAX (include/mcgra.h)
STRATA_MAX = CLASS_MAX * (CLASS_MAX + 1) // 2      # one stratum per unordered class pair
CLASS_STRATA = ("one", "same", "own", "blocks")


def class_strata(C, how):
    """(table, names) of a partition of the unordered class pairs of C classes into strata: table a symmetric uint8 array
    [C][C], table[i][j] the stratum of a pair with one end in class i and the other in class j, names the strata's names.
    how "one": every pair in one stratum ("all"); "same": 0 = both ends in one class, 1 = not ("same", "different"); "own":
    stratum c = both ends in class c, stratum C = the ends in different classes ("0", ..., "different"); "blocks": one stratum
    per unordered class pair i <= j in lexicographic order ("i-j")."""
    if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or not 1 <= C <= CLASS_MAX:
        raise ValueError(f"class_strata: C = {C!r}; an integer number of classes in [1, {CLASS_MAX}]")
    C = int(C)
    i, j = np.indices((C, C))
    if how == "one":
        table, names = np.zeros((C, C), np.uint8), ("all",)
    elif how == "same":
        table, names = (i != j).astype(np.uint8), ("same", "different")
    elif how == "own":
        table, names = np.where(i == j, i, C).astype(np.uint8), tuple(str(c) for c in range(C)) + ("different",)
    elif how == "blocks":
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        table = (lo * C - lo * (lo - 1) // 2 + hi - lo).astype(np.uint8)          # the pairs (lo, lo), ..., (lo, C - 1) follow lo's
        names = tuple(f"{a}-{b}" for a in range(C) for b in range(a, C))
    else:
        raise ValueError(f"class_strata: how = {how!r}; one of {', '.join(CLASS_STRATA)}")
    return table, names


def class_auc_stats(ints, names=None, threshold=None):
    """The dict of class_auc from its integers: ints = the G rows (pairs_g, P_g, T_g, above_g, hits_g) of mcgra_class_auc.
    Every double is the correctly rounded quotient of two Python integers, NaN on a zero denominator.  No device is involved.
    Returns, per stratum as tuples of length G: "count", "positives", "negatives", "T", "above", "hits", "auc" T_g / (2 P_g
    N_g), "pair_share" pairs_g / m, "edge_share" P_g / P, "precision" hits_g / above_g, "recall" hits_g / P_g; and overall
    "auc_within" sum T_g / sum 2 P_g N_g (the chance that an edge outranks a non-edge of its own stratum, ties half),
    "auc_adjusted" sum P_g AUC_g / sum P_g over the strata with P_g N_g > 0 (the covariate-adjusted AUC of Janes and Pepe,
    Biometrika 96, 2009: ONE Fraction, rounded once), "pairs" (m), "names", "threshold", "ints" (the rows).  threshold None:
    no "above", "hits", "precision" and "recall"."""
    nan = float("nan")
    rows = [tuple(int(v) for v in r) for r in ints]
    if not 1 <= len(rows) <= STRATA_MAX or any(len(r) != 5 or min(r) < 0 for r in rows):
        raise ValueError(f"class_auc_stats: {len(rows)} rows; the entry returns 1 to {STRATA_MAX} rows of five counts")
    names = tuple(str(g) for g in range(len(rows))) if names is None else tuple(names)
    if len(names) != len(rows):
        raise ValueError(f"class_auc_stats: {len(names)} names for {len(rows)} strata")
    count, pos, T, above, hits = (tuple(r[q] for r in rows) for q in range(5))
    neg = tuple(c - p for c, p in zip(count, pos))
    if min(neg) < 0 or any(t > 2 * p * n for t, p, n in zip(T, pos, neg)) or any(h > min(p, a) for h, p, a in zip(hits, pos, above)):
        raise ValueError("class_auc_stats: the rows are not counts of one selection (P_g <= pairs_g, T_g <= 2 P_g N_g, "
                         "hits_g <= min(P_g, above_g))")
    ratio = lambda a, b: a / b if b else nan
    m, P = sum(count), sum(pos)
    live = [g for g in range(len(rows)) if pos[g] and neg[g]]
    adjusted = sum((Fraction(T[g], 2 * neg[g]) for g in live), Fraction(0))          # sum P_g AUC_g
    res = {"names": names, "threshold": None if threshold is None else float(threshold), "pairs": m,
           "count": count, "positives": pos, "negatives": neg, "T": T, "above": above, "hits": hits,
           "auc": tuple(ratio(t, 2 * p * n) for t, p, n in zip(T, pos, neg)),
           "pair_share": tuple(ratio(c, m) for c in count), "edge_share": tuple(ratio(p, P) for p in pos),
           "precision": tuple(ratio(h, a) for h, a in zip(hits, above)), "recall": tuple(ratio(h, p) for h, p in zip(hits, pos)),
           "auc_within": ratio(sum(T), sum(2 * p * n for p, n in zip(pos, neg))),
           "auc_adjusted": float(adjusted / sum(pos[g] for g in live)) if live else nan, "ints": rows}
    if threshold is None:
        del res["above"], res["hits"], res["precision"], res["recall"]
    return res


def _node_classes(classes, n, idx):
    """classes as an int64 numpy vector of length n and the largest class among the selected nodes (idx None: all; ids outside
    [0, n) are left to the entry to refuse).  ValueError for a wrong length, a dtype that is not integer, a negative class of
    a selected node."""
    if isinstance(classes, torch.Tensor):
        classes = classes.detach().cpu().numpy()
    cl = np.asarray(classes)
    if cl.dtype == bool or not np.issubdtype(cl.dtype, np.integer):
        raise ValueError(f"class_auc: classes of dtype {cl.dtype}; the node classes are integers")
    if cl.shape != (n,):
        raise ValueError(f"class_auc: classes of shape {tuple(cl.shape)}; one class per node of the graph, ({n},)")
    cl = cl.astype(np.int64)
    sel = cl
    if idx is not None:
        ix = idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
        ix = ix.reshape(-1).astype(np.int64)
        sel = cl[ix[(ix >= 0) & (ix < n)]]
    if sel.size and sel.min() < 0:
        raise ValueError(f"class_auc: a selected node of class {int(sel.min())}; the classes are 0, 1, ...")
    return cl, int(sel.max()) if sel.size else 0


@_on_operand_device
def class_auc(real, pred, classes, idx=None, strata="blocks", threshold=None):
    """What the attack knows beyond the node classes (mcgra_class_auc): the candidates of auc_delong -- the unordered pairs of
    positions a > b of a REPEAT-FREE idx (None: all nodes), score pred[idx[a], idx[b]], label real[idx[a], idx[b]] -- split into
    strata by the classes of their two ends, and per stratum the AUC of ITS edges against ITS non-edges: a scoring that has
    learnt nothing but "same class" scores 0.5 inside every stratum.  classes: one integer per node of the graph (tensor, array
    or list of length n, indexed by node id).  strata: "one", "same", "own" or "blocks" (class_strata's partitions of C = the
    largest selected class + 1 classes) or a (table, names) pair of one's own, table symmetric [C][C] with entries below
    len(names).  With a threshold also the candidates at or above it per stratum (threshold_pairs' float32 comparison) and the
    edges among them.  Returns class_auc_stats' dict.  Exact integers from the device (a sort of the edges by stratum and
    score, a search inside the stratum's segment), correctly rounded quotients on the host, the same bits on every call.
    ValueError for more than 16 classes, classes of a wrong length or dtype, a negative class of a selected node, a table that
    is not [C][C]; McgraError for whatever the entry refuses: an asymmetric table, a selected class the table does not hold, a
    NaN threshold, a repeated or out-of-range id, a selected NaN / inf score or a selected label other than 0 / 1."""
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    cl, top = _node_classes(classes, n, idx)
    if isinstance(strata, str):
        if top >= CLASS_MAX:
            raise ValueError(f"class_auc: a selected node of class {top}; at most {CLASS_MAX} classes, 0 to {CLASS_MAX - 1}")
        table, names = class_strata(top + 1, strata)
    else:
        table, names = strata
        table, names = np.ascontiguousarray(np.asarray(table), dtype=np.uint8), tuple(names)
        if table.ndim != 2 or table.shape[0] != table.shape[1] or not 1 <= table.shape[0] <= CLASS_MAX:
            raise ValueError(f"class_auc: a strata table of shape {tuple(table.shape)}; [C][C] with C in [1, {CLASS_MAX}]")
    G = len(names)
    node_class = torch.as_tensor(np.clip(cl, -1, 2 ** 31 - 1).astype(np.int32), device=pred.device)     # what is clipped is refused
    out = (C.c_int64 * (5 * max(G, 1)))()
    check(lib.mcgra_class_auc(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, _p(node_class),
                              table.shape[0], table.ctypes.data_as(C.POINTER(C.c_uint8)), G,
                              float("inf") if threshold is None else float(threshold), out))
    return class_auc_stats([out[5 * g:5 * g + 5] for g in range(G)], names, threshold)


# the summands of mcgra_attack_finalize, in the order in which it adds them (mcgra_attack_finalize_components' slots)
ENSEMBLE_COMPONENTS = ("learned", "feature", "H_A1", "H_A2", "Y_A2", "ori_HA", "ori_YA", "label")
SUBSET_MAX_K = 8            # MCGRA_SUBSET_MAX_K (include/mcgra.h)
SUBSET_MAX_MASKS = 255      # MCGRA_SUBSET_MAX_MASKS
ENSEMBLE_BASE = 0x1f        # the five summands that no flag switches off


def _subset_masks(op, masks, K):
    """masks as a list of Python ints, each in [1, 2^K); ValueError otherwise."""
    masks = list(masks)
    if not 1 <= len(masks) <= SUBSET_MAX_MASKS:
        raise ValueError(f"{op}: {len(masks)} masks; 1 to {SUBSET_MAX_MASKS}")
    for q in masks:
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q < (1 << K):
            raise ValueError(f"{op}: mask {q!r}; an integer in [1, {1 << K}) selects among {K} components")
    return [int(q) for q in masks]


@_on_operand_device
def subset_auc(real, comps, masks, idx=None):
    """Which summand carries an ensemble (mcgra_subset_auc): for every mask of `masks` the AUC of the candidates of auc_delong --
    the unordered pairs of positions a > b of a REPEAT-FREE idx (None: all nodes), label real[idx[a], idx[b]] -- scored by the
    float32 sum of the components the mask selects, added in ascending k (bit k of a mask: component k), in ONE pass over the
    pairs.  comps: a [K, n, n] tensor or a list of K n x n tensors, K from 1 to 8; masks: 1 to 255 integers in [1, 2^K),
    repeats allowed.  Returns {"pairs", "positives", "negatives", "masks", "T" (per mask auc_delong's integer T on the
    materialised sum), "auc" (per mask the nearest double of T / (2 P N), NaN when P or N is 0)}: exact integers from the device,
    the same bits on every call.  ValueError for a wrong K, shape or mask; McgraError for whatever the entry refuses: a repeated
    or out-of-range id, a selected label other than 0 / 1, a selected component value or subset sum that is NaN or inf."""
    if isinstance(comps, torch.Tensor):
        comps = comps.unbind(0) if comps.dim() == 3 else ()
    comps = list(comps)
    if not 1 <= len(comps) <= SUBSET_MAX_K:
        raise ValueError(f"subset_auc: comps is a [K, n, n] tensor or a list of K n x n tensors, K in [1, {SUBSET_MAX_K}]")
    K = len(comps)
    masks = _subset_masks("subset_auc", masks, K)
    n = real.shape[0]
    if real.dim() != 2 or any(not isinstance(c, torch.Tensor) or tuple(c.shape) != (n, n) for c in comps) or real.shape[1] != n:
        raise ValueError(f"subset_auc: real and every component are {n} x {n} tensors")
    real, ix, n, rows = _ranked(idx, real)
    comps = [_rows_f32(c, real.device) for c in comps]
    if len({c.stride(0) for c in comps}) > 1:          # one leading dimension for all of them
        comps = [c.contiguous() for c in comps]
    ptrs = (C.c_void_p * K)(*[c.data_ptr() for c in comps])
    out = (C.c_uint64 * (3 + len(masks)))()
    check(lib.mcgra_subset_auc(_stream(), n, _p(real), real.stride(0), ptrs, K, comps[0].stride(0), _p(ix), rows,
                               (C.c_uint32 * len(masks))(*masks), len(masks), out))
    m, P, N = (int(v) for v in out[:3])
    T = [int(v) for v in out[3:]]
    return {"pairs": m, "positives": P, "negatives": N, "masks": masks, "T": T,
            "auc": [float(Fraction(t, 2 * P * N)) if P and N else float("nan") for t in T]}


def ablation_masks(present, used):
    """The subsets of the ensemble's summands that main.py --ablate ranks, as a de-duplicated ordered list of at most 25 masks
    (bit k: ENSEMBLE_COMPONENTS[k]): `used`; each present component alone; `used` without each of its components (not the empty
    set); components 0-4 with each subset of {ori_HA, ori_YA, label} that is present, in the binary order of (useH_A, useY_A,
    useY) -- the paper's flag table.  present holds the base five, used is a non-empty subset of present.  No device."""
    full = (1 << len(ENSEMBLE_COMPONENTS)) - 1
    for name, v in (("present", present), ("used", used)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= full:
            raise ValueError(f"ablation_masks: {name} = {v!r}; a mask of the {len(ENSEMBLE_COMPONENTS)} components")
    present, used = int(present), int(used)
    if present & ENSEMBLE_BASE != ENSEMBLE_BASE or not used or used & ~present:
        raise ValueError(f"ablation_masks: present = {present:#x}, used = {used:#x}; present holds the base five "
                         f"({ENSEMBLE_BASE:#x}) and used is a non-empty subset of it")
    bits = [k for k in range(len(ENSEMBLE_COMPONENTS)) if present >> k & 1]
    table = [used] + [1 << k for k in bits] + [used & ~(1 << k) for k in bits if used >> k & 1 and used != 1 << k]
    table += flag_table_masks(present)
    return list(dict.fromkeys(table))


def flag_table_masks(present):
    """Components 0-4 plus each subset of {5, 6, 7} that `present` holds, in the binary order of (useH_A, useY_A, useY)."""
    out = []
    for q in range(8):
        extra = q << 5
        if extra & ~int(present) == 0:
            out.append(ENSEMBLE_BASE | extra)
    return out


def shapley_shares(K, value):
    """The exact Shapley values of K players of the game v(empty) = 1/2, v(S) = value[mask of S] (a Fraction for every non-zero
    mask below 2^K): share_i = sum over S without i of |S|! (K - |S| - 1)! / K! (v(S + i) - v(S)), as Fractions whose sum is
    v(full) - 1/2 exactly.  No device."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= SUBSET_MAX_K:
        raise ValueError(f"shapley_shares: K = {K!r}; 1 to {SUBSET_MAX_K} players")
    K = int(K)
    if set(value) != set(range(1, 1 << K)) or not all(isinstance(v, Fraction) for v in value.values()):
        raise ValueError(f"shapley_shares: value maps every mask in [1, {1 << K}) to a Fraction")
    v = dict(value)
    v[0] = Fraction(1, 2)
    fact = [math.factorial(q) for q in range(K + 1)]
    shares = []
    for i in range(K):
        s = Fraction(0)
        for S in range(1 << K):
            if not S >> i & 1:
                size = bin(S).count("1")
                s += Fraction(fact[size] * fact[K - size - 1], fact[K]) * (v[S | 1 << i] - v[S])
        shares.append(s)
    return shares


# mcgra_node_rank_metrics (csrc/node_rank.hip): the header's MCGRA_NODE_RANK_MAX_NIDX, the workgroup's lane count, and the
# row-length classes (candidates per row, n_idx - 1: a row runs in the smallest class that holds it)
NODE_RANK_MAX_NIDX = 16384
NODE_RANK_THREADS = 512
NODE_RANK_CLASSES = (1024, 2048, 4096, 8192, 16384)
NODE_RANK_DEGREE_BINS = ((1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, None))


def _node_rates(cols, n_idx):
    """The per-node rates and the summary of node_rank_metrics from the five integer columns (numpy int64 [rows, 5]): one
    float64 division of exact integers each, NaN where the denominator is 0."""
    P, wins, ties, hits, first = (cols[:, q] for q in range(5))
    N = n_idx - 1 - P
    nan = np.full(len(P), np.nan)

    def div(num, den):
        ok = den > 0
        return np.where(ok, num.astype(np.float64) / np.where(ok, den, 1).astype(np.float64), nan)

    auc = div(2 * wins + ties, 2 * P * N)
    rprec = div(hits, P)
    rr = div(np.ones_like(first), first)
    mean_rank = div(P * N - wins - ties + P, P * N)

    def mean(x):
        return float(np.mean(x)) if len(x) else float("nan")

    scored, has_pos = (P > 0) & (N > 0), P > 0
    by_degree = []
    for lo, hi in NODE_RANK_DEGREE_BINS:
        sel = (P >= lo) & (has_pos if hi is None else P <= hi)
        by_degree.append((lo, hi, int(sel.sum()), mean(auc[sel & scored]), mean(rprec[sel])))
    summary = {"scored": int(scored.sum()), "macro_auc": mean(auc[scored]), "mrr": mean(rr[has_pos]),
               "hits_at_1": mean((first[has_pos] == 1).astype(np.float64)), "r_precision": mean(rprec[has_pos]),
               "by_degree": by_degree}
    return {"auc": auc, "r_precision": rprec, "reciprocal_rank": rr, "mean_rank": mean_rank}, summary


@_on_operand_device
def node_rank_metrics(real, pred, idx=None):
    """Whose neighbourhood leaked (mcgra_node_rank_metrics): for each position a of idx (REPEAT-FREE node ids; None: all nodes
    in order) the candidates are the positions b != a, with score pred[idx[a], idx[b]] and label real[idx[a], idx[b]] -- row a
    of the gathered submatrix without its diagonal, also for an asymmetric pred -- ranked best first: score descending
    (float32 values, -0.0 == +0.0), ties by ascending position b.  One workgroup ranks one row in LDS; n_idx <=
    NODE_RANK_MAX_NIDX (McgraNotSupported beyond).  Returns a dict, one entry per position of idx:
      "nodes" the ids; "positives" P, "wins" / "ties" the (positive, negative) candidate pairs whose positive scores higher /
      the same, "hits" the positives among the P best, "first_rank" 1 + the candidates strictly above the best positive (0
      when P = 0): int64 device tensors, exact;
      "auc" (2 wins + ties) / (2 P N) with N = n_idx - 1 - P, "r_precision" hits / P, "reciprocal_rank" 1 / first_rank,
      "mean_rank" (P N - wins - ties + P) / (P N), the reference's calc_mrr (gcn_parameterized.py:18-26: the mean over a row's
      true edges of their rank among its false ones, over N) on that row: float64 numpy arrays, one division of exact
      integers each (on the host, from the copied integer columns), NaN where the denominator is 0;
    and "summary": "scored" (nodes with P > 0 and N > 0), "macro_auc" over those, "mrr", "hits_at_1" (first_rank == 1) and
    "r_precision" over the nodes with P > 0 -- plain means in index order -- and "by_degree", a list of (lo, hi, count,
    mean auc, mean r_precision) over P in 1, 2, 3-4, 5-8, 9-16, 17-32, 33 and more (hi None).
    McgraError for a repeated or out-of-range id, a candidate NaN / inf score or a candidate label other than 0 / 1."""
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    out = torch.empty(max(rows, 0), 5, device=pred.device, dtype=torch.int64)
    check(lib.mcgra_node_rank_metrics(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows, _p(out)))
    rates, summary = _node_rates(out.cpu().numpy(), rows)
    res = {"nodes": ix if ix is not None else torch.arange(n, device=pred.device, dtype=torch.int64)}
    res.update({k: out[:, q] for q, k in enumerate(("positives", "wins", "ties", "hits", "first_rank"))})
    res.update(rates)
    res["summary"] = summary
    return res


# mcgra_knn_graph (csrc/knn_graph.hip): the header's MCGRA_KNN_MAX_NIDX and MCGRA_KNN_MAX_K, the row-length classes of the
# select (selected nodes per row: a row runs in the smallest class that holds it), the names of header[8] and of out[m][7]
KNN_MAX_NIDX = 16384
KNN_MAX_K = 1024
KNN_CLASSES = (1024, 4096, 16384)
KNN_HEADER = ("pairs", "k", "E_U", "E_M", "E_G", "H_D", "H_U", "H_M")
KNN_COLUMNS = ("in", "d_U", "d_M", "d_G", "h_D", "h_U", "h_M")
KNN_IN_BINS = ((0, 0),) + NODE_RANK_DEGREE_BINS


def knn_graph_stats(header, cols):
    """The doubles of knn_graph from its integers: header = {"pairs", "k", "E_U", "E_M", "E_G", "H_D", "H_U", "H_M"} and cols =
    {"in", "d_U", "d_M", ...} (sequences over the m positions; only the first three are read).  No device is involved; every
    double is one float64 division of exact integers, NaN on a zero denominator (and without the truth, E_G == -1, where "hits"
    is None).  Returns {"nodes", "k", "directed", "union", "mutual", "hubness"}:
      each graph = {"edges" (the m k arcs for "directed"), "positives" (E_G; 2 E_G for "directed": a true edge can be found
      from either end), "hits" (H_D / H_U / H_M), "precision" hits / edges, "recall" hits / positives, "f1" 2 hits /
      (edges + positives)}, "union" and "mutual" also "isolated", their nodes of degree 0;
      "hubness" = {"max_in", "orphans" (in == 0: in nobody's list), "skewness" of the in-degrees (Radovanovic et al., JMLR
      2010) = m3 / m2^1.5 with m2 = sum (in - k)^2 / m, m3 = sum (in - k)^3 / m (the mean of in is exactly k), computed as
      sign(S3) sqrt(S3^2 m / S2^3) from the integer sums: one rational, one rounding, one square root; NaN when m2 == 0,
      "in_hist" a list of (lo, hi, nodes) over in = 0, 1, 2, 3-4, 5-8, 9-16, 17-32, 33 and more (hi None)}."""
    nan = float("nan")
    h = {q: int(header[q]) for q in KNN_HEADER}
    ind, dU, dM = (np.asarray(cols[q], dtype=np.int64).reshape(-1) for q in ("in", "d_U", "d_M"))
    m, k = len(ind), h["k"]
    if m < 2 or len(dU) != m or len(dM) != m or h["pairs"] != m * (m - 1) // 2 or int(ind.sum()) != m * k:
        raise ValueError("knn_graph_stats: the columns do not belong to the header")
    have = h["E_G"] >= 0

    def graph(edges, positives, hits):
        if not have:
            return {"edges": edges, "positives": None, "hits": None, "precision": nan, "recall": nan, "f1": nan}
        return {"edges": edges, "positives": positives, "hits": hits, "precision": _ratio(hits, edges),
                "recall": _ratio(hits, positives), "f1": _ratio(2 * hits, edges + positives)}

    res = {"nodes": m, "k": k, "directed": graph(m * k, 2 * h["E_G"], h["H_D"]),
           "union": graph(h["E_U"], h["E_G"], h["H_U"]), "mutual": graph(h["E_M"], h["E_G"], h["H_M"])}
    res["union"]["isolated"] = int((dU == 0).sum())
    res["mutual"]["isolated"] = int((dM == 0).sum())
    dev = ind - k                      # int64 holds the sum of cubes while m^4 < 2^63 (2^56 at the capacity); else Python integers
    if m > 40000:
        dev = dev.astype(object)
    S2, S3 = int((dev * dev).sum()), int((dev * dev * dev).sum())
    res["hubness"] = {"max_in": int(ind.max()), "orphans": int((ind == 0).sum()),
                      "skewness": math.copysign(math.sqrt(S3 * S3 * m / S2 ** 3), S3) if S2 else nan,
                      "in_hist": [(lo, hi, int(((ind >= lo) & (ind <= (ind.max() if hi is None else hi))).sum()))
                                  for lo, hi in KNN_IN_BINS]}
    return res


@_on_operand_device
def knn_graph(pred, k, idx=None, real=None, lists=False, edges=False):
    """The k-nearest-neighbour graph of the scores (mcgra_knn_graph): a local cut beside the global cuts of topk_metrics and
    threshold_pairs.  For each position a of idx (REPEAT-FREE node ids; None: all nodes in order) the candidates are the positions
    b != a with score pred[idx[a], idx[b]] -- row a of the gathered submatrix without its diagonal, also for an asymmetric pred --
    ranked best first as node_rank_metrics does: score descending (float32 values, -0.0 == +0.0), ties by ascending position b.
    L_k(a) is the first k of them; D has the arc a -> b iff b is in L_k(a), U the edge {a, b} iff either arc exists, Mu iff both;
    with real, G has {a, b}, a > b, iff real[idx[a], idx[b]] == 1.  1 <= k <= min(m - 1, KNN_MAX_K) and m <= KNN_MAX_NIDX
    (McgraError for k outside [1, m - 1], McgraNotSupported beyond the two capacities).  Returns {"k", "nodes" (m), the header
    integers "pairs", "E_U", "E_M", "E_G", "H_D", "H_U", "H_M" (edges of U, Mu, G; arcs of D, edges of U and of Mu that are edges
    of G; -1 for the last four without real), the columns "in", "d_U", "d_M", "d_G", "h_D", "h_U", "h_M" (device int64 [m], row =
    position in idx: in-degree in D, degrees in U, Mu, G, and how many of L_k(a), of the U- and of the Mu-neighbours are
    G-neighbours; -1 for the last four without real), "stats" (knn_graph_stats of them)}; with lists also "lists" (device int32
    [m, k]: L_k(a) as positions, in ranking order); with edges also U's edge list in ascending packed position a (a - 1) / 2 + b:
    "pairs_list" [E_U, 2] int64 = (idx[a], idx[b]), a > b, "scores" [E_U] float32 (the bits as stored), "kind" [E_U] uint8 (bit 0
    a -> b, bit 1 b -> a, 3 mutual) and "hits" [E_U] bool (None without real).  Exact integers from the device (a radix select of
    each row in LDS, bit matrices, popcounts), the same bits on every call.  McgraError for a repeated or out-of-range id, a
    candidate NaN / inf score or a selected label other than 0 / 1."""
    pred, real, ix, n, rows = _ranked(idx, pred, real)
    k, dev = int(k), pred.device
    header = (C.c_int64 * 8)()
    out = torch.empty(max(rows, 0), 7, device=dev, dtype=torch.int64)
    ok = 2 <= rows <= KNN_MAX_NIDX and 1 <= k <= min(rows - 1, KNN_MAX_K)      # otherwise the entry refuses: allocate nothing
    nn = torch.empty(rows, k, device=dev, dtype=torch.int32) if lists and ok else None
    cap = rows * k if edges and ok else 0
    pairs = torch.empty(cap, 2, device=dev, dtype=torch.int64) if cap else None
    scores = torch.empty(cap, device=dev, dtype=torch.float32) if cap else None
    kind = torch.empty(cap, device=dev, dtype=torch.uint8) if cap else None
    hits = torch.empty(cap, device=dev, dtype=torch.uint8) if cap and real is not None else None
    check(lib.mcgra_knn_graph(_stream(), n, _p(pred), pred.stride(0), _p(real), real.stride(0) if real is not None else 0,
                              _p(ix), rows, k, header, _p(out), _p(nn), cap, _p(pairs), _p(scores), _p(kind), _p(hits)))
    cols = out.t().contiguous()
    res = {"k": k, "nodes": rows}
    res.update(zip(KNN_HEADER, (int(v) for v in header)))
    res.update(zip(KNN_COLUMNS, cols))
    res["stats"] = knn_graph_stats(res, dict(zip(KNN_COLUMNS[:3], cols[:3].cpu().numpy())))
    if lists:
        res["lists"] = nn
    if edges:
        E = res["E_U"]
        res.update({"pairs_list": pairs[:E], "scores": scores[:E], "kind": kind[:E],
                    "hits": None if hits is None else hits[:E].view(torch.bool)})
    return res


def _curve_first_cap(entries, drop_intermediate):
    """The first attempt's capacity: levels + 1 <= entries + 1 always suffices, and without drop_intermediate little less
    does; with it a curve keeps the corners only, so an eighth of the entries (at least 2^20 points) is tried first and
    mcgra_rank_curves says what is needed when that is too small (measured, DESIGN.md 3d: a modified_adj at n = 2 708 keeps
    679 000 ROC points of 7.3 million entries, one at N = 10 000 1.1 million of 10^8)."""
    return entries + 1 if not drop_intermediate else min(entries + 1, max(1 << 20, entries // 8))


def _rank_curves(real, pred, idx, drop_intermediate, want_roc, want_pr, want_best, first_cap=None):
    """One mcgra_rank_curves call (a second one, sized from its counts, when the first capacity is too small; never a
    third).  Returns (counts, roc, pr, best): counts = (P, N, levels, ROC points, PR points); roc / pr = (tps, fps, thresholds)
    device tensors of exactly that many points (int64, int64, float32) or None; best = (tp, fp, level, threshold) or None."""
    real, pred, ix, n, rows = _ranked(idx, real, pred)
    cap = max(1, int(first_cap) if first_cap is not None else _curve_first_cap(rows * rows, drop_intermediate))
    counts, best, thr = (C.c_int64 * 5)(), (C.c_int64 * 3)(), C.c_float(float("nan"))
    for attempt in range(2):
        def bufs(want):
            if not want:
                return None, None, None
            return tuple(torch.empty(cap, device=pred.device, dtype=t) for t in (torch.int64, torch.int64, torch.float32))
        roc, pr = bufs(want_roc), bufs(want_pr)
        rc = lib.mcgra_rank_curves(_stream(), n, _p(real), real.stride(0), _p(pred), pred.stride(0), _p(ix), rows,
                                   1 if drop_intermediate else 0, cap, _p(roc[0]), _p(roc[1]), _p(roc[2]), _p(pr[0]),
                                   _p(pr[1]), _p(pr[2]), counts, best if want_best else None,
                                   C.byref(thr) if want_best else None)
        if rc == -4 and counts[2] > 0 and attempt == 0:       # MCGRA_ENOMEM with counts written: cap was too small
            cap = max(counts[3] if want_roc else 0, counts[4] if want_pr else 0)
            continue
        check(rc)
        break
    P, N, levels, n_roc, n_pr = (int(c) for c in counts)
    roc = tuple(t[:n_roc] for t in roc) if want_roc else None
    pr = tuple(t[:n_pr] for t in pr) if want_pr else None
    got_best = (int(best[0]), int(best[1]), int(best[2]), thr.value) if want_best and P > 0 else None
    return (P, N, levels, n_roc, n_pr), roc, pr, got_best


def _roc_rates(counts, roc):
    """(fpr, tpr, thresholds) of roc_curve from the integer ROC points: fps / fps[-1] (= N) and tps / tps[-1] (= P), one
    float64 division each (by a device tensor: a host scalar would be turned into a multiplication by its reciprocal, a
    second rounding); NaN for an absent class."""
    P, N = counts[0], counts[1]
    tps, fps, thr = (roc[0].to(torch.float64), roc[1].to(torch.float64), roc[2])
    nan = torch.full((tps.numel(),), float("nan"), device=tps.device, dtype=torch.float64)
    fpr = fps / fps[-1] if N > 0 else nan
    tpr = tps / tps[-1] if P > 0 else nan.clone()
    return fpr, tpr, thr


def _pr_rates(counts, pr):
    """(precision, recall, thresholds) of precision_recall_curve from the integer PR points (descending thresholds): reversed,
    with sklearn's last point (1, 0) appended; precision 0 where tp + fp == 0, recall 1 everywhere when P == 0."""
    P = counts[0]
    tps, fps, thr = (t.flip(0) for t in pr)
    ps = (tps + fps).to(torch.float64)
    t64 = tps.to(torch.float64)
    precision = torch.where(ps != 0, t64 / torch.where(ps != 0, ps, torch.ones_like(ps)), torch.zeros_like(ps))
    recall = t64 / t64[0] if P > 0 else torch.ones_like(t64)      # t64[0]: the last level's tp = P (a device tensor)
    one, zero = torch.ones(1, device=t64.device, dtype=torch.float64), torch.zeros(1, device=t64.device, dtype=torch.float64)
    return torch.cat((precision, one)), torch.cat((recall, zero)), thr


def _best_f1(counts, best):
    if best is None:
        nan = float("nan")
        return {"f1": nan, "threshold": nan, "tp": 0, "fp": 0, "precision": nan, "recall": nan}
    tp, fp, _, thr = best
    return {"f1": _ratio(2 * tp, tp + fp + counts[0]), "threshold": thr, "tp": tp, "fp": fp,
            "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, counts[0])}


@_on_operand_device
def roc_curve(real, pred, idx=None, drop_intermediate=True):
    """sklearn.metrics.roc_curve(real[idx][:, idx].reshape(-1), pred[idx][:, idx].reshape(-1), drop_intermediate=) without
    gathering the submatrix or leaving the device (mcgra_rank_curves): (fpr, tpr, thresholds), float64, float64, float32
    device tensors, thresholds[0] = +inf.  The counts behind the rates are exact integers; a rate is one float64 division.
    fpr is NaN when no selected label is 0, tpr when none is 1 (sklearn's warnings are not reproduced).  Arguments and
    refusals as roc_auc."""
    counts, roc, _, _ = _rank_curves(real, pred, idx, drop_intermediate, True, False, False)
    return _roc_rates(counts, roc)


@_on_operand_device
def precision_recall_curve(real, pred, idx=None, drop_intermediate=False):
    """sklearn.metrics.precision_recall_curve of the same selection (mcgra_rank_curves): (precision, recall, thresholds),
    thresholds ascending, the last precision 1 and the last recall 0.  recall is 1 everywhere when no selected label is 1."""
    counts, _, pr, _ = _rank_curves(real, pred, idx, drop_intermediate, False, True, False)
    return _pr_rates(counts, pr)


@_on_operand_device
def rank_curves(real, pred, idx=None, drop_intermediate=True, _first_cap=None):
    """Both curves and the best F1 from one classify, one emit and one sort (mcgra_rank_curves).  Returns a dict: "roc" =
    roc_curve's triple, "pr" = precision_recall_curve's (with this drop_intermediate), "positives", "negatives", "levels"
    (distinct selected scores), "roc_points", "pr_points", and "best_f1" = {"f1", "threshold", "tp", "fp", "precision",
    "recall"} of the threshold that maximises F1 = 2 tp / (tp + fp + P) over ALL distinct scores (exact comparison, ties to the
    higher threshold; NaN when no selected label is 1)."""
    counts, roc, pr, best = _rank_curves(real, pred, idx, drop_intermediate, True, True, True, _first_cap)
    return {"roc": _roc_rates(counts, roc), "pr": _pr_rates(counts, pr), "positives": counts[0], "negatives": counts[1],
            "levels": counts[2], "roc_points": counts[3], "pr_points": counts[4], "best_f1": _best_f1(counts, best)}


def _decode_rank_metrics(real, Z, mode, idx, want_auc, want_ap):
    real, Z, ix, n, rows = _ranked(idx, real, factor=Z)
    auc, ap = C.c_double(), C.c_double()
    check(lib.mcgra_decode_rank_metrics(_stream(), n, Z.shape[1], _p(Z), Z.stride(0), int(mode), _p(real), real.stride(0),
                                        _p(ix), rows, C.byref(auc) if want_auc else None,
                                        C.byref(ap) if want_ap else None))
    return auc.value, ap.value


@_on_operand_device
def decode_rank_metrics(real, Z, mode, idx=None):
    """rank_metrics(real, decode_scores(Z, mode), idx), bit for bit, without the n x n score matrix
    (mcgra_decode_rank_metrics).  Z, mode and refusals as decode_auc."""
    return _decode_rank_metrics(real, Z, mode, idx, True, True)


@_on_operand_device
def decode_average_precision(real, Z, mode, idx=None):
    """The second value of decode_rank_metrics alone."""
    return _decode_rank_metrics(real, Z, mode, idx, False, True)[1]


@_on_operand_device
def decode_scores(Z, mode):
    """The n x n scores decode_auc ranks, materialised (mcgra_decode_scores): dot_product_decode2 modes 0, 1, 2, 4 from one
    fp32 dot product per pair, bitwise symmetric; any width."""
    Z = _rows_f32(Z, Z.device)
    n, d = Z.shape
    out = torch.empty(n, n, device=Z.device, dtype=torch.float32)
    check(lib.mcgra_decode_scores(_stream(), n, d, _p(Z), Z.stride(0), int(mode), _p(out), n))
    return out


PAIR_METRICS = _lib.PAIR_METRICS      # the link-stealing distances, in the id order of MCGRA_PAIR_* (include/mcgra.h)


def pair_metric_id(metric):
    """A link-stealing metric given by name (PAIR_METRICS) or by id as its id; ValueError for anything else."""
    if isinstance(metric, str):
        if metric in PAIR_METRICS:
            return PAIR_METRICS.index(metric)
    elif isinstance(metric, (int, np.integer)) and not isinstance(metric, bool) and 0 <= int(metric) < len(PAIR_METRICS):
        return int(metric)
    raise ValueError(f"pair distance metric {metric!r}: one of {', '.join(PAIR_METRICS)} (or its id 0 .. {len(PAIR_METRICS) - 1})")


@_on_operand_device
def pair_distance_scores(Z, metric):
    """The link-stealing baseline's scores, materialised (mcgra_pair_distance_scores): out[i, j] = 0.0 - dist(Z[i], Z[j])
    for one of the eight metrics of PAIR_METRICS (He et al., USENIX Security 2021, Attack-0), higher = more like an edge.
    Z: n x d on the device, any d.  Each distance is one fp32 chain over k ascending, so the matrix is bitwise symmetric and the
    same bits on every call.  McgraError for a NaN / inf in Z."""
    m = pair_metric_id(metric)
    Z = _rows_f32(Z, Z.device)
    n, d = Z.shape
    out = torch.empty(n, n, device=Z.device, dtype=torch.float32)
    check(lib.mcgra_pair_distance_scores(_stream(), n, d, _p(Z), Z.stride(0), m, _p(out), n))
    return out


@_on_operand_device
def pair_distance_rank_metrics(real, Z, metric, idx=None):
    """How well a distance between two nodes' rows of Z tells the edges of `real` from the non-edges, without the n x n score
    matrix (mcgra_pair_distance_rank_metrics).  The population is auc_delong's: the m unordered pairs of positions a > b of a
    REPEAT-FREE idx (None: all nodes), label real[idx[a], idx[b]].  Returns {"pairs" (m), "positives" (P), "negatives" (N),
    "T" (twice the Mann-Whitney U), "auc" T / (2 P N), "ap"}: the integers and "auc" are bit for bit
    auc_delong(real, pair_distance_scores(Z, metric), idx)'s, "ap" is sklearn's average_precision_score on those pairs.  P or
    N == 0: "auc" NaN; P == 0: "ap" NaN; N == 0: "ap" 1.0.  McgraError for a NaN / inf in Z, a selected score that overflows,
    a selected label other than 0 / 1, a repeated or out-of-range id."""
    m = pair_metric_id(metric)
    real, Z, ix, n, rows = _ranked(idx, real, factor=Z)
    auc, ap = C.c_double(), C.c_double()
    counts = (C.c_int64 * 4)()
    check(lib.mcgra_pair_distance_rank_metrics(_stream(), n, Z.shape[1], _p(Z), Z.stride(0), m, _p(real), real.stride(0), _p(ix),
                                               rows, C.byref(auc), C.byref(ap), counts))
    pairs, P, N, T = (int(v) for v in counts)
    if P and N:      # the device's one rounding is the exact rational's
        exact = float(Fraction(T, 2 * P * N))
        assert exact == auc.value, (exact, auc.value)
    return {"pairs": pairs, "positives": P, "negatives": N, "T": T, "auc": auc.value, "ap": ap.value}


DP_MECHANISMS = ("edgerand", "lapgraph")      # MCGRA_DP_EDGERAND, MCGRA_DP_LAPGRAPH (include/mcgra.h)
DP_MAX_N = 65535                               # a packed pair position fits 32 bits


def dp_mechanism_id(mechanism):
    """An edge-DP mechanism given by name (DP_MECHANISMS) as its id; ValueError for anything else."""
    if isinstance(mechanism, str) and mechanism in DP_MECHANISMS:
        return DP_MECHANISMS.index(mechanism)
    raise ValueError(f"dp mechanism {mechanism!r}: one of {', '.join(DP_MECHANISMS)}")


def dp_perturb_graph(adj, mechanism, eps, seed, replicate=0, want_noisy=False, out=None):
    """The graph a defended victim is trained on and answers from (mcgra_dp_perturb_graph): adj's graph under EdgeRand
    (randomised response on every node pair) or LapGraph (Laplace noise on every pair, then the noisy top-E~) of Wu et al.,
    "LinkTeller" (IEEE S&P 2022), with edge-level privacy budget eps.  adj: n x n on the device, 2 <= n <= 65 535; only its
    strict lower triangle is read, and a value there other than 0 / 1 is a McgraError.  Every pair's randomness is one
    Philox4x32-10 draw keyed by (seed, replicate, packed position): the same bits on every call, rank and device.
    Returns (perturbed, info): perturbed n x n float32 on adj's device (0 / 1, symmetric, zero diagonal; written into `out`
    when one is given, whose columns beyond n stay as they are), info = {"mechanism", "eps", "seed", "replicate", "pairs" m,
    "edges" E, "target" (LapGraph's E~; -1 for EdgeRand), "edges_out" = kept + added, "kept", "added", "removed",
    "flip_probability" q and "eps_realised" ln((1 - q) / q) (EdgeRand: the probability realised by the 32-bit threshold; NaN
    for LapGraph), "count_noise" (LapGraph: the Laplace noise of the edge count; NaN for EdgeRand)}; with want_noisy (LapGraph
    only) info["noisy"] = the noisy cells, n x n float32, mirrored, 0 on the diagonal.
    ValueError, before anything is called on the device, for an unknown mechanism, an eps that is not a finite number above 0,
    a seed outside [0, 2^64), a replicate outside [0, 2^32), want_noisy with EdgeRand, an adj that is not n x n with n in range
    or not on a device, and an `out` that is not n float32 rows of unit inner stride on adj's device."""
    mech = dp_mechanism_id(mechanism)
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not math.isfinite(eps) or not eps > 0:
        raise ValueError(f"dp_perturb_graph: eps = {eps!r}; a finite number above 0")
    for name, v, bits in (("seed", seed, 64), ("replicate", replicate, 32)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << bits:
            raise ValueError(f"dp_perturb_graph: {name} = {v!r}; an integer in [0, 2^{bits})")
    if want_noisy and mech != DP_MECHANISMS.index("lapgraph"):
        raise ValueError("dp_perturb_graph: want_noisy asks for LapGraph's noisy cells; EdgeRand has none")
    if not isinstance(adj, torch.Tensor) or adj.dim() != 2 or adj.shape[0] != adj.shape[1] or not 2 <= adj.shape[0] <= DP_MAX_N:
        raise ValueError(f"dp_perturb_graph: adj of shape {tuple(getattr(adj, 'shape', ()))}; n x n with 2 <= n <= {DP_MAX_N}")
    n = adj.shape[0]
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, n)
                            or out.stride(1) != 1 or out.stride(0) < n or out.device != adj.device):
        raise ValueError(f"dp_perturb_graph: out must be {n} x {n} float32 rows of unit inner stride on adj's device")
    return _dp_perturb_graph(adj, mech, float(eps), int(seed), int(replicate), bool(want_noisy), out)


@_on_operand_device
def _dp_perturb_graph(adj, mech, eps, seed, replicate, want_noisy, out):
    adj = _rows_f32(adj, adj.device)
    n = adj.shape[0]
    if out is None:
        out = torch.empty(n, n, device=adj.device, dtype=torch.float32)
    noisy = torch.empty(n, n, device=adj.device, dtype=torch.float32) if want_noisy else None
    counts, realised = (C.c_int64 * 6)(), (C.c_double * 2)()
    check(lib.mcgra_dp_perturb_graph(_stream(), n, _p(adj), adj.stride(0), mech, eps, seed, replicate, _p(out), out.stride(0),
                                     _p(noisy), n if want_noisy else 0, counts, realised))
    m, E, target, kept, added, removed = (int(c) for c in counts)
    lap = mech == DP_MECHANISMS.index("lapgraph")
    info = {"mechanism": DP_MECHANISMS[mech], "eps": eps, "seed": seed, "replicate": replicate, "pairs": m, "edges": E,
            "target": target, "edges_out": kept + added, "kept": kept, "added": added, "removed": removed,
            "flip_probability": float("nan") if lap else realised[0], "eps_realised": float("nan") if lap else realised[1],
            "count_noise": realised[0] if lap else float("nan")}
    if want_noisy:
        info["noisy"] = noisy
    return out, info


@_device_operands
def gcn_forward(X, adj, W, b, Wlin, blin, emb_nlayer=0):
    """GCN.forward (eval) and, when emb_nlayer > 0, embedding_GCN.forward."""
    X, adj, Wlin, blin = _f32(X), _f32(adj), _f32(Wlin), _f32(blin)
    W, b = [_f32(w) for w in W], [_f32(x) for x in b]
    n, nfeat = X.shape
    L = len(W)
    dims = (C.c_int32 * (L + 1))(*([nfeat] + [w.shape[1] for w in W]))
    Wp = (C.c_void_p * L)(*[w.data_ptr() for w in W])
    bp = (C.c_void_p * L)(*[x.data_ptr() for x in b])
    nclass = Wlin.shape[0]
    out = torch.empty(n, nclass, device=X.device, dtype=torch.float32)
    emb = torch.empty(n, W[emb_nlayer - 1].shape[1], device=X.device, dtype=torch.float32) if emb_nlayer else None
    check(lib.mcgra_gcn_forward(_stream(), n, nfeat, L, dims, _p(X), _p(adj), Wp, bp, _p(Wlin), _p(blin), nclass,
                                emb_nlayer, _p(emb), _p(out)))
    return out, emb


INFLUENCE_OUTPUTS = ("log_posteriors", "posteriors")      # MCGRA_INFLUENCE_LOG_POSTERIORS, MCGRA_INFLUENCE_POSTERIORS (include/mcgra.h)
INFLUENCE_SYMMETRIZE = ("directed", "max")
INFLUENCE_MAX_N = 65535
INFLUENCE_MAX_WIDTH = 64                                  # MCGRA_INFLUENCE_MAX_WIDTH: one lane owns one column


def victim_gcn_tensors(model):
    """(W, b, Wlin, blin) of a models.gcn.GCN, as gcn_forward and influence_scores take them; ValueError for a victim that is
    not one (GraphSAGE's self weights, GAT's attention heads, a GCN without relu or without biases)."""
    gc, lin = getattr(model, "gc", None), getattr(model, "linear1", None)
    if (type(model).__name__ != "GCN" or not gc or lin is None or not getattr(model, "with_relu", True)
            or any(getattr(l, "weight", None) is None or getattr(l, "bias", None) is None for l in gc) or lin.bias is None):
        raise ValueError("influence_scores: the victim must be a models.gcn.GCN with relu and biases (GraphSAGE and GAT victims "
                         "are not covered)")
    return [l.weight for l in gc], [l.bias for l in gc], lin.weight, lin.bias


def influence_scores(model_or_tensors, X, adj, delta=1e-4, output="posteriors", symmetrize="max"):
    """The LinkTeller influence attack of Wu et al. (IEEE S&P 2022) on a GCN victim (mcgra_influence_scores): entry (v, u) of the
    directed matrix is || O(X with row v scaled by 1 + Delta)_u - O(X)_u ||_2 / Delta, Delta = float32(delta), O the victim's
    log-posteriors (output "log_posteriors") or their exp ("posteriors"); symmetrize "max" (the pair score
    max(I[a -> b], I[b -> a]), bitwise symmetric) or "directed" (the row is the source).  model_or_tensors: a models.gcn.GCN or
    (W, b, Wlin, blin) as gcn_forward takes them; X n x nfeat; adj any dense n x n float32 propagation matrix with a symmetric
    support, n <= 65 535, every width and the class count <= 64.  The differences are carried along the support, never two
    forwards subtracted; outside the L-hop reach of a source the entry is exactly +0.0; the same bits on every call.
    Returns (matrix, info): n x n float32 on adj's device, info = {"delta" (Delta as a float), "output", "symmetrize", "nnz"
    (non-zero cells of adj), "reached" (ordered pairs within reach), "max_reach"}.  Rank the matrix with auc_delong,
    topk_metrics and top_pairs.  ValueError, before anything is called on the device, for a bad argument; McgraError for an
    asymmetric support or a NaN / infinity in an operand or in the victim's base output."""
    if not (isinstance(output, str) and output in INFLUENCE_OUTPUTS):
        raise ValueError(f"influence_scores: output {output!r}: one of {', '.join(INFLUENCE_OUTPUTS)}")
    if not (isinstance(symmetrize, str) and symmetrize in INFLUENCE_SYMMETRIZE):
        raise ValueError(f"influence_scores: symmetrize {symmetrize!r}: one of {', '.join(INFLUENCE_SYMMETRIZE)}")
    if isinstance(delta, bool) or not isinstance(delta, (int, float, np.integer, np.floating)):
        raise ValueError(f"influence_scores: delta = {delta!r}; a number")
    with np.errstate(over="ignore"):
        d32 = float(np.float32(delta))
    if not math.isfinite(d32) or d32 == 0.0 or abs(d32) >= 1.0:
        raise ValueError(f"influence_scores: delta = {delta!r}; its float32 must be finite, not 0 and below 1 in magnitude")
    if isinstance(model_or_tensors, (tuple, list)):
        if len(model_or_tensors) != 4:
            raise ValueError("influence_scores: the victim as tensors is (W, b, Wlin, blin)")
        W, b, Wlin, blin = model_or_tensors
    else:
        W, b, Wlin, blin = victim_gcn_tensors(model_or_tensors)
    W, b = list(W), list(b)
    if not 1 <= len(W) <= _lib.MAX_LAYERS or len(b) != len(W):
        raise ValueError(f"influence_scores: {len(W)} layers with {len(b)} biases; 1 to {_lib.MAX_LAYERS} layers, one bias each")
    ts = [X, adj, Wlin, blin] + W + b
    if any(not isinstance(t, torch.Tensor) for t in ts):
        raise ValueError("influence_scores: X, adj and every weight must be tensors")
    if X.dim() != 2 or adj.dim() != 2 or adj.shape[0] != adj.shape[1] or adj.shape[0] != X.shape[0] or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"influence_scores: X of shape {tuple(X.shape)} and adj of shape {tuple(adj.shape)}; n x nfeat and n x n")
    widths = [X.shape[1]]
    for l, (w, x) in enumerate(zip(W, b)):
        if w.dim() != 2 or w.shape[0] != widths[-1] or w.shape[1] < 1 or tuple(x.shape) != (w.shape[1],):
            raise ValueError(f"influence_scores: layer {l} has a weight of shape {tuple(w.shape)} and a bias of shape "
                             f"{tuple(x.shape)} behind {widths[-1]} columns")
        widths.append(w.shape[1])
    if Wlin.dim() != 2 or Wlin.shape[1] != widths[-1] or Wlin.shape[0] < 1 or tuple(blin.shape) != (Wlin.shape[0],):
        raise ValueError(f"influence_scores: the head has a weight of shape {tuple(Wlin.shape)} and a bias of shape "
                         f"{tuple(blin.shape)} behind {widths[-1]} columns")
    if adj.shape[0] > INFLUENCE_MAX_N or max(widths[1:] + [Wlin.shape[0]]) > INFLUENCE_MAX_WIDTH:
        raise ValueError(f"influence_scores: n = {adj.shape[0]}, widths {widths[1:]}, {Wlin.shape[0]} classes; up to "
                         f"{INFLUENCE_MAX_N} nodes and {INFLUENCE_MAX_WIDTH} columns")
    return _influence_scores(adj, X, W, b, Wlin, blin, float(delta), INFLUENCE_OUTPUTS.index(output),
                             INFLUENCE_SYMMETRIZE.index(symmetrize))


@_device_operands
def _influence_scores(adj, X, W, b, Wlin, blin, delta, output, symmetrize):
    dev = adj.device
    adj = _rows_f32(adj, dev)
    X, Wlin, blin = (_f32(t).to(dev) for t in (X, Wlin, blin))
    W, b = [_f32(w).to(dev) for w in W], [_f32(x).to(dev) for x in b]
    n, nfeat = X.shape
    L = len(W)
    dims = (C.c_int32 * (L + 1))(*([nfeat] + [w.shape[1] for w in W]))
    Wp = (C.c_void_p * L)(*[w.data_ptr() for w in W])
    bp = (C.c_void_p * L)(*[x.data_ptr() for x in b])
    out = torch.empty(n, n, device=dev, dtype=torch.float32)
    counts = (C.c_int64 * 3)()
    check(lib.mcgra_influence_scores(_stream(), n, nfeat, L, dims, _p(X), _p(adj), adj.stride(0), Wp, bp, _p(Wlin), _p(blin),
                                     Wlin.shape[0], delta, output, symmetrize, _p(out), out.stride(0), counts))
    info = {"delta": float(np.float32(delta)), "output": INFLUENCE_OUTPUTS[output], "symmetrize": INFLUENCE_SYMMETRIZE[symmetrize],
            "nnz": int(counts[0]), "reached": int(counts[1]), "max_reach": int(counts[2])}
    return out, info


# ---------------------------------------------------------------- the engine
def attack_config(n, dims, nclass, emb_nlayer, measure, weight_sup, weight_param, lr, num_edges, n_attack, eps=0.0,
                  act="relu", head_act="none", has_self=False, fin_layers=(1, 2), plan=None):
    """mcgra_attack_config_t of these arguments (AttackEngine's, without the device)."""
    dims = [int(d) for d in dims]
    cfg = AttackConfig()
    cfg.n, cfg.nfeat, cfg.nclass = int(n), dims[0], int(nclass)
    cfg.nlayer, cfg.emb_nlayer = len(dims) - 1, int(emb_nlayer)
    for i, d in enumerate(dims):
        cfg.dims[i] = d
    if measure not in _lib.MEASURES:
        raise ValueError(f"measure {measure!r}: topology_attack.py:194-208 knows {sorted(_lib.MEASURES)}")
    cfg.measure = _lib.MEASURES[measure]
    cfg.n_attack = int(n_attack)
    cfg.weight_sup = float(weight_sup)
    for i in range(10):
        cfg.w[i] = float(weight_param[i])
    cfg.lr, cfg.eps = float(lr), float(eps)
    cfg.num_edges = float(min(num_edges, 1e300))
    # plan: a sharded.RowBlockPlan makes this engine one of plan.world row-block ranks (include/mcgra.h)
    cfg.row_begin, cfg.row_end = (0, cfg.n) if plan is None else (int(plan.row_begin), int(plan.row_end))
    cfg.shard_world, cfg.shard_rows = (0, 0) if plan is None else (int(plan.world), int(plan.rows_per_rank))
    cfg.act = {"relu": 0, "elu": 1}[act]
    cfg.head_act = {"none": 0, "elu": 1}[head_act]
    cfg.has_self = int(bool(has_self))
    cfg.fin_layers[0], cfg.fin_layers[1] = int(fin_layers[0]), int(fin_layers[1])
    return cfg


def attack_plan(cfg):
    """What mcgra_attack_create would decide for this AttackConfig in this environment (mcgra_attack_plan): needs no device.
    Returns the _lib.AttackPlan (.flags(): its diagnostic text as a dict)."""
    out = _lib.AttackPlan()
    check(lib.mcgra_attack_plan(C.byref(cfg), C.byref(out)))
    return out


class AttackEngine:
    """One mcgra_attack_t.  Mirrors the state PGDAttack keeps across the loop of
    topology_attack.py:161-298 (adj_changes + Adam moments) in HBM."""

    def __init__(self, n, dims, nclass, emb_nlayer, measure, weight_sup, weight_param, lr, num_edges,
                 n_attack, eps=0.0, device="cuda:0", act="relu", head_act="none", has_self=False, fin_layers=(1, 2),
                 plan=None):
        _lib.require_device()
        self.device = torch.device(device)
        self.n, self.nclass, self.dims = int(n), int(nclass), list(int(d) for d in dims)
        cfg = attack_config(n, dims, nclass, emb_nlayer, measure, weight_sup, weight_param, lr, num_edges, n_attack, eps, act,
                            head_act, has_self, fin_layers, plan)
        self._h = C.c_void_p(0)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_create(C.byref(self._h), C.byref(cfg)))
        self.cfg = cfg
        self._keep = []

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib.mcgra_attack_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_model(self, W, b, Wlin, blin, Ws=None):
        dev = self.device
        Ws = [_dev_f32(w, dev) for w in Ws] if Ws is not None else None
        W = [_dev_f32(w, dev) for w in W]
        b = [_dev_f32(x, dev) for x in b]
        Wlin, blin = _dev_f32(Wlin, dev), _dev_f32(blin, dev)
        L = len(W)
        Wp = (C.c_void_p * L)(*[w.data_ptr() for w in W])
        bp = (C.c_void_p * L)(*[x.data_ptr() for x in b])
        Wsp = (C.c_void_p * L)(*[w.data_ptr() for w in Ws]) if Ws is not None else None
        with torch.cuda.device(dev):
            check(lib.mcgra_attack_set_model(self._h, _stream(), Wp, bp, _p(Wlin), _p(blin), Wsp))
            torch.cuda.current_stream().synchronize()

    def set_graph(self, features, adj, ori_adj, feature_adj, labels, idx_attack):
        dev = self.device
        X = _dev_f32(features, dev)
        A = _dev_f32(adj, dev)
        F = _dev_f32(feature_adj, dev)
        O = None
        if ori_adj is not None:
            O = _dev_f32(ori_adj, dev)
            if not bool((O != 0).any()):
                O = None          # dataset.init_matrix (dataset.py:433): all zeros
        lab = _dev_i32(labels, dev)
        idx = _dev_i32(idx_attack, dev)
        with torch.cuda.device(dev):
            check(lib.mcgra_attack_set_graph(self._h, _stream(), _p(X), _p(A), _p(O), _p(F), _p(lab), _p(idx)))

    def set_adj_changes(self, packed):
        t = _dev_f32(packed, self.device)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_set_adj_changes(self._h, _stream(), _p(t)))
            torch.cuda.current_stream().synchronize()

    def get_adj_changes(self):
        n = self.n
        out = torch.empty(n * (n - 1) // 2, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_get_adj_changes(self._h, _stream(), _p(out)))
        return out

    def step(self, want_scalars=False, noise=None):
        with torch.cuda.device(self.device):
            if want_scalars:
                buf = (C.c_double * 10)()
                check(lib.mcgra_attack_step(self._h, _stream(), _p(noise), buf))
                keys = ("loss", "origin_loss", "c1", "c2", "c6", "c7", "c9", "c10", "clamp_sum", "nll")
                return dict(zip(keys, list(buf)))
            check(lib.mcgra_attack_step(self._h, _stream(), _p(noise), None))
        return None

    # ---- row-block sharded step (mcgra_attack_shard_*, driven by mc-gra_amd/sharded.py) ----------------------------
    def exchange_bytes(self):
        return int(lib.mcgra_attack_exchange_bytes(self._h))

    def bind_exchange(self, arena):
        assert arena.dtype == torch.uint8 and arena.is_contiguous() and arena.device == self.device
        self._keep.append(arena)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_bind_exchange(self._h, _p(arena), arena.numel()))

    def shard_begin(self, what, want_scalars=False):
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_shard_begin(self._h, _stream(), int(what), int(bool(want_scalars))))

    def shard_next(self):
        ex = _lib.Exchange()
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_shard_next(self._h, _stream(), C.byref(ex)))
        return (ex.kind, ex.count, ex.offset, ex.offset2, ex.chunk_bytes)

    def shard_scalars(self):
        buf = (C.c_double * 10)()
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_shard_scalars(self._h, _stream(), buf))
        keys = ("loss", "origin_loss", "c1", "c2", "c6", "c7", "c9", "c10", "clamp_sum", "nll")
        return dict(zip(keys, list(buf)))

    def get_rows(self):
        """Rows [row_begin, row_end) of the learnable adjacency (dense form of adj_changes)."""
        r0, r1 = self.cfg.row_begin, (self.cfg.row_end or self.n)
        out = torch.empty(max(r1 - r0, 0), self.n, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_get_rows(self._h, _stream(), _p(out)))
        return out

    def product_mode(self):
        """0: fp32 MFMA SYMM, 1: bf16 split through hipBLASLt, 2: bf16 split, hand-written kernel (mcgra_attack_product_mode)."""
        return int(lib.mcgra_attack_product_mode(self._h))

    def path_stats(self):
        a, b = C.c_longlong(0), C.c_longlong(0)
        check(lib.mcgra_attack_path_stats(self._h, C.byref(a), C.byref(b)))
        return {"lowrank_steps": a.value, "general_steps": b.value}

    def fused_steps(self):
        """Low-rank steps that ran as the fused step (mcgra_attack_fused_steps)."""
        return int(lib.mcgra_attack_fused_steps(self._h))

    def gram_split_steps(self):
        """Gram-evaluation steps whose products ran on the fp16 split kernel (mcgra_attack_gram_split_steps)."""
        return int(lib.mcgra_attack_gram_split_steps(self._h))

    def leading_dim(self):
        ptr, r, c, ld = C.c_void_p(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib.mcgra_attack_buffer(self._h, b"M", C.byref(ptr), C.byref(r), C.byref(c), C.byref(ld)))
        return ld.value

    def monitor(self, want_sparsity=False):
        out = torch.empty(self.n, self.nclass, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            if want_sparsity:
                s = C.c_double(0)
                check(lib.mcgra_attack_monitor(self._h, _stream(), _p(out), C.byref(s)))
                return out, s.value
            check(lib.mcgra_attack_monitor(self._h, _stream(), _p(out), None))
        return out, None

    def finalize(self, decode_mode, H_A=None, Y_A=None, label_adj=None):
        dev = self.device
        H_A = _dev_f32(H_A, dev) if H_A is not None else None
        Y_A = _dev_f32(Y_A, dev) if Y_A is not None else None
        label_adj = _dev_f32(label_adj, dev) if label_adj is not None else None
        out = torch.empty(self.n, self.n, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            check(lib.mcgra_attack_finalize(self._h, _stream(), int(decode_mode), _p(H_A), _p(Y_A), _p(label_adj),
                                            _p(out)))
            torch.cuda.current_stream().synchronize()
        return out

    def finalize_components(self, decode_mode, H_A=None, Y_A=None, label_adj=None, out_mask=None, want_out=True):
        """finalize with its summands kept apart (mcgra_attack_finalize_components): (out, comps, present) -- comps the
        [8, n, n] stack in the order of ENSEMBLE_COMPONENTS (the slot of an input that is None: zeros), present the mask of the
        slots that were written, out the float32 sum of the components of out_mask in ascending order (None: every present one;
        then finalize's out bit for bit), or None with want_out=False.  8 n^2 floats stay on the device."""
        dev = self.device
        H_A = _dev_f32(H_A, dev) if H_A is not None else None
        Y_A = _dev_f32(Y_A, dev) if Y_A is not None else None
        label_adj = _dev_f32(label_adj, dev) if label_adj is not None else None
        have = ENSEMBLE_BASE | (H_A is not None) << 5 | (Y_A is not None) << 6 | (label_adj is not None) << 7
        out_mask = have if out_mask is None else int(out_mask)
        out = torch.empty(self.n, self.n, device=dev, dtype=torch.float32) if want_out else None
        comps = torch.empty(len(ENSEMBLE_COMPONENTS), self.n, self.n, device=dev, dtype=torch.float32)
        present = C.c_uint(0)
        with torch.cuda.device(dev):
            for k in range(len(ENSEMBLE_COMPONENTS)):
                if not have >> k & 1:
                    comps[k].zero_()
            check(lib.mcgra_attack_finalize_components(self._h, _stream(), int(decode_mode), _p(H_A), _p(Y_A), _p(label_adj),
                                                       out_mask, _p(out), _p(comps), C.byref(present)))
            torch.cuda.current_stream().synchronize()
        return out, comps, int(present.value)

    def buffer(self, name):
        """Copy of a named intermediate (parity tests)."""
        ptr, r, c, ld = C.c_void_p(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib.mcgra_attack_buffer(self._h, name.encode(), C.byref(ptr), C.byref(r), C.byref(c), C.byref(ld)))
        out = torch.empty(r.value, c.value, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_copy_buffer(self._h, _stream(), name.encode(), _p(out), c.value))
            torch.cuda.current_stream().synchronize()
        return out

    def masked_fused_steps(self):
        """Fused steps whose decode relu-masked pairs of live embedding rows (they stand; only a dead row falls back)."""
        return int(lib.mcgra_attack_masked_fused_steps(self._h))

    def cut_product_steps(self):
        """Steps whose product was cut in two: a row-block rank's so that the P1 all-to-all runs beside its own row panels, a
        large monolithic graph's so that the tail's first pass runs beside the product's last rounds."""
        return int(lib.mcgra_attack_cut_product_steps(self._h))

    def product_replay(self, reps=10):
        """Mean launch time [ms] of `reps` back-to-back launches of the last fused step's N x N x N product, nothing beside
        them (mcgra_attack_product_replay: a measurement aid, no engine state changes)."""
        ms = C.c_double(0)
        with torch.cuda.device(self.device):
            check(lib.mcgra_attack_product_replay(self._h, _stream(), int(reps), C.byref(ms)))
        return ms.value

    def test_mutate(self, what):
        """TEST ONLY (mcgra_attack_test_mutate): 'p1' wipes the product's result, 'rk' drops the tail's rank-k terms, 'calc' drops
        the MSELoss / KL per-pair terms c1 / c2, 'klstats' wipes the KL row statistics, None disarms."""
        check(lib.mcgra_attack_test_mutate(self._h, {None: 0, "p1": 1, "rk": 2, "calc": 3, "klstats": 4}[what]))

    def profile(self, enable=True):
        check(lib.mcgra_attack_profile(self._h, int(enable)))

    def gemm_stats(self, reset=True):
        n, ms, fl = C.c_int64(0), C.c_double(0), C.c_double(0)
        check(lib.mcgra_attack_gemm_stats(self._h, int(reset), C.byref(n), C.byref(ms), C.byref(fl)))
        return dict(launches=n.value, ms=ms.value, flops=fl.value)
