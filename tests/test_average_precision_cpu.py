"""CPU-side checks of the average precision beside the AUC (mcgra_rank_metrics, mcgra_decode_rank_metrics, main.py --ap):
the truth helper of the GPU tests against sklearn, the resolving power of the test inputs, the command line, the C ABI of the
two entries and their refusals before a device is touched (no compute: there is no GPU here)."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import ap_truth as T

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
def cases():
    from tests.test_gpu_auc import CASES
    return CASES


@pytest.mark.parametrize("name", ["all_equal", "negative_subnormal", "perm", "quantised", "repeats", "signed_zeros", "subset"])
def test_truth_helper_equals_sklearn(cases, name):
    real, pred, idx = cases[name]
    got, ref = T.average_precision(real, pred, idx), T.sklearn_average_precision(real, pred, idx)
    print(f"{name}: helper {got!r} sklearn {ref!r} diff {abs(got - ref):.3e}")
    assert abs(got - ref) <= 1e-15, (name, got, ref)
    assert 0.0 < got < 1.0


def test_the_cases_are_the_seven(cases):
    assert sorted(cases) == ["all_equal", "negative_subnormal", "perm", "quantised", "repeats", "signed_zeros", "subset"]


def test_quantised_case_resolves_the_tie_convention(cases):
    """With five score levels most positives are tied with negatives: counting a tie (>=, average precision) and not counting
    it (>) are 6e-2 apart, far beyond any tolerance the GPU tests use."""
    real, pred, idx = cases["quantised"]
    ge, gt = T.average_precision(real, pred, idx), T.average_precision(real, pred, idx, strict=True)
    print(f"quantised: >= {ge!r}  > {gt!r}")
    assert abs(ge - gt) > 1e-2, (ge, gt)


def test_truth_helper_single_class_and_exact_form():
    rng = np.random.RandomState(0)
    s = rng.rand(20, 20).astype(np.float32)
    assert math.isnan(T.average_precision(np.zeros((20, 20), np.float32), s))
    assert T.average_precision(np.ones((20, 20), np.float32), s) == 1.0
    lab = (rng.rand(20, 20) < 0.3).astype(np.float32)
    q5 = (rng.randint(0, 4, (20, 20)) * 0.5).astype(np.float32)
    p, q = T.level_counts(lab, q5)
    assert abs(T.from_counts(p, q) - T.from_counts_exact(p, q)) <= 1e-15
    assert T.from_counts(p, q) == T.average_precision(lab, q5)


def test_parser_has_ap_and_it_is_off(pkg):
    from mc_gra_amd import main as M
    p = M.build_parser()
    assert p.parse_args([]).ap is False
    assert p.parse_args(["--ap"]).ap is True
    assert p.parse_args(["--mode", "notrain_test", "--ap"]).ap is True
    assert "--ap" in M.__doc__


def test_rank_metric_entries_are_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    lib = ctypes.CDLL(LIB)
    for s in ("mcgra_rank_metrics", "mcgra_decode_rank_metrics"):
        assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(pkg._lib.lib, s).restype is ctypes.c_int
    assert len(pkg._lib.lib.mcgra_rank_metrics.argtypes) == 10 and len(pkg._lib.lib.mcgra_decode_rank_metrics.argtypes) == 12
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()
    from mc_gra_amd import engine as E
    for f in ("rank_metrics", "average_precision", "decode_rank_metrics", "decode_average_precision"):
        assert callable(getattr(E, f)), f


def test_rank_metric_entries_refuse_before_touching_a_device(pkg):
    """Argument, size, width and mode checks come first: they need no GPU (the pointers here are never followed).  The same
    codes as mcgra_roc_auc / mcgra_decode_auc give for the same arguments, plus auc = ap = NULL."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    a, b = ctypes.c_double(), ctypes.c_double()
    A, B = ctypes.byref(a), ctypes.byref(b)

    def rm(n, ldl=8, lds=8, idx=None, n_idx=None, auc=A, ap=B, lab=p, sc=p):
        return L.mcgra_rank_metrics(None, n, lab, ldl, sc, lds, idx, n if n_idx is None else n_idx, auc, ap)

    def roc(n, ldl=8, lds=8, idx=None, n_idx=None, lab=p, sc=p):
        return L.mcgra_roc_auc(None, n, lab, ldl, sc, lds, idx, n if n_idx is None else n_idx, A)

    assert rm(8, auc=None, ap=None) == -1 and b"rank_metrics" in L.mcgra_last_error()
    for kw in (dict(n=0), dict(n=8, ldl=7), dict(n=8, lds=7), dict(n=8, idx=p, n_idx=0), dict(n=8, lab=None), dict(n=8, sc=None)):
        assert rm(**kw) == -1 and roc(**kw) == -1, kw
        assert rm(auc=None, **kw) == -1 and rm(ap=None, **kw) == -1, kw
    big = dict(n=65536, ldl=65536, lds=65536)
    assert rm(**big) == -3 and roc(**big) == -3
    assert rm(8, idx=p, n_idx=65536) == -3 and roc(8, idx=p, n_idx=65536) == -3

    def drm(n, d, ldz, mode, ldl=8, auc=A, ap=B):
        return L.mcgra_decode_rank_metrics(None, n, d, p, ldz, mode, p, ldl, None, n, auc, ap)

    def dauc(n, d, ldz, mode, ldl=8):
        return L.mcgra_decode_auc(None, n, d, p, ldz, mode, p, ldl, None, n, A)

    assert drm(8, 4, 4, 0, auc=None, ap=None) == -1 and b"decode_rank_metrics" in L.mcgra_last_error()
    assert drm(8, 129, 129, 0) == -3 and b"129" in L.mcgra_last_error() and dauc(8, 129, 129, 0) == -3
    for mode in (3, 5, 6):
        assert drm(8, 4, 4, mode) == -3 and dauc(8, 4, 4, mode) == -3
    for args in ((8, 4, 4, 7), (8, 4, 4, -1), (8, 4, 3, 0), (0, 4, 4, 0), (8, 0, 4, 0)):
        assert drm(*args) == -1 and dauc(*args) == -1, args
    assert drm(8, 4, 4, 0, ldl=7) == -1 and dauc(8, 4, 4, 0, ldl=7) == -1
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(drm(8, 200, 200, 4, auc=None))


def test_engine_entries_refuse_wrong_shapes_before_touching_a_device(pkg):
    """The shape checks of roc_auc / decode_auc, on host tensors: nothing reaches the library (__wrapped__: without the
    device guard, which would itself refuse a host tensor)."""
    import torch
    from mc_gra_amd import engine as E
    sq, wide, other = torch.zeros(5, 5), torch.zeros(5, 6), torch.zeros(4, 4)
    for f in (E.rank_metrics, E.average_precision, E.roc_auc):
        for real, pred in ((wide, wide), (sq, other), (sq, wide), (torch.zeros(5), sq)):
            with pytest.raises(AssertionError):
                f.__wrapped__(real, pred)
    for f in (E.decode_rank_metrics, E.decode_average_precision, E.decode_auc):
        for real, Z in ((wide, torch.zeros(5, 3)), (sq, torch.zeros(4, 3)), (sq, torch.zeros(5))):
            with pytest.raises(AssertionError):
                f.__wrapped__(real, Z, 0)
