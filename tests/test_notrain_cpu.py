"""CPU-side checks of main.py --mode notrain_test: the dataset -> decode mode rule, the command line, the C ABI of the two
entries it runs on, and which engine call each prior takes (no compute: there is no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


def test_decode_branch_follows_main_dot_product_decode(pkg):
    from mc_gra_amd import main as M
    assert [M.decode_branch(d) for d in ("cora", "citeseer", "AIDS")] == [0, 0, 0]
    assert [M.decode_branch(d) for d in ("brazil", "usair", "polblogs")] == [4, 4, 4]


def test_parser_offers_the_three_modes(pkg):
    from mc_gra_amd import main as M
    p = M.build_parser()
    assert p.parse_args([]).mode == "evaluate"
    for mode in ("evaluate", "prepare", "notrain_test"):
        assert p.parse_args(["--mode", mode]).mode == mode
    with pytest.raises(SystemExit):
        p.parse_args(["--mode", "search"])
    assert "notrain_test" in M.__doc__


def test_decode_entries_are_declared_exported_and_bound(pkg):
    from tests.test_cabi_symbols import header_symbols
    lib = ctypes.CDLL(LIB)
    for s in ("mcgra_decode_auc", "mcgra_decode_scores"):
        assert s in header_symbols() and s in pkg._lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(pkg._lib.lib, s).restype is ctypes.c_int
    assert len(pkg._lib.lib.mcgra_decode_auc.argtypes) == 11 and len(pkg._lib.lib.mcgra_decode_scores.argtypes) == 8
    assert sorted(pkg._lib.SYMBOLS) == header_symbols()


def test_prior_aucs_routes_each_prior(pkg, monkeypatch):
    """The two matrices through roc_auc, thin priors through decode_auc, a prior wider than 128 columns through
    decode_scores + roc_auc; the dataset picks the mode."""
    import torch
    from mc_gra_amd import main as M
    calls = []

    def roc_auc(real, pred, idx=None):
        calls.append(("roc_auc", tuple(pred.shape), idx))
        return 0.25

    def decode_auc(real, Z, mode, idx=None):
        calls.append(("decode_auc", tuple(Z.shape), mode, idx))
        return 0.75

    def decode_scores(Z, mode):
        calls.append(("decode_scores", tuple(Z.shape), mode))
        return torch.zeros(Z.shape[0], Z.shape[0])

    monkeypatch.setattr(M.engine, "roc_auc", roc_auc)
    monkeypatch.setattr(M.engine, "decode_auc", decode_auc)
    monkeypatch.setattr(M.engine, "decode_scores", decode_scores)
    n = 9
    adj, fa = torch.eye(n), torch.zeros(n, n)
    lab = np.ones((n, n), np.float32)
    res = M.prior_aucs(adj, fa, torch.zeros(n, 129), torch.zeros(n, 128), torch.zeros(n, 4), lab, "cora")
    assert res == {"feature": 0.25, "layer1": 0.25, "layer2": 0.75, "out": 0.75, "label": 0.25}
    assert calls == [("roc_auc", (n, n), None), ("decode_scores", (n, 129), 0), ("roc_auc", (n, n), None),
                     ("decode_auc", (n, 128), 0, None), ("decode_auc", (n, 4), 0, None), ("roc_auc", (n, n), None)]
    del calls[:]
    M.prior_aucs(adj, fa, torch.zeros(n, 16), torch.zeros(n, 16), torch.zeros(n, 4), lab, "usair")
    assert [c[2] for c in calls if c[0] == "decode_auc"] == [4, 4, 4]


def test_decode_entries_refuse_before_touching_a_device(pkg):
    """Width, mode and argument checks come first: they need no GPU (the pointers here are never followed)."""
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    out = ctypes.c_double()
    auc = lambda n, d, ldz, mode, ldl=8: L.mcgra_decode_auc(None, n, d, p, ldz, mode, p, ldl, None, n, ctypes.byref(out))
    assert auc(8, 129, 129, 0) == -3 and b"129" in L.mcgra_last_error()
    for mode in (3, 5, 6):
        assert auc(8, 4, 4, mode) == -3
        assert L.mcgra_decode_scores(None, 8, 4, p, 4, mode, p, 8) == -3
    for bad in (auc(8, 4, 4, 7), auc(8, 4, 4, -1), auc(8, 4, 3, 0), auc(0, 4, 4, 0), auc(8, 0, 4, 0), auc(8, 4, 4, 0, ldl=7),
                L.mcgra_decode_scores(None, 8, 4, p, 4, 0, p, 7), L.mcgra_decode_scores(None, 8, 4, p, 4, 9, p, 8)):
        assert bad == -1
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(auc(8, 200, 200, 4))
