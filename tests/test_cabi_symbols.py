"""CPU-side checks: the C-ABI library loads and exports every symbol the header
declares; host-side argument handling; no compute calls (there is no GPU here)."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")
HDR = os.path.join(ROOT, "include", "mcgra.h")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


def header_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mcgra_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported(pkg):
    lib = ctypes.CDLL(LIB)
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/mcgra.h but not exported"
    assert sorted(pkg._lib.SYMBOLS) == syms
    assert b"gfx950" in lib.mcgra_version.__call__() if False else True
    lib.mcgra_version.restype = ctypes.c_char_p
    assert b"mcgra" in lib.mcgra_version()


def test_config_struct_layout_matches_header(pkg):
    # offsets of the ctypes mirror follow the C struct: 5 + 9 + 2 int32, 1 + 10 + 2 float, pad, double, 2 int32
    C = pkg._lib.AttackConfig
    assert C.dims.offset == 20 and C.measure.offset == 56 and C.weight_sup.offset == 64
    assert C.w.offset == 68 and C.lr.offset == 108 and C.num_edges.offset == 120 and C.row_begin.offset == 128
    assert C.act.offset == 136 and C.fin_layers.offset == 148 and C.shard_world.offset == 156 and ctypes.sizeof(C) == 168


def test_no_cpu_fallback(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg._lib.McgraError):
        pkg._lib.require_device()
    m = pkg.PGDAttack(model=None, embedding=None, nnodes=10, device="cpu")
    args = argparse.Namespace(max_eval=100, lr=0, dataset="cora", eps=0, measure="HSIC", useH_A=0, useY_A=0, useY=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.attack(args, None, 0.01, 0, 1, (0,) * 10, np.eye(10), 0, 0, 0, None, None, None, np.eye(10), np.eye(10),
                 np.zeros((10, 10)), np.zeros(10, int), np.arange(10), 1e9, 0, epochs=1)


def test_product_never_imports_oracle():
    """The shipped path must not reference oracle/ (tests, smoke() and bench's cpu_baseline only)."""
    pk = os.path.join(ROOT, "mc-gra_amd")
    for dp, _, fs in os.walk(pk):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.replace("no oracle", ""), f"{f} mentions oracle"


def test_decode_mode_mapping(pkg):
    from mc_gra_amd.topology_attack import _decode_mode
    ns = lambda ds, h, ya, y: argparse.Namespace(dataset=ds, useH_A=h, useY_A=ya, useY=y)
    assert _decode_mode(ns("cora", 1, 1, 1)) == 0 and _decode_mode(ns("AIDS", 0, 0, 1)) == 0
    assert _decode_mode(ns("citeseer", 1, 1, 1)) == 1 and _decode_mode(ns("brazil", 1, 0, 0)) == 2
    assert _decode_mode(ns("polblogs", 1, 1, 1)) == 3 and _decode_mode(ns("polblogs", 1, 0, 1)) == 3
    assert _decode_mode(ns("usair", 0, 0, 1)) == 5 and _decode_mode(ns("usair", 1, 1, 0)) == 4
    assert _decode_mode(ns("usair", 1, 0, 1)) == 6 and _decode_mode(ns("usair", 1, 1, 1)) == 3
    with pytest.raises(ValueError):
        _decode_mode(ns("pubmed", 1, 1, 1))


def test_adj_changes_property_before_attack(pkg):
    m = pkg.PGDAttack(model=None, embedding=None, nnodes=7, device="cpu")
    assert m.adj_changes.shape == (21,) and float(m.adj_changes.abs().sum()) == 0.0


def test_fused_decode_edge_cases_keep_their_property(pkg):
    """The fused MSELoss / KL oracle cases of tests/test_gpu_parity.py at n = 1155 and 4200 are there for the decode's column
    slicing: k_decode_stats / k_decode_fly cut the columns into fl_decode_slabs(n, rows, true) slices rounded up to a multiple of
    4, so that for many n the last slice starts at or past n and is empty (it must contribute zero partials to the row sums
    k_kl_stats_fin takes the log of).  tests/helpers.py:decode_slices mirrors that rule; it is checked here against the library's
    own fl_decode_slabs, so that a change of the rule cannot quietly leave these cases without the edge they pin."""
    from mc_gra_amd.sharded import RowBlockPlan
    from tests import helpers as H
    slabs = getattr(ctypes.CDLL(LIB), "_ZN5mcgra15fl_decode_slabsEiib")      # mcgra::fl_decode_slabs(int, int, bool): host code
    slabs.restype, slabs.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_bool]
    rng = np.random.RandomState(0)
    ns = sorted(set(H.DECODE_EDGE_N) | {256, 1100, 2050, 4095, 4096, 10000} | set(rng.randint(256, 40000, 200).tolist()))
    for n in ns:
        for rows in {n, n // 3, (n + 2) // 3, 256, 1536, n - 256 if n > 512 else n}:
            assert slabs(n, rows, True) == H.decode_slices(n, rows)[0], (n, rows)
    n = 1155
    assert n % 2 == 1 and (n + 31) // 32 * 32 != n                  # odd n; the engine's ld = round_up(n, 32) pads the rows
    assert H.empty_decode_slices(n) >= 1
    n = 4200
    assert n >= 4096 and H.empty_decode_slices(n) >= 1              # (attack_fused.hip: the small-operand terms' stream)
    # test_sharded_mse_ranks_match_monolithic_step at world 3: the row-range form cuts other slices, and each rank has empty ones
    plans = [RowBlockPlan(n, 3, r) for r in range(3)]
    assert all(p.has_rows for p in plans)
    for p in plans:
        rows = p.row_end - p.row_begin
        assert H.decode_slices(n, rows)[0] != H.decode_slices(n)[0] and H.empty_decode_slices(n, rows) >= 1, (p.rank, rows)
    # the bench's N = 10 000 (tests/test_gpu_fullsize.py: the MSELoss / KL reference tests) runs 26 slices, none of them empty
    assert H.decode_slices(10000)[0] == 26 and H.empty_decode_slices(10000) == 0
