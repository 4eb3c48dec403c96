"""The forward's skinny products on the three-plane bf16 kernel (skinny_x3.hip) and the N x N x N product forked behind the
early pack, beside that forward (attack_fused.hip: fork_p1).  Run with -m gpu."""
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


@pytest.fixture(scope="module")
def E(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + ".engine")


def _errs(y, ref):
    d = (y.double() - ref).abs()
    scale = ref.abs().max().item()
    return d.max().item() / scale, (d.pow(2).mean().sqrt().item()) / scale


@pytest.mark.parametrize("n", [10000, 2708, 1283])
def test_skinny_x3_against_fp64_and_gemm_f32(E, n):
    """Y = M V at the widths of the forward ([r o Tv | Tu] of 16-wide layers, and the 33-column form with r): max and rms
    error against float64 in the class of the fp32 GEMM it replaces (gemm_f32), on an adjacency-like M in [0, 1] whose rows
    are padded to 128-byte lines as the engine keeps them; n = 1283 is a multiple of neither 32 nor 256."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(n)
    ld = (n + 31) & ~31
    base = torch.rand(n, ld, device="cuda:0", generator=g)
    base[:, n:] = float("nan")                           # (padding columns are never read)
    M = base[:, :n]
    M[torch.rand(n, n, device="cuda:0", generator=g) < 0.9] = 0.0
    M64 = M.double()
    for nc in (16, 32, 33):
        V = torch.randn(n, nc, device="cuda:0", generator=g) * 0.3
        ref = M64 @ V.double()
        y = E.sgemm_skinny_x3(M, V)
        yf = E.sgemm(M.contiguous(), V)
        assert torch.isfinite(y).all()
        mx, rms = _errs(y, ref)
        mxf, rmsf = _errs(yf, ref)
        assert mx < 4 * mxf + 1e-7 and rms < 4 * rmsf + 1e-8, (nc, mx, rms, mxf, rmsf)
        assert mx < 2e-6, (nc, mx)


def test_product_behind_the_pack_is_bit_identical(pkg, monkeypatch):
    """The product forked behind the early pack, beside the forward (MCGRA_P1_BEHIND_PACK default with MCGRA_FWD_X3), against
    the product forked behind the forward (MCGRA_P1_BEHIND_PACK=0) with the same forward kernel: same bits over steps with
    and without monitor calls in front of them, through an adjacency replaced while a monitor call's pack is in flight; the
    learnable adjacency stays bitwise symmetric."""
    import torch
    z = H.synthetic_case(1283, 11, (16, 16), 4, seed=23)
    monkeypatch.setenv("MCGRA_FWD_X3", "1")
    early = H.engine_from(pkg, z)
    monkeypatch.setenv("MCGRA_P1_BEHIND_PACK", "0")
    late = H.engine_from(pkg, z)
    monkeypatch.delenv("MCGRA_P1_BEHIND_PACK")
    monkeypatch.delenv("MCGRA_FWD_X3")
    a1 = H.init_adj_changes(1283, 98, 0.03)
    for t in range(7):
        for e in (early, late):
            if t != 3:
                e.monitor()
            e.step()
            if t == 4:
                e.monitor()
                e.set_adj_changes(a1)          # the monitor call above has forked a pack of the OLD adjacency
        assert torch.equal(early.get_adj_changes(), late.get_adj_changes()), t
        assert torch.equal(early.buffer("G_sym"), late.buffer("G_sym")), t
        m = early.buffer("M")
        assert torch.equal(m, m.t()), t
    assert early.fused_steps() == 7 and late.fused_steps() == 7
    la, lb = early.monitor()[0], late.monitor()[0]
    assert torch.equal(la, lb)

