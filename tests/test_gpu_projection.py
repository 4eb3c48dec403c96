"""The edge-budget projection (PGDAttack.projection + bisection, topology_attack.py:338-347, 397-412; project() in
mc-gra_amd/csrc/attack.hip) behind every Adam kernel that can run in front of it, pinned to the EXACT root of its own
pre-projection state.  Run with -m gpu.

The yardstick does not depend on the gradient.  After a step the engine's own Adam moments give back, in float32, the state
a_pre the Adam kernel must have left for project() (helpers.pre_projection_state), and the float64 root miu* of
sum(clip(a_pre - x, 0, 1)) = num_edges (helpers.exact_projection_root) gives what the projection must make of it.  Adam's +-lr
moves on noise-level gradients, which force the 2e-3 of test_projection_bisection_matches_oracle, never reach the comparison.

The bound on an entry, with K the number of entries strictly between the clamps at the root (the slope of the sum):

    tol = 1e-5 + 2^-23 * num_edges / K + 2^-21

  1e-5                     the reference's bisection epsilon: its last midpoint is an endpoint of a bracket narrower than 1e-5
                           that holds the root;
  2^-23 * num_edges / K    one float32 rounding of the sum the bisection compares with the budget (the reference sums in
                           float32, the engine rounds its float64 sum to float32), divided by the slope: how far in x that moves
                           the sign change;
  2^-21                    the float32 reconstruction of a_pre (an ulp of a value in [1, 2) is 2^-23; the kernels contract
                           p - step * (m / denom) into one fused multiply-add, numpy rounds twice) and the float32 subtraction
                           a_pre - miu, on both sides of the comparison.

The start (helpers.projection_case) is uniform on [0, 1.05), so about 4 % of the entries exceed 1 before the projection whatever
the gradient's sign: an Adam kernel that clamps although the projection is still to come -- clip(clip(a, 0, 1) - miu, 0, 1) in
place of clip(a - miu, 0, 1) -- moves them by up to 0.05.  tests/test_projection_cases_cpu.py holds the properties of every case.

Measured distances per case: DESIGN.md, beside the description of the tail and the projection."""
import numpy as np
import pytest

from oracle import mcgra_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

FUSED = ("fused_mse_300", "fused_kl_300", "fused_hsic_1100")
# the routes of the free-running tests: the fused steps in front of project() (MSELoss and KL: any n >= 256; HSIC: split product,
# early pack) and the general step's one-pass tail
STATE_ROUTES = ("fused_mse_300", "fused_kl_300", "fused_hsic_1100", "rankk_adam_hsic_300")


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def tol_of(num_edges, K):
    return 1e-5 + 2.0 ** -23 * float(num_edges) / K + 2.0 ** -21


def make_engine(pkg, monkeypatch, cid, num_edges):
    """(engine, inputs) of a projection case with the given budget; `num_edges` may be "tight" / "loose" (helpers.PROJ_BUDGETS)."""
    n, measure, ori, env = H.PROJ_CASES[cid]
    z = H.projection_case(n, measure, ori)
    z["num_edges"] = np.array(H.projection_budget(z, num_edges) if isinstance(num_edges, str) else float(num_edges))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = H.engine_from(pkg, z)
    for k in env:
        monkeypatch.delenv(k)
    return eng, z


def packed(eng, name):
    return O.pack_tril(eng.buffer(name).cpu().numpy())


def assert_route(eng, cid, steps, z=None):
    """The case took the Adam kernel it is there for.  fused_steps() / path_stats() tell the fused step from the general one; the
    general step's two tails are told apart by G_A: rankk_nt leaves the unmirrored gradient there for k_adam_sym
    (G_sym = G_A + G_A^T + cn M), the one-pass kernel behind rankk_apply_adam never writes it.  z: the inputs, when the engine
    has taken exactly one step from their start (the G_A relation needs the start's norm)."""
    n, measure, ori, env = H.PROJ_CASES[cid]
    if cid in FUSED:
        assert eng.fused_steps() == steps, (cid, eng.fused_steps())
        if measure == "HSIC":
            assert eng.path_stats() == {"lowrank_steps": steps, "general_steps": 0}
        return
    assert eng.fused_steps() == 0, cid
    if n < 256 or z is None:      # (below 256 neither rank-k tail exists: normalisation backward, fp32 GEMM, k_adam_sym)
        return
    a0 = H.a0_of(z).astype(np.float64)
    cn = np.float32(float(z["weight_sup"]) * 0.001 / np.sqrt((a0 ** 2).sum()))
    GA, gs = eng.buffer("G_A").cpu().numpy().astype(np.float64), eng.buffer("G_sym").cpu().numpy().astype(np.float64)
    off = ~np.eye(n, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs((GA + GA.T + float(cn) * O.unpack_sym(H.a0_of(z), n) - gs)[off]).max()
    separate = bool(np.isfinite(d) and d <= 1e-5 * np.abs(gs).max())
    assert separate == ("MCGRA_NO_FUSED_TAIL" in env), (cid, d, np.abs(gs).max())


@pytest.mark.parametrize("which", sorted(H.PROJ_BUDGETS))
@pytest.mark.parametrize("cid", sorted(H.PROJ_CASES))
def test_first_projected_step_sits_on_the_exact_root(pkg, monkeypatch, cid, which):
    """One step from the known start, one engine per (Adam kernel, budget).  On the packed lower triangle:
      1. |M_after - clip(a_pre - miu*, 0, 1)| <= tol (module docstring) on every entry;
      2. ONE shift: over the entries with 2e-5 < M_after < 1 - 2e-5, a_pre - M_after spreads by at most 2^-21 (the rounding of a_pre's
         reconstruction and of the subtraction, both ways); the stored halves agree bit for bit, the diagonal is zero, all of M in [0, 1];
      3. |sum(M_after) - num_edges| <= K tol + pairs 2^-24 (the shift's error times the slope, plus the entries' own rounding);
      4. the reference's algorithm on the same vector, oracle.projection(a_pre, num_edges), within 2 tol: both miu lie within one
         bracket of the same root;
      5. the step's clamp_sum scalar is the float64 sum of M_after's lower triangle to 1e-12 (float32 values accumulated in
         doubles: exact at these sizes)."""
    eng, z = make_engine(pkg, monkeypatch, cid, which)
    n, ne, lr = z["adj"].shape[0], float(z["num_edges"]), float(z["lr"])
    pairs = n * (n - 1) // 2
    a0 = H.a0_of(z)
    sc = eng.step(want_scalars=True)
    assert_route(eng, cid, 1, z)
    M = eng.buffer("M").cpu().numpy()
    a = O.pack_tril(M)
    pre = H.pre_projection_state(a0, packed(eng, "adam_m"), packed(eng, "adam_v"), 1, lr)
    p8, a8 = pre.astype(np.float64), a.astype(np.float64)
    # (the case's properties, here on the engine's own state: the budget binds and a premature clamp would show)
    assert np.clip(p8, 0, 1).sum() - ne > 1e-3 * ne and int((pre > 1 + 1e-3).sum()) >= 100
    miu, K = H.exact_projection_root(pre, ne)
    tol = tol_of(ne, K)
    d_val = float(np.abs(a8 - np.clip(p8 - miu, 0, 1)).max())
    free = (a > 2e-5) & (a < 1 - 2e-5)
    shift = (p8 - a8)[free]
    spread = float(shift.max() - shift.min())
    d_sum = float(a8.sum() - ne)
    d_ref = float(np.abs(a8 - O.projection(pre, ne)).max())
    print(f"\n[projection] {cid} {which}: n={n} num_edges={ne:.1f} K={K} tol={tol:.3e} |M-exact|={d_val:.3e} "
          f"|miu-miu*|={abs(float(np.median(shift)) - miu):.3e} spread={spread:.3e} sum-budget={d_sum:+.3e} "
          f"(allowed {K * tol + pairs * 2.0 ** -24:.3e}) |M-oracle.projection|={d_ref:.3e} above1={int((pre > 1.001).sum())} "
          f"below0={int((pre < 0).sum())} at1={int((a == 1).sum())} at0={int((a == 0).sum())}")
    assert int(free.sum()) >= pairs // 4
    assert d_val <= tol, (cid, which, d_val, tol)
    assert spread <= 2.0 ** -21, (cid, which, spread)
    assert np.array_equal(M, M.T) and np.all(np.diag(M) == 0) and M.min() >= 0 and M.max() <= 1
    assert abs(d_sum) <= K * tol + pairs * 2.0 ** -24, (cid, which, d_sum)
    assert d_ref <= 2 * tol, (cid, which, d_ref, tol)
    assert sc["clamp_sum"] == pytest.approx(float(a8.sum()), rel=1e-12)
    eng.close()


@pytest.mark.parametrize("cid", STATE_ROUTES)
def test_step_after_a_projected_step_rebuilds_d_r_and_the_norm(pkg, monkeypatch, cid):
    """Free-running, tight budget.  Engine A takes two steps; engine B takes one, is handed its own state again
    (set_adj_changes(get_adj_changes()): everything derived from M is dropped and rebuilt), and takes the second.  The projection
    changed M behind the Adam kernel, so A must rebuild d, r and |adj_changes|_2 as well -- by the same kernel (k_prep: the row sums
    an Adam pass emits for the next normalisation are switched off when a projection can follow), hence the same bits: the second
    step's mirrored gradient, state and ten scalars.  And the second step's norm term, origin_loss - nll, is
    0.001 |M_after|_2 of the projected state (float64 on the host, 1e-6): the same sum feeds cn in the Adam kernels."""
    import torch
    A, z = make_engine(pkg, monkeypatch, cid, "tight")
    B, _ = make_engine(pkg, monkeypatch, cid, "tight")
    A.step(want_scalars=True); B.step(want_scalars=True)
    a1 = A.get_adj_changes()
    assert torch.equal(a1, B.get_adj_changes())
    B.set_adj_changes(B.get_adj_changes())
    sa, sb = A.step(want_scalars=True), B.step(want_scalars=True)
    assert_route(A, cid, 2); assert_route(B, cid, 2)
    assert torch.equal(A.buffer("G_sym"), B.buffer("G_sym"))
    assert torch.equal(A.buffer("M"), B.buffer("M"))
    assert sa == sb, (sa, sb)
    norm = 0.001 * float(np.sqrt((a1.cpu().numpy().astype(np.float64) ** 2).sum()))
    assert norm > 0 and sa["origin_loss"] - sa["nll"] == pytest.approx(norm, rel=1e-6)
    # The second step's own projection, from a state that holds thousands of exact zeros and Adam's t = 2 bias corrections: on the
    # exact root of ITS pre-projection state where the budget binds again, the plain clamp (to the 2^-21 of the reconstruction)
    # where it clearly does not; in between float32 summation decides, and nothing is asserted.
    ne, lr = float(z["num_edges"]), float(z["lr"])
    pre2 = H.pre_projection_state(a1.cpu().numpy(), packed(A, "adam_m"), packed(A, "adam_v"), 2, lr).astype(np.float64)
    a2 = A.get_adj_changes().cpu().numpy().astype(np.float64)
    s2 = float(np.clip(pre2, 0, 1).sum())
    if s2 - ne > 1e-3 * ne:
        miu, K = H.exact_projection_root(pre2, ne)
        d2, allowed = float(np.abs(a2 - np.clip(pre2 - miu, 0, 1)).max()), tol_of(ne, K)
    elif s2 < ne * (1 - 1e-3):
        d2, allowed = float(np.abs(a2 - np.clip(pre2, 0, 1)).max()), 2.0 ** -21
    else:
        d2, allowed = 0.0, 0.0
    print(f"\n[projection] {cid} second step: clamp sum before projection {s2:.1f} (budget {ne:.1f}), |M-exact|={d2:.3e} (allowed {allowed:.3e})")
    assert d2 <= allowed, (cid, d2, allowed)
    assert sa["clamp_sum"] <= ne * (1 + 1e-4)
    A.close(); B.close()


@pytest.mark.parametrize("cid", STATE_ROUTES)
def test_monitoring_forward_after_a_projected_step(pkg, monkeypatch, cid):
    """step(); monitor(); step() gives the bits of step(); step(): the forward the monitor leaves for the next step is the forward
    of the PROJECTED adjacency.  Its log-probabilities are the bits of an engine that rebuilt everything from that adjacency
    (one step, then set_adj_changes of its own state, then monitor()), and of a FRESH engine handed the adjacency -- bit for
    bit where the fresh engine runs the same forward kernels (the general step); after a fused step the monitor is the fused
    forward, a fresh engine's the general one, and the suite's bound between those two is 1e-4 on the log-probabilities
    (test_fused_lowrank_step_matches_general_path_and_oracle)."""
    import torch
    E, _ = make_engine(pkg, monkeypatch, cid, "tight")
    A, _ = make_engine(pkg, monkeypatch, cid, "tight")
    C, _ = make_engine(pkg, monkeypatch, cid, "tight")
    F, _ = make_engine(pkg, monkeypatch, cid, "tight")
    E.step(); lp, _ = E.monitor(); lp = lp.clone(); E.step()
    A.step(); a1 = A.get_adj_changes().clone(); A.step()
    assert_route(E, cid, 2); assert_route(A, cid, 2)
    assert torch.equal(E.buffer("M"), A.buffer("M")) and torch.equal(E.buffer("G_sym"), A.buffer("G_sym"))
    C.step(); assert torch.equal(C.get_adj_changes(), a1)
    C.set_adj_changes(a1); lc, _ = C.monitor()
    assert torch.equal(lp, lc)
    F.set_adj_changes(a1); lf, _ = F.monitor()
    if cid in FUSED:
        assert float((lp - lf).abs().max()) < 1e-4
    else:
        assert torch.equal(lp, lf)
    assert bool(torch.isfinite(lp).all())
    for e in (E, A, C, F):
        e.close()


@pytest.mark.parametrize("cid", ("fused_mse_300", "rankk_adam_hsic_300"))
def test_budget_in_reach_but_not_binding_is_the_plain_clamp(pkg, monkeypatch, cid):
    """num_edges = 0.49 n^2 is below 0.5 n^2, so the Adam kernel leaves its result unclamped and project() runs -- but the clamp
    sum never exceeds the budget (test_projection_cases_cpu.py), so project() must be the plain clamp: the state and both moments
    (lower triangle) after step one are the bits of an engine whose budget is out of reach (1e30), which clamps in the Adam kernel.
    The second steps take d and r from different kernels (k_prep here, the Adam pass's row sums there): their mirrored gradients
    agree within the suite's path-to-path bound, 3e-5 of the largest magnitude."""
    n = H.PROJ_CASES[cid][0]
    X, _ = make_engine(pkg, monkeypatch, cid, 0.49 * n * n)
    Y, _ = make_engine(pkg, monkeypatch, cid, 1e30)
    sx, sy = X.step(want_scalars=True), Y.step(want_scalars=True)
    for name in ("M", "adam_m", "adam_v"):
        assert np.array_equal(packed(X, name), packed(Y, name)), name
    Mx = X.buffer("M").cpu().numpy()
    assert np.array_equal(Mx, Y.buffer("M").cpu().numpy()) and Mx.max() == 1.0 and Mx.min() == 0.0
    assert sx["clamp_sum"] == sy["clamp_sum"] < 0.49 * n * n
    X.step(); Y.step()
    assert_route(X, cid, 2); assert_route(Y, cid, 2)
    gx, gy = X.buffer("G_sym").cpu().numpy(), Y.buffer("G_sym").cpu().numpy()
    assert np.abs(gx - gy).max() <= H.FLOOR * np.abs(gy).max(), np.abs(gx - gy).max() / np.abs(gy).max()
    X.close(); Y.close()


def test_projected_fused_step_matches_the_general_step(pkg, monkeypatch):
    """MSELoss, n = 300, tight budget, one step from the same start through the fused step (k_tail_adam) and through the general
    one (rankk_apply_adam).  The suite's idiom for two gradient paths: fewer than 2e-3 of the entries differ by more than
    0.05 lr (Adam's +-lr on noise-level gradients; a moved entry shifts the root by lr / K, far below tol) plus 2 tol (each
    projection's own distance from the exact root of its own state)."""
    fused, z = make_engine(pkg, monkeypatch, "fused_mse_300", "tight")
    monkeypatch.setenv("MCGRA_NO_FUSED_LR", "1")
    gen = H.engine_from(pkg, z)
    monkeypatch.delenv("MCGRA_NO_FUSED_LR")
    fused.step(); gen.step()
    assert fused.fused_steps() == 1 and gen.fused_steps() == 0
    a = fused.get_adj_changes().cpu().numpy()
    b = gen.get_adj_changes().cpu().numpy()
    pre = H.pre_projection_state(H.a0_of(z), packed(fused, "adam_m"), packed(fused, "adam_v"), 1, float(z["lr"]))
    _, K = H.exact_projection_root(pre, float(z["num_edges"]))
    tol = tol_of(float(z["num_edges"]), K)
    off = np.abs(a.astype(np.float64) - b) > 0.05 * float(z["lr"]) + 2 * tol
    print(f"\n[projection] fused vs general, MSELoss n=300 tight: {int(off.sum())} of {off.size} entries differ, max {np.abs(a - b).max():.3e}")
    assert off.mean() < 2e-3, int(off.sum())
    fused.close(); gen.close()
