"""The inputs of tests/test_gpu_projection.py have the properties those tests rely on -- on the numpy oracle alone, no GPU.

A projection test checks nothing when the budget does not bind, when no entry exceeds 1 before the projection (a premature clamp
in the Adam kernel is then the identity), when nothing ends on either clamp bound, or when the reference's own bisection is
further from the exact root than the bound the GPU tests hold the engine to.  A case that misses one of these is changed
(helpers.PROJ_CASES, PROJ_A0_SCALE, PROJ_BUDGETS), never the condition."""
import numpy as np
import pytest

from oracle import mcgra_oracle as O
from tests import helpers as H


def test_exact_root_on_a_vector_solved_by_hand():
    """a = (0.2, 0.5, 0.9, 1.4, 1.7), budget 2: at x = 0.3 the entries give 0 + 0.2 + 0.6 + 1 + 1 = 2.8, at x = 0.7 they give
    0 + 0 + 0.2 + 0.7 + 1 = 1.9; between 0.5 and 0.7 the active entries are 0.9 and 1.4 (1.7 - x >= 1): 0.9 + 1.4 - 2 x + 1 = 2
    gives x = 0.65, slope -2."""
    miu, K = H.exact_projection_root(np.array([0.2, 0.5, 0.9, 1.4, 1.7]), 2.0)
    assert miu == pytest.approx(0.65, abs=1e-14) and K == 2
    a = np.random.RandomState(3).rand(5000) * 1.3 - 0.1
    for ne in (10.0, 700.0, 2400.0):
        miu, K = H.exact_projection_root(a, ne)
        assert abs(np.clip(a - miu, 0, 1).sum() - ne) <= 1e-9 * ne
        assert K == int(((a - miu > 0) & (a - miu < 1)).sum()) > 0
    with pytest.raises(AssertionError):
        H.exact_projection_root(a, 1e9)                  # a budget that does not bind has no root to find


def test_pre_projection_state_is_the_oracles_adam_step():
    """pre_projection_state, from the moments AFTER a step, gives the bits AdamState.step returned for that step (t = 1 and 2)."""
    rng = np.random.RandomState(11)
    p = (rng.rand(4000) * 1.05).astype(np.float32)
    adam = O.AdamState(0.01, np.zeros_like(p), np.zeros_like(p))
    for t in (1, 2):
        g = (rng.randn(p.size) * 10.0 ** rng.uniform(-9, 1, p.size)).astype(np.float32)
        new = adam.step(p, g)
        assert np.array_equal(H.pre_projection_state(p, adam.m, adam.v, t, 0.01), new)
        p = np.clip(new, 0, 1)


@pytest.mark.parametrize("which", sorted(H.PROJ_BUDGETS))
@pytest.mark.parametrize("cid", sorted(H.PROJ_CASES))
def test_projection_case_conditions(cid, which):
    n, measure, ori, _ = H.PROJ_CASES[cid]
    z = H.projection_case(n, measure, ori)
    a0, pre = H.projection_oracle_pre(n, measure, ori)
    pairs = n * (n - 1) // 2
    assert a0.size == pairs and a0.max() < H.PROJ_A0_SCALE and a0.min() >= 0
    ne = H.projection_budget(z, which)
    assert ne < 0.5 * n * n                                      # the engine's may_project
    p8 = pre.astype(np.float64)
    # the budget binds on the first step, by more than float32 summation can decide otherwise
    assert np.clip(p8, 0, 1).sum() - ne > 1e-3 * ne
    # a premature clamp is visible: entries above 1 before the projection ...
    assert int((pre > 1 + 1e-3).sum()) >= 100
    # ... and the bracket's left end (min - 1) comes from entries below 0
    if measure in ("HSIC", "MSELoss"):
        assert int((pre < 0).sum()) >= 100
    miu, K = H.exact_projection_root(pre, ne)
    assert K >= pairs // 4
    proj = O.projection(pre, ne)
    if which == "loose":                                         # both clamps after the shift are exercised
        assert int((proj == 1).sum()) >= 100 and int((proj == 0).sum()) >= 100
    # the reference's float32 bisection on the same vector sits within its own epsilon of the exact root
    assert np.abs(proj.astype(np.float64) - np.clip(p8 - miu, 0, 1)).max() <= 1e-5
    free = (proj > 0) & (proj < 1)
    assert np.abs((p8 - proj)[free] - miu).max() <= 1e-5


def test_budget_in_reach_but_not_binding():
    """num_edges = 0.49 n^2 is below the engine's 0.5 n^2 (project() runs) and far above the clamp sum the first step leaves, and
    above what a second step can add (lr per pair): the bisection never starts."""
    for cid in ("fused_mse_300", "rankk_adam_hsic_300"):
        n, measure, ori, _ = H.PROJ_CASES[cid]
        _, pre = H.projection_oracle_pre(n, measure, ori)
        s = float(np.clip(pre.astype(np.float64), 0, 1).sum())
        assert s + 0.01 * pre.size < 0.9 * 0.49 * n * n < 0.5 * n * n
