"""The inputs of tests/test_gpu_terms.py, checked with the float64 oracle alone (no GPU): a term case whose reference gradient is
zero, or whose path is not the one the test means, would pass whatever the engine does.

(a) each isolated term's largest reference gradient magnitude is non-zero and finite -- except on the pairs that are degenerate on
    purpose (helpers.is_degenerate: c10 on a one-class victim), which must be exactly zero;
(b) the N x N contribution of the tiny w1 = w2 = T of the fused HSIC step's sets is at most 1e-2 of the isolated term's;
(c) no dead embedding row and, where a fused step is the subject, no relu-masked pair;
(d) nothing is skipped.
Every term of every step-implementation case is checked here, and nll / c9 / c10 on the victim shapes at the sizes of the general
and the fused MSELoss step; the GPU tests assert the same conditions (helpers.assert_term_conditions) on every case they run,
the n = 1100 HSIC shapes included (a float64 oracle step there takes 0.5 s: too slow to repeat here for every shape)."""
import numpy as np
import pytest

from oracle import mcgra_oracle as O
from tests import helpers as H

def test_float64_switch_is_scoped():
    """oracle64_from evaluates in float64 and leaves the module's float32 default behind, also when a step raises."""
    z = H.synthetic_case(40, 5, (8, 8), 3, seed=1)
    o = H.oracle64_from(z)
    assert O.F32 is np.float32
    o.step()
    assert O.F32 is np.float32 and o.last["G_sym"].dtype == np.float64 and o.last["em"].dtype == np.float64
    assert o.adj_changes.dtype == np.float32
    f = H.oracle_from(z)
    f.step()
    assert f.last["G_sym"].dtype == np.float32
    with pytest.raises(ZeroDivisionError):
        with H.oracle_precision(np.float64):
            1 / 0
    assert O.F32 is np.float32
    # the float64 run is the float32 run's limit, not another function: same gradient to float32 rounding
    assert np.abs(f.last["G_sym"] - o.last["G_sym"]).max() <= 1e-3 * np.abs(o.last["G_sym"]).max()


def test_term_sets_switch_one_term_on():
    for term in H.TERMS:
        ws, wp = H.term_weights(term)
        assert (ws != 0) + sum(x != 0 for x in wp) == 1, term
        ws, wp = H.term_weights(term, tiny=1e-12, factor=2.0)
        on = [i for i, x in enumerate(wp) if x != 0]
        assert on == ([H._SLOT[term]] if term in ("c1", "c2") else sorted({0, 1} | ({H._SLOT[term]} if term != "nll" else set()))), term
        assert (wp[0] == 1e-12) == (term not in ("c1", "c2"))       # the guard's factor never scales T
    assert H.term_weights("all") == (1.0, H.ALL_TERMS)
    assert H.term_bound(5e-7, "HSIC") == 3e-5 and H.term_bound(0.13, "HSIC") == 3e-4 and H.term_bound(6e-5, "KL") == 6e-5
    assert H.term_bound(0.13, "KL") == 1e-4


def test_default_synthetic_cases_keep_their_bits():
    a, b = H.synthetic_case(60, 11, (16, 8), 4, seed=3), H.synthetic_case(60, 11, (16, 8), 4, seed=3, gain=0.25, emb_nlayer=1)
    for k in ("W0", "W1", "Wlin"):
        assert np.array_equal(a[k] * np.float32(0.25), b[k])
    for k in ("b0", "b1", "blin", "features", "adj", "labels", "idx_attack"):
        assert np.array_equal(a[k], b[k])
    assert int(a["emb_nlayer"]) == 2 and int(b["emb_nlayer"]) == 1


@pytest.mark.parametrize("term", H.TERMS)
@pytest.mark.parametrize("case", [("HSIC", 1100), ("MSELoss", 700), ("KL", 700), "s48_gat_hsic_init", "s48_sage_kl", "s80_hsic_l3"], ids=str)
def test_step_implementation_cases_meet_their_conditions(case, term):
    spec = H.golden_spec(case, term) if isinstance(case, str) else H.step_case(case[0], case[1], term)
    c = H.term_conditions(spec, term, spec[0] == "syn" and spec[6] == "HSIC")
    H.assert_term_conditions(spec, term, c, fused_subject=spec[0] == "syn")
    assert not H.is_degenerate(spec, term)


@pytest.mark.parametrize("term", ["nll", "c9", "c10"])
@pytest.mark.parametrize("shape", [s for s, _ in H.victim_shapes()] + [(11, w, 4, 2) for w in H.GENERAL_WIDTHS], ids=str)
def test_victim_shape_cases_meet_their_conditions(shape, term):
    for measure, n in (("HSIC", 300), ("MSELoss", 700 if shape[1] not in H.GENERAL_WIDTHS else 300)):
        spec = H.syn_spec(n, shape, measure)
        c = H.term_conditions(spec, term, measure == "HSIC")
        H.assert_term_conditions(spec, term, c, fused_subject=measure != "HSIC")
    degenerate = [(s, t) for s, _ in H.victim_shapes() for t in ("nll", "c9", "c10") if H.is_degenerate(H.syn_spec(300, s, "HSIC"), t)]
    assert len(degenerate) <= 2
