"""Every loss term on its own, on every step implementation, against the FLOAT64 oracle -- and the same across victim shapes.

The other oracle comparisons of the suite bound the error by the largest magnitude of the whole gradient, with every term on: the
supervised term is 1e-5 ... 1e-12 of that, c10 inside an HSIC run 1e-6, c6 / c7 less, so the backward chains that carry them
could return zeros there.  Here one term set (tests/helpers.py: TERM_SETS) is on at a time and the bound is relative to that term's
own largest gradient magnitude:

    bound = min(cap, max(float32-oracle distance, floor))      (helpers.term_bound)

yardstick: the float32 oracle's distance from the float64 oracle for the same case, term and step; floor 3e-5: the suite's
path-to-path allowance; cap 3e-4 (HSIC) / 1e-4 (MSELoss, KL): the suite's oracle bounds.  Values follow the same rule.

Every comparison has its resolving-power guard: the engine runs once more with the term's weight multiplied by 1 + 4 bound (the
oracle keeps the original weight) and the SAME comparison function must then report a failure at every step.

Two terms cannot be held to the cap by ANY float32 evaluation, the float32 oracle's included (CONDITIONED below: c10 under HSIC,
c9 under KL): their bound is the float32 oracle's distance where that exceeds the cap, so the engine must still be no further
from float64 than the reference algorithm in its own precision.

The inputs are checked with the oracle alone in tests/test_term_cases_cpu.py and again here on every case (helpers.
assert_term_conditions): non-zero finite reference gradients, the N x N contribution of the tiny w1 = w2 = T that the fused HSIC
step needs, no dead embedding row, no relu-masked pair, and -- where c6 / c7 is the term -- no entry on Info_entropy's clamp bounds,
where the gradient jumps.  c2 and c7, the terms that go through the decode, start from helpers.SPARSE_START: from the dense start
of the other cases modified_adj1 sits above the clamp everywhere (c7 has no gradient) and the decode backward cancels to 1e-3.
Figures of one full run on an MI355X: DESIGN.md section 5 ("Term isolation").

Found by these cases and fixed in the engine: the general step's calc_kl VALUES (nxn_kernels.hip: k_kl_rows took every row's
log-sum-exp in float32) and the operand of c10 under HSIC (attack.hip: small_term centred the STORED float32 softmax(output2);
s80_hsic_l3-c10 was 4.82e-5 from float64 against the float32 oracle's 3.62e-5, 1.013e-05 with the rows recomputed from the logits in
float64 and rounded after the centring)."""
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

STEPS = 2
VALUE_KEYS = ("c1", "c2", "c6", "c7", "c9", "c10")
PATH_ENV = {"fused": {}, "general": {"MCGRA_NO_FUSED_LR": "1"}, "gram": {"MCGRA_NO_LOWRANK": "1"}, "ranks2": {}}


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _with_weights(z, ws, wp):
    z = dict(z)
    z["weight_sup"], z["weight_param"] = np.array(float(ws)), np.array(wp, np.float64)
    return z


class _Mono:
    """One engine on one path: the step's scalars and its mirrored gradient."""

    def __init__(self, pkg, z, path, monkeypatch):
        for k, v in PATH_ENV[path].items():
            monkeypatch.setenv(k, v)
        try:
            self.eng = H.engine_from(pkg, z)
        finally:
            for k in PATH_ENV[path]:
                monkeypatch.delenv(k)
        self.engines = [self.eng]

    def set(self, a):
        self.eng.set_adj_changes(a)

    def step(self):
        sc = self.eng.step(want_scalars=True)
        M, G = self.eng.buffer("M"), self.eng.buffer("G_sym")
        assert bool((M == M.T).all()), "the learnable adjacency must stay symmetric bit for bit"
        assert bool((G == G.T).all()), "the mirrored gradient must be symmetric bit for bit"
        return sc, G.cpu().numpy().astype(np.float64)


class _Ranks:
    """Row-block ranks of one attack in lockstep (the harness of test_sharded_ranks_match_monolithic_step): the ranks' rows of
    the mirrored gradient, gathered."""

    def __init__(self, pkg, z, world):
        from mc_gra_amd.sharded import RowBlockPlan, HipShardBackend
        n = z["adj"].shape[0]
        self.plans = [RowBlockPlan(n, world, r) for r in range(world)]
        self.bks = [HipShardBackend(H.engine_from(pkg, z, plan=p), p) for p in self.plans]
        self.engines = [b.eng for b in self.bks]

    def set(self, a):
        for e in self.engines:
            e.set_adj_changes(a)

    def step(self):
        import torch
        from mc_gra_amd import sharded as S
        sc = S.run_lockstep(self.bks, S.SHARD_STEP, want_scalars=True)
        assert all(s == sc[0] for s in sc), "scalars are identical on every rank"
        G = torch.cat([b.eng.buffer("G_sym")[p.row_begin:p.row_end] for b, p in zip(self.bks, self.plans) if p.has_rows], 0)
        rows = torch.cat([b.eng.get_rows() for b in self.bks if b.plan.has_rows], 0)
        assert float((rows - rows.T).abs().max()) == 0.0, "ranks must agree on mirrored entries bit for bit"
        assert float((G - G.T).abs().max()) == 0.0
        return sc[0], G.cpu().numpy().astype(np.float64)


def grad_error(G, st):
    """THE comparison (the test and its guard both use it): max|G_engine - G_64| over the term's own max|G_64|; where the
    reference gradient is exactly zero (a case that is degenerate on purpose), the engine's largest magnitude."""
    assert np.isfinite(G).all()
    if st["gmax"] == 0.0:
        return float(np.abs(G).max())
    return float(np.abs(G - st["G64"]).max() / st["gmax"])


# Terms whose conditioning is inherent: float32 cannot hold them to the cap, the float32 ORACLE (the reference algorithm in the
# engine's own precision) included.  For these the bound is the float32 oracle's distance for the same case, term and step
# wherever that exceeds the cap -- so the engine must still be no further from float64 than the reference's own float32 run --
# and the rule of term_bound everywhere else.  Largest figures of a full run on an MI355X (engine / float32 oracle, of the term's
# largest gradient magnitude; DESIGN.md has the table):
#   HSIC c10: linear_HSIC(Y_A, softmax(output2)) on node arrays.  output2 comes from the UNNORMALISED adjacency, its softmax
#     is the same row to 2e-3 on every node (n = 1100: spread 1.8e-3 of its magnitude), and HSIC centres it: float32's 1e-7 on
#     the softmax is 5e-5 of what is left, before Xc^T Yc sums it.  Gradient 1.2e-3 / 1.3e-1 (n = 1100, first step; 1.3e-2 / 1.3e-1, value
#     3.8e-4 / 5.1 before the engine took the centred softmax from the logits in float64 (node_kernels.hip: k_softmax8_gather);
#     what is left is the float32 rounding of the logits themselves.  The oracle's Gram form does not centre Y at all.
#   KL c9: calc_kl(H_A, em) on node arrays with |em| up to 26: both softmaxes are saturated and the gradient is their
#     difference.  7.6e-4 / 1.6e-3 (n = 700, second step).
CONDITIONED = {("HSIC", "c10"), ("KL", "c9")}


def _bound(yardstick, measure, term):
    b = H.term_bound(yardstick, measure)
    return max(b, float(yardstick)) if (measure, term) in CONDITIONED else b


def grad_bound(st, measure, term):
    return 0.0 if st["gmax"] == 0.0 else _bound(st["d32"], measure, term)


def expected_path(z, path, n_steps):
    """What fused_steps() / path_stats() / product_mode() must say, from helpers.shard_rule (the suite's own statement of the
    engine's create-time rule; not PGDAttack._replicated_reason, which asks the engine) and the conditions documented at
    mcgra_attack_path_stats / mcgra_attack_product_mode (include/mcgra.h): a fused step when the rule accepts the configuration;
    else, for HSIC with an N x N term, the unfused low-rank step on a ReLU chain whose embedding is at most 32 wide and the Gram
    evaluation otherwise; the fused MSELoss / KL steps are no low-rank steps."""
    cfg, w = H.cfg_from(z), H.weights_from(z)
    n = z["adj"].shape[0]
    dims = [w.W[0].shape[0]] + [x.shape[1] for x in w.W]
    ori = z["ori_adj"] if "ori_adj" in z and np.any(z["ori_adj"]) else None
    w1, w2 = cfg.weight_param[0], cfg.weight_param[1]
    why = H.shard_rule(cfg.measure, cfg.eps, ori, w.Ws, w.act, w.head_act, "CE", n, dims, w1, w2, cfg.num_edges, cfg.emb_nlayer)
    fused = why is None and path in ("fused", "ranks2")
    he = dims[cfg.emb_nlayer]
    lowrank = general = 0
    hsic_nxn = cfg.measure == "HSIC" and (w1 != 0 or w2 != 0)
    lr_ok = cfg.measure == "HSIC" and w.act == "relu" and he <= 32 and path != "gram"
    if hsic_nxn:
        lowrank, general = (n_steps, 0) if lr_ok else (0, n_steps)
    mode = 3 if (lr_ok and cfg.eps == 0 and n >= 1024) else 0
    return dict(fused=n_steps if fused else 0, stats={"lowrank_steps": lowrank, "general_steps": general}, mode=mode, why=why)


def check_term(pkg, monkeypatch, spec, term, path):
    measure = str(H.case_from(spec)["measure"])
    z0, cond, (ws, wp), traj = H.term_case(spec, term, measure == "HSIC" and spec[0] == "syn")
    T = cond["T"]
    # the conditions on the inputs (tests/test_term_cases_cpu.py checks them without a GPU): the case must be able to fail
    H.assert_term_conditions(spec, term, cond, fused_subject=path in ("fused", "ranks2"))
    for st in traj:
        assert st["finite"] and (spec[0] != "syn" or st["dead"] == 0)
        H.assert_clear_of_the_clamp(term, st)
    bounds = [grad_bound(st, measure, term) for st in traj]

    def run(factor):
        z = _with_weights(z0, *H.term_weights(term, T, factor))
        r = _Ranks(pkg, z, 2) if path == "ranks2" else _Mono(pkg, z, path, monkeypatch)
        out = []
        for st in traj:
            r.set(st["a"])                                   # teacher forcing: the float64 oracle's (float32-exact) state
            sc, G = r.step()
            out.append((sc, G))
        return z, r, out

    z, r, out = run(1.0)
    exp = expected_path(z, path, STEPS)
    for e in r.engines:
        assert e.fused_steps() == exp["fused"], (e.fused_steps(), exp)
        if measure != "HSIC" or wp[0] != 0 or wp[1] != 0:
            assert e.path_stats() == exp["stats"], (e.path_stats(), exp)
        if "MCGRA_SPLIT_BF16" not in os.environ:
            assert e.product_mode() == exp["mode"], (e.product_mode(), exp)
    errs = []
    for t, (st, (sc, G)) in enumerate(zip(traj, out)):
        err = grad_error(G, st)
        errs.append(err)
        print(f"[terms] {spec} {path} {term} step {t}: T={T:g} gmax64={st['gmax']:.3e} engine={err:.3e} oracle32={st['d32']:.3e} "
              f"bound={bounds[t]:.1e}", flush=True)
    for t, (st, (sc, G)) in enumerate(zip(traj, out)):
        assert errs[t] <= bounds[t], (t, errs[t], st["d32"], bounds[t])
        for k in (("nll",) if term == "all" else (term,)):      # (all terms on: the gradient and nll; each value has its own case)
            v64, v32 = st["v64"][k], st["v32"][k]
            vb = _bound(abs(v32 - v64) / abs(v64), measure, term) if v64 != 0 else 0.0
            print(f"[terms] {spec} {path} {term} step {t}: value {k} engine={sc[k]:.9e} oracle64={v64:.9e} oracle32={v32:.9e} "
                  f"bound={vb:.1e}", flush=True)
            assert np.isfinite(sc[k])
            assert abs(sc[k] - v64) <= vb * abs(v64) + (1e-6 if v64 == 0 else 0.0), (t, k, sc[k], v64, v32, vb)
        if term != "all":
            on = {term} | ({"c1", "c2"} if T else set())
            for k in VALUE_KEYS:
                if k not in on:
                    assert sc[k] == 0.0, (t, k, sc[k])
    # resolving power: a scale error of 4 bounds in the term's own weight must be seen by the same comparison, at every step
    # (a pair that is degenerate on purpose has no gradient of its own to scale)
    bmax = max(bounds)
    if bmax > 0 and not H.is_degenerate(spec, term):
        _, _, off = run(1.0 + 4.0 * bmax)
        for t, (st, (sc, G)) in enumerate(zip(traj, off)):
            assert grad_error(G, st) > bounds[t], ("the bound cannot see a scale error of 4 bounds in its own term", t,
                                                    grad_error(G, st), bounds[t])


# ---- part 2: every term alone on every step implementation ------------------------------------------------------------------
GOLDEN_VICTIMS = ["s48_gat_hsic_init", "s48_sage_kl", "s80_hsic_l3"]      # elu + GAT head, self weights, three layers: general only


def _part2():
    out = []
    for term in H.TERMS:      # (the paths of one (case, term) are neighbours: they share the oracle's cached trajectory)
        for spec, paths in ((H.step_case("HSIC", 1100, term), ("fused", "general", "gram")), (H.step_case("MSELoss", 700, term), ("fused", "general")),
                            (H.step_case("KL", 700, term), ("fused", "general"))):
            for path in paths + (("ranks2",) if term in ("nll", "c9") else ()):
                out.append(pytest.param(spec, term, path, id=f"{spec[6]}-n{spec[1]}-{term}-{path}"))
        for name in GOLDEN_VICTIMS:
            out.append(pytest.param(H.golden_spec(name, term), term, "fused", id=f"{name}-{term}-default"))
    return out


@pytest.mark.parametrize("spec,term,path", _part2())
def test_each_term_alone_matches_the_float64_oracle(pkg, monkeypatch, spec, term, path):
    """One term set (c2 and c7, the terms that go through the decode: from helpers.SPARSE_START), two teacher-forced steps, engine
    against the float64 oracle relative to the TERM's largest gradient magnitude: the fused HSIC step (n = 1100, default fp16-split product), the fused MSELoss and KL steps (n = 700), the general step on the
    same cases (MCGRA_NO_FUSED_LR=1), the Gram evaluation (MCGRA_NO_LOWRANK=1), the general-only victims of three committed
    fixtures with their weights replaced by the term set, and two row-block ranks in lockstep (nll, c9).  Asserted per step: the
    gradient, the term's value, exact zeros for the other terms' values, bitwise symmetry of M and G_sym, the path that ran,
    and the resolving-power guard (module docstring)."""
    check_term(pkg, monkeypatch, spec, term, path)


# ---- part 3: the victim-shape matrix ---------------------------------------------------------------------------------------
SHAPE_TERMS = ("all", "nll", "c10", "c9")      # the node kernels carry nll, c10 and c9


def _part3():
    out = []
    for shape, what in H.victim_shapes():
        tag = "f%d-%s-c%d-e%d" % (shape[0], "x".join(map(str, shape[1])), shape[2], shape[3])
        he = shape[1][shape[3] - 1]
        runs = [("HSIC", 1100, "fused"), ("MSELoss", 700, "fused"), ("KL", 700, "fused"), ("HSIC", 300, "general"), ("MSELoss", 700, "general")]
        if he == 32:
            runs = [r for r in runs if r[0] != "HSIC"]      # (he = 32 is a row of the MSELoss / KL steps)
        if shape == (11, (24, 8), 6, 2):
            runs.append(("HSIC", 1283, "fused"))            # the odd-n case
        for term in SHAPE_TERMS:
            for measure, n, path in runs:
                out.append(pytest.param(H.syn_spec(n, shape, measure), term, path, id=f"{tag}-{measure}-n{n}-{term}-{path}"))
    for widths in H.GENERAL_WIDTHS:
        for term in SHAPE_TERMS:
            for measure, n in (("HSIC", 300), ("MSELoss", 300)):
                out.append(pytest.param(H.syn_spec(n, (11, widths, 4, 2), measure), term, "general",
                                        id=f"general-{widths[0]}x{widths[1]}-{measure}-n{n}-{term}"))
    return out


@pytest.mark.parametrize("spec,term,path", _part3())
def test_victim_shapes_match_the_float64_oracle(pkg, monkeypatch, spec, term, path):
    """The same comparison, bound and guard across victim shapes (tests/helpers.py: victim_shapes, GENERAL_WIDTHS): both sides of
    the create-time switches of the node kernels that carry the small terms -- odd widths, nfeat = 1, one class, 32 / 33 classes,
    fc = 64 / 65, he = 8 / 32, summed widths 64 / 72, emb_nlayer = 1 and 3, and the 32-column rounds of the general tail's rank-k
    update (32 / 36 / 64 / 68 / 128 / 132 columns).  path "fused" is the engine's default: the step the create-time rule picks,
    which expected_path() takes from helpers.shard_rule and asserts with fused_steps() / path_stats() / product_mode();
    "general" is MCGRA_NO_FUSED_LR=1.  One class makes the c10 gradient exactly zero: asserted as exact zeros (under HSIC the
    gradient is then the tiny N x N contribution alone, compared as usual)."""
    check_term(pkg, monkeypatch, spec, term, path)
