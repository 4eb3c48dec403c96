"""mcgra_attack_plan: what mcgra_attack_create decides for a configuration, asked without a device (csrc/attack_plan.hip).
The rule it is compared with is tests/helpers.py: shard_rule, the suite's own statement of it."""
import itertools

import pytest

from tests import helpers as H

SWITCHES = ("MCGRA_SPLIT_BF16", "MCGRA_TESTING", "MCGRA_KEEP_GSYM", "MCGRA_NO_FWD_REUSE", "MCGRA_NO_FUSED_TAIL", "MCGRA_NO_LOWRANK",
            "MCGRA_GRAM_SPLIT", "MCGRA_OVERLAP", "MCGRA_GRAM_OVERLAP", "MCGRA_GRAM_KX_EARLY", "MCGRA_SMALL_SIDE", "MCGRA_NO_FUSED_LR",
            "MCGRA_NO_FUSED_POST", "MCGRA_EARLY_PACK", "MCGRA_EARLY_P1", "MCGRA_EARLY_TAIL", "MCGRA_MSE_DECODE_SIDE",
            "MCGRA_MSE_SMALL_INLINE", "MCGRA_PLANES_MM", "MCGRA_FWD_X3", "MCGRA_P1_BEHIND_PACK", "MCGRA_A2A_OVERLAP")
WP = (0.01, 0.01, 0, 0, 0, 10, 10, 0, 10, 1000)
VICTIMS = {"gcn": dict(act="relu", head_act="none", has_self=False), "gat": dict(act="elu", head_act="elu", has_self=False),
           "sage": dict(act="relu", head_act="none", has_self=True)}
FUSED_OF = {"HSIC": 1, "MSELoss": 2, "KL": 3}


@pytest.fixture(scope="module")
def E():
    import mcgra_loader
    mcgra_loader.load()
    from mc_gra_amd import engine
    return engine


@pytest.fixture
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _cfg(E, measure, n, dims, victim="gcn", emb_nlayer=2, nclass=7, wp=WP, eps=0.0, num_edges=1e30, plan=None):
    return E.attack_config(n, dims, nclass, emb_nlayer, measure, 1.0, wp, 0.01, num_edges, n, eps=eps, plan=plan, **VICTIMS[victim])


def test_the_query_agrees_with_the_rule_on_the_whole_grid(E, no_switches):
    """plan.shardable == (helpers.shard_rule(...) is None), (plan.fused != 0) == the same rule without its projection term, and
    plan.fused names the measure -- for EVERY combination of the grid below; each fused measure must be accepted and refused
    somewhere in it."""
    f = 11
    measures = ("HSIC", "MSELoss", "KL", "CKA", "DP", "KDE")
    ns = (200, 255, 256, 300, 1023, 1024, 2708, 10000)
    shapes = (([f, 16, 16], 2), ([f, 8, 8], 2), ([f, 24, 24], 2), ([f, 32, 32], 2), ([f, 32, 32, 32], 2), ([f, 16, 16, 16], 3),
              ([f, 16, 16, 16, 16], 2), ([f, 16, 16, 16, 16, 16], 2), ([f, 64, 64], 2))
    seen = {m: set() for m in FUSED_OF}
    count = 0
    for split in (None, "0", "1", "2", "3"):
        if split is None:
            no_switches.delenv("MCGRA_SPLIT_BF16", raising=False)
        else:
            no_switches.setenv("MCGRA_SPLIT_BF16", split)
        for measure, n, (dims, le), victim, eps, (w1, w2), edges in itertools.product(
                measures, ns, shapes, VICTIMS, (0.0, 0.1), ((.01, .01), (.01, 0.0), (0.0, 0.0)), (5.0, 1e30)):
            v = VICTIMS[victim]
            what = (split, measure, n, dims, le, victim, eps, w1, w2, edges)
            try:
                plan = E.attack_plan(_cfg(E, measure, n, dims, victim, le, wp=(w1, w2) + WP[2:], eps=eps, num_edges=edges))
                shardable, fused, why = bool(plan.shardable), plan.fused, plan.why
            except NotImplementedError as e:      # what create refuses outright can be neither fused nor sharded
                assert measure == "KDE" and dims[le] > 32, (what, e)
                shardable, fused, why = False, 0, str(e)
            rule = lambda projection: H.shard_rule(measure, eps, None, [1] if v["has_self"] else None, v["act"], v["head_act"], "CE",
                                                   n, dims, w1, w2, edges, le, projection=projection)
            what += (why,)
            assert shardable == (rule(True) is None), what
            assert (fused != 0) == (rule(False) is None), what
            assert fused in (0, FUSED_OF.get(measure, 0)), what
            assert bool(why) == (not shardable), what
            if measure in seen:
                seen[measure].add(shardable)
            count += 1
    assert count == 5 * 6 * 8 * 9 * 3 * 2 * 3 * 2
    assert all(s == {True, False} for s in seen.values()), seen


# (expected values: see test_pinned_plans_of_the_bench_shapes)
HSIC_BIG = dict(lr_ok=1, split_on=1, split_planes=2, split_mode=2, product_mode=3, gram_split=1, overlap=1, side_streams=1, gram_ovl=1,
                kx_early_on=0, small_side_on=1, fused=1, fcols=52, late_mean=1, planes_mm_on=1, fwd_x3=1, p1_behind_pack_on=1,
                early_p1_on=0, a2a_overlap=0, sharded=0, ld=10016, hsum=32, hmax=16, lr_ldv=36, sgw=0, fyw=0)
HSIC_MID = dict(HSIC_BIG, planes_mm_on=0, fwd_x3=0, p1_behind_pack_on=0)
ELEMENTWISE = dict(lr_ok=0, split_on=0, split_planes=3, split_mode=0, product_mode=0, gram_split=0, overlap=0, side_streams=1,
                   gram_ovl=0, kx_early_on=0, small_side_on=1, fcols=32, late_mean=0, planes_mm_on=0, fwd_x3=0,
                   p1_behind_pack_on=0, lr_ldv=0)
PINNED = [
    ("hsic-10000", dict(measure="HSIC", n=10000, dims=[128, 16, 16]), HSIC_BIG),
    ("hsic-4096", dict(measure="HSIC", n=4096, dims=[128, 16, 16]), dict(HSIC_MID, ld=4096)),
    ("hsic-2708", dict(measure="HSIC", n=2708, dims=[1433, 16, 16]), dict(HSIC_MID, ld=2720)),
    # below 1024: the fp32 product (split_planes keeps its initial 3), no fused step; the low-rank step still wants the side streams
    ("hsic-300", dict(measure="HSIC", n=300, dims=[128, 16, 16]),
     dict(lr_ok=1, split_on=0, split_planes=3, split_mode=0, product_mode=0, gram_split=0, overlap=0, side_streams=1, gram_ovl=0,
          kx_early_on=0, small_side_on=1, fused=0, fcols=0, late_mean=0, planes_mm_on=0, fwd_x3=0, p1_behind_pack_on=0, ld=320,
          lr_ldv=36)),
    ("mse-300", dict(measure="MSELoss", n=300, dims=[128, 16, 16]), dict(ELEMENTWISE, fused=2, ld=320)),
    ("mse-10000", dict(measure="MSELoss", n=10000, dims=[128, 16, 16]), dict(ELEMENTWISE, fused=2, ld=10016)),
    ("kl-2708", dict(measure="KL", n=2708, dims=[1433, 16, 16]), dict(ELEMENTWISE, fused=3, ld=2720)),
    # three 16-wide layers, embedding depth 2: summed widths 48 <= 64
    ("hsic-30000-3layer", dict(measure="HSIC", n=30000, dims=[256, 16, 16, 16]), dict(HSIC_BIG, ld=30016, hsum=48)),
    # a GAT as the engine sees it (5 x 16 = 80 wide, ELU): no low-rank form; every step a Gram evaluation on the split kernel,
    # its first product forked by the monitoring forward
    ("gat-hsic-3312", dict(measure="HSIC", n=3312, dims=[3703, 80, 80], victim="gat", nclass=6),
     dict(lr_ok=0, split_on=0, split_planes=2, split_mode=0, product_mode=0, gram_split=1, overlap=0, side_streams=1, gram_ovl=1,
          kx_early_on=1, small_side_on=1, fused=0, fcols=0, late_mean=0, planes_mm_on=0, fwd_x3=0, p1_behind_pack_on=0, ld=3328,
          hsum=160, hmax=80, lr_ldv=0)),
    # rank 0 of two row-block ranks: 256 * ceil(10000 / 512) = 5120 rows each
    ("hsic-10000-rank0of2", dict(measure="HSIC", n=10000, dims=[128, 16, 16], world=2),
     dict(HSIC_BIG, late_mean=0, planes_mm_on=0, fwd_x3=0, p1_behind_pack_on=0, early_p1_on=1, a2a_overlap=1, sharded=1, world=2,
          rank=0, rpr=5120, npad=10240, row0=0, row1=5120, sgw=22, fyw=74)),
]


class _Rows:
    def __init__(self, n, world, rank):
        self.world, self.rows_per_rank = world, 256 * -(-n // (256 * world))
        self.row_begin = rank * self.rows_per_rank
        self.row_end = min(n, self.row_begin + self.rows_per_rank)


@pytest.mark.parametrize("kw,want", [pytest.param(kw, want, id=name) for name, kw, want in PINNED])
def test_pinned_plans_of_the_bench_shapes(E, no_switches, kw, want):
    """Whole plans of bench.py's shapes (widths 16, 16; embedding depth 2; eps 0; 7 classes) with no switch set: the configurations
    that only the benchmark runs, pinned without a GPU.  Every expected cell was derived by hand from mcgra_attack_create of the
    commit BEFORE plan_attack existed -- its create-time code followed line by line for these inputs -- and not read off the new
    code.  product_mode is the query's field, the rest are lines of its text."""
    kw = dict(kw)
    world = kw.pop("world", 0)
    n = kw["n"]
    plan = E.attack_plan(_cfg(E, plan=_Rows(n, world, 0) if world else None, **kw))
    got = dict(plan.flags(), product_mode=plan.product_mode)
    assert got["fused"] == plan.fused and got["lr_ok"] == plan.lowrank and got["shardable"] == plan.shardable == 1 - (want["fused"] == 0)
    assert {k: got[k] for k in want} == want
    assert got["wdt"] == kw["dims"][1:] and got["L"] == len(kw["dims"]) - 1 and got["Le"] == 2


def test_refusals_are_those_of_create(E, no_switches):
    """The codes of mcgra_attack_create's argument checks, with the reason in mcgra_last_error; a row-block rank of a configuration
    that cannot be sharded is no error of the query (shardable / why say it)."""
    from mc_gra_amd import _lib
    ok = dict(measure="HSIC", n=2708, dims=[1433, 16, 16])

    def rc_of(cfg):
        out = _lib.AttackPlan()
        rc = _lib.lib.mcgra_attack_plan(cfg, out)
        return rc, _lib.lib.mcgra_last_error().decode()

    cases = []
    cases.append((_cfg(E, **dict(ok, n=1)), -1, "n=1"))
    cases.append((_cfg(E, "HSIC", 2708, [1433, 16], emb_nlayer=1), -1, "nlayer=1"))
    c = _cfg(E, **ok); c.measure = 99
    cases.append((c, -3, "measure 99"))
    cases.append((_cfg(E, "KDE", 2708, [1433, 40, 40]), -3, "embedding width 40"))
    c = _cfg(E, **ok); c.act = 2
    cases.append((c, -1, "act"))
    c = _cfg(E, plan=_Rows(2708, 2, 0), **ok); c.row_end = 1000
    cases.append((c, -1, "row block [0, 1000)"))
    c = _cfg(E, **ok); c.row_begin = 5
    cases.append((c, -1, "without shard_world"))
    for cfg, code, word in cases:
        rc, msg = rc_of(cfg)
        assert rc == code and word in msg, (rc, code, word, msg)
    with pytest.raises(_lib.McgraNotSupported, match="measure 99"):
        c = _cfg(E, **ok); c.measure = 99
        E.attack_plan(c)
    # a row-block rank of an unshardable configuration: create refuses, the query reports
    plan = E.attack_plan(_cfg(E, plan=_Rows(300, 2, 0), **dict(ok, n=300)))
    assert plan.shardable == 0 and plan.fused == 0 and "1024" in plan.why.decode()


def test_the_python_layer_asks_the_engine(E, no_switches):
    """PGDAttack._replicated_reason is the query's answer (plus its two terms that no engine configuration holds) -- MCGRA_SPLIT_BF16=1
    below n = 1024 included, where the engine takes the single-plane split product and the fused step."""
    from mc_gra_amd.topology_attack import PGDAttack
    ok = dict(measure="HSIC", eps=0.0, ori_np=None, Ws=None, act="relu", head_act="none", loss_type="CE", n=300,
              dims=[1433, 16, 16], w1=0.01, w2=0.01, num_edges=1e30)
    assert "1024" in PGDAttack._replicated_reason(**ok)
    for split, shards in (("1", True), ("2", True), ("3", True), ("0", False), ("10", True), ("01", False)):      # the first character decides
        no_switches.setenv("MCGRA_SPLIT_BF16", split)
        assert (PGDAttack._replicated_reason(**ok) is None) == shards, split
        assert (H.shard_rule(**ok) is None) == shards, split
    no_switches.delenv("MCGRA_SPLIT_BF16")
    no_switches.setenv("MCGRA_NO_FUSED_LR", "1")
    assert "MCGRA_NO_FUSED_LR" in PGDAttack._replicated_reason(**dict(ok, n=2708))
