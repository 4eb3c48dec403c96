"""mcgra_attack_plan against the engine it describes: the smallest shapes at which the create-time rule changes sides."""
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = [("MSELoss", 256, {}), ("KL", 256, {}), ("HSIC", 1024, {}), ("HSIC", 300, {}), ("HSIC", 256, dict(act="elu", head_act="elu")),
         ("MSELoss", 255, {})]      # (255: below what the fused tail takes)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


class _Rank0:
    """rank 0 of two row-block ranks with 256 ceil(n / 512) rows each"""

    def __init__(self, n):
        self.world, self.rows_per_rank = 2, 256 * -(-n // 512)
        self.row_begin, self.row_end = 0, min(n, self.rows_per_rank)


@pytest.mark.parametrize("measure,n,victim", [pytest.param(*c, id=f"{c[0]}-n{c[1]}" + ("-gat" if c[2] else "")) for c in CASES])
def test_the_engine_does_what_the_query_says(pkg, monkeypatch, measure, n, victim):
    """A plain engine's product_mode() and, after one step, whether it ran fused are the query's; a row-block rank of the same
    configuration is created exactly when the query says shardable, and refused with the query's reason otherwise (no collective
    runs)."""
    import numpy as np
    from mc_gra_amd import engine as E
    monkeypatch.delenv("MCGRA_SPLIT_BF16", raising=False)
    z = H.synthetic_case(n, 11, [16, 16], 4, seed=3, measure=measure)
    for k, v in victim.items():
        z[k] = np.array(v)
    cfg, w = H.cfg_from(z), H.weights_from(z)
    plan = E.attack_plan(E.attack_config(n, [11, 16, 16], 4, cfg.emb_nlayer, measure, cfg.weight_sup, cfg.weight_param, cfg.lr,
                                         cfg.num_edges, len(z["idx_attack"]), act=w.act, head_act=w.head_act))
    eng = H.engine_from(pkg, z)
    assert eng.product_mode() == plan.product_mode
    eng.step()
    assert eng.fused_steps() == (1 if plan.fused else 0), (eng.fused_steps(), plan.fused, plan.why)
    eng.close()
    mk = lambda: pkg.AttackEngine(n, [11, 16, 16], 4, cfg.emb_nlayer, measure, cfg.weight_sup, cfg.weight_param, cfg.lr, cfg.num_edges,
                                  len(z["idx_attack"]), act=w.act, head_act=w.head_act, plan=_Rank0(n))
    if plan.shardable:
        mk().close()
    else:
        with pytest.raises(pkg._lib.McgraNotSupported) as e:
            mk()
        assert plan.why and plan.why.decode() in str(e.value)
    assert bool(plan.shardable) == (measure != "HSIC" or n >= 1024) * (n >= 256) * (not victim)      # (the cases are on both sides)
