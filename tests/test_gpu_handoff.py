"""What one engine call leaves for the next (csrc/engine.h: Carry) against every call that may come in between.

A monitor call never changes state (tests/test_gpu_parity.py holds that pair by pair), so the truth for ANY call sequence is the same
sequence on a second engine with every monitor call removed: no switch, no tolerance, no fixture.  The sequence is
`step, [monitor], X, step, [monitor], step`, the monitor calls on the engine under test only; X is an interloper that meets whatever the
monitor call left behind -- an adoptable forward, a pack, a Gram product or a row-block rank's product still running on a side stream.

What this file can and cannot hold.  A stale adoption or a wrongly kept flag gives different bits on every run, and these tests
catch it.  A MISSING STREAM WAIT is a race that may pass: that part is held by the table of entries and the invariants beside Carry,
and by review -- no case here is looped to make a race show."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


# name: (n, measure, environment at create, row-block rank, the path the three steps must have taken: counter, value)
CONFIGS = {
    "fused_hsic": (1283, "HSIC", {}, False, ("fused_steps", 3)),                          # early pack, fused_fwd_valid
    "gram_every_step": (1100, "HSIC", {"MCGRA_NO_LOWRANK": "1"}, False, ("gram_split_steps", 3)),      # kx_early, fwd_cached
    "general_mse": (255, "MSELoss", {}, False, ("fused_steps", 0)),                   # one below the fused minimum: fwd_cached, prep_valid
    "one_rank": (1100, "HSIC", {}, True, ("fused_steps", 3)),                             # p1_early and p1_inflight across a return
}
INTERLOPERS = ("nothing", "monitor", "scratch_reads", "set_model", "set_graph", "new_start", "finalize")
CHANGES_THE_TRUTH = ("set_model", "new_start")      # ... of the step behind it: each needs its resolving-power guard


def _case(cfg):
    n, measure = CONFIGS[cfg][:2]
    return H.synthetic_case(n, 11, (16, 16), 4, seed=n, measure=measure)


class _Driver:
    """One engine, monolithic or a one-rank row-block engine driven with run_lockstep, behind the same five verbs."""

    def __init__(self, pkg, z, rank):
        self.z = z
        if rank:
            _, (self.bk,) = H.shard_engines(pkg, z, 1)
            self.eng = self.bk.eng
        else:
            self.bk, self.eng = None, H.engine_from(pkg, z)

    def step(self):
        from mc_gra_amd import sharded as S
        S.run_lockstep([self.bk], S.SHARD_STEP) if self.bk else self.eng.step()
        return (self.eng.get_rows() if self.bk else self.eng.buffer("G_sym")).clone()

    def monitor(self):
        from mc_gra_amd import sharded as S
        S.run_lockstep([self.bk], S.SHARD_MONITOR) if self.bk else self.eng.monitor()

    def state(self):
        return [self.eng.get_adj_changes().clone(), self.eng.buffer("adam_m").clone(), self.eng.buffer("adam_v").clone()]

    def counters(self):
        e = self.eng
        return dict(e.path_stats(), fused_steps=e.fused_steps(), gram_split_steps=e.gram_split_steps(),
                    cut_product_steps=e.cut_product_steps(), masked_fused_steps=e.masked_fused_steps())

    def interlope(self, what, under_test):
        """Returns what the interloper computed (finalize), or None."""
        e, z = self.eng, self.z
        n = z["adj"].shape[0]
        if what == "monitor":
            if under_test:      # (a monitor call: removed from the truth like the others)
                self.monitor()
        elif what == "scratch_reads":      # the scratch under a forked Kx / pack; the values read are not asserted
            e.buffer("G_A"); e.buffer("A1")
        elif what == "set_model":
            w = H.weights_from(H.synthetic_case(n, 11, (16, 16), 4, seed=n + 1000, measure=str(z["measure"])))
            e.set_model(w.W, w.b, w.Wlin, w.blin, w.Ws)
        elif what == "set_graph":
            a = e.get_adj_changes().clone()
            e.set_graph(z["features"], z["adj"], None, z["feature_adj"], z["labels"], z["idx_attack"])
            e.set_adj_changes(a)
        elif what == "new_start":
            e.set_adj_changes(H.init_adj_changes(n, 99, 0.03))
        elif what == "finalize":
            lab = z["labels"]
            fin = e.finalize(0, e.buffer("HA"), e.buffer("YA"), (lab[:, None] == lab[None, :]).astype(np.float32)).clone()
            e.set_adj_changes(e.get_adj_changes().clone())
            return fin
        return None

    def run(self, what, under_test):
        grads = [self.step()]
        if under_test:
            self.monitor()
        fin = self.interlope(what, under_test)
        grads.append(self.step())
        if under_test:
            self.monitor()
        grads.append(self.step())
        return grads, fin


_UNDISTURBED = {}      # cfg -> the second step's gradient of the truth run without an interloper (the guards' yardstick), computed once


def _undisturbed_second_step(pkg, cfg, truth_grads=None):
    if cfg not in _UNDISTURBED:
        _UNDISTURBED[cfg] = truth_grads[1] if truth_grads is not None else _Driver(pkg, _case(cfg), CONFIGS[cfg][3]).run("nothing", False)[0][1]
    return _UNDISTURBED[cfg]


@pytest.mark.parametrize("what", INTERLOPERS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_what_a_monitor_call_leaves_survives_or_is_dropped(pkg, monkeypatch, cfg, what):
    """`step, monitor, X, step, monitor, step` gives the bits of `step, X, step, step`: the gradient (a rank: its rows) after every
    step, the state (adj_changes and both Adam moments) at the end, finalize's output where X is a finalize, and every path counter.
    An interloper that changes the truth (another model, another start) must also move the step behind it away from the
    undisturbed run's, so that a stale adoption cannot pass by coincidence."""
    import torch
    n, measure, env, rank, path = CONFIGS[cfg]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    z = _case(cfg)
    test, truth = _Driver(pkg, z, rank), _Driver(pkg, z, rank)
    (g_test, fin_test), (g_truth, fin_truth) = test.run(what, True), truth.run(what, False)
    for t in range(3):
        assert torch.equal(g_test[t], g_truth[t]), t
    for a, b in zip(test.state(), truth.state()):
        assert torch.equal(a, b)
    if what == "finalize":
        assert torch.equal(fin_test, fin_truth)
    assert test.counters() == truth.counters()
    if what == "nothing":      # the configuration exercises the path it is here for
        assert truth.counters()[path[0]] == path[1], truth.counters()
        _undisturbed_second_step(pkg, cfg, g_truth)
    if what in CHANGES_THE_TRUTH:
        assert not torch.equal(g_truth[1], _undisturbed_second_step(pkg, cfg)), "the interloper does not move the next step: no resolving power"
