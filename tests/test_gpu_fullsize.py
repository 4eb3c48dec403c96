"""BASELINE.json's full size (synthetic N = 10 000, d = 128, 2-layer GCN, HSIC, priors H_A+Y_A+Y) on the GPU.

Parity with the REFERENCE at this size: tests/golden/bench10k_hsic.npz holds what the reference's own
PGDAttack.attack (topology_attack.py:161-324, torch CPU) produced on exactly the bench's inputs
(tests/golden/make_golden.py --only bench10k: bench.make_inputs + bench.make_a0 handed to the reference classes);
test_bench_workload_matches_reference_at_10k drives the engine the way bench.py does (default fp16-split product on
the side stream, fused tail, monitor forward adopted by the next step) and holds per-step gradients, states and the
recovered-adjacency AUC against it; test_fused_elementwise_workload_matches_reference_at_10k does the same for the
MSELoss and KL workloads (bench10k_mse.npz, bench10k_kl.npz).  The oracle cannot run at this size in seconds, so the other tests carry
size-independent properties -- state invariants, bit-determinism, agreement of the two independent evaluations of
linear_HSIC (low-rank vs Gram), bit-identity of the row-block sharded phases, gradient linearity."""
import os
import sys

import numpy as np
import pytest

os.environ.setdefault("MCGRA_KEEP_GSYM", "1")     # these tests read each step's mirrored gradient ("G_sym")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
WL = "synthetic-10k-hsic"
# (workload, mutation, start) of the MSELoss / KL mutation guards: each defect on the starts where it misses the first-step
# bar by 30 times or more (test_mutations_turn_the_fused_10k_reference_tests_red says by how much on every start)
MUTATION_CASES = [("synthetic-10k-mse", "calc", "run"), ("synthetic-10k-mse", "calc", "one0"), ("synthetic-10k-mse", "rk", "run"),
                  ("synthetic-10k-mse", "rk", "one1"), ("synthetic-10k-kl", "calc", "one0"), ("synthetic-10k-kl", "rk", "run"),
                  ("synthetic-10k-kl", "rk", "one1"), ("synthetic-10k-kl", "klstats", "run"), ("synthetic-10k-kl", "klstats", "one1")]


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import mcgra_loader
    pkg = mcgra_loader.load()
    import bench
    return pkg, torch, bench, torch.device("cuda:0")


def _engine(ctx, seed=0, **kw):
    pkg, torch, bench, dev = ctx
    return bench.build_engine(pkg, torch, dev, WL, seed, **kw)


from tests.helpers import tril_pos as _tril_pos  # noqa: E402


def test_tril_pos_helper():
    n = 7
    ii, jj = np.tril_indices(n, -1)
    i, j = _tril_pos(np.arange(n * (n - 1) // 2))
    assert np.array_equal(i, ii) and np.array_equal(j, jj)


def _reference_run_errors(ctx, z, z64, name, steps=None, check=True, mutate=None, wl=WL):
    """Drive the engine the way bench.py does from the start `name` of the fixture of workload `wl`; returns the per-step
    gradient errors against the reference (and, step 0, against the float64 evaluation), asserting the bars when `check`."""
    pkg, torch, bench, dev = ctx
    seed, lr = int(z["seed"]), float(z["lr"])
    n = bench.WORKLOADS[wl][0]
    assert str(z["workload"]) == wl, (str(z["workload"]), wl)
    assert lr == bench.workload_lr(wl, n) and float(z["start_scale"]) == bench.start_scale(wl, n), "fixture is of another bench start"
    pi, pj = _tril_pos(z["packed_pos"])
    ti, tj = torch.as_tensor(pi, device=dev), torch.as_tensor(pj, device=dev)
    sd, sc = int(z[f"{name}_a0_seed"]), float(z[f"{name}_a0_scale"])
    if mutate:          # the defect injector is accepted only by an engine created under MCGRA_TESTING=1
        os.environ["MCGRA_TESTING"] = "1"
    try:
        eng, inp, adj_dev = bench.build_engine(pkg, torch, dev, wl, seed)
    finally:
        os.environ.pop("MCGRA_TESTING", None)
    if bench.WORKLOADS[wl][5] == "HSIC":
        assert eng.product_mode() == 3, "the default product of this size is the 2-plane fp16 split"
    if mutate:
        eng.test_mutate(mutate)
    if (sd, sc) != (seed, bench.start_scale(wl, n)):
        eng.set_adj_changes(torch.as_tensor(bench.make_a0(n, sd, sc), device=dev))
    G, A = z[f"{name}_g"], z[f"{name}_a"]
    errs = []
    for t in range(G.shape[0] if steps is None else steps):
        eng.step()
        eng.monitor()                                   # bench.py's step: the next step adopts this forward
        Gs = eng.buffer("G_sym")
        g = Gs[ti, tj].cpu().numpy()
        gmax = float(z[f"{name}_g_absmax"][t])
        err_ref = np.abs(g - G[t]).max() / gmax
        err_true = ref_true = None
        ref_flips = 0.0
        if t == 0 and f"{name}_g64ref" in z64.files:
            # the truth: the REFERENCE's own code run in float64 (make_golden.py --only bench10k_ref64) -- independent of oracle/
            g64 = z64[f"{name}_g64ref"]
            err_true = np.abs(g - g64).max() / gmax
            ref_true = np.abs(G[t] - g64).max() / gmax
            # rms distances: the engine sits on the exact gradient, so its rms distance from the reference's fp32 gradient is
            # the reference's own rms distance from exact (2.0e-3 / 1.8e-3 / 6e-4 of gmax on the three starts)
            rms = lambda d: float(np.sqrt(np.mean(np.square(d.astype(np.float64))))) / gmax
            rms_ref, rms_true, ref_rms = rms(g - G[t]), rms(g - g64), rms(G[t] - g64)
            if check:
                assert rms_true <= 3e-5, (name, rms_true)
                assert rms_ref <= 3e-3 and rms_ref <= ref_rms + 1e-4, (name, rms_ref, ref_rms)
            # entries whose gradient has another sign in the reference's fp32 evaluation than in exact arithmetic: Adam's
            # first step is lr * sign(g), so the reference itself moves these the "wrong" way
            ref_flips = float((np.sign(G[t]) != np.sign(g64)).mean())
        errs.append((err_ref, err_true, ref_true))
        if not check:
            continue
        if err_true is not None:
            assert abs(float(z64[f"{name}_g64ref_absmax"]) - gmax) <= (ref_true + 2e-3) * gmax
            assert err_true <= 3e-4, (name, t, err_true)
            assert err_ref <= ref_true + 3e-4, (name, t, err_ref, ref_true)
        else:
            assert err_ref <= 2e-3, (name, t, err_ref)
        # whole-matrix sums (fp64): the packed gradient is half of the mirrored matrix
        gsum = float(Gs.double().sum()) * 0.5
        ref_l1 = float(np.sqrt(z[f"{name}_g_sqsum"][t]) * np.sqrt(n * (n - 1) / 2))     # >= sum |g|
        assert abs(gsum - float(z[f"{name}_g_sum"][t])) <= ((ref_true or 0.0) + 2e-3) * ref_l1, (name, t, gsum, float(z[f"{name}_g_sum"][t]))
        assert abs(float(Gs.abs().max()) - gmax) <= ((ref_true or 0.0) + 2e-3) * gmax
        M = eng.buffer("M")
        a = M[ti, tj].cpu().numpy()
        # (the reference's hook sees adj_changes after optimizer.step(), before the clamp of :283)
        moved = np.abs(a - np.clip(A[t], 0, 1)) > 0.05 * lr
        assert moved.mean() <= (ref_flips + 0.002 if t == 0 else 0.01), (name, t, moved.mean(), ref_flips)
        asum = float(M.double().sum()) * 0.5
        ref_sum = float(z[f"{name}_a_clip_sum"][t])
        assert abs(asum - ref_sum) <= 1e-4 * ref_sum, (name, t, asum, ref_sum)
        del M
    return eng, inp, adj_dev, errs


def test_bench_workload_matches_reference_at_10k(ctx):
    """The configuration the headline number is quoted on, against the reference itself (fixture generated from
    /root/reference by make_golden.py; nothing here reads the reference).  `run`: the 4-step loop from the bench's own
    start (bench.make_a0 at bench.start_scale: kappa / N, where BOTH the N x N terms c1 / c2 and the small-operand terms
    c9 / c10 carry the gradient -- profiles/r03_nxn_share_10k.json: c1 0.78, c2 0.11, c9 0.84, c10 0.28 of the gradient's
    largest magnitude at step 0); `one0` / `one1`: single steps from other seeded starts at half / twice that scale (the
    N x N terms / the small-operand terms in charge), i.e. steps whose starting state is the reference's own by
    construction (a 50 M-entry adj_changes per step cannot be stored, so the later steps of `run` free-run: Adam moves
    an entry whose gradient sits at the fp32 noise level by +-lr on its sign alone; such entries are counted).
    What this pins at N = 10 000 against topology_attack.py:161-324: the forward chains, the fp16-split product
    (split2_m16_kernel) through c1, the fp16-split rank-k rounds of k_tail_reduce (backward of both GCN chains, i.e.
    the CE loss, c9, c10 and c2's path through the embedding), the small-operand terms, the normalisation backward, Adam,
    the post-loop ensemble and the AUC.  test_mutations_turn_the_10k_reference_test_red checks that it does: with P1
    wiped or the rank-k terms dropped the same comparison fails by orders of magnitude.  (Not visible at this size, by the
    loss's own weights: the Info_entropy terms c6 / c7 -- k_decode_fly's gradient -- at 1e-5 ... 1e-6 of the gradient, and
    the low-rank term of c2 that acts on adj_norm directly, 4e-5; these are pinned against the oracle with the other terms
    switched off, tests/test_gpu_parity.py.)

    Bars.  AUC: north_star's 1e-4.  Gradient: at this size and state the reference's OWN fp32 gradient is 1.2e-2 / 1.2e-2 /
    3.5e-3 of the gradient's largest magnitude away from a float64 evaluation of the same algorithm
    (tests/golden/bench10k_hsic_ref64.npz: the reference's own code with torch's default dtype set to float64, make_golden.py
    --only bench10k_ref64; the numpy oracle in float64 agrees with it to 2e-10: its Gram-then-centre evaluation of linear_HSIC on the
    all-positive feature_adj cancels three digits) and has the other SIGN than the exact gradient on 0.2 % of the
    entries.  So the engine is held to 3e-4 of the EXACT gradient (measured: 4e-6 ... 4e-5) -- the bar the small goldens
    hold against the reference -- to the reference within the reference's own distance from the exact gradient plus
    3e-4, and its first Adam step to the reference's within the reference's own sign flips plus 0.2 %; free-running
    steps, which have no float64 truth, to 2e-3."""
    _check_against_reference_at_10k(ctx, WL)


def _check_against_reference_at_10k(ctx, wl):
    """The reference test of workload `wl` (bench.WORKLOADS) against tests/golden/bench10k_<measure>{,_ref64,_fp64}.npz."""
    pkg, torch, bench, dev = ctx
    tag = "bench10k_" + wl.rsplit("-", 1)[1]
    z = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}.npz"))
    z64 = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}_ref64.npz"))
    assert str(z["workload"]) == wl and str(z64["workload"]) == wl and np.array_equal(z["packed_pos"], z64["packed_pos"])
    # (the numpy oracle in float64, make_truth64.py, agrees with the reference in float64 to 2e-10 of gmax for HSIC, 2e-15 for
    # MSELoss / KL: two independent float64 evaluations of topology_attack.py:161-283)
    zo = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}_fp64.npz"))
    starts = ["run"] + sorted({k[:4] for k in z.files if k.startswith("one")})
    assert len(starts) >= 3
    for nm in starts:
        assert np.abs(zo[f"{nm}_g64"] - z64[f"{nm}_g64ref"]).max() <= 1e-8 * float(z64[f"{nm}_g64ref_absmax"])
    sp = z["sample_pos"]
    for name in starts:
        eng, inp, adj_dev, errs = _reference_run_errors(ctx, z, z64, name, wl=wl)
        assert len(errs) == z[f"{name}_g"].shape[0]
        assert eng.path_stats()["general_steps"] == 0 and eng.fused_steps() == len(errs)
        lab = torch.as_tensor(inp["labels"], device=dev)
        final = eng.finalize(0, eng.buffer("HA"), eng.buffer("YA"), (lab[:, None] == lab[None, :]).float())
        auc = bench.gpu_auc(adj_dev, final, torch)
        assert abs(auc - float(z[f"{name}_auc"])) <= 1e-4, (name, auc, float(z[f"{name}_auc"]))
        fs = final[torch.as_tensor(sp[:, 0], device=dev), torch.as_tensor(sp[:, 1], device=dev)].cpu().numpy()
        ref_fs = z[f"{name}_final_sample"]
        assert np.mean(np.abs(fs - ref_fs) > 1e-3 * max(1.0, np.abs(ref_fs).max())) < 0.01
        assert abs(float(final.double().sum()) - float(z[f"{name}_final_sum"])) <= 1e-4 * abs(float(z[f"{name}_final_sum"]))
        if name == "run":      # priors computed by set_graph against the reference's H_A2 / Y_A
            assert np.abs(eng.buffer("HA")[:64].cpu().numpy() - z["H_A2_sample"]).max() <= 1e-5 * np.abs(z["H_A2_sample"]).max()
            assert np.abs(eng.buffer("YA")[:64].cpu().numpy() - z["Y_A_sample"]).max() <= 2e-5
        del eng, final
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mutation,name", [("p1", "run"), ("p1", "one0"), ("p1", "one1"), ("rk", "run"), ("rk", "one1")])
def test_mutations_turn_the_10k_reference_test_red(ctx, monkeypatch, mutation, name):
    """Mutation guard of the test above (with the old dense start it would have passed with P1 = 0).
    mcgra_attack_test_mutate (an explicit test-only call: the engine reads no such switch from the environment) with 'p1'
    wipes the result of split2_m16_kernel before the tail reads it, 'rk' drops the rank-k terms of
    k_tail_reduce (fp16-split products) from the gradient: the first-step comparison against the exact gradient must
    then fail its 3e-4 bar by a wide margin -- i.e. the kernels are visible to the fixture at this size."""
    pkg, torch, bench, dev = ctx
    z = np.load(os.path.join(ROOT, "tests", "golden", "bench10k_hsic.npz"))
    z64 = np.load(os.path.join(ROOT, "tests", "golden", "bench10k_hsic_ref64.npz"))
    eng, _, _, errs = _reference_run_errors(ctx, z, z64, name, steps=1, check=False, mutate=mutation)
    err_ref, err_true, _ = errs[0]
    assert eng.fused_steps() == 1
    assert err_true > 30 * 3e-4, (mutation, name, err_ref, err_true)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("wl", ["synthetic-10k-mse", "synthetic-10k-kl"])
def test_fused_elementwise_workload_matches_reference_at_10k(ctx, wl):
    """bench.py's synthetic-10k-mse / synthetic-10k-kl (calc = MSELoss / calc_kl: the fused elementwise steps of
    attack_fused.hip -- k_decode_stats, k_decode_fly<H, V7, 1|2>, k_kl_stats_fin / k_kl_v_fin, k_tail_reduce<V, 1|2> -- at
    the size the bench quotes them: 26 column slices of the decode, 157 x 157 tail tiles, the small-operand terms on their
    own stream) against the reference, the same way and with the same bars as the HSIC test above: fixtures
    tests/golden/bench10k_{mse,kl}.npz (make_golden.py --only bench10k_mse / bench10k_kl: the reference's 4-step run from
    the bench's own start and single steps from two other seeded starts), bench10k_{mse,kl}_ref64.npz (the first
    gradients of the reference's own code in float64) and bench10k_{mse,kl}_fp64.npz (the numpy oracle in float64).
    Every step is a fused one; no general step.

    Measured (MI355X; max |g - g64| / gmax of the first step at the sampled positions, run / one0 / one1): the reference's own
    fp32 gradient sits 7.2e-7 / 7.9e-7 / 3.6e-7 from its float64 gradient for MSELoss (rms 1.5e-7 / 1.8e-7 / 9.3e-8) and
    1.1e-5 / 4.7e-7 / 3.2e-6 for KL (rms 6.4e-7 / 1.2e-7 / 1.2e-7) -- no N x N x N product and no Gram cancellation here, unlike
    HSIC's 1.2e-2.  The engine: 8.1e-7 / 7.4e-7 / 3.5e-7 (MSELoss) and 8.5e-6 / 3.9e-7 / 2.2e-6 (KL), i.e. at or below the
    reference's own rounding and 35x (KL) to 370x (MSELoss) under the 3e-4 bar; free-running steps of `run` to the reference: <= 1.3e-6 (MSELoss), 3.2e-5 (KL).
    AUC: within 6e-9 of the reference's on every start.  The bars stay the HSIC test's: a kernel defect that matters misses
    them by far more (test_mutations_turn_the_fused_10k_reference_tests_red)."""
    _check_against_reference_at_10k(ctx, wl)


@pytest.mark.parametrize("wl,mutation,name", MUTATION_CASES)
def test_mutations_turn_the_fused_10k_reference_tests_red(ctx, wl, mutation, name):
    """Mutation guard of the MSELoss / KL reference tests above: 'calc' drops the measure's per-pair terms c1 / c2 (the
    multipliers kmse1 = kmse2 = 0 of the decode and of the tail's first pass), 'klstats' wipes the KL row statistics
    (lseA / lse1 after k_decode_stats), 'rk' drops the tail's rank-k terms.  Each must miss the first-step bar against the
    exact gradient (3e-4 of gmax) by 30 times or more -- on the start named here.

    Measured first-step error against the float64 gradient, in units of the bar (run / one0 / one1): 'calc' MSELoss 67 / 53 /
    14, KL 8.5 / 46 / 1.6; 'rk' 2 400 ... 2 700 on every start of both; 'klstats' 2e8 / 1e9 / 3e7.  The per-pair terms carry
    the gradient where the small-operand terms c9 / c10 leave them room: scripts/nxn_share.py at N = 10 000 (the numpy oracle,
    one term at a time) gives c2 3.2e-2 / 2.4e-2 / 6.3e-3 of the gradient's largest magnitude for MSELoss and 2.0e-3 / 1.1e-2 /
    3.8e-4 for KL (c1 at most 3.3e-3) at the starts' scales -- so 'calc' is held on the starts where c2 is in charge: run
    and one0 (MSELoss), one0 (KL, the half-scale start)."""
    pkg, torch, bench, dev = ctx
    tag = "bench10k_" + wl.rsplit("-", 1)[1]
    z = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}.npz"))
    z64 = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}_ref64.npz"))
    eng, _, _, errs = _reference_run_errors(ctx, z, z64, name, steps=1, check=False, mutate=mutation, wl=wl)
    err_ref, err_true, _ = errs[0]
    assert eng.fused_steps() == 1 and eng.path_stats()["general_steps"] == 0
    assert err_true > 30 * 3e-4, (wl, mutation, name, err_ref, err_true)
    del eng
    torch.cuda.empty_cache()


def test_state_invariants_and_determinism_at_10k(ctx):
    pkg, torch, bench, dev = ctx
    outs = []
    for _ in range(2):
        eng, inp, _ = _engine(ctx)
        sc = [eng.step(want_scalars=True) for _ in range(3)]
        outs.append((eng.get_adj_changes().clone(), [s["loss"] for s in sc]))
        M = eng.buffer("M")
        assert torch.equal(M, M.t()), "learnable adjacency must stay symmetric"
        assert float(M.diagonal().abs().max()) == 0.0
        assert float(M.min()) >= 0.0 and float(M.max()) <= 1.0          # clamp of :283
        assert eng.path_stats() == {"lowrank_steps": 3, "general_steps": 0}
        assert all(np.isfinite(s["loss"]) for s in sc)
        del eng
        torch.cuda.empty_cache()
    assert torch.equal(outs[0][0], outs[1][0]), "two runs must give identical bits"
    assert outs[0][1] == outs[1][1]


def test_the_build_bench_times_gives_the_parity_builds_bits_at_10k(ctx, monkeypatch):
    """Every in-process parity test creates its engines under MCGRA_KEEP_GSYM=1 (k_tail_adam / k_adam_sym then also store the
    mirrored packed gradient, "G_sym"); bench.py and a user's run do not.  The two forms of the Adam pass must be the same
    arithmetic: three bench steps (step + monitoring forward) of the headline workload WITHOUT the switch give the state of the
    engine WITH it, bit for bit -- and the engine without it refuses to hand out G_sym."""
    pkg, torch, bench, dev = ctx
    outs = []
    for keep in (True, False):
        if keep:
            monkeypatch.setenv("MCGRA_KEEP_GSYM", "1")
        else:
            monkeypatch.delenv("MCGRA_KEEP_GSYM", raising=False)
        eng, inp, _ = _engine(ctx)
        for _ in range(3):
            eng.step(); eng.monitor()
        outs.append(eng.buffer("M").clone())
        assert eng.fused_steps() == 3
        if keep:
            assert float(eng.buffer("G_sym").abs().max()) > 0
        else:
            with pytest.raises(Exception, match="MCGRA_KEEP_GSYM"):
                eng.buffer("G_sym")
        del eng
        torch.cuda.empty_cache()
    monkeypatch.setenv("MCGRA_KEEP_GSYM", "1")
    assert torch.equal(outs[0], outs[1])


def test_defect_injector_is_refused_outside_a_testing_engine(ctx, monkeypatch):
    """mcgra_attack_test_mutate (the mutation guards' defect injector) is accepted only by an engine created under
    MCGRA_TESTING=1; a production engine refuses to arm it (disarming is always allowed)."""
    pkg, torch, bench, dev = ctx
    monkeypatch.delenv("MCGRA_TESTING", raising=False)
    eng, _, _ = bench.build_engine(pkg, torch, dev, "cora-shape-hsic", 0)
    with pytest.raises(Exception, match="MCGRA_TESTING"):
        eng.test_mutate("p1")
    eng.test_mutate(None)
    del eng
    torch.cuda.empty_cache()


def test_early_tail_pass_beside_the_product_is_bit_identical_at_10k(ctx, monkeypatch):
    """n >= 8192: the product is cut behind five of its 6.25 rounds (1 280 of 1 600 tiles = eight groups of four row panels), and
    the tail's first pass over the rows those tiles complete in both orientations (8 192 of 10 000) runs beside the last rounds;
    the rest of the pass follows the join.  Same tiles through the same ragged round, same tile pairs by the same arithmetic:
    the state after three bench steps (step + monitoring forward) is bit-identical to MCGRA_EARLY_TAIL=0, and the step that
    returns its loss terms (value partials in one launch) keeps the product in one piece."""
    pkg, torch, bench, dev = ctx
    outs = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("MCGRA_EARLY_TAIL", env)
        eng, inp, _ = _engine(ctx)
        for _ in range(3):
            eng.step(); eng.monitor()
        assert eng.cut_product_steps() == (3 if env is None else 0)
        if env is None:
            eng.step(want_scalars=True)
            assert eng.cut_product_steps() == 3
            eng.step()
            assert eng.cut_product_steps() == 4
        else:
            eng.step(want_scalars=True); eng.step()
        outs.append(eng.buffer("M").clone())
        assert eng.fused_steps() == 5
        del eng
        torch.cuda.empty_cache()
    assert torch.equal(outs[0], outs[1])


def test_lowrank_and_gram_evaluations_agree_at_10k(ctx, monkeypatch):
    pkg, torch, bench, dev = ctx
    fast, _, _ = _engine(ctx)
    monkeypatch.setenv("MCGRA_NO_LOWRANK", "1")
    gram, _, _ = _engine(ctx)
    monkeypatch.delenv("MCGRA_NO_LOWRANK")
    for t in range(2):
        a = fast.step(want_scalars=True)
        b = gram.step(want_scalars=True)
        gf, gg = fast.buffer("G_sym"), gram.buffer("G_sym")
        err = float((gf - gg).abs().max()) / float(gg.abs().max())
        assert err < 5e-5, (t, err)
        # the scalar values differ more than the gradients: the Gram evaluation sums 10^8 products of fp32 Gram entries
        # (measured ~5e-5 relative at this size; the low-rank value is the one closer to an fp64 evaluation)
        for k in ("loss", "c1", "c2", "c6", "c7"):
            assert a[k] == pytest.approx(b[k], rel=3e-4, abs=1e-6), (t, k)
        gram.set_adj_changes(fast.get_adj_changes())
    assert gram.path_stats()["general_steps"] == 2 and gram.gram_split_steps() == 2


def test_sharded_ranks_match_monolithic_at_10k(ctx):
    """Two row-block ranks of the headline workload on one GPU (lockstep emulation, collectives as copies): every
    N x N pass of a rank touches its 5120 rows only; the union of the rows equals the monolithic step's adjacency up to
    the entries Adam moves on rounding noise, and the ranks agree bit for bit on mirrored entries."""
    pkg, torch, bench, dev = ctx
    from mc_gra_amd import sharded as S
    n = bench.WORKLOADS[WL][0]
    full, _, _ = _engine(ctx)
    plans = [S.RowBlockPlan(n, 2, r) for r in range(2)]
    bks = [S.HipShardBackend(_engine(ctx, plan=p)[0], p) for p in plans]
    for t in range(2):
        a = full.step(want_scalars=True); full.monitor()
        sc = S.run_lockstep(bks, S.SHARD_STEP, want_scalars=True)
        S.run_lockstep(bks, S.SHARD_MONITOR)
        rows = torch.cat([b.eng.get_rows() for b in bks], 0)
        ref = full.buffer("M")
        assert float(((rows - ref).abs() > 0.05 * bench.workload_lr(WL, n)).float().mean()) < 2e-3, f"step {t}"
        assert float((rows - rows.T).abs().max()) == 0.0
        for k in ("loss", "c1", "c2", "c9", "c10"):
            assert sc[0][k] == sc[1][k] and sc[0][k] == pytest.approx(a[k], rel=1e-4), (t, k)
    assert all(b.eng.fused_steps() == 2 for b in bks)


def test_gradient_is_linear_in_the_loss_weights_at_10k(ctx):
    """d loss / d adj_changes is linear in (weight_sup, w1, w2, w6, w7, w9, w10): G(w_a + w_b) = G(w_a) + G(w_b) with
    the norm term of :173 attributed to weight_sup.  Checked with the N x N terms split from the rest."""
    pkg, torch, bench, dev = ctx
    n, f, c, hid, nl, measure, wp = bench.WORKLOADS[WL]
    inp = bench.make_inputs(n, f, c, hid, nl, 0)
    X = torch.as_tensor(inp["features"], device=dev)
    fadj = bench.feature_adj_cora(X, torch)
    adj_dev = torch.as_tensor(inp["adj"], device=dev)
    a0 = torch.as_tensor(bench.make_a0(n, 0, bench.start_scale(WL, n)), device=dev)

    def grad(weight_sup, weights):
        eng = pkg.AttackEngine(n, inp["dims"], c, 2, measure, weight_sup, weights, bench.workload_lr(WL, n), 1e30, n, device=dev)
        eng.set_model(inp["W"], inp["b"], inp["Wlin"], inp["blin"])
        eng.set_graph(X, adj_dev, None, fadj, inp["labels"], inp["idx_attack"])
        eng.set_adj_changes(a0)
        eng.step()
        out = eng.buffer("G_sym").clone()
        del eng
        torch.cuda.empty_cache()
        return out

    wa = (wp[0], wp[1], 0, 0, 0, 0, 0, 0, 0, 0)                  # the N x N HSIC terms
    wb = (0, 0, 0, 0, 0, wp[5], wp[6], 0, wp[8], wp[9])          # entropy and small-operand terms
    g_all = grad(1.0, wp)
    g_sum = grad(0.0, wa) + grad(1.0, wb)
    err = float((g_all - g_sum).abs().max()) / float(g_all.abs().max())
    assert err < 2e-5, err


# ---- BASELINE.json configs[4]: N = 30 000, d = 256, 3-layer GCN, on ONE MI355X (58 GB of N x N buffers + 7 GB of planes)
WL30 = "synthetic-30k-hsic-3layer"


def test_config4_shape_30k_3layer_properties(ctx, monkeypatch):
    """The largest BASELINE shape through the default path (fused low-rank step, fp16-split product, 3-layer chains:
    rank-k panels of 48 + 32 columns in two rounds): state invariants, bit-determinism of two runs, and agreement of
    the low-rank evaluation with the Gram evaluation (the reference's formulation: four fp32 MFMA products) on the
    N x N terms.  The oracle cannot run at this size; the same code paths are pinned to the reference at N <= 10 000."""
    pkg, torch, bench, dev = ctx
    outs = []
    for rep in range(2):
        eng, inp, _ = bench.build_engine(pkg, torch, dev, WL30, 0)
        assert eng.product_mode() == 3
        sc = []
        for t in range(2):
            sc.append(eng.step(want_scalars=True)); eng.monitor()
        M = eng.buffer("M")
        assert torch.equal(M, M.t()) and float(M.diagonal().abs().max()) == 0.0
        assert float(M.min()) >= 0.0 and float(M.max()) <= 1.0
        assert eng.path_stats() == {"lowrank_steps": 2, "general_steps": 0} and eng.fused_steps() == 2
        assert all(np.isfinite(s["loss"]) for s in sc)
        outs.append((eng.get_adj_changes().clone(), [s["loss"] for s in sc]))
        del eng, M
        torch.cuda.empty_cache()
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], "two runs must give identical bits"
    del outs
    nxn = (0.01, 0.01, 0, 0, 0, 10, 10, 0, 0, 0)       # without the small-operand terms the N x N terms carry the gradient
    fast, _, _ = bench.build_engine(pkg, torch, dev, WL30, 0, weight_param=nxn)
    a = fast.step(want_scalars=True)
    gf = fast.buffer("G_sym")
    del fast
    torch.cuda.empty_cache()
    monkeypatch.setenv("MCGRA_NO_LOWRANK", "1")
    gram, _, _ = bench.build_engine(pkg, torch, dev, WL30, 0, weight_param=nxn)
    monkeypatch.delenv("MCGRA_NO_LOWRANK")
    b = gram.step(want_scalars=True)
    gg = gram.buffer("G_sym")
    assert gram.path_stats()["general_steps"] == 1 and gram.gram_split_steps() == 1
    err = float((gf - gg).abs().max()) / float(gg.abs().max())
    assert err < 1e-4, err
    for k in ("loss", "c1", "c2", "c6", "c7"):
        assert a[k] == pytest.approx(b[k], rel=1e-3, abs=1e-6), k


def test_masked_bench_workload_stays_fused_at_10k(ctx, monkeypatch):
    """`synthetic-10k-hsic-masked`: the headline shape with 10 x 10 nodes whose embeddings have disjoint supports -- 200
    relu-masked decode pairs, no dead row.  Rounds 1 - 3 redid every such step with the Gram evaluation (3x slower); the
    fused step stands and its gradient equals the Gram evaluation's."""
    pkg, torch, bench, dev = ctx
    wl = "synthetic-10k-hsic-masked"
    fast, _, _ = bench.build_engine(pkg, torch, dev, wl, 0)
    monkeypatch.setenv("MCGRA_NO_LOWRANK", "1")
    gram, _, _ = bench.build_engine(pkg, torch, dev, wl, 0)
    monkeypatch.delenv("MCGRA_NO_LOWRANK")
    for t in range(2):
        a = fast.step(want_scalars=True); fast.monitor()
        b = gram.step(want_scalars=True)
        gf, gg = fast.buffer("G_sym"), gram.buffer("G_sym")
        assert float((gf - gg).abs().max()) <= 5e-5 * float(gg.abs().max()), t
        for k in ("loss", "c1", "c2", "c9"):
            assert a[k] == pytest.approx(b[k], rel=3e-4, abs=1e-6), (t, k)
        gram.set_adj_changes(fast.get_adj_changes())
    assert fast.fused_steps() == 2 and fast.masked_fused_steps() == 2 and fast.path_stats()["general_steps"] == 0
    assert gram.path_stats()["general_steps"] == 2
