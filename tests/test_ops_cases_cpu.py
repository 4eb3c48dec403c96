"""The standalone ops without a device: (a) the float64 truths of tests/ops_truth.py are the reference's formulas -- they
reproduce the reference's own values in tests/golden/ops.npz within the float32 class of its run (the tolerances of
tests/test_oracle_golden.py for the same keys); (b) every case of tests/test_gpu_ops.py can tell a wrong kernel from a right
one: under each defect that applies to it the float64 answer moves by at least 10 of the case's bounds (a condition on the
inputs: a case that misses it gets other inputs, never another factor); (c) the refusals the arguments alone decide, with
pointers that are never followed; (d) the wrappers refuse what they cannot hand to the C ABI.
mutual_information has a section of its own: its truth against the reference's double run (tests/golden/ops_kde.npz), its
cases against their defects, a float32 emulation of the kernel values that has to stay within a third of the tolerances the
GPU test asserts, and the bins of kde_bin (csrc/kde_kernels.hip) against torch.linspace bit for bit."""
import argparse
import ctypes
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import ops_truth as T

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mc-gra_amd", "libmcgra_hip.so")
OPS = np.load(os.path.join(H.GOLDEN, "ops.npz"))
FACTOR = 10.0


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


# ------------------------------------------------------------------------------------------ (a) truths vs the reference
@pytest.mark.parametrize("sg", [1.0, 5.0])
def test_truth_gaussian_hsic_is_the_reference(sg):
    x, y = OPS["ghsic_x"], OPS["ghsic_y"]
    ref = float(OPS[f"ghsic_reg_{sg}"])
    assert abs(T.hsic_regular(x, y, sg) - ref) <= 2e-5 * abs(ref) + 1e-9
    ref = float(OPS[f"ghsic_norm_{sg}"])
    assert abs(T.hsic_normalized(x, y, sg) - ref) <= 2e-4 * abs(ref)


def test_truth_hsic_py_remainder_is_the_reference():
    x, y, z = OPS["ghsic_x"], OPS["ghsic_y"], OPS["ghsic_z"]
    sxx, syy, szz, syz = T.sigma_estimation(x, x), T.sigma_estimation(y, y), T.sigma_estimation(z, z), T.sigma_estimation(y, z)
    assert abs(sxx - float(OPS["ghsic_sigma_xx"])) <= 1e-5 * float(OPS["ghsic_sigma_xx"])
    assert abs(syy - float(OPS["ghsic_sigma_yy"])) <= 1e-5 * float(OPS["ghsic_sigma_yy"])
    assert abs(syz - float(OPS["ghsic_sigma_yz"])) <= 1e-5 * float(OPS["ghsic_sigma_yz"])
    assert rel(T.distmat(x), OPS["ghsic_distmat"]) < 1e-6
    ref = float(OPS["ghsic_reg_auto"])
    assert abs(T.hsic_regular(x, y, sxx, syy) - ref) <= 1e-4 * abs(ref)
    ref = float(OPS["ghsic_norm_auto"])
    assert abs(T.hsic_normalized(x, y, sxx, syy) - ref) <= 2e-4 * abs(ref)
    assert abs(T.distcorr(x, 2.0) - float(OPS["ghsic_distcorr_2.0"])) <= 1e-5
    for sg, (a, b, c), (px, py) in ((None, (syy, szz, syz), (sxx, syy)), (1.5, (1.5, 1.5, 1.5), (1.5, 1.5))):
        ref = float(OPS[f"ghsic_mmd_{sg}"])
        assert abs(T.mmd(y, z, a, b, c) - ref) <= 2e-5 * abs(ref)
        ref = float(OPS[f"ghsic_mmdp_{sg}"])
        assert abs(T.mmd_pxpy_pxy(x, y, px, py) - ref) <= 2e-4 * abs(ref) + 1e-8


@pytest.mark.parametrize("tag", ["a", "b"])
def test_truth_linear_hsic_is_the_reference(tag):
    X, Y, ref = OPS[f"hsic_{tag}_X"], OPS[f"hsic_{tag}_Y"], float(OPS[f"hsic_{tag}_val"])
    v = T.linear_hsic(X, Y)
    assert abs(v - ref) <= 2e-5 * abs(ref)
    # the form the kernel evaluates, |Xc^T Yc|_F^2, is the same number (the defects are stated on it)
    Xc, Yc = X.astype(np.float64) - X.mean(0, dtype=np.float64), Y.astype(np.float64) - Y.mean(0, dtype=np.float64)
    assert abs(((Xc.T @ Yc) ** 2).sum() - v) <= 1e-10 * abs(v)


def test_truth_elementwise_ops_are_the_reference():
    assert abs(T.info_entropy(OPS["ie_in"]) - float(OPS["ie_val"])) < 1e-6
    assert abs(T.mse(OPS["mse_X"], OPS["mse_Y"]) - float(OPS["mse_val"])) <= 1e-5 * abs(float(OPS["mse_val"]))
    assert rel(T.normalize_adj(OPS["norm_in"]), OPS["norm_out"]) < 1e-6
    got = T.get_modified_adj(OPS["gma_a"], OPS["gma_ori"], 30)
    assert got.dtype == np.float32 and np.array_equal(got, OPS["gma_out"])          # data movement: bit exact
    assert np.array_equal(T.pack_tril(T.get_modified_adj(OPS["gma_a"], None, 30)), OPS["gma_a"])
    assert rel(T.dot_product_decode(OPS["dd2_Z"]), OPS["dd_out"]) < 2e-6


def test_truth_decode2_is_the_reference(pkg):
    from mc_gra_amd.topology_attack import _decode_mode
    keys = [k for k in OPS.files if k.startswith("dd2_") and k != "dd2_Z"]
    assert len(keys) == 10
    seen = set()
    for k in keys:
        _, ds, use = k.split("_")
        mode = _decode_mode(argparse.Namespace(dataset=ds, useH_A=use[0] == "1", useY_A=use[1] == "1", useY=use[2] == "1"))
        seen.add(mode)
        assert rel(T.dot_product_decode2(OPS["dd2_Z"], mode), OPS[k]) < 2e-6, (k, mode)
    assert seen == set(range(7))


def test_truth_gcn_forward_is_a_log_softmax_of_the_chain():
    """No reference fixture holds a bare forward; the float64 chain is pinned to its definition instead: probabilities sum to
    one, the embedding is the chain's relu output, one layer by hand."""
    X, adj, W, b, Wlin, blin = T.gcn_case("n300_l1")
    lp, emb = T.gcn_forward(X, adj, W, b, Wlin, blin, emb_nlayer=1)
    assert np.abs(np.exp(lp).sum(1) - 1).max() < 1e-12 and emb.min() == 0.0
    H1 = np.maximum(adj.astype(np.float64) @ (X.astype(np.float64) @ W[0]) + b[0], 0)
    Z = H1 @ Wlin.T.astype(np.float64) + blin
    assert np.array_equal(emb, H1) and np.abs(lp - (Z - np.log(np.exp(Z).sum(1))[:, None])).max() < 1e-12


# ------------------------------------------------------------------------------------ (b) each case resolves each defect
def _resolves(truth, bound, wrong):
    """A scalar: |wrong - truth| >= FACTOR bound.  A matrix: in at least one element."""
    with np.errstate(invalid="ignore"):
        return bool(np.any(np.abs(np.asarray(wrong) - np.asarray(truth)) >= FACTOR * np.asarray(bound)))


GAUSS_BIG = [(m, dx, dy, s) for m in T.GAUSS_M if m > 2 for dx, dy in T.GAUSS_WIDTHS for s in T.GAUSS_SIGMAS]


@pytest.mark.parametrize("m,dx,dy,sg", GAUSS_BIG)
def test_gaussian_cases_resolve_their_defects(m, dx, dy, sg):
    """hsic_regular (one sigma and two), mmd_pxpy_pxy and distcorr carry the generic defects of the row loop and of the final
    reduction.  hsic_normalized is a quotient of three means that the same kernels form on the same buffers: a dropped column
    or row leaves all three short alike and largely cancels, so those defects are charged to hsic_regular at the same inputs
    (one GPU test runs both); the row mean taken at the wrong index is charged to both."""
    x, y = T.gauss_case(m, dx, dy, sg)
    sy = T.sigma_y_of(sg)
    generic = T.generic_defects(m)
    assert set(generic) >= {"lastcol", "lastrow"} and ("tail256" in generic) == (m % 256 != 0) and ("past1024" in generic) == (m > 1024)
    for fn, bf, args, defects in ((T.hsic_regular, T.hsic_regular_bound, (x, y, sg), generic + ["ymean_by_row"]),
                                  (T.hsic_regular, T.hsic_regular_bound, (x, y, sg, sy), generic + ["ymean_by_row"]),
                                  (T.hsic_normalized, T.hsic_normalized_bound, (x, y, sg), ["ymean_by_row"]),
                                  (T.hsic_normalized, T.hsic_normalized_bound, (x, y, sg, sy), ["ymean_by_row"]),
                                  (T.mmd_pxpy_pxy, T.mmd_pxpy_pxy_bound, (x, y, sg, sy), generic + ["no_extra_1_over_m"]),
                                  (T.distcorr, T.distcorr_bound, (x, sg), generic)):
        v, b = fn(*args), bf(*args)
        assert np.isfinite(v) and 0 < b < 1e-3 * abs(v), (fn.__name__, v, b)
        for d in defects:
            assert _resolves(v, b, fn(*args, defect=d)), (fn.__name__, args[2:], d, v, b, fn(*args, defect=d))
    D, B = T.distmat(x), T.distmat_bound(x)
    assert (B > 0).all() and (np.abs(D.diagonal()) <= B.diagonal()).all()
    assert _resolves(D, B, T.distmat(x, defect="sqnorm_lastcol"))


def test_gaussian_small_cases_are_what_their_assertions_say():
    """m = 1, 2 get assertions of their own on the GPU: at m = 1 the centred kernel matrix is 0, hsic_regular is 0 and the
    normalised form 0 / 0 = nan (hsic.py:131-134 divides without a guard); m = 2 is finite."""
    for dx, dy in T.GAUSS_WIDTHS:
        x, y = T.gauss_case(1, dx, dy, 1.0)
        assert T.hsic_regular(x, y, 1.0) == 0.0 and np.isnan(T.hsic_normalized(x, y, 1.0)) and T.distcorr(x, 1.0) == 1.0
        assert T.mmd_pxpy_pxy(x, y, 1.0, 1.5) == 0.0
        x, y = T.gauss_case(2, dx, dy, 1.0)
        assert T.hsic_regular(x, y, 1.0) > 0 and np.isfinite(T.hsic_normalized(x, y, 1.0))


@pytest.mark.parametrize("mx,my", T.MMD_SHAPES)
@pytest.mark.parametrize("d", T.MMD_D)
def test_mmd_cases_resolve_their_defects(mx, my, d):
    x, y = T.mmd_case(mx, my, d)
    assert mx != my and len(set(T.MMD_SIGMAS)) == 3 and np.array_equal(y[-1], x[0])
    v, b = T.mmd(x, y, *T.MMD_SIGMAS), T.mmd_bound(x, y, *T.MMD_SIGMAS)
    assert 0 < b < 1e-3 * abs(v)
    for df in T.generic_defects(mx, my) + ["cross_mxmx", "ynorm_from_x"]:
        assert _resolves(v, b, T.mmd(x, y, *T.MMD_SIGMAS, defect=df)), (df, v, b, T.mmd(x, y, *T.MMD_SIGMAS, defect=df))


@pytest.mark.parametrize("shape", T.LINEAR_HSIC_SHAPES)
def test_linear_hsic_cases_resolve_their_defects(shape):
    X, Y = T.linear_hsic_case(*shape)
    v, b = T.linear_hsic(X, Y), T.linear_hsic_bound(X, Y)
    assert 0 < b < 1e-3 * v
    for df in T.generic_defects(shape[0], shape[2]):
        assert _resolves(v, b, T.linear_hsic(X, Y, defect=df)), (df, v, b)


@pytest.mark.parametrize("n", T.IE_N)
def test_info_entropy_cases_resolve_their_defects(n):
    P = T.ie_case(n)
    lo, hi = np.float32(1e-4), np.float32(1) - np.float32(1e-4)
    assert float(lo) == T.IE_LO and float(hi) == T.IE_HI
    assert P.min() < -0.09 and P.max() > 1.09 and all((P == v).any() for v in (lo, hi, 0.0, 1.0))
    v, b = T.info_entropy(P), T.info_entropy_bound(P)
    assert 0 < b < 1e-5 * v
    for df in T.generic_defects(n) + ["no_lo", "no_hi"]:
        assert _resolves(v, b, T.info_entropy(P, defect=df)), (df, v, b)


@pytest.mark.parametrize("count", T.MSE_COUNTS)
def test_mse_cases_resolve_their_defects(count):
    X, Y = T.mse_case(count)
    v, b = T.mse(X, Y), T.mse_bound(X, Y)
    assert 0 < b < 1e-6 * v
    defects = (["lastcol"] if count > 1 else []) + (["past_grid"] if count > 1024 * 256 else [])
    assert ("past_grid" in defects) == (count == 1024 * 256 + 3)
    for df in defects:
        assert _resolves(v, b, T.mse(X, Y, defect=df)), (df, v, b)
    if count == T.MSE_COUNTS[-1]:
        X, Y = T.mse_one_element_case()
        assert (X != Y).sum() == 1 and X[-1] != Y[-1]
        v, b = T.mse(X, Y), T.mse_bound(X, Y)
        assert v == 0.75 ** 2 / count and _resolves(v, b, T.mse(X, Y, defect="lastcol")) and _resolves(v, b, T.mse(X, Y, defect="past_grid"))


@pytest.mark.parametrize("n", T.ADJ_N)
def test_adjacency_cases_show_a_misplaced_element(n):
    """Data movement is compared bit for bit; the case's part is that no two elements are alike, with and without ori_adj."""
    a, ori = T.adj_case(n)
    assert len(np.unique(a)) == a.size == n * (n - 1) // 2 and len(np.unique(ori)) == n * n
    M = T.get_modified_adj(a, None, n)
    assert M.dtype == np.float32 and np.array_equal(M, M.T) and not M.diagonal().any()
    assert len(np.unique(M[np.tril_indices(n, -1)])) == a.size and np.array_equal(T.pack_tril(M), a)
    full = T.get_modified_adj(a, ori, n)
    assert np.array_equal(full.astype(np.float64), M.astype(np.float64) + ori)      # the sum is exact
    rows, cols = T.tril_indices(n)
    assert rows[0] == 1 and cols[0] == 0 and (rows > cols).all() and (np.diff(rows * n + cols) > 0).all()


@pytest.mark.parametrize("n", T.NORM_N)
def test_normalize_adj_cases_resolve_their_defects(n):
    A = T.norm_case(n)
    d = (A.astype(np.float64) + np.eye(n)).sum(1)
    assert not A[3].any() and d[3] == 1 and A[5].any() and A[5].astype(np.float64).sum() == 0 and d[5] == 1 and d[9] == 0
    assert (np.delete(d, 9) > 0.4).all() and np.array_equal(A, A.T)
    v, b = T.normalize_adj(A), T.normalize_adj_bound(A)
    assert np.isfinite(v).all() and not v[9].any() and not v[:, 9].any() and v[3, 3] == 1 and v[5, 5] == 1
    for df in ("lastcol", "tail256"):
        assert _resolves(v, b, T.normalize_adj(A, defect=df)), df
    # a kernel that took the row sum without the identity would wipe row 5 (inf -> 0): far beyond the bound
    assert abs(v[5, 20]) > 1e3 * b[5, 20] > 0


@pytest.mark.parametrize("n,d", T.DECODE_SHAPES)
def test_decode_cases_resolve_their_defects(n, d):
    Z = T.decode_case(n, d)
    assert not Z[4].any() and (Z < 0).any() and (d >= 192) == ((n, d) == (300, 200))       # 64 (h + 1) 4 > 48 KB from h = 192
    v, b = T.dot_product_decode(Z), T.dot_product_decode_bound(Z)
    assert (b >= 0).all() and b.max() < 1e-4
    for df in ("no_relu", "lastcol"):
        assert _resolves(v, b, T.dot_product_decode(Z, defect=df)), df
    for kind in ("plain", "decades"):
        Zk = T.decode_case(n, d, kind)
        if kind == "decades":
            mag = np.abs(Zk[Zk != 0])
            assert (Zk < 0).any() and (Zk > 0).any() and mag.max() / mag.min() > 1e4
        for mode in (range(7) if kind == "plain" else (5, 6)):
            v, b = T.dot_product_decode2(Zk, mode), T.dot_product_decode2_bound(Zk, mode)
            assert np.isfinite(v).all() and (b >= 0).all() and b.max() < 1e-3 * np.abs(v).max(), (kind, mode, b.max())
            defects = ["no_eye"] + (["p2"] if mode in (5, 6) else []) + (["lastcol", "tail256"] if mode == 3 else [])
            for df in defects:
                assert _resolves(v, b, T.dot_product_decode2(Zk, mode, defect=df)), (kind, mode, df)
    S = Z.astype(np.float64) @ Z.T.astype(np.float64)
    assert not S[4].any() and not T.dot_product_decode2(Z, 3)[4].any()          # mode 3 with an all-zero row of S


@pytest.mark.parametrize("name", list(T.GCN_CASES))
def test_gcn_cases_resolve_their_defects(name):
    c = T.gcn_case(name)
    n, _, widths, _ = T.GCN_CASES[name]
    for emb in range(1, len(widths) + 1):
        (v, e), (b, be) = T.gcn_forward(*c, emb_nlayer=emb), T.gcn_forward_bound(*c, emb_nlayer=emb)
        assert e.shape == (n, widths[emb - 1]) and be.shape == e.shape and (e > 0).any() and (e == 0).any()
        assert b.max() < 1e-3 and be.max() < 1e-4
    for df in [d for d in T.generic_defects(n) if d != "lastcol"]:
        assert _resolves(v, b, T.gcn_forward(*c, emb_nlayer=emb, defect=df)[0]), df


def test_bounds_are_first_order_sums_with_a_named_safety_factor():
    assert T.U == 2.0 ** -24 and 1 <= T.SAFETY <= 4 and T.GEMM == 4e-7
    x, y = T.gauss_case(257, 7, 3, 1.0)
    E = T._dist_err(x, x)
    r = (x.astype(np.float64) ** 2).sum(1)
    assert np.allclose(E[0, 0], 10 * T.U * 4 * r[0]) and np.allclose(T.distmat_bound(x), T.SAFETY * E)


# ------------------------------------------------------------------------------------------------ mutual_information
KDE_OPS = np.load(os.path.join(H.GOLDEN, "ops_kde.npz"))


@pytest.mark.parametrize("tag", [str(c) for c in KDE_OPS["cases"]])
def test_truth_mutual_information_is_the_reference(tag):
    """The float64 truth against the reference module's run on double tensors: the value to 1e-12, the gradients (stored as
    float32 in the fixture) to 1e-7 of their largest magnitude."""
    z = KDE_OPS
    v, gx, gy = T.mutual_information(z[f"{tag}_x"], z[f"{tag}_y"])
    assert abs(v - float(z[f"{tag}_val64"][0])) <= 1e-12
    assert rel(gx, z[f"{tag}_gx64"]) <= 1e-7 and rel(gy, z[f"{tag}_gy64"]) <= 1e-7


def test_mutual_information_cases_cover_every_kernel_form():
    """What the shapes are there for: the three template widths from both sides of their switches, one and several blocks of
    k_kde_stats (64 rows) and k_kde_grad (128 rows) with and without a ragged tail, dozens of partials for k_kde_tables'
    loop, both sides of the c > 32 switch, and wide square operands that reach 6, 7, 25 and 32 columns -- and 33, refused."""
    shapes = {(m, c) for _, m, c in T.MI_CASES}
    assert {c for _, c in shapes} >= {1, 2, 7, 8, 9, 16, 17, 32, 33} and {m for m, _ in shapes} >= {1, 2, 63, 64, 65, 128, 129, 257, 1030, 5000}
    assert (32, 32) in shapes and (33, 33) in shapes and set(T.MI_RAW_CASES) <= set(T.MI_CASES)
    for case in T.MI_CASES:
        X, Y = T.mi_case(*case)
        assert X.dtype == Y.dtype == np.float32 and X.shape == Y.shape == case[1:]
        if case[2] > T.KDE_MAXC:
            assert T.kde_reach(X, Y) == T.MI_REACH[case] <= T.KDE_MAXC, case
    X, Y = T.mi_case("reach32", 300, 300)
    assert X.max() == 27.0 == X[5, 27] and Y.max() <= 26.0
    Xr, Yr = T.mi_refused_case()
    assert Xr.max() == 27.5 and (Xr != X).sum() == 1 and T.kde_reach(Xr, Yr) == 33


@pytest.mark.parametrize("kind,m,c", T.MI_CASES)
def test_mutual_information_cases_resolve_their_defects(kind, m, c):
    """Under every defect that applies the truth's value moves by FACTOR of its bound, or a gradient by FACTOR tolerances
    (KDE_GRAD_TOL of that operand's largest magnitude); and the float32 emulation of the kernel values -- what a correct
    evaluation returns -- uses at most a third of either, the condition that keeps the tolerances honest."""
    X, Y = T.mi_case(kind, m, c)
    v, gx, gy, b = T.mi_truth(kind, m, c)
    mx, my = np.abs(gx).max(), np.abs(gy).max()
    assert np.isfinite(v) and np.isfinite(gx).all() and np.isfinite(gy).all() and mx > 0 and my > 0
    assert 1e3 * 2.0 ** -53 < b < 1e-4 * max(abs(v), 1e-2), (v, b)       # float32's part, well above the device's double arithmetic
    ev, egx, egy = T.mutual_information_f32(X, Y)
    assert abs(ev - v) <= b / 3, (abs(ev - v), b)
    assert np.abs(egx - gx).max() <= T.KDE_GRAD_TOL / 3 * mx and np.abs(egy - gy).max() <= T.KDE_GRAD_TOL / 3 * my, (
        np.abs(egx - gx).max() / mx, np.abs(egy - gy).max() / my)
    if c > T.KDE_MAXC:           # cut at the reach: exact zeros from there on, something below it
        act = T.MI_REACH[(kind, m, c)]
        assert not egx[:, act:].any() and not egy[:, act:].any() and egx[:, :act].any() and egy[:, :act].any()
        assert np.abs(gx[:, act:]).max() <= 1e-30 * mx and np.abs(gy[:, act:]).max() <= 1e-30 * my
    defects = T.mi_defects(kind, m, c)
    assert set(defects) <= set(T.MI_DEFECTS) and "no_marginal" in defects
    for d in defects:
        dv, dgx, dgy = T.mutual_information(X, Y, defect=d)
        moved = (abs(dv - v) >= FACTOR * b or np.abs(dgx - gx).max() >= FACTOR * T.KDE_GRAD_TOL * mx
                 or np.abs(dgy - gy).max() >= FACTOR * T.KDE_GRAD_TOL * my)
        assert moved, (d, abs(dv - v) / b, np.abs(dgx - gx).max() / mx, np.abs(dgy - gy).max() / my)


def test_every_mutual_information_defect_is_met_by_some_case():
    met = {d for case in T.MI_CASES for d in T.mi_defects(*case)}
    assert met == set(T.MI_DEFECTS)
    assert "cols8" in T.mi_defects("nxn20", 257, 257) and "cols8" not in T.mi_defects("nxn2", 1030, 1030)
    assert "lastcol" not in T.mi_defects("nxn1", 33, 33) and "lastcol" in T.mi_defects("emb", 32, 32)


def test_kde_bins_are_torch_linspace_bit_for_bit():
    """kde_bin's formula (csrc/kde_kernels.hip), evaluated in numpy with float32 roundings, against the reference's
    torch.linspace(0, nb, nb).float() for every width up to 64 and every square size the cases and the fixture use."""
    import torch
    for nb in list(range(1, 65)) + [160, 200, 257, 300, 1030]:
        assert T.kde_bins(nb).tobytes() == torch.linspace(0, nb, nb).float().numpy().tobytes(), nb


# ------------------------------------------------------------------------------------------------------- (c) refusals
EINVAL, ENOSUP = -1, -3


def _entries(L):
    """name -> (call(**overrides), the default arguments); every pointer is the never-followed address 64."""
    p = ctypes.c_void_p(64)
    dims = (ctypes.c_int32 * 3)(11, 8, 8)
    ptrs = (ctypes.c_void_p * 2)(64, 64)

    def entry(fn, order, **defaults):
        def call(**kw):
            a = dict(defaults, **kw)
            return fn(None, *[a[k] for k in order])
        return call, defaults

    return {
        "get_modified_adj": entry(L.mcgra_get_modified_adj, ("n", "a", "ori", "out"), n=4, a=p, ori=None, out=p),
        "pack_tril": entry(L.mcgra_pack_tril, ("n", "M", "ld", "out"), n=4, M=p, ld=4, out=p),
        "normalize_adj": entry(L.mcgra_normalize_adj, ("n", "adj", "out"), n=4, adj=p, out=p),
        "info_entropy": entry(L.mcgra_info_entropy, ("n", "prob", "out"), n=4, prob=p, out=p),
        "dot_product_decode": entry(L.mcgra_dot_product_decode, ("n", "d", "Z", "out"), n=4, d=3, Z=p, out=p),
        "dot_product_decode2": entry(L.mcgra_dot_product_decode2, ("n", "d", "Z", "mode", "out"), n=4, d=3, Z=p, mode=0, out=p),
        "mutual_information": entry(L.mcgra_mutual_information, ("m", "c", "X", "Y", "out", "gX", "gY"), m=4, c=4, X=p, Y=p, out=p,
                                    gX=None, gY=None),
        "linear_hsic": entry(L.mcgra_linear_hsic, ("m", "dx", "dy", "X", "Y", "out"), m=4, dx=3, dy=2, X=p, Y=p, out=p),
        "hsic_regular": entry(L.mcgra_hsic_regular, ("m", "dx", "dy", "X", "Y", "sigma", "out"), m=4, dx=3, dy=2, X=p, Y=p,
                              sigma=1.0, out=p),
        "hsic_normalized": entry(L.mcgra_hsic_normalized, ("m", "dx", "dy", "X", "Y", "sigma", "out"), m=4, dx=3, dy=2, X=p, Y=p,
                                 sigma=1.0, out=p),
        "hsic_regular2": entry(L.mcgra_hsic_regular2, ("m", "dx", "dy", "X", "Y", "sx", "sy", "normalized", "out"), m=4, dx=3, dy=2,
                               X=p, Y=p, sx=1.0, sy=2.0, normalized=0, out=p),
        "hsic_normalized_cca": entry(L.mcgra_hsic_normalized_cca, ("m", "dx", "dy", "X", "Y", "sx", "sy", "out"), m=4, dx=3, dy=2,
                                     X=p, Y=p, sx=1.0, sy=2.0, out=p),
        "distmat": entry(L.mcgra_distmat, ("m", "d", "X", "out"), m=4, d=3, X=p, out=p),
        "mmd": entry(L.mcgra_mmd, ("mx", "my", "d", "X", "Y", "sx", "sy", "sxy", "out"), mx=4, my=5, d=3, X=p, Y=p, sx=1.0, sy=2.0,
                     sxy=1.5, out=p),
        "mmd_pxpy_pxy": entry(L.mcgra_mmd_pxpy_pxy, ("m", "dx", "dy", "X", "Y", "sx", "sy", "out"), m=4, dx=3, dy=2, X=p, Y=p,
                              sx=1.0, sy=2.0, out=p),
        "mse": entry(L.mcgra_mse, ("count", "X", "Y", "out"), count=4, X=p, Y=p, out=p),
        "gcn_forward": entry(L.mcgra_gcn_forward, ("n", "nfeat", "nlayer", "dims", "X", "adj", "W", "b", "Wlin", "blin", "nclass",
                                                   "emb_nlayer", "emb", "out"), n=4, nfeat=11, nlayer=2, dims=dims, X=p, adj=p,
                             W=ptrs, b=ptrs, Wlin=p, blin=p, nclass=3, emb_nlayer=0, emb=None, out=p),
    }


OPTIONAL = {"ori", "gX", "gY", "emb"}           # pointers that may be NULL
SIZES = {"n", "m", "mx", "my", "d", "dx", "dy", "c", "count", "nfeat", "nclass"}


def test_standalone_entries_refuse_before_touching_a_device(pkg):
    """MCGRA_EINVAL for a null operand and for a size below the entry's minimum, from every standalone entry, with no GPU in
    the machine and pointers that are never followed."""
    L = pkg._lib.lib
    entries = _entries(L)
    from tests.test_cabi_symbols import header_symbols
    standalone = {"mcgra_" + k for k in entries}
    assert standalone <= set(header_symbols())
    for name, (call, defaults) in entries.items():
        for arg, val in defaults.items():
            if isinstance(val, (ctypes.c_void_p, ctypes.Array)) and arg not in OPTIONAL:
                assert call(**{arg: None}) == EINVAL, (name, arg)
                assert L.mcgra_last_error(), name
            elif arg in SIZES:
                for bad in (0, -1):
                    assert call(**{arg: bad}) == EINVAL, (name, arg, bad)
    assert entries["dot_product_decode"][0](n=1) == EINVAL                   # a strict lower triangle needs two nodes
    for mode in (-1, 7, 100):
        assert entries["dot_product_decode2"][0](mode=mode) == EINVAL and b"decode_mode" in L.mcgra_last_error()
    nan = float("nan")
    for bad in (0.0, -1.0, nan):
        for name, args in (("hsic_regular2", ("sx", "sy")), ("mmd", ("sx", "sy", "sxy")), ("mmd_pxpy_pxy", ("sx", "sy")),
                           ("hsic_normalized_cca", ("sx", "sy"))):
            for a in args:
                assert entries[name][0](**{a: bad}) == EINVAL, (name, a, bad)
        for name in ("hsic_regular", "hsic_normalized"):                      # sigma=None of the reference: the host mirror's part
            assert entries[name][0](sigma=bad) == ENOSUP and b"median" in L.mcgra_last_error(), (name, bad)
    assert entries["hsic_normalized_cca"][0](m=8193) == ENOSUP and b"8193" in L.mcgra_last_error()
    assert entries["mutual_information"][0](m=40, c=33) == ENOSUP and b"square" in L.mcgra_last_error()
    g = entries["gcn_forward"][0]
    assert g(nfeat=12) == EINVAL                                                # dims[0] != nfeat
    for nl in (0, -1, pkg._lib.MAX_LAYERS + 1):
        assert g(nlayer=nl) == EINVAL, nl
    assert g(dims=(ctypes.c_int32 * 3)(11, 0, 8)) == EINVAL and b"width" in L.mcgra_last_error()
    with pytest.raises(pkg._lib.McgraNotSupported):
        pkg._lib.check(entries["hsic_regular"][0](sigma=0.0))
    with pytest.raises(pkg._lib.McgraError):
        pkg._lib.check(entries["mse"][0](count=0))


def test_gemm_family_refuses_null_operands_before_touching_a_device(pkg):
    L, p = pkg._lib.lib, ctypes.c_void_p(64)
    assert L.mcgra_sgemm(None, 0, 0, 4, 4, 4, 1.0, None, 4, p, 4, 0.0, p, 4) == EINVAL
    assert L.mcgra_sgemm(None, 0, 0, 4, 4, 4, 1.0, p, 4, p, 4, 0.0, None, 4) == EINVAL
    assert L.mcgra_sgemm(None, 0, 0, -1, 4, 4, 1.0, p, 4, p, 4, 0.0, p, 4) == EINVAL
    assert L.mcgra_ssyrk_lower(None, 0, 4, 1.0, p, 4, 0.0, p, 4) == EINVAL and L.mcgra_ssyrk_lower(None, 4, 4, 1.0, None, 4, 0.0, p, 4) == EINVAL
    assert L.mcgra_ssymm_lower(None, 4, 0, 1.0, p, 4, p, 4, 0.0, p, 4) == EINVAL and L.mcgra_ssymm_lower(None, 4, 4, 1.0, p, 4, None, 4, 0.0, p, 4) == EINVAL
    for fn in (L.mcgra_ssymm_split_bf16, L.mcgra_ssymm_split_f16):
        assert fn(None, 0, p, 4, p, 4, None, p, 4) == EINVAL and fn(None, 4, p, 4, None, 4, None, p, 4) == EINVAL
    assert L.mcgra_sgemm_skinny_x3(None, 8, p, 8, p, 4, 49, p, 49) == EINVAL and L.mcgra_sgemm_skinny_x3(None, 8, None, 8, p, 4, 4, p, 4) == EINVAL


# ---------------------------------------------------------------------------------------------- (d) the wrappers' operands
def test_wrappers_refuse_host_tensors_by_name(pkg):
    """A CPU tensor handed to a standalone wrapper is a ValueError naming the op, before anything else is called (its
    data_ptr() would be followed on the device)."""
    import torch
    from mc_gra_amd import engine as E
    from mc_gra_amd import hsic as HS
    sq, tall, vec = torch.zeros(5, 5), torch.zeros(5, 3), torch.zeros(10)
    calls = {
        "sgemm": lambda: E.sgemm(sq, sq), "ssyrk_lower": lambda: E.ssyrk_lower(tall), "ssymm_lower": lambda: E.ssymm_lower(sq, tall),
        "ssymm_split_bf16": lambda: E.ssymm_split_bf16(sq, sq), "ssymm_split_f16": lambda: E.ssymm_split_f16(sq, sq),
        "sgemm_skinny_x3": lambda: E.sgemm_skinny_x3(sq, tall), "normalize_adj_tensor": lambda: E.normalize_adj_tensor(sq),
        "get_modified_adj": lambda: E.get_modified_adj(vec, None, 5), "pack_tril": lambda: E.pack_tril(sq),
        "info_entropy": lambda: E.info_entropy(sq), "dot_product_decode": lambda: E.dot_product_decode(tall),
        "dot_product_decode2": lambda: E.dot_product_decode2(tall, 0), "linear_hsic": lambda: E.linear_hsic(tall, tall),
        "mutual_information": lambda: E.mutual_information(tall, tall), "hsic_regular": lambda: E.hsic_regular(tall, tall, 1.0),
        "hsic_normalized": lambda: E.hsic_normalized(tall, tall, 1.0), "mse": lambda: E.mse(tall, tall),
        "gcn_forward": lambda: E.gcn_forward(tall, sq, [torch.zeros(3, 4)], [torch.zeros(4)], torch.zeros(2, 4), torch.zeros(2)),
        "roc_auc": lambda: E.roc_auc(sq, sq), "decode_scores": lambda: E.decode_scores(tall, 0),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name):
            call()
    for name, call in {"distmat": lambda: HS.distmat(tall), "distcorr": lambda: HS.distcorr(tall), "mmd": lambda: HS.mmd(tall, tall, 1.0),
                       "mmd_pxpy_pxy": lambda: HS.mmd_pxpy_pxy(tall, tall, 1.0), "hsic_regular": lambda: HS.hsic_regular(tall, tall, 1.0),
                       "hsic_normalized": lambda: HS.hsic_normalized(tall, tall, 1.0), "sigma_estimation": lambda: HS.sigma_estimation(tall, tall),
                       "hsic_normalized_cca": lambda: HS.hsic_normalized_cca(tall, tall, 1.0)}.items():
        with pytest.raises(ValueError, match=name):
            call()


def test_gemm_family_refuses_what_it_cannot_read_as_float32_rows(pkg):
    """The strided family converts nothing (a copy would break out= aliasing): a dtype other than float32 or an inner stride
    other than 1 is a ValueError.  Checked on the undecorated functions: the refusal needs no device."""
    import torch
    from mc_gra_amd import engine as E
    f, dbl, tr = torch.zeros(8, 8), torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, 8).t()
    assert tr.stride(1) != 1
    thin, thin64, thin_t = torch.zeros(8, 4), torch.zeros(8, 4, dtype=torch.float64), torch.zeros(4, 8).t()
    rs64, rs_strided = torch.zeros(8, dtype=torch.float64), torch.zeros(16)[::2]
    bad = [
        (E.sgemm, (dbl, f)), (E.sgemm, (f, dbl)), (E.sgemm, (tr, f)), (E.sgemm, (f, tr)), (E.sgemm, (f, f), dict(out=dbl)),
        (E.sgemm, (f, f), dict(out=tr)), (E.sgemm, (torch.zeros(8, 8, dtype=torch.float16), f)),
        (E.ssyrk_lower, (thin64,)), (E.ssyrk_lower, (thin_t,)), (E.ssyrk_lower, (thin,), dict(out=dbl)),
        (E.ssymm_lower, (dbl, thin)), (E.ssymm_lower, (f, thin64)), (E.ssymm_lower, (tr, thin)), (E.ssymm_lower, (f, thin_t)),
        (E.ssymm_split_bf16, (dbl, f)), (E.ssymm_split_bf16, (f, tr)), (E.ssymm_split_bf16, (f, f, rs64)),
        (E.ssymm_split_bf16, (f, f, rs_strided)), (E.ssymm_split_f16, (f, dbl)), (E.ssymm_split_f16, (tr, f)),
        (E.ssymm_split_f16, (f, f, rs64)), (E.ssymm_split_f16, (f, f, None, tr)),
        (E.sgemm_skinny_x3, (dbl, thin)), (E.sgemm_skinny_x3, (f, thin64)), (E.sgemm_skinny_x3, (tr, thin)), (E.sgemm_skinny_x3, (f, thin_t)),
    ]
    for case in bad:
        fn, args, kw = case if len(case) == 3 else (*case, {})
        with pytest.raises(ValueError, match=fn.__name__):
            fn.__wrapped__(*args, **kw)
    assert E._strided_f32("sgemm", f, thin, None, torch.zeros(8, 12)[:, :8]) is None           # a padded leading dimension is fine
    # the converting helper: what the kernels read, and the operand itself where it already is that
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4).t().requires_grad_()
    y = E._f32(x)
    assert y.dtype == torch.float32 and y.is_contiguous() and not y.requires_grad and torch.equal(y, x.detach().float())
    assert E._f32(f) is not None and E._f32(f).data_ptr() == f.data_ptr() and E._f32(None) is None
