"""The standalone ops of include/mcgra.h against their float64 truths (tests/ops_truth.py), beyond one block of rows: every
case runs the C ABI through the host wrappers, compares with the float64 truth and asserts |got - truth| <= bound, the a-priori
bound of the float32 evaluation computed from the same inputs (elementwise for a matrix; a scalar's bound holds the rounding of
the returned float).  Every op runs twice and must return the same bits: these kernels add no floats atomically and reduce in a
fixed order.  tests/test_ops_cases_cpu.py shows without a device that each case here would tell a wrong kernel from a right
one.  Each test prints max |error| / bound (DESIGN.md section 5 holds the table).  Run with -m gpu.

mutual_information (the whole arithmetic of measure KDE) is held to the same kind of truth at every form of its three kernels,
through the wrapper and the raw C ABI with a gradient output absent.  Its kernels came out right at every case: the largest
value error is 0.12 of its bound, the largest gradient error 0.26 of the 3e-6 it is held to.  What was wrong lay around them:
engine.mutual_information handed float64 or half tensors to the C ABI as they were and allocated the gradients in the
operands' dtype, and the wide-square branch took floorf of an infinite maximum (status 0 with a 0 / 0 value); both are fixed
and tested here."""
import numpy as np
import pytest

from tests import ops_truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


@pytest.fixture(scope="module")
def HS(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + ".hsic")


def dev(a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def twice(fn):
    """fn() as a numpy array, after a second call has returned the same bits."""
    a, b = fn(), fn()
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), "two runs on the same inputs differ"
    return a


def within(op, case, got, truth, bound):
    got, truth, bound = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.asarray(bound, np.float64)
    assert got.shape == truth.shape == bound.shape, (op, case, got.shape, truth.shape)
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    print(f"[ops] {op} {case}: max |error| / bound = {float(np.max(ratio)):.4f} (max |error| {float(np.max(err)):.3e})")
    assert np.all(err <= bound), (op, case, float(np.max(ratio)), float(np.max(err)))


# -------------------------------------------------------------------------------------------------- the Gaussian family
@pytest.mark.parametrize("sg", T.GAUSS_SIGMAS)
@pytest.mark.parametrize("dx,dy", T.GAUSS_WIDTHS)
@pytest.mark.parametrize("m", [m for m in T.GAUSS_M if m > 2])
def test_gaussian_family_within_the_float32_bound(E, HS, m, dx, dy, sg):
    """hsic_regular, hsic_normalized, both with one bandwidth per operand as well, mmd_pxpy_pxy, distcorr and distmat: m crosses
    the 256-thread row loop with and without a ragged tail, a second block of k_row_sqnorm and k_reduce_rows' own loop
    (m = 1030); the odd widths put sgemm on its unaligned loads with lda = d."""
    xn, yn = T.gauss_case(m, dx, dy, sg)
    x, y, sy, case = dev(xn), dev(yn), T.sigma_y_of(sg), (m, dx, dy, sg)
    within("hsic_regular", case, twice(lambda: E.hsic_regular(x, y, sg)), T.hsic_regular(xn, yn, sg), T.hsic_regular_bound(xn, yn, sg))
    within("hsic_normalized", case, twice(lambda: E.hsic_normalized(x, y, sg)), T.hsic_normalized(xn, yn, sg),
           T.hsic_normalized_bound(xn, yn, sg))
    assert twice(lambda: HS.hsic_regular(x, y, sg)).tobytes() == twice(lambda: E.hsic_regular(x, y, sg)).tobytes()
    within("hsic_regular2", case, twice(lambda: E.hsic_regular2(x, y, sg, sy)), T.hsic_regular(xn, yn, sg, sy),
           T.hsic_regular_bound(xn, yn, sg, sy))
    within("hsic_regular2(normalized)", case, twice(lambda: E.hsic_regular2(x, y, sg, sy, True)), T.hsic_normalized(xn, yn, sg, sy),
           T.hsic_normalized_bound(xn, yn, sg, sy))
    within("mmd_pxpy_pxy", case, twice(lambda: E.mmd_pxpy_pxy(x, y, sg, sy)), T.mmd_pxpy_pxy(xn, yn, sg, sy),
           T.mmd_pxpy_pxy_bound(xn, yn, sg, sy))
    within("distcorr", case, twice(lambda: HS.distcorr(x, sg)), T.distcorr(xn, sg), T.distcorr_bound(xn, sg))
    D = twice(lambda: HS.distmat(x))
    B = T.distmat_bound(xn)
    within("distmat", case, D, T.distmat(xn), B)
    assert D.tobytes() == np.ascontiguousarray(D.T).tobytes(), "distmat is not symmetric bit for bit"
    assert (np.abs(D.diagonal()) <= B.diagonal()).all()


@pytest.mark.parametrize("dx,dy", T.GAUSS_WIDTHS)
def test_gaussian_family_at_one_and_two_points(E, HS, dx, dy):
    """m = 1: the centred kernel matrix is 0, so hsic_regular is exactly 0 and mmd_pxpy_pxy = 1 - 2 + 1 = 0; hsic_normalized
    divides by sqrt(0) sqrt(0) without a guard (hsic.py:131-134) and the reference returns 0 / 0 = nan: so does the op.
    m = 2: finite, within the bound."""
    for sg in T.GAUSS_SIGMAS:
        xn, yn = T.gauss_case(1, dx, dy, sg)
        x, y, sy = dev(xn), dev(yn), T.sigma_y_of(sg)
        assert twice(lambda: E.hsic_regular(x, y, sg)) == 0.0 and twice(lambda: E.hsic_regular2(x, y, sg, sy)) == 0.0
        assert np.isnan(twice(lambda: E.hsic_normalized(x, y, sg))) and np.isnan(twice(lambda: E.hsic_regular2(x, y, sg, sy, True)))
        assert np.isnan(T.hsic_normalized(xn, yn, sg))
        within("mmd_pxpy_pxy", (1, dx, dy, sg), twice(lambda: E.mmd_pxpy_pxy(x, y, sg, sy)), 0.0, T.mmd_pxpy_pxy_bound(xn, yn, sg, sy))
        within("distcorr", (1, dx, dy, sg), twice(lambda: HS.distcorr(x, sg)), 1.0, T.distcorr_bound(xn, sg))
        within("distmat", (1, dx, dy, sg), twice(lambda: HS.distmat(x)), T.distmat(xn), T.distmat_bound(xn))
        xn, yn = T.gauss_case(2, dx, dy, sg)
        x, y, case = dev(xn), dev(yn), (2, dx, dy, sg)
        within("hsic_regular", case, twice(lambda: E.hsic_regular(x, y, sg)), T.hsic_regular(xn, yn, sg), T.hsic_regular_bound(xn, yn, sg))
        within("hsic_normalized", case, twice(lambda: E.hsic_normalized(x, y, sg)), T.hsic_normalized(xn, yn, sg),
               T.hsic_normalized_bound(xn, yn, sg))
        within("hsic_regular2", case, twice(lambda: E.hsic_regular2(x, y, sg, sy)), T.hsic_regular(xn, yn, sg, sy),
               T.hsic_regular_bound(xn, yn, sg, sy))
        within("mmd_pxpy_pxy", case, twice(lambda: E.mmd_pxpy_pxy(x, y, sg, sy)), T.mmd_pxpy_pxy(xn, yn, sg, sy),
               T.mmd_pxpy_pxy_bound(xn, yn, sg, sy))
        within("distcorr", case, twice(lambda: HS.distcorr(x, sg)), T.distcorr(xn, sg), T.distcorr_bound(xn, sg))
        D = twice(lambda: HS.distmat(x))
        within("distmat", case, D, T.distmat(xn), T.distmat_bound(xn))
        assert D[0, 1].tobytes() == D[1, 0].tobytes()


@pytest.mark.parametrize("d", T.MMD_D)
@pytest.mark.parametrize("mx,my", T.MMD_SHAPES)
def test_mmd_rectangular_within_the_float32_bound(E, mx, my, d):
    """The one rectangular use of k_gauss_kernel (y's squared norms, my columns, a leading dimension padded from my), with
    three different bandwidths: mx != my in both orders, and a single x."""
    xn, yn = T.mmd_case(mx, my, d)
    x, y = dev(xn), dev(yn)
    within("mmd", (mx, my, d), twice(lambda: E.mmd(x, y, *T.MMD_SIGMAS)), T.mmd(xn, yn, *T.MMD_SIGMAS), T.mmd_bound(xn, yn, *T.MMD_SIGMAS))


@pytest.mark.parametrize("m,dx,dy", T.LINEAR_HSIC_SHAPES)
def test_linear_hsic_within_the_float32_bound(E, m, dx, dy):
    """K = m on the transposed sgemm: one block of rows, 1 x 1 operands past k_reduce_rows' 1024, and m = 3000 where the
    product is split over K."""
    Xn, Yn = T.linear_hsic_case(m, dx, dy)
    X, Y = dev(Xn), dev(Yn)
    within("linear_hsic", (m, dx, dy), twice(lambda: E.linear_hsic(X, Y)), T.linear_hsic(Xn, Yn), T.linear_hsic_bound(Xn, Yn))


# ------------------------------------------------------------------------------------------------ elementwise reductions
@pytest.mark.parametrize("n", T.IE_N)
def test_info_entropy_within_the_float32_bound(E, n):
    Pn = T.ie_case(n)
    P = dev(Pn)
    within("info_entropy", n, twice(lambda: E.info_entropy(P)), T.info_entropy(Pn), T.info_entropy_bound(Pn))


@pytest.mark.parametrize("count", T.MSE_COUNTS)
def test_mse_within_the_float32_bound(E, count):
    """One element, one block with and without a tail, and the grid stride of 1024 x 256 threads just not taken and taken."""
    Xn, Yn = T.mse_case(count)
    X, Y = dev(Xn), dev(Yn)
    within("mse", count, twice(lambda: E.mse(X, Y)), T.mse(Xn, Yn), T.mse_bound(Xn, Yn))


def test_mse_of_operands_that_differ_in_their_last_element(E):
    Xn, Yn = T.mse_one_element_case()
    X, Y = dev(Xn), dev(Yn)
    got = twice(lambda: E.mse(X, Y))
    within("mse", "last element", got, T.mse(Xn, Yn), T.mse_bound(Xn, Yn))
    assert got > 0 and twice(lambda: E.mse(X, X)) == 0.0


# ------------------------------------------------------------------------------------------------------- data movement
@pytest.mark.parametrize("n", T.ADJ_N)
def test_get_modified_adj_and_pack_tril_move_every_element(E, n):
    """Bit exact, with and without ori_adj, through a second block in x (n > 256); pack_tril inverts get_modified_adj."""
    an, orin = T.adj_case(n)
    a, ori = dev(an), dev(orin)
    M = twice(lambda: E.get_modified_adj(a, None, n))
    assert M.tobytes() == T.get_modified_adj(an, None, n).tobytes()
    assert twice(lambda: E.get_modified_adj(a, ori, n)).tobytes() == T.get_modified_adj(an, orin, n).tobytes()
    assert twice(lambda: E.pack_tril(E.get_modified_adj(a, None, n))).tobytes() == an.tobytes()
    assert twice(lambda: E.pack_tril(ori)).tobytes() == T.pack_tril(orin).tobytes()         # an asymmetric matrix: the lower triangle


@pytest.mark.parametrize("n", T.NORM_N)
def test_normalize_adj_within_the_float32_bound(E, n):
    """An isolated node, a row whose entries cancel (d = 1 only with the identity) and a row with d = 0 (inf -> 0)."""
    An = T.norm_case(n)
    A = dev(An)
    got = twice(lambda: E.normalize_adj_tensor(A))
    within("normalize_adj", n, got, T.normalize_adj(An), T.normalize_adj_bound(An))
    assert not got[9].any() and not got[:, 9].any() and got[3, 3] == 1.0 and got[5, 5] == 1.0 and got[5, 20] != 0


# -------------------------------------------------------------------------------------------------------------- decodes
@pytest.mark.parametrize("n,d", T.DECODE_SHAPES)
def test_dot_product_decode_within_the_float32_bound(E, n, d):
    """d = 200 takes the 32-rows-per-block form of k_row_normalize; row 4 is all zero; negative products keep relu live."""
    Zn = T.decode_case(n, d)
    Z = dev(Zn)
    got = twice(lambda: E.dot_product_decode(Z))
    within("dot_product_decode", (n, d), got, T.dot_product_decode(Zn), T.dot_product_decode_bound(Zn))
    assert (got >= 0).all() and (got == 0).any()


@pytest.mark.parametrize("mode", range(7))
@pytest.mark.parametrize("n,d", T.DECODE_SHAPES)
def test_dot_product_decode2_within_the_float32_bound(E, n, d, mode):
    """All seven branches on the same operands (mode 3 meets an all-zero row of Z Z^T); the powf branches (p = 3, 5) also on
    entries of mixed sign over several decades."""
    for kind in ("plain", "decades") if mode in (5, 6) else ("plain",):
        Zn = T.decode_case(n, d, kind)
        Z = dev(Zn)
        got = twice(lambda: E.dot_product_decode2(Z, mode))
        within(f"dot_product_decode2[{mode}]", (n, d, kind), got, T.dot_product_decode2(Zn, mode), T.dot_product_decode2_bound(Zn, mode))
        if mode == 3:
            assert not got[4].any()


# ---------------------------------------------------------------------------------------------------------- GCN forward
@pytest.mark.parametrize("name,emb", [("n300_l3", 1), ("n300_l3", 2), ("n300_l3", 3), ("n300_l1", 1), ("n1030_l2", 2), ("n1030_l2", 0)])
def test_gcn_forward_within_the_float32_bound(E, name, emb):
    """Log-probabilities and the embedding against the float64 chain, the sgemm constant carried layer by layer."""
    c = T.gcn_case(name)
    X, adj, W, b, Wlin, blin = c
    args = (dev(X), dev(adj), [dev(w) for w in W], [dev(x) for x in b], dev(Wlin), dev(blin))
    (lp, e), (blp, be) = T.gcn_forward(*c, emb_nlayer=emb), T.gcn_forward_bound(*c, emb_nlayer=emb)
    within("gcn_forward", (name, emb), twice(lambda: E.gcn_forward(*args, emb_nlayer=emb)[0]), lp, blp)
    if emb:
        within("gcn_forward(embedding)", (name, emb), twice(lambda: E.gcn_forward(*args, emb_nlayer=emb)[1]), e, be)
    else:
        assert E.gcn_forward(*args)[1] is None


# --------------------------------------------------------------------------------------------------- mutual_information
EINVAL, ENOSUP = -1, -3
POISON = -7.25


def mi_twice(E, X, Y):
    """(value, gX, gY) as numpy arrays, after a second call has returned the same bits of all three."""
    runs = [E.mutual_information(X, Y, want_grad=True) for _ in range(2)]
    a, b = ([t.detach().cpu().numpy() for t in r] for r in runs)
    assert all(x.dtype == np.float32 and x.tobytes() == y.tobytes() for x, y in zip(a, b)), "two runs on the same inputs differ"
    return a


def mi_raw(pkg, E, X, Y, want_x, want_y):
    """The raw C ABI on device tensors; the outputs are poisoned first and an output not asked for is handed over as NULL.
    Returns (status, out, gX buffer, gY buffer) as numpy arrays."""
    import torch
    m, c = X.shape
    out, gX, gY = (torch.full(s, POISON, device=DEV) for s in ((1,), (m, c), (m, c)))
    rc = pkg._lib.lib.mcgra_mutual_information(E._stream(), m, c, E._p(X), E._p(Y), E._p(out), E._p(gX if want_x else None),
                                               E._p(gY if want_y else None))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), gX.cpu().numpy(), gY.cpu().numpy()


@pytest.mark.parametrize("kind,m,c", T.MI_CASES)
def test_mutual_information_within_the_float32_bound(E, kind, m, c):
    """mcgra_mutual_information (k_kde_stats, k_kde_tables, k_kde_grad of csrc/kde_kernels.hip) at every form it has: 8, 16 and
    32 columns from both sides of each switch; one block of k_kde_stats' 64 rows and of k_kde_grad's 128, with and without a
    ragged tail, up to the 79 partials k_kde_tables sums at m = 5000; c = 32 against c = 33, where a square operand is cut at
    the reach of its values (6, 7, 25 and 32 columns).
    The value: a kernel value k = expf(-0.5f (t t)), t = (v - b) / 0.32f, carries relative to k, on its exponent z = -0.5 t^2,
    6 u |z| from t (the subtraction u, the division 2 u, doubled by the square), u |z| from the square's rounding and
    0.75 u |z| for 0.32f against the reference's 0.32, and 2 u for expf: (8 |z| + 2) u.  Everything after the kernel values is
    double, so the bound is SAFETY sum (|dV/dk1| e_k1 + |dV/dk2| e_k2) + u |V| with dV/dk from the truth's own backward
    (ops_truth.mutual_information_bound).  The gradients: within 3e-6 of that operand's largest float64 gradient magnitude,
    the figure tests/test_gpu_parity.py holds this op to; tests/test_ops_cases_cpu.py shows that a correct float32 evaluation
    uses at most a third of it at every case, and that every defect it knows moves a case by ten."""
    Xn, Yn = T.mi_case(kind, m, c)
    X, Y = dev(Xn), dev(Yn)
    v, gx, gy, bound = T.mi_truth(kind, m, c)
    val, GX, GY = mi_twice(E, X, Y)
    assert val.shape == () and GX.shape == GY.shape == (m, c)
    assert twice(lambda: E.mutual_information(X, Y)).tobytes() == val.tobytes()
    within("mutual_information", (kind, m, c), val, v, bound)
    for nm, G, g in (("gX", GX, gx), ("gY", GY, gy)):
        tol = T.KDE_GRAD_TOL * np.abs(g).max()
        err = np.abs(G.astype(np.float64) - g).max()
        print(f"[ops] mutual_information({nm}) {(kind, m, c)}: max |error| / bound = {err / tol:.4f} (max |error| {err:.3e})")
        assert np.isfinite(G).all() and err <= tol, (kind, m, c, nm, err / tol)
    if c > T.KDE_MAXC:
        act = T.MI_REACH[(kind, m, c)]
        for G in (GX, GY):
            assert not G[:, act:].any() and G[:, :act].any()


@pytest.mark.parametrize("kind,m,c", T.MI_RAW_CASES)
def test_mutual_information_with_a_gradient_output_absent(pkg, E, kind, m, c):
    """The attack engine never asks for both gradients.  gX = NULL, gY = NULL and both: the value and the gradient that is
    asked for are the bits of the call with both, and a buffer not handed over keeps its poison."""
    X, Y = (dev(a) for a in T.mi_case(kind, m, c))
    rc, val, GX, GY = mi_raw(pkg, E, X, Y, True, True)
    assert rc == 0 and val[0] != POISON and not (GX == POISON).any() and not (GY == POISON).any()
    w = [t.cpu().numpy() for t in E.mutual_information(X, Y, want_grad=True)]
    assert val[0].tobytes() == w[0].tobytes() and GX.tobytes() == w[1].tobytes() and GY.tobytes() == w[2].tobytes()
    for want_x, want_y in ((False, True), (True, False), (False, False)):
        rc, v1, g1x, g1y = mi_raw(pkg, E, X, Y, want_x, want_y)
        assert rc == 0 and v1.tobytes() == val.tobytes(), (want_x, want_y)
        assert g1x.tobytes() == GX.tobytes() if want_x else (g1x == POISON).all(), (want_x, want_y)
        assert g1y.tobytes() == GY.tobytes() if want_y else (g1y == POISON).all(), (want_x, want_y)


def test_mutual_information_refusals_write_nothing(pkg, E):
    """A wide square operand whose values reach 33 columns (one entry raised from 27.0, the last accepted, to 27.5) is
    MCGRA_ENOSUP and the message names the value and the reach; a wide operand that is not square is MCGRA_ENOSUP; one with an
    infinite entry is MCGRA_EINVAL by name (floorf of an infinite maximum has no int: the op used to return 0 / 0 with status
    0).  None of them writes to out, gX or gY."""
    import torch
    L = pkg._lib.lib
    untouched = lambda r: all((a == POISON).all() for a in r[1:])
    X, Y = (dev(a) for a in T.mi_refused_case())
    r = mi_raw(pkg, E, X, Y, True, True)
    msg = L.mcgra_last_error()
    assert r[0] == ENOSUP and b"27.5" in msg and b"33" in msg and untouched(r), (r[0], msg)
    with pytest.raises(pkg._lib.McgraNotSupported, match="27.5"):
        E.mutual_information(X, Y, want_grad=True)
    r = mi_raw(pkg, E, X[:40, :33].contiguous(), Y[:40, :33].contiguous(), True, True)
    assert r[0] == ENOSUP and b"square" in L.mcgra_last_error() and untouched(r)
    Xn, Yn = T.mi_case("nxn1", 33, 33)
    for which, bad in ((0, np.inf), (1, -np.inf), (1, np.inf)):
        ops = [Xn.copy(), Yn.copy()]
        ops[which][7, 31] = bad
        r = mi_raw(pkg, E, dev(ops[0]), dev(ops[1]), True, True)
        msg = L.mcgra_last_error()
        assert r[0] == EINVAL and b"mutual_information" in msg and b"finite" in msg and untouched(r), (which, bad, r[0], msg)
    with pytest.raises(pkg._lib.McgraError, match="mutual_information"):
        E.mutual_information(dev(ops[0]), dev(ops[1]))
    assert torch.isfinite(E.mutual_information(dev(Xn), dev(Yn)))          # and the op goes on working afterwards


# --------------------------------------------------------------------------------------------------- wrappers' operands
def variants(t):
    """The same values as t in forms the C ABI cannot read: float64, non-contiguous, with autograd history."""
    import torch
    if t.dim() == 2:
        strided = t.t().contiguous().t()
    else:
        strided = torch.stack([t, t], 1)[:, 0]
    assert not strided.is_contiguous() or t.numel() <= 1 or 1 in t.shape
    return [t.double(), strided, t.clone().requires_grad_()]


def test_converting_wrappers_take_any_float_tensor(E, HS):
    """Every value-returning and dense-matrix wrapper hands the C ABI float32 contiguous data whatever it is given: a float64
    copy, a non-contiguous view and a requires_grad tensor return the bits of the plain operand."""
    X, Y = dev(T.linear_hsic_case(257, 16, 7)[0]), dev(T.linear_hsic_case(257, 16, 7)[1])
    A, P, Z = dev(T.norm_case(257)), dev(T.ie_case(257)), dev(T.decode_case(257, 7))
    an, orin = T.adj_case(257)
    a, ori = dev(an), dev(orin)
    MX, MY = (dev(t) for t in T.mi_case("emb", 129, 17))
    ops = {
        "mutual_information": (lambda X_, Y_: E.mutual_information(X_, Y_), [MX, MY]),
        "mutual_information(value)": (lambda X_, Y_: E.mutual_information(X_, Y_, want_grad=True)[0], [MX, MY]),
        "mutual_information(gX)": (lambda X_, Y_: E.mutual_information(X_, Y_, want_grad=True)[1], [MX, MY]),
        "mutual_information(gY)": (lambda X_, Y_: E.mutual_information(X_, Y_, want_grad=True)[2], [MX, MY]),
        "normalize_adj_tensor": (lambda A_: E.normalize_adj_tensor(A_), [A]),
        "get_modified_adj": (lambda a_, o_: E.get_modified_adj(a_, o_, 257), [a, ori]),
        "pack_tril": (lambda o_: E.pack_tril(o_), [ori]),
        "info_entropy": (lambda P_: E.info_entropy(P_), [P]),
        "dot_product_decode": (lambda Z_: E.dot_product_decode(Z_), [Z]),
        "dot_product_decode2": (lambda Z_: E.dot_product_decode2(Z_, 5), [Z]),
        "linear_hsic": (lambda X_, Y_: E.linear_hsic(X_, Y_), [X, Y]),
        "hsic_regular": (lambda X_, Y_: E.hsic_regular(X_, Y_, 1.0), [X, Y]),
        "hsic_normalized": (lambda X_, Y_: E.hsic_normalized(X_, Y_, 1.0), [X, Y]),
        "hsic_regular2": (lambda X_, Y_: E.hsic_regular2(X_, Y_, 1.0, 1.5), [X, Y]),
        "mmd": (lambda X_, Y_: E.mmd(X_, Y_, 1.0, 1.5, 2.0), [X, (X[:100] * 0.9 + 0.1).contiguous()]),
        "mmd_pxpy_pxy": (lambda X_, Y_: E.mmd_pxpy_pxy(X_, Y_, 1.0, 1.5), [X, Y]),
        "mse": (lambda X_, Y_: E.mse(X_, Y_), [X, X * 0.5]),
        "hsic.distmat": (lambda X_: HS.distmat(X_), [X]),
        "hsic.hsic_regular": (lambda X_, Y_: HS.hsic_regular(X_, Y_, 2.0), [X, Y]),
    }
    for name, (fn, operands) in ops.items():
        plain = fn(*operands).detach().cpu().numpy()
        forms = [variants(t) for t in operands]
        for k in range(3):
            got = fn(*[f[k] for f in forms])
            assert got.dtype.is_floating_point and not got.requires_grad
            assert got.detach().cpu().numpy().tobytes() == plain.tobytes(), (name, k)
        mixed = fn(*[f[i % 3] for i, f in enumerate(forms)])
        assert mixed.detach().cpu().numpy().tobytes() == plain.tobytes(), (name, "mixed")
    import torch
    for form in zip(variants(MX), variants(MY)):          # the gradients: float32 of the operands' shape, whatever the operands are
        for t in E.mutual_information(*form, want_grad=True):
            assert t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.grad_fn is None
            assert t.shape in ((), MX.shape)
    c = T.gcn_case("n300_l3")
    X, adj, W, b, Wlin, blin = (dev(c[0]), dev(c[1]), [dev(w) for w in c[2]], [dev(x) for x in c[3]], dev(c[4]), dev(c[5]))
    lp, emb = E.gcn_forward(X, adj, W, b, Wlin, blin, emb_nlayer=2)
    for k in range(3):
        v = lambda t: variants(t)[k]
        lp2, emb2 = E.gcn_forward(v(X), v(adj), [v(w) for w in W], [v(x) for x in b], v(Wlin), v(blin), emb_nlayer=2)
        assert lp2.cpu().numpy().tobytes() == lp.cpu().numpy().tobytes() and emb2.cpu().numpy().tobytes() == emb.cpu().numpy().tobytes(), k


def test_gemm_family_refuses_and_keeps_out_aliasing(E):
    """On device tensors: float64 or a transposed view is a ValueError (nothing is converted), and a padded leading dimension
    still writes into the caller's own `out`."""
    import torch
    A = torch.randn(40, 24, device=DEV)
    B = torch.randn(24, 36, device=DEV)
    for bad in ((A.double(), B), (A, B.double()), (A.t().contiguous().t(), B), (A, B.t().contiguous().t())):
        with pytest.raises(ValueError, match="sgemm"):
            E.sgemm(*bad)
    buf = torch.zeros(40, 64, device=DEV)
    out = buf[:, :36]
    ret = E.sgemm(A, B, out=out)
    assert ret.data_ptr() == buf.data_ptr()
    ref = A.double().cpu().numpy() @ B.double().cpu().numpy()
    bound = 4e-7 * (np.abs(A.cpu().numpy()).astype(np.float64) @ np.abs(B.cpu().numpy()).astype(np.float64))
    assert (np.abs(buf[:, :36].cpu().numpy() - ref) <= bound).all() and not buf[:, 36:].any()


def test_a_host_operand_beside_a_device_one_is_refused(E, HS):
    """The first operand names the device; a second one left on the host is a ValueError too where its pointer would be handed
    on, and is moved where the wrapper always moved it (the ranking metrics' scores and node ids)."""
    import torch
    X = dev(T.linear_hsic_case(257, 16, 7)[0])
    host = X.cpu()
    for name, call in {"mse": lambda: E.mse(X, host), "linear_hsic": lambda: E.linear_hsic(X, host), "sgemm": lambda: E.sgemm(X, host, tb=True),
                       "hsic_regular": lambda: E.hsic_regular(X, host, 1.0), "mmd": lambda: HS.mmd(X, host, 1.0),
                       "mutual_information": lambda: E.mutual_information(X, host, want_grad=True),
                       "get_modified_adj": lambda: E.get_modified_adj(X[0], torch.zeros(6, 6), 6),
                       "gcn_forward": lambda: E.gcn_forward(X, X, [host], [host[0]], host, host[0])}.items():
        with pytest.raises(ValueError, match=name):
            call()
    real = (torch.rand(40, 40, device=DEV) < 0.2).float()
    pred = torch.rand(40, 40, device=DEV)
    idx = torch.arange(0, 40, 2)
    assert E.roc_auc(real, pred.cpu(), idx) == E.roc_auc(real, pred, idx.to(DEV)) == E.roc_auc(real, pred, idx.tolist())
