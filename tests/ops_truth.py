"""Float64 truths of the standalone ops of include/mcgra.h, their a-priori float32 error bounds, and the inputs of
tests/test_gpu_ops.py.

One plain numpy function per op, float64 throughout, written from the reference's formulas (the line numbers are the ones
include/mcgra.h cites).  Nothing here imports the oracle: its versions round to float32 on the way.

Beside each truth stands ``<op>_bound``: what the float32 evaluation of the kernels in csrc/capi.hip may be off by, computed
in float64 from the same inputs.  Every bound is the first-order sum of the rounding steps the kernel takes (spelled out in
its docstring), times SAFETY.  u = 2^-24 is the unit roundoff of float32; an operation "within 1 ulp" is charged 2 u.
Reductions run in double on the device and add nothing at this level.  The bounds are not fitted to any GPU result.

A truth takes ``defect=``: the value a kernel with that defect would return, in float64 (tests/test_ops_cases_cpu.py
requires every case to sit at least 10 bounds away from each defect that applies to it).  The generic defects:
  lastcol   the last column dropped from the row reduction
  lastrow   the last row dropped from the final reduction
  tail256   everything past the last whole 256 columns of a row dropped
  past1024  everything past the first 1024 rows dropped from the final reduction
the others are named where they apply.

mutual_information (measure KDE's arithmetic, csrc/kde_kernels.hip) returns gradients too and stands at the end of the file
with its own defects, a float32 emulation of its kernel values and its own cases; its bins alone come from torch.linspace,
as the reference's do.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
GEMM = 4e-7               # |sgemm - exact| <= GEMM * sum_k |a_ik| |b_kj| (tests/test_gpu_parity.py::test_sgemm_matches_fp64)
SAFETY = 2.0              # over the first-order sum of the rounding steps
POW_ULPS = 2.0            # powf(x, p) is charged POW_ULPS * max(p, 1) ulps
F32_EPS12 = float(np.float32(1e-12))      # F.normalize's eps as the float32 the kernels hold
IE_LO, IE_HI = float(np.float32(1e-4)), float(np.float32(1 - 1e-4))      # torch.clamp's bounds on a float32 tensor


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _sig(s):
    """sigma as the float the C ABI receives."""
    return float(np.float32(s))


def _masks(nrow, ncol, defect):
    rows, cols = np.ones(nrow, bool), np.ones(ncol, bool)
    if defect == "lastcol":
        cols[-1] = False
    elif defect == "lastrow":
        rows[-1] = False
    elif defect == "tail256":
        cols[256 * (ncol // 256):] = False
    elif defect == "past1024":
        rows[1024:] = False
    return rows, cols


def _rsum(T, defect=None):
    """sum of T as one row reduction per row and a final reduction over the rows, with a generic defect."""
    if defect not in ("lastcol", "lastrow", "tail256", "past1024"):
        return T.sum()
    rows, cols = _masks(T.shape[0], T.shape[1], defect)
    return T[rows][:, cols].sum()


# ------------------------------------------------------------------------------------------------ hsic.py: distances
def _dist(X, Y, ynorm_from_x=False, sqnorm_lastcol=False):
    """distmat (hsic.py:20-27), and its cross block (hsic.py:83-84): r_i - 2 <x_i, y_j> + q_j."""
    X, Y = _f64(X), _f64(Y)
    sq = (lambda V: (V[:, :-1] ** 2).sum(1)) if sqnorm_lastcol else (lambda V: (V * V).sum(1))
    r, q = sq(X), sq(Y)
    if ynorm_from_x:
        q = r[np.arange(len(Y)) % len(X)]
    return r[:, None] - 2.0 * (X @ Y.T) + q[None, :]


def _dist_err(X, Y):
    """First-order error of one distance entry.  k_row_sqnorm: d products and d - 1 additions in float, (d) u r_i; the Gram
    entry from sgemm: d products accumulated in float, d u sum_k |x_ik y_jk|; 2 a is exact; (r_i + q_j) - 2 a: two more
    roundings on at most r_i + q_j + 2 |a|.  Together (d + 3) u (r_i + q_j + 2 sum_k |x_ik y_jk|)."""
    X, Y = _f64(X), _f64(Y)
    r, q = (X * X).sum(1), (Y * Y).sum(1)
    return (X.shape[1] + 3) * U * (r[:, None] + q[None, :] + 2.0 * (np.abs(X) @ np.abs(Y).T))


def distmat(X, defect=None):
    """hsic.distmat (hsic.py:20-27).  defect 'sqnorm_lastcol': the last feature left out of |x_i|^2."""
    return _dist(X, X, sqnorm_lastcol=defect == "sqnorm_lastcol")


def distmat_bound(X):
    """SAFETY x _dist_err, elementwise (on the diagonal the truth is 0 and the bound 4 (d + 3) u r_i)."""
    return SAFETY * _dist_err(X, X)


def _gauss(X, Y, sigma, scale, **kw):
    """exp(-D / (scale sigma^2)): scale 2 within an operand (hsic.py:37, :73), 1 for mmd's cross block (:85)."""
    s = _sig(sigma)
    return np.exp(-_dist(X, Y, **kw) / (scale * s * s))


def _gauss_err(X, Y, sigma, scale):
    """(K, first-order error of a stored kernel entry).  The coefficient 1.f / (scale sigma sigma) carries two roundings and
    the product with the distance one more: 3 u |t| on the exponent t, beside the distance's own error times the
    coefficient; expf is within 1 ulp and its result is what is stored: 2 u K.
    E_K = K (E_D c + 3 u |t|) + 2 u K."""
    s = _sig(sigma)
    c = 1.0 / (scale * s * s)
    D = _dist(X, Y)
    K = np.exp(-D * c)
    return K, K * (_dist_err(X, Y) * c + 3 * U * np.abs(D) * c) + 2 * U * K


def sigma_estimation(X, Y):
    """hsic.sigma_estimation (hsic.py:5-17): the median squared distance within cat([X, Y]) (strict lower triangle)."""
    V = np.concatenate([_f64(X), _f64(Y)])
    tri = _dist(V, V)[np.tril_indices(len(V), -1)]
    med = np.median(tri)
    if med <= 0:
        med = np.mean(tri)
    return max(float(med), 1e-2)


def distcorr(X, sigma=1.0, defect=None):
    """hsic.distcorr (hsic.py:50-53): mean(exp(-distmat(X) / (2 sigma^2)))."""
    K = _gauss(X, X, sigma, 2.0)
    return _rsum(K, defect) / K.size


def distcorr_bound(X, sigma=1.0):
    """mean of the kernel entries' errors (the mean itself is a double reduction); the host mirror takes the value as
    mmd(X, one far point) + 1: one float rounding of mean - 1 and one of the sum."""
    K, E = _gauss_err(X, X, sigma, 2.0)
    a = K.mean()
    return SAFETY * E.mean() + U * abs(a - 1.0) + U * abs(a)


# ------------------------------------------------------------------------------------------ hsic.py: HSIC and the MMDs
def _hsic(x, y, sx, sy, defect=None):
    Kx, Ky = _gauss(x, x, sx, 2.0), _gauss(y, y, sy, 2.0)
    Kxc = Kx - Kx.mean(1)[:, None]              # Kx H (hsic.py:46): row i minus its mean
    Kyc = Ky - Ky.mean(1)[:, None]
    T = Kxc * (Kyc if defect == "ymean_by_row" else Kyc.T)
    return _rsum(T, defect) / T.size


def _hsic_err(x, y, sx, sy):
    """First-order error of mean(Kxc o Kyc^T) as k_hsic_gauss_rows forms it: each factor is the float difference of a stored
    kernel entry (E_K) and a row mean cast to float (the mean of that row's E_K, and u |mean| for the cast), one rounding
    u |K - mean| for the difference; the product and both reductions are double."""
    Kx, Ex = _gauss_err(x, x, sx, 2.0)
    Ky, Ey = _gauss_err(y, y, sy, 2.0)
    mx, my = Kx.mean(1), Ky.mean(1)
    cx, cy = Kx - mx[:, None], Ky - my[None, :]
    ecx = Ex + Ex.mean(1)[:, None] + U * np.abs(mx)[:, None] + U * np.abs(cx)
    ecy = Ey + Ey.mean(1)[None, :] + U * np.abs(my)[None, :] + U * np.abs(cy)
    return (np.abs(cy) * ecx + np.abs(cx) * ecy).mean()


def hsic_regular(x, y, sigma, sigma_y=None, defect=None):
    """hsic.hsic_regular (hsic.py:117-124) with one sigma, or one per operand (kernelmat :39-41).
    defect 'ymean_by_row': y's row mean indexed by the row instead of the column."""
    return _hsic(x, y, sigma, sigma if sigma_y is None else sigma_y, defect)


def hsic_regular_bound(x, y, sigma, sigma_y=None):
    """SAFETY x _hsic_err + u |value| (the returned float)."""
    sy = sigma if sigma_y is None else sigma_y
    return SAFETY * _hsic_err(x, y, sigma, sy) + U * abs(_hsic(x, y, sigma, sy))


def hsic_normalized(x, y, sigma, sigma_y=None, defect=None):
    """hsic.hsic_normalized (hsic.py:127-135): Pxy / (sqrt(Pxx) sqrt(Pyy)); 0 / 0 = nan at m = 1, as the reference."""
    sy = sigma if sigma_y is None else sigma_y
    with np.errstate(invalid="ignore", divide="ignore"):
        return _hsic(x, y, sigma, sy, defect) / (np.sqrt(_hsic(x, x, sigma, sigma, defect)) * np.sqrt(_hsic(y, y, sy, sy, defect)))


def hsic_normalized_bound(x, y, sigma, sigma_y=None):
    """The three means carry _hsic_err each; the quotient and the square roots are double on the host:
    E_xy / (sqrt(Pxx) sqrt(Pyy)) + |v| (E_xx / (2 Pxx) + E_yy / (2 Pyy)), times SAFETY, + u |v|."""
    sy = sigma if sigma_y is None else sigma_y
    pxy, pxx, pyy = _hsic(x, y, sigma, sy), _hsic(x, x, sigma, sigma), _hsic(y, y, sy, sy)
    v = pxy / math.sqrt(pxx * pyy)
    e = _hsic_err(x, y, sigma, sy) / math.sqrt(pxx * pyy) + abs(v) * (_hsic_err(x, x, sigma, sigma) / (2 * pxx)
                                                                       + _hsic_err(y, y, sy, sy) / (2 * pyy))
    return SAFETY * e + U * abs(v)


def mmd(x, y, sx, sy, sxy, defect=None):
    """hsic.mmd (hsic.py:68-89): mean(Kx) + mean(Ky) - 2 mean(Kxy), Kxy = exp(-Dxy / sxy^2) over mx x my.
    The generic defects act on the cross term; 'cross_mxmx': the cross term normalised by mx mx; 'ynorm_from_x': y's squared
    norms taken from x's vector."""
    Kxy = _gauss(x, y, sxy, 1.0, ynorm_from_x=defect == "ynorm_from_x")
    c = _rsum(Kxy, defect) / (len(x) * len(x) if defect == "cross_mxmx" else Kxy.size)
    return _gauss(x, x, sx, 2.0).mean() + _gauss(y, y, sy, 2.0).mean() - 2.0 * c


def mmd_bound(x, y, sx, sy, sxy):
    """The three means of stored kernel entries (mean E_K each, the cross one twice), times SAFETY, + u |value|."""
    e = _gauss_err(x, x, sx, 2.0)[1].mean() + _gauss_err(y, y, sy, 2.0)[1].mean() + 2.0 * _gauss_err(x, y, sxy, 1.0)[1].mean()
    return SAFETY * e + U * abs(mmd(x, y, sx, sy, sxy))


def mmd_pxpy_pxy(x, y, sx, sy, defect=None):
    """hsic.mmd_pxpy_pxy (hsic.py:92-114): mean(Kx o Ky) - 2 mean(colmean(Kx) o colmean(Ky)) + mean(Kx) mean(Ky).
    The generic defects act on the first term; 'no_extra_1_over_m': the middle term summed, not averaged, over the columns."""
    Kx, Ky = _gauss(x, x, sx, 2.0), _gauss(y, y, sy, 2.0)
    A = _rsum(Kx * Ky, defect) / Kx.size
    B = (Kx.mean(0) * Ky.mean(0)).sum() if defect == "no_extra_1_over_m" else (Kx.mean(0) * Ky.mean(0)).mean()
    return A - 2.0 * B + Kx.mean() * Ky.mean()


def mmd_pxpy_pxy_bound(x, y, sx, sy):
    """Products and means are double on stored kernel entries: E_A = mean(Ky E_x + Kx E_y), E_B = mean_j(my_j mean_i E_x +
    mx_j mean_i E_y), E_C = mean(Ky) mean(E_x) + mean(Kx) mean(E_y); SAFETY (E_A + 2 E_B + E_C) + u |value|."""
    Kx, Ex = _gauss_err(x, x, sx, 2.0)
    Ky, Ey = _gauss_err(y, y, sy, 2.0)
    ea = (Ky * Ex + Kx * Ey).mean()
    eb = (Ky.mean(0) * Ex.mean(0) + Kx.mean(0) * Ey.mean(0)).mean()
    ec = Ky.mean() * Ex.mean() + Kx.mean() * Ey.mean()
    return SAFETY * (ea + 2.0 * eb + ec) + U * abs(mmd_pxpy_pxy(x, y, sx, sy))


# ----------------------------------------------------------------------------------------------------- utils.CudaCKA
def _center(K):
    """CudaCKA.centering (utils.py:1060-1065): H K H = K - row means - column means + the mean."""
    return K - K.mean(1)[:, None] - K.mean(0)[None, :] + K.mean()


def linear_hsic(X, Y, defect=None):
    """CudaCKA.linear_HSIC (utils.py:1080-1084): sum(center(X X^T) o center(Y Y^T)).  A defect is stated on the form the
    kernel evaluates, |Xc^T Yc|_F^2 with column-centred operands: 'lastrow' / 'tail256' / 'past1024' drop rows of the sum
    over m, 'lastcol' the last column of the dx x dy product."""
    X, Y = _f64(X), _f64(Y)
    if defect is None:
        return (_center(X @ X.T) * _center(Y @ Y.T)).sum()
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    keep = np.ones(len(X), bool)
    if defect == "lastrow":
        keep[-1] = False
    elif defect == "tail256":
        keep[256 * (len(X) // 256):] = False
    elif defect == "past1024":
        keep[1024:] = False
    Q = Xc[keep].T @ Yc[keep]
    return ((Q[:, :-1] if defect == "lastcol" else Q) ** 2).sum()


def linear_hsic_bound(X, Y):
    """k_colmean_center_col: the column mean is a double sum cast to float (u |mu|), the centred entry one float
    subtraction (u |x - mu|).  Q = Xc^T Yc on sgemm: GEMM sum_i |xc_ia| |yc_ib| plus the operands' errors carried through;
    the sum of squares is double: sum 2 |Q| E_Q.  Times SAFETY, + u |value|."""
    X, Y = _f64(X), _f64(Y)
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    ex = U * np.abs(X.mean(0))[None, :] + U * np.abs(Xc)
    ey = U * np.abs(Y.mean(0))[None, :] + U * np.abs(Yc)
    Q = Xc.T @ Yc
    EQ = GEMM * (np.abs(Xc).T @ np.abs(Yc)) + ex.T @ np.abs(Yc) + np.abs(Xc).T @ ey
    return SAFETY * (2.0 * np.abs(Q) * EQ).sum() + U * (Q * Q).sum()


# ------------------------------------------------------------------------------------------------ topology_attack.py
def info_entropy(P, defect=None):
    """Info_entropy (topology_attack.py:44-47): -mean(q log2 q), q = clamp(p, 1e-4, 1 - 1e-4) (float32 bounds).
    'no_lo' / 'no_hi': that clamp missing (without the lower one an entry <= 0 is counted as 0, the most forgiving reading:
    a nan or -inf would only show more)."""
    P = _f64(P)
    q = P if defect == "no_lo" else np.maximum(P, IE_LO)
    q = q if defect == "no_hi" else np.minimum(q, IE_HI)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(q > 0, q * np.log2(np.where(q > 0, q, 1.0)), 0.0)
    return -_rsum(t, defect) / t.size


def info_entropy_bound(P):
    """ie_term: the clamp is exact; log2 within 1 ulp (2 u |l|) and one rounding of q l: 3 u |q log2 q| a term; double
    reductions.  SAFETY 3 u mean|q log2 q| + u |value|."""
    q = np.clip(_f64(P), IE_LO, IE_HI)
    t = q * np.log2(q)
    return SAFETY * 3 * U * np.abs(t).mean() + U * abs(t.mean())


def mse(X, Y, defect=None):
    """torch.nn.MSELoss()(X, Y).  'lastcol': the last element dropped; 'past_grid': everything past 1024 x 256 elements."""
    e = (_f64(X) - _f64(Y)).reshape(-1)
    n = e.size
    if defect == "lastcol":
        e = e[:-1]
    elif defect == "past_grid":
        e = e[:1024 * 256]
    return (e * e).sum() / n


def mse_bound(X, Y):
    """k_sqdiff_part: e = x - y is one float rounding (u |e|), its square and the sums are double: 2 u e^2 a term.
    SAFETY 2 u value + u value."""
    return (SAFETY * 2 + 1) * U * mse(X, Y)


def normalize_adj(A, defect=None):
    """utils.normalize_adj_tensor, dense branch (utils.py:223-229): D^-1/2 (A + I) D^-1/2, D = rowsum(A + I), inf -> 0.
    'lastcol' / 'tail256' act on the row sum."""
    A = _f64(A)
    n = len(A)
    mx = A + np.eye(n)
    cols = _masks(n, n, defect if defect in ("lastcol", "tail256") else None)[1]
    d = mx[:, cols].sum(1)
    with np.errstate(divide="ignore"):
        r = d ** -0.5
    r[np.isinf(r)] = 0.0
    return r[:, None] * mx * r[None, :]


def normalize_adj_bound(A):
    """k_prep sums a row in float: a thread adds its 4 ceil(n / 1024) entries in turn, the block adds 256 threads in a tree
    of 6 + 4 steps, + 1 for the identity: E_d = (4 ceil(n / 1024) + 11) u (sum_j |a_ij| + 1).  r = 1 / sqrtf(d): the root
    and the quotient within 1 ulp each, E_d / (2 d) + 4 u relative; (r_i (a + I)_ij) r_j: two roundings, one more for a + 1
    on the diagonal.  Relative error of an entry: E_di / (2 d_i) + E_dj / (2 d_j) + 11 u; times SAFETY."""
    A = _f64(A)
    n = len(A)
    d = (A + np.eye(n)).sum(1)
    ed = (4 * math.ceil(n / 1024) + 11) * U * (np.abs(A).sum(1) + 1.0)
    rho = np.divide(ed, np.abs(d), out=np.zeros(n), where=d != 0)
    return SAFETY * np.abs(normalize_adj(A)) * (0.5 * rho[:, None] + 0.5 * rho[None, :] + 11 * U)


def tril_indices(n):
    """torch.tril_indices(n, n, -1): row-major over the strict lower triangle."""
    return np.tril_indices(n, -1)


def get_modified_adj(a, ori, n):
    """PGDAttack.get_modified_adj (topology_attack.py:365-379); the dtype of `a` is kept (data movement and one addition)."""
    m = np.zeros((n, n), dtype=np.asarray(a).dtype)
    m[tril_indices(n)] = a
    m = m + m.T
    out = (1 - np.eye(n, dtype=m.dtype)) * m
    return out if ori is None else out + ori


def pack_tril(M):
    """M[tril_indices]: the inverse data movement (mcgra_pack_tril)."""
    return np.asarray(M)[tril_indices(len(M))]


def _normalize_rows(Z, p=2, lastcol=False):
    """F.normalize(Z, p, dim=1): z / max(|z|_p, 1e-12)."""
    V = np.abs(Z[:, :-1] if lastcol else Z)
    nrm = (V ** p).sum(1) ** (1.0 / p)
    return Z / np.maximum(nrm, F32_EPS12)[:, None]


def _normalize_err(Z, p=2):
    """Relative error of a row of F.normalize as k_row_normalize forms it (one thread per row, k ascending).
    p = 2: d products and d - 1 additions, (d + 1) u on the sum, half of it through sqrtf (1 ulp), the quotient 1 ulp:
    ((d + 1) / 2 + 4) u.
    p = 3, 5: every term is powf(|z|, p), POW_ULPS p ulps, d - 1 additions: e_s = 2 POW_ULPS p u + (d - 1) u on the sum
    s; the root powf(s, 1.f / p) sees e_s / p, the rounding of its exponent u |ln s| / p and POW_ULPS ulps of its own; the
    quotient 1 ulp."""
    d = Z.shape[1]
    if p == 2:
        return np.full(len(Z), ((d + 1) / 2 + 4) * U)
    s = (np.abs(Z) ** p).sum(1)
    with np.errstate(divide="ignore"):
        ln = np.where(s > 0, np.abs(np.log(np.where(s > 0, s, 1.0))), 0.0)
    return (2 * POW_ULPS * p * U + (d - 1) * U) / p + U * ln / p + 2 * POW_ULPS * U + 2 * U


def dot_product_decode(Z, defect=None):
    """PGDAttack.dot_product_decode (topology_attack.py:414-419): relu(Zn Zn^T) on the strict lower triangle, packed.
    'no_relu'; 'lastcol': the last column left out of the row norm."""
    Zn = _normalize_rows(_f64(Z), 2, defect == "lastcol")
    S = Zn @ Zn.T
    return pack_tril(S if defect == "no_relu" else np.maximum(S, 0.0))


def dot_product_decode_bound(Z):
    """Zn Zn^T on sgemm, GEMM sum_k |zn_ik| |zn_jk|, and both rows' normalisation errors on the same sum; relu is
    1-Lipschitz.  SAFETY (GEMM + e_i + e_j) sum_k |zn_ik zn_jk|."""
    Z = _f64(Z)
    Zn, e = np.abs(_normalize_rows(Z)), _normalize_err(Z)
    return pack_tril(SAFETY * (GEMM + e[:, None] + e[None, :]) * (Zn @ Zn.T))


def _dd2_p(mode):
    return {5: 3, 6: 5}.get(mode, 2)


def dot_product_decode2(Z, mode, defect=None):
    """PGDAttack.dot_product_decode2 (topology_attack.py:421-467), `mode` as include/mcgra.h numbers its branches.
    'p2': p = 2 where the mode says 3 or 5; 'no_eye': the identity not subtracted; 'lastcol' / 'tail256': on the row norm of
    Z Z^T (mode 3)."""
    Z = _f64(Z)
    n = len(Z)
    if mode in (1, 4, 5, 6):
        Z = _normalize_rows(Z, 2 if defect == "p2" else _dd2_p(mode))
    S = Z @ Z.T
    if mode == 3:
        cols = _masks(n, n, defect if defect in ("lastcol", "tail256") else None)[1]
        S = S / np.maximum(np.sqrt((S[:, cols] ** 2).sum(1)), F32_EPS12)[:, None]
    R = np.maximum(S - (0.0 if defect == "no_eye" else np.eye(n)), 0.0)
    return 1.0 / (1.0 + np.exp(-R)) if mode in (0, 1) else R


def dot_product_decode2_bound(Z, mode):
    """S = Zs Zs^T on sgemm: E_S = (GEMM + e_i + e_j) sum_k |zs_ik zs_jk| (e = 0 where Z is taken as given).
    mode 3: the row norm is a double sum of squares cast to float, relative sum_j |S_ij| E_ij / |S_i|^2 + u; its reciprocal
    (1 ulp) and the product: E = E_S / |S_i| + |S_ij| / |S_i| (that + 3 u).
    s - 1 on the diagonal: u |s - 1|.  relu: 1-Lipschitz.  modes 0, 1: sigmoid is 1/4-Lipschitz, and expf (1 ulp), 1 + e
    and the reciprocal (1 ulp) leave 5 u of its value.  Times SAFETY."""
    Z = _f64(Z)
    n = len(Z)
    e = np.zeros(n)
    if mode in (1, 4, 5, 6):
        e = _normalize_err(Z, _dd2_p(mode))
        Z = _normalize_rows(Z, _dd2_p(mode))
    S = Z @ Z.T
    E = (GEMM + e[:, None] + e[None, :]) * (np.abs(Z) @ np.abs(Z).T)
    if mode == 3:
        nr = np.sqrt((S * S).sum(1))
        den = np.maximum(nr, F32_EPS12)
        rho = np.divide((np.abs(S) * E).sum(1), nr * nr, out=np.zeros(n), where=nr > 0) + U
        S = S / den[:, None]
        E = E / den[:, None] + np.abs(S) * (rho + 3 * U)[:, None]
    E = E + U * np.abs(np.diag(np.diag(S) - 1.0))
    if mode in (0, 1):
        R = np.maximum(S - np.eye(n), 0.0)
        E = E / 4 + 5 * U / (1.0 + np.exp(-R))
    return SAFETY * E


def gcn_forward(X, adj, W, b, Wlin, blin, emb_nlayer=0, defect=None):
    """GCN.forward in eval mode (models/gcn.py:164-174) and embedding_GCN.forward (:71-76): (log-probabilities, embedding
    or None).  'lastrow' / 'tail256' / 'past1024': terms dropped from the sum over the n neighbours of adj @ support."""
    X, adj = _f64(X), _f64(adj)
    n = len(adj)
    keep = np.ones(n, bool)
    if defect == "lastrow":
        keep[-1] = False
    elif defect == "tail256":
        keep[256 * (n // 256):] = False
    elif defect == "past1024":
        keep[1024:] = False
    H, emb = X, None
    for l in range(len(W)):
        H = np.maximum(adj[:, keep] @ (H @ _f64(W[l]))[keep] + _f64(b[l])[None, :], 0.0)
        if l + 1 == emb_nlayer:
            emb = H
    Z = H @ _f64(Wlin).T + _f64(blin)[None, :]
    Z = Z - Z.max(1)[:, None]
    return Z - np.log(np.exp(Z).sum(1))[:, None], emb


def gcn_forward_bound(X, adj, W, b, Wlin, blin, emb_nlayer=0):
    """The sgemm constant carried layer by layer.  T_0 = X W_0: GEMM |X| |W_0|.  adj @ T: GEMM |adj| |T| + |adj| E_T; the bias
    one rounding, u |P|; relu 1-Lipschitz.  T_{l+1} = H W_{l+1} and the head H Wlin^T + blin are one fmaf chain over k
    terms: (k + 2) u (|H| |W| + |b|) + E_H |W|.  log_softmax: a shift of every logit moves logsumexp by at most the largest
    shift, so E_Z + max_k E_Z; its own arithmetic (z - max, expf 1 ulp, c additions, logf 1 ulp, two subtractions):
    u (2 max_k |z_k - max| + c + 4 + 2 |lse| + 2 |l|).  Returns (bound of the log-probabilities, of the embedding or None);
    times SAFETY."""
    X, adj = _f64(X), _f64(adj)
    aadj = np.abs(adj)
    T = X @ _f64(W[0])
    ET = GEMM * (np.abs(X) @ np.abs(_f64(W[0])))
    Eemb = None
    for l in range(len(W)):
        P = adj @ T + _f64(b[l])[None, :]
        EH = GEMM * (aadj @ np.abs(T)) + aadj @ ET + U * np.abs(P)
        H = np.maximum(P, 0.0)
        if l + 1 == emb_nlayer:
            Eemb = SAFETY * EH
        if l + 1 < len(W):
            Wn = _f64(W[l + 1])
            T = H @ Wn
            ET = (len(Wn) + 2) * U * (H @ np.abs(Wn)) + EH @ np.abs(Wn)
    Wl = _f64(Wlin).T
    Z = H @ Wl + _f64(blin)[None, :]
    EZ = (len(Wl) + 2) * U * (H @ np.abs(Wl) + np.abs(_f64(blin))[None, :]) + EH @ np.abs(Wl)
    c = Z.shape[1]
    zs = Z - Z.max(1)[:, None]
    lse = np.log(np.exp(zs).sum(1))
    lp = zs - lse[:, None]
    arith = U * (2 * np.abs(zs).max(1)[:, None] + c + 4 + 2 * np.abs(lse)[:, None] + 2 * np.abs(lp))
    return SAFETY * (EZ + EZ.max(1)[:, None] + arith), Eemb


# =========================================================================================================== the cases
# The inputs of tests/test_gpu_ops.py: float32 arrays from fixed seeds, built once a process.  The shapes are the smallest
# that cross each boundary of the kernels (a second turn of a 256-thread row loop with and without a ragged tail, a second
# block of 256 in x, k_reduce_rows' loop past 1024 row values, k_sqdiff_part's grid stride past 1024 x 256 elements,
# k_row_normalize's 32-row form from h = 192, sgemm's unaligned leading dimensions and its split-K).
GAUSS_M = (1, 2, 255, 256, 257, 300, 1030)
GAUSS_WIDTHS = ((7, 3), (1, 1), (33, 8))
GAUSS_SIGMAS = (1.0, 5.0)
MMD_SHAPES = ((300, 257), (257, 1030), (1030, 45), (1, 300))
MMD_D = (3, 6)
MMD_SIGMAS = (0.75, 1.5, 2.5)           # sx, sy, sxy
LINEAR_HSIC_SHAPES = ((257, 16, 7), (1030, 1, 1), (3000, 33, 7))
IE_N = (257, 300, 1030)
MSE_COUNTS = (1, 255, 257, 1024 * 256 - 1, 1024 * 256 + 3)
ADJ_N = (2, 255, 257, 300, 1030)
NORM_N = (257, 1030)
DECODE_SHAPES = ((257, 7), (300, 200), (1030, 16))
GCN_CASES = {            # name: (n, nfeat, layer widths, classes)
    "n300_l3": (300, 11, (24, 32, 8), 9),
    "n300_l1": (300, 11, (5,), 2),
    "n1030_l2": (1030, 11, (16, 16), 4),
}
GENERIC = ("lastcol", "lastrow", "tail256", "past1024")


def generic_defects(nrow, ncol=None):
    """The generic defects that drop anything at this shape."""
    ncol = nrow if ncol is None else ncol
    out = []
    if ncol > 1:
        out.append("lastcol")
    if nrow > 1:
        out.append("lastrow")
    if ncol % 256:
        out.append("tail256")
    if nrow > 1024:
        out.append("past1024")
    return out


def sigma_y_of(sigma):
    """The second operand's bandwidth of the hsic_regular2 cases (sigma_x != sigma_y)."""
    return 1.5 * sigma


@functools.lru_cache(maxsize=None)
def gauss_case(m, dx, dy, sigma):
    """Two clusters that x and y share, 7 points in 10 in the first, Gaussian scatter around each centre: within a cluster
    the squared distances are about sigma^2 / 2, between the clusters 4 sigma^2 more, in both spaces.  y depends on x through
    the cluster alone.  Every column of the centred product then carries about 1 / m of the value, so a dropped column
    shows (with one cloud of independent points the last column can carry next to nothing), and the row means of both
    kernel matrices differ between the clusters, so a row mean taken at the wrong index shows."""
    rng = np.random.RandomState(7000 + 13 * m + dx)
    side = np.where(np.arange(m) % 10 < 7, -1.0, 1.0)
    xs = 0.5 * rng.randn(m, dx) + side[:, None] * rng.choice([-1.0, 1.0], dx)[None, :]
    ys = 0.5 * rng.randn(m, dy) + side[:, None] * rng.choice([-1.0, 1.0], dy)[None, :]
    return (xs * (sigma / math.sqrt(dx))).astype(np.float32), (ys * (sigma / math.sqrt(dy))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mmd_case(mx, my, d):
    """Two clouds a shift apart; the LAST point of y lies on top of x's first (a random last point can carry almost exactly
    the mean of its row, and then a dropped last column would not show)."""
    rng = np.random.RandomState(8000 + mx + 3 * my + d)
    x = (rng.randn(mx, d) * 0.7).astype(np.float32)
    y = (rng.randn(my, d) * 0.9 + 0.5).astype(np.float32)
    y[-1] = x[0]
    return x, y


@functools.lru_cache(maxsize=None)
def linear_hsic_case(m, dx, dy):
    rng = np.random.RandomState(9000 + m + dx)
    X = (rng.randn(m, dx) + 0.3).astype(np.float32)
    mix = rng.randn(dx, dy) / math.sqrt(dx)
    Y = (X.astype(np.float64) @ mix + 0.5 * rng.randn(m, dy) - 0.2).astype(np.float32)
    return X, Y


@functools.lru_cache(maxsize=None)
def ie_case(n):
    """Values over [-0.1, 1.1] so both clamps are live, and entries planted exactly at the clamps' float32 bounds, 0 and 1."""
    rng = np.random.RandomState(10000 + n)
    P = (rng.rand(n, n) * 1.2 - 0.1).astype(np.float32)
    P[0, :4] = (np.float32(1e-4), np.float32(1) - np.float32(1e-4), 0.0, 1.0)
    P[n - 1, n - 4:] = (1.0, 0.0, np.float32(1) - np.float32(1e-4), np.float32(1e-4))
    P[n // 2, n - 1] = 0.37          # the last column and the last row carry ordinary entries too
    return P


@functools.lru_cache(maxsize=None)
def mse_case(count):
    """Independent Gaussian operands; the last pair is 3 apart, so that the last element carries weight."""
    rng = np.random.RandomState(11000 + count % 9973)
    X, Y = rng.randn(count).astype(np.float32), rng.randn(count).astype(np.float32)
    Y[-1] = X[-1] + np.float32(3.0)
    return X, Y


@functools.lru_cache(maxsize=None)
def mse_one_element_case():
    """Operands past the 1024 x 256 grid that differ in their last element alone."""
    X = mse_case(1024 * 256 + 3)[0]
    Y = X.copy()
    Y[-1] = X[-1] + np.float32(0.75)
    return X, Y


@functools.lru_cache(maxsize=None)
def adj_case(n):
    """A packed vector of distinct values (k + 1, exact in float32 up to n = 1030) and an ori_adj of distinct values."""
    a = np.arange(1, n * (n - 1) // 2 + 1, dtype=np.float32)
    rng = np.random.RandomState(12000 + n)
    ori = (rng.permutation(n * n).reshape(n, n) + 1).astype(np.float32) / np.float32(4.0)
    return a, ori


@functools.lru_cache(maxsize=None)
def norm_case(n):
    """A symmetric weighted graph with: node 3 isolated (row sum 0, d = 1); node 5 with entries +0.5 / -0.5 whose sum is 0
    although the row is not (d = 1 only because of the added identity); node 9 with the single entry -1, so d = 0 and
    r = inf -> 0."""
    rng = np.random.RandomState(13000 + n)
    A = np.triu(rng.rand(n, n) * (rng.rand(n, n) < 0.3), 1)
    A = A + A.T
    for i in (3, 5, 9):
        A[i, :] = 0
        A[:, i] = 0
    A[5, 20] = A[20, 5] = 0.5
    A[5, n - 1] = A[n - 1, 5] = -0.5
    A[9, 40] = A[40, 9] = -1.0
    return A.astype(np.float32)


@functools.lru_cache(maxsize=None)
def decode_case(n, d, kind="plain"):
    """Rows of mixed sign (negative products, so relu is live); row 4 all zero.  kind 'decades': magnitudes over several
    decades as well (the powf branches)."""
    rng = np.random.RandomState(14000 + n + d)
    Z = rng.randn(n, d) * (1.2 / math.sqrt(d))           # <z_i, z_i> about 1.4: the subtracted identity shows under the sigmoid
    if kind == "decades":
        Z = Z * 10.0 ** rng.uniform(-2, 2, size=(n, d))
    Z[4] = 0.0
    return Z.astype(np.float32)


@functools.lru_cache(maxsize=None)
def gcn_case(name):
    n, nfeat, widths, nclass = GCN_CASES[name]
    rng = np.random.RandomState(15000 + n + len(widths))
    A = np.triu((rng.rand(n, n) < 8.0 / n).astype(np.float64), 1)
    A = A + A.T
    adj = normalize_adj(A).astype(np.float32)
    X = rng.randn(n, nfeat).astype(np.float32)
    dims = (nfeat,) + tuple(widths)
    W = tuple((rng.randn(dims[l], dims[l + 1]) / math.sqrt(dims[l])).astype(np.float32) for l in range(len(widths)))
    b = tuple((0.1 * rng.randn(dims[l + 1])).astype(np.float32) for l in range(len(widths)))
    Wlin = (rng.randn(nclass, dims[-1]) / math.sqrt(dims[-1])).astype(np.float32)
    blin = (0.1 * rng.randn(nclass)).astype(np.float32)
    return X, adj, W, b, Wlin, blin


# ------------------------------------------------------------------------------------- utils.MutualInformation (KDE)
KDE_SIGMA = 2 * 0.4 ** 2                        # self.sigma (utils.py:985), the double
KDE_SIGMA_F32 = float(np.float32(KDE_SIGMA))    # the float32 scalar the kernels divide by
KDE_EPS = 1e-10                                 # self.epsilon (utils.py:988)
KDE_MAXC = 32                                   # the widest template of csrc/kde_kernels.hip
KDE_ROWS = 64                                   # rows per block of k_kde_stats
KDE_GRAD_TOL = 3e-6                             # of the operand's largest float64 gradient magnitude
                                                # (tests/test_gpu_parity.py::test_mutual_information_op_against_the_reference)
MI_DEFECTS = ("lastrow", "tail64", "first_block", "m_padded", "lastcol", "cols8", "bins_from_reach", "joint_transposed",
              "no_marginal")


def kde_bins(nb):
    """torch.linspace(0, nb, nb).float() (utils.py:990-991) by the formula of kde_bin in csrc/kde_kernels.hip, every step
    rounded to float32: step = nb / (nb - 1), step * j below the middle, fma(-step, nb - 1 - j, nb) from it on (the fma is
    taken exactly in double and rounded once: its operands are float32, so the double product is exact)."""
    if nb <= 1:
        return np.zeros(max(nb, 0), np.float32)
    step = np.float32(nb) / np.float32(nb - 1)
    j = np.arange(nb)
    lo = (step * j.astype(np.float32)).astype(np.float32)
    hi = (np.float64(nb) - np.float64(step) * (nb - 1 - j).astype(np.float64)).astype(np.float32)
    return np.where(j < nb // 2, lo, hi).astype(np.float32)


def kde_reach(X, Y):
    """The number of leading columns a wide square operand is evaluated on (mcgra_mutual_information): bin j sits at
    j c / (c - 1) >= j and a float32 kernel value is exactly 0 once b - v > 4.62, so act = floor(max |v| + 4.7) + 1.
    Not capped: beyond KDE_MAXC the op refuses."""
    vmax = np.float32(max(np.abs(X).max(), np.abs(Y).max()))
    return int(np.floor(vmax + np.float32(4.7))) + 1


def _kde_dH(p):
    """d (-p log2(p + eps)) / dp"""
    return -(np.log2(p + KDE_EPS) + p / ((p + KDE_EPS) * math.log(2.0)))


def _mi(X, Y, defect=None, f32_kernel=False):
    """utils.MutualInformation(sigma=0.4, num_bins=c, normalize=True) on X, Y [m x c] (utils.py:980-1049) and its backward by
    hand, in float64.  `values - bins.unsqueeze(0).unsqueeze(0)` (:995) puts bin j against column j:
      k_ij = exp(-0.5 ((v_ij - b_j) / sigma)^2),  pdf = mean_i k / (sum_j mean_i k + eps) (:998-1000),
      joint = k1^T k2 / (sum + eps) (:1004-1010),  H = -sum p log2(p + eps),  V = 2 (H1 + H2 - H12) / (H1 + H2) (:1035-1043).
    Backward: dV/dH12 = -2 / S and dV/dH1 = dV/dH2 = 2 H12 / S^2 with S = H1 + H2; through p = q / (sum q + eps):
    g_q = (g_p - sum g_p p) / (sum q + eps); dV/dk1_ia = g_q1_a / m + sum_b g_J_ab k2_ib (k2 likewise with the joint's table
    transposed); dk/dv = -k (v - b) / sigma^2.
    f32_kernel: the kernel values as the device forms them, (v - b) / 0.32f, t t, expf(-0.5 t t), every step rounded to
    float32, on the columns within reach of a wide square operand; everything after them in float64 as on the device.
    Returns a dict: val, gX, gY, dk1, dk2 (dV/dk), z1, z2 (the exponents), k1, k2."""
    X32, Y32 = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    m, c = X32.shape
    wide = c > KDE_MAXC
    rows, cols, mdiv = np.ones(m, bool), np.ones(c, bool), float(m)
    if f32_kernel:
        bins = kde_bins(c)
    else:
        import torch
        bins = torch.linspace(0, c, c).float().numpy()
    if defect == "lastrow":
        rows[-1] = False
    elif defect == "tail64":
        rows[KDE_ROWS * (m // KDE_ROWS):] = False
    elif defect == "first_block":
        rows[KDE_ROWS:] = False
    elif defect == "m_padded":
        mdiv = float(KDE_ROWS * ((m + KDE_ROWS - 1) // KDE_ROWS))
    elif defect == "lastcol":
        cols[-1] = False
    elif defect == "cols8":
        cols[8:] = False
    elif defect == "bins_from_reach":
        act = min(kde_reach(X32, Y32), c)
        bins = np.concatenate([kde_bins(act), np.full(c - act, 1e30, np.float32)])
    if f32_kernel and wide:
        cols[min(kde_reach(X32, Y32), c):] = False
    b = bins.astype(np.float64)[None, :]
    if f32_kernel:
        s32 = np.float32(KDE_SIGMA)
        t = ((X32 - bins[None, :]).astype(np.float32) / s32).astype(np.float32), ((Y32 - bins[None, :]).astype(np.float32) / s32).astype(np.float32)
        h = [(np.float32(-0.5) * (tt * tt).astype(np.float32)).astype(np.float32) for tt in t]
        with np.errstate(under="ignore"):
            k1, k2 = (np.exp(hh.astype(np.float64)).astype(np.float32).astype(np.float64) for hh in h)
        z1, z2 = (hh.astype(np.float64) for hh in h)
        sig = KDE_SIGMA_F32
    else:
        sig = KDE_SIGMA
        z1, z2 = -0.5 * ((_f64(X32) - b) / sig) ** 2, -0.5 * ((_f64(Y32) - b) / sig) ** 2
        with np.errstate(under="ignore"):
            k1, k2 = np.exp(z1), np.exp(z2)
    k1, k2 = k1 * cols[None, :], k2 * cols[None, :]
    q1, q2 = k1[rows].sum(0) / mdiv, k2[rows].sum(0) / mdiv
    n1, n2 = q1.sum() + KDE_EPS, q2.sum() + KDE_EPS
    p1, p2 = q1 / n1, q2 / n2
    J = k1[rows].T @ k2[rows]
    nJ = J.sum() + KDE_EPS
    P = J / nJ
    H1, H2, H12 = -(p1 * np.log2(p1 + KDE_EPS)).sum(), -(p2 * np.log2(p2 + KDE_EPS)).sum(), -(P * np.log2(P + KDE_EPS)).sum()
    S = H1 + H2
    val = 2.0 * (S - H12) / S
    gH, gH12 = 2.0 * H12 / (S * S), -2.0 / S
    gp1, gp2, gP = gH * _kde_dH(p1), gH * _kde_dH(p2), gH12 * _kde_dH(P)
    gq1, gq2 = (gp1 - (gp1 * p1).sum()) / n1 / m, (gp2 - (gp2 * p2).sum()) / n2 / m      # d pdf / d k = 1 / m
    gJ = (gP - (gP * P).sum()) / nJ
    if defect == "no_marginal":
        gq1, gq2 = 0.0 * gq1, 0.0 * gq2
    if defect == "joint_transposed":
        gJ = gJ.T
    dk1 = (gq1[None, :] + k2 @ gJ.T) * cols[None, :]
    dk2 = (gq2[None, :] + k1 @ gJ) * cols[None, :]
    gX = dk1 * k1 * (-(_f64(X32) - b) / (sig * sig))
    gY = dk2 * k2 * (-(_f64(Y32) - b) / (sig * sig))
    if f32_kernel:
        gX, gY = gX.astype(np.float32).astype(np.float64), gY.astype(np.float32).astype(np.float64)
    return dict(val=float(val), gX=gX, gY=gY, dk1=dk1, dk2=dk2, z1=z1, z2=z2, k1=k1, k2=k2)


def mutual_information(X, Y, defect=None):
    """(value, dvalue/dX, dvalue/dY) of utils.MutualInformation(sigma=0.4, num_bins=X.shape[1], normalize=True)(X, Y)
    (utils.py:980-1049) in float64; the bins are torch.linspace(0, c, c).float() as float32 values, as the reference's double
    run has them.  Defects (the sums are the two column sums of the kernel values and their c x c product):
      lastrow          the last row left out of all three sums
      tail64           the rows past the last whole 64 left out of them
      first_block      only the first 64 rows counted
      m_padded         the marginals' mean taken over m rounded up to 64.  The normalised pdf does not see a common factor, so
                       the value keeps; what moves is the marginal part of the gradient, whose d pdf / d k stays 1 / m: it
                       comes out (padded m) / m too large
      lastcol          the last column dropped (non-square operands; a wide square operand's last column carries nothing)
      cols8            a wide square operand cut at 8 columns whatever its values reach
      bins_from_reach  the bins of a wide square operand spaced for the evaluated width, not for N
      joint_transposed the joint's gradient table indexed [b][a]
      no_marginal      the gradient without the part through the marginals"""
    r = _mi(X, Y, defect)
    return r["val"], r["gX"], r["gY"]


def mutual_information_f32(X, Y):
    """The same with the kernel values rounded as the device rounds them (see _mi): what a correct float32 evaluation
    returns, up to the last bit of expf.  tests/test_ops_cases_cpu.py holds it to a third of the tolerances."""
    r = _mi(X, Y, f32_kernel=True)
    return r["val"], r["gX"], r["gY"]


def mutual_information_bound(X, Y, r=None):
    """The value's bound.  A kernel value k = expf(-0.5f (t t)), t = (v - b) / 0.32f, carries relative to k: on the exponent
    z = -0.5 t^2 twice the relative error of t -- the subtraction u, the division 2 u, so 6 u |z| -- one rounding of the
    square, u |z|, and 0.32f against the reference's 0.32 (2.24e-8 = 0.375 u on sigma), 0.75 u |z|: below 8 u |z|; expf within
    1 ulp: 2 u.  e_k = (8 |z| + 2) u k.  Everything after the kernel values is double on the device, so the value moves by
    sum |dV/dk1| e_k1 + sum |dV/dk2| e_k2 to first order, dV/dk from the truth's own backward; times SAFETY, + u |V| for the
    returned float.  r: _mi(X, Y) where the caller has it."""
    r = _mi(X, Y) if r is None else r
    e1 = (8.0 * np.abs(r["z1"]) + 2.0) * U * r["k1"]
    e2 = (8.0 * np.abs(r["z2"]) + 2.0) * U * r["k2"]
    return SAFETY * float((np.abs(r["dk1"]) * e1).sum() + (np.abs(r["dk2"]) * e2).sum()) + U * abs(r["val"])


MI_EMB = ((1, 7), (2, 7), (63, 8), (64, 8), (65, 9), (128, 16), (129, 17), (257, 32), (1030, 32), (5000, 32), (300, 1), (32, 32))
MI_LOGP = ((300, 2), (1030, 7), (1030, 9))
MI_CASES = tuple(("emb", m, c) for m, c in MI_EMB) + tuple(("logp", m, c) for m, c in MI_LOGP) + (
    ("nxn1", 33, 33), ("nxn1", 257, 257), ("nxn1", 1030, 1030), ("nxn2", 1030, 1030), ("nxn20", 257, 257), ("reach32", 300, 300))
MI_RAW_CASES = (("emb", 65, 9), ("nxn2", 1030, 1030))        # the raw C ABI with one or both gradient outputs absent
MI_REACH = {("nxn1", 33, 33): 6, ("nxn1", 257, 257): 6, ("nxn1", 1030, 1030): 6, ("nxn2", 1030, 1030): 7, ("nxn20", 257, 257): 25,
            ("reach32", 300, 300): 32}


def mi_defects(kind, m, c):
    """The defects that change anything at this case.  'lastcol' needs a last column that carries something: the bin of
    column c - 1 is c, which the values of a wide square operand never come near (that is why it is cut at its reach), nor
    do log-probabilities and probabilities (<= 1) once c > 5."""
    wide = c > KDE_MAXC
    out = []
    if m > 1:
        out.append("lastrow")
    if m % KDE_ROWS and m > KDE_ROWS:
        out.append("tail64")
    if m > KDE_ROWS:
        out.append("first_block")
    if m % KDE_ROWS:
        out.append("m_padded")
    if not wide and c > 1 and (kind == "emb" or c <= 5):
        out.append("lastcol")
    if wide and MI_REACH[(kind, m, c)] > 8:
        out.append("cols8")
    if wide:
        out.append("bins_from_reach")
    if c > 1:
        out.append("joint_transposed")
    out.append("no_marginal")
    return out


@functools.lru_cache(maxsize=None)
def mi_case(kind, m, c):
    """Operands of mutual_information; in every kind Y depends on X and follows another law, so the joint is neither
    symmetric nor the product of its marginals.
      emb      X uniform over [-1, c + 1], so every bin is met; Y a noisy affine function of X with a drift per column
      logp     X a log-softmax, Y a softmax of correlated logits (the operands of c10)
      nxn<hi>  X uniform over [0, hi], Y = clip(0.5 X + 0.5 hi r^2, 0, hi) with r uniform: the N x N operands
      reach32  nxn26 with X's largest entry planted at exactly 27.0: floor(27 + 4.7) + 1 = 32 columns, the last reach the op
               accepts (mi_refused_case raises the entry to 27.5)"""
    assert m >= 1 and c >= 1
    rng = np.random.RandomState(16000 + 31 * m + c)
    if kind == "emb":
        X = rng.uniform(-1.0, c + 1.0, (m, c))
        j = np.arange(c)
        if m > 1:       # with few rows too, every column meets its bin.  Not at m = 1: the joint of one row is the product of its
            # marginals, the value 0 but for eps, and only kernel sums small enough for eps to count leave anything to compare
            X[j % m, j] = j * (c / max(c - 1.0, 1.0)) + 0.15 * np.sin(1.0 + j)
        if m > 2:       # and the last row meets all of them: among thousands of uniform rows it would carry next to nothing
            X[m - 1] = j * (c / max(c - 1.0, 1.0)) + 0.2 * np.cos(3.0 * j)
        Y = 0.97 * X + 0.4 + 0.3 * np.cos(j)[None, :] + 0.3 * rng.randn(m, c)
    elif kind == "logp":
        L = 2.0 * rng.randn(m, c)
        L2 = 0.7 * L + 1.4 * rng.randn(m, c)
        X = L - L.max(1)[:, None]
        X = X - np.log(np.exp(X).sum(1))[:, None]
        Y = np.exp(L2 - L2.max(1)[:, None])
        Y = Y / Y.sum(1)[:, None]
    else:
        assert m == c
        hi = 26.0 if kind == "reach32" else float(kind[3:])
        X = rng.uniform(0.0, hi, (m, c))
        Y = np.clip(0.5 * X + 0.5 * hi * rng.rand(m, c) ** 2, 0.0, hi)
        if kind == "reach32":
            X[5, 27] = 27.0
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def mi_refused_case():
    """The reach32 operands with the planted entry raised to 27.5: floor(27.5 + 4.7) + 1 = 33 columns, refused."""
    X, Y = mi_case("reach32", 300, 300)
    X = X.copy()
    X[5, 27] = 27.5
    return X, Y


@functools.lru_cache(maxsize=None)
def mi_truth(kind, m, c):
    """(value, gX, gY, bound of the value) of a case, computed once a process."""
    X, Y = mi_case(kind, m, c)
    r = _mi(X, Y)
    return r["val"], r["gX"], r["gY"], mutual_information_bound(X, Y, r)
