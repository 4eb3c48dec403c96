"""The truth of the LinkTeller influence attack (mcgra_influence_scores, include/mcgra.h) in float64.

truth()        the literal definition: for every source v, the victim's forward on X with row v scaled by 1 + Delta, minus the
               forward on X, through forward() -- a float64 copy of models.gcn.GCN.forward (eval mode) -- with A a scipy.sparse
               matrix, so that a row the perturbation cannot reach is computed from identical inputs in an identical order and
               differs by exactly 0.  Delta is exactly float64(float32(delta)).  All sources at once: arrays [node, source, column].
difference()   the form the kernels compute (differences carried, the base pre-activations kept), in any precision, and the wrong
               readings of the definition (VARIANTS) that the cases must tell from the truth.
bound()        for every entry, the error a float32 evaluation of the computed form may have: gamma(k) M[v, u] (below), and the
               entries whose chain reads a pre-activation so close to 0 that float32 and float64 may take different relu branches.

The bound.  u = 2^-24, gamma(k) = k u / (1 - k u).  M is the computed chain with every operand replaced by its magnitude: |A|, |W|,
|dT|, relu as the identity, and the softmax correction added, not subtracted:
    dT0abs_v = |Delta| (|x_v| |W_0|);  dPabs = |A| dTabs;  dHabs = dPabs;  dTabs' = dHabs |W'|;  dZabs = dHabs |Wlin|^T;
    cabs = sum_j p_j expm1(dZabs_j) >= |sum_j p_j expm1(dZ_j)|;  dlabs_k = dZabs_k - log1p(-cabs);
    M = || dlabs ||_2 / |Delta|  (log-posteriors),  || p_k expm1(dlabs_k) ||_2 / |Delta|  (posteriors).
Every float32 operation of the chain errs by at most u times the magnitude it carries, a sum of d terms by gamma(d), and zero terms
add no error, so the counts are those of the NON-ZERO terms:
    k_chain = (fx + 1)                              T0 = X W_0 over the fx non-zero features of a row at most, times Delta
            + sum_l (d + 1 + h_l)                   layer l: at most d non-zero cells in a row of A, the relu's one addition, the
                                                    h_l terms of the next product (the head's for the last layer)
            + (nc + 2 e1 + el + 1 + 1)              p_j expm1(dZ_j) summed over nc classes, log1p, the subtraction
            + (e1 + 1)                              posteriors: p_k expm1(dlogp_k)
            + (nc + 3)                              the squares, their sum, the root, the division
with e1, el, ee the errors of expm1f, log1pf and expf in ulps (ULP below), and d_l = min(d, max_v |F_l(v)|): layer 0 sums one term.
p = exp(O) also carries the error of the BASE output O: an ABSOLUTE error e_O of O, so a RELATIVE error of p, in both places p
enters.  O_k = Z_k - logsumexp(Z), so |dO_k| <= 2 max_j |dZ_j| plus the roundings of the log-softmax itself:
    e_O(u) = u [ 2 k_Z Zabs_u + 6 Zabs_u + nc + ee + 5 el + 5 ],   k_Z = fx + L (d + 1) + sum_l h_l,
Zabs_u the base chain of row u in magnitudes (|A|, |X|, |W|, |b|; the largest class).  That error multiplies what p multiplies, the
TRUE values, not the chain in magnitudes:  Mp = || c ||_2 / |Delta| (log-posteriors),  || |dp_k| + p_k c ||_2 / |Delta| (posteriors),
c = sum_j p_j |expm1(dZ_j)| / (1 - sum_j p_j |expm1(dZ_j)|).  Together, inside the reach:
    |got - truth| <= gamma(k_chain) M[v, u] + 1.01 e_O(u) Mp[v, u] + 64 2^-53 (Zabs_u + 1) / |Delta|,
the last term being the literal truth's own cancellation noise in float64 (about 1e-11, far below the others); outside the reach
both are exactly 0 and the bound is 0.

The exclusions.  relu(P + dP) - relu(P) is computed from the float32 P.  Where |P| > |dP| the branch is the same in any precision
and P does not enter the result; where |P| <= |dP| the result carries P's own float32 error, which is of the order of dP itself.
An entry (v, u) is excluded when its chain reads a unit (l, w, c) -- w in F_{l+1}(v) with a path of non-zero cells on to u -- with
|P^l_wc| <= 2 dPabs^l_wc(v) + gamma(k_P) Pabs^l_wc, the second term being the float32 rounding margin of P (k_P its operation count,
Pabs its chain in magnitudes)."""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24
# twice the worst error measured on the device over the arguments the cases reach (profiles/influence.txt), in ulps
ULP = {"expm1": 2 * 1.357, "log1p": 2 * 0.566, "exp": 2 * 0.841}
OUTPUTS = ("log_posteriors", "posteriors")
VARIANTS = ("additive", "no_self_loop", "jacobian", "base_mask", "no_division", "swapped", "linear_softmax", "raw_for_normalised")


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


class Model:
    """A case's operands in float64 (the float32 values, widened): A as scipy.sparse CSR."""
    def __init__(self, case, dtype=np.float64):
        self.A = sp.csr_matrix(case["A"].astype(dtype))
        self.A.eliminate_zeros()
        self.X = case["X"].astype(dtype)
        self.W = [w.astype(dtype) for w in case["W"]]
        self.b = [x.astype(dtype) for x in case["b"]]
        self.Wlin, self.blin = case["Wlin"].astype(dtype), case["blin"].astype(dtype)
        self.delta = dtype(np.float32(case["delta"]))
        self.n, self.L, self.nclass = self.X.shape[0], len(self.W), self.Wlin.shape[0]


def _matmul(H, W):
    """H [..., k] @ W [k, c] by einsum's own loops: the same summation order for every row, whatever its position."""
    return np.einsum("...k,kc->...c", H, W)


def _spmm(A, T):
    """A [n x n] sparse times T [n, ...]: row u of the result reads the rows N(u) of T only."""
    return (A @ T.reshape(T.shape[0], -1)).reshape(T.shape)


def _log_softmax(Z):
    mx = Z.max(axis=-1, keepdims=True)
    return Z - mx - np.log(np.exp(Z - mx).sum(axis=-1, keepdims=True))


def forward(m, T0):
    """models.gcn.GCN.forward (eval: no dropout) behind the first product T0 = X W_0, which may be [n, h] or a stack [n, s, h] of
    one forward per source: x = adj @ (x @ W) + b; relu; log_softmax(linear1(x)).  Returns (O, [P^0 .. P^{L-1}])."""
    T, Ps = T0, []
    for l in range(m.L):
        P = _spmm(m.A, T) + m.b[l]
        Ps.append(P)
        H = np.maximum(P, 0.0)
        if l + 1 < m.L:
            T = _matmul(H, m.W[l + 1])
    return _log_softmax(_matmul(H, m.Wlin.T) + m.blin), Ps


def reach(A, L):
    """R[u, v] = u in F_L(v): F_0 = {v}, F_{l+1} = the nodes with a non-zero cell towards F_l.  Dense bool."""
    S = sp.csr_matrix((np.asarray(A) != 0).astype(np.float64))
    R = np.eye(S.shape[0])
    for _ in range(L):
        R = ((S @ R) > 0).astype(np.float64)
    return R > 0


def counts(case):
    """{nnz, reached, max_reach} of the entry's counts."""
    R = reach(case["A"], len(case["W"]))
    return {"nnz": int(np.count_nonzero(case["A"])), "reached": int(R.sum()), "max_reach": int(R.sum(axis=0).max()) if R.size else 0}


def truth(case, output="posteriors"):
    """The directed influence matrix I[v, u] by the literal definition, float64."""
    m = Model(case)
    T0 = m.X @ m.W[0]
    O, _ = forward(m, T0)
    n = m.n
    Ts = np.repeat(T0[:, None, :], n, axis=1)                     # [node, source, column]
    pert = ((1.0 + m.delta) * m.X) @ m.W[0]                       # row v: (x_v scaled) W_0
    Ts[np.arange(n), np.arange(n), :] = pert
    Ov, _ = forward(m, Ts)
    D = Ov - O[:, None, :]
    if output == "posteriors":
        D = np.exp(Ov) - np.exp(O)[:, None, :]
    return np.sqrt((D * D).sum(axis=-1)).T / m.delta


def symmetrize(I):
    return np.maximum(I, I.T)


def difference(case, output="posteriors", dtype=np.float64, variant=None, parts=False):
    """The computed form (module docstring of csrc/influence.hip) in `dtype`, all sources at once; `variant`: a wrong reading."""
    if variant == "raw_for_normalised":
        case = dict(case, A=case["A_raw"])
    if variant == "no_self_loop":
        A = case["A"].copy()
        np.fill_diagonal(A, 0)
        case = dict(case, A=A)
    m = Model(case, dtype)
    n = m.n
    T0 = (m.X @ m.W[0]).astype(dtype)
    O, Ps = forward(m, T0)
    dT = np.zeros((n, n, T0.shape[1]), dtype)
    src = m.delta * T0
    if variant == "additive":
        src = m.delta * np.repeat(m.W[0].sum(axis=0)[None, :], n, axis=0)
    dT[np.arange(n), np.arange(n), :] = src
    dPs = []
    for l in range(m.L):
        dP = _spmm(m.A, dT)
        dPs.append(dP)
        P = Ps[l][:, None, :]
        if variant in ("jacobian", "base_mask"):
            dH = np.where(P > 0, dP, 0)
        else:
            dH = np.where(P > 0, np.maximum(dP, -P), np.maximum(P + dP, 0))
        dH = dH.astype(dtype)
        if l + 1 < m.L:
            dT = _matmul(dH, m.W[l + 1]).astype(dtype)
    dZ = _matmul(dH, m.Wlin.T).astype(dtype)
    p = np.exp(O)[:, None, :]
    if variant in ("jacobian", "linear_softmax"):
        dl = dZ - (p * dZ).sum(axis=-1, keepdims=True)
        D = dl if output == "log_posteriors" else p * dl
    else:
        dl = dZ - np.log1p((p * np.expm1(dZ)).sum(axis=-1, keepdims=True))
        D = dl if output == "log_posteriors" else p * np.expm1(dl)
    I = (np.sqrt((D * D).sum(axis=-1)).T / (1 if variant == "no_division" else m.delta)).astype(dtype)
    if variant == "swapped":
        I = I.T.copy()
    return (I, Ps, dPs, dZ, O) if parts else I


def bound(case, output="posteriors"):
    """{"bound" [v, u], "M" [v, u], "excluded" [v, u] bool, "reach" [v, u] bool, "crossing" (units the perturbation switches), "k"
    (the largest operation count)} of the module docstring, from the truth's operands alone."""
    m = Model(case)
    n, L, nc = m.n, m.L, m.nclass
    Aabs = abs(m.A)
    S = sp.csr_matrix((m.A != 0).astype(np.float64))
    fx = max(1, int((case["X"] != 0).sum(axis=1).max()))
    d = max(1, int(np.diff(m.A.indptr).max())) if m.A.nnz else 1
    hs = [w.shape[1] for w in m.W]
    # the base forward, its magnitudes and the margin of every pre-activation
    T0 = m.X @ m.W[0]
    O, Ps = forward(m, T0)
    Tabs = np.abs(m.X) @ np.abs(m.W[0])
    Pabs, kP = [], []
    k = fx
    for l in range(L):
        Pa = Aabs @ Tabs + np.abs(m.b[l])
        k += d + 1
        Pabs.append(Pa)
        kP.append(k)
        k += hs[l]
        Tabs = Pa @ (np.abs(m.W[l + 1]) if l + 1 < L else np.abs(m.Wlin.T))
    Zabs = (Tabs + np.abs(m.blin)).max(axis=1)
    k_Z = fx + L * (d + 1) + sum(hs)
    e_O = U * (2.0 * k_Z * Zabs + 6.0 * Zabs + nc + ULP["exp"] + 5.0 * ULP["log1p"] + 5.0)      # [u]
    fr, width = np.eye(n), [1]
    for l in range(1, L):
        fr = ((S @ fr) > 0).astype(np.float64)
        width.append(int(fr.sum(axis=0).max()))
    k_chain = ((fx + 1) + sum(min(d, width[l]) + 1 + hs[l] for l in range(L)) + (nc + 2 * ULP["expm1"] + ULP["log1p"] + 2)
               + (ULP["expm1"] + 1) + (nc + 3))
    # the chain in magnitudes, and the units near a relu's corner
    dT = np.zeros((n, n, hs[0]))
    dT[np.arange(n), np.arange(n), :] = abs(m.delta) * (np.abs(m.X) @ np.abs(m.W[0]))
    taint = np.zeros((n, n), bool)                                # [node, source]
    front = np.eye(n, dtype=bool)
    crossing = 0
    _, _, dPs, dZ, _ = difference(case, output, parts=True)
    for l in range(L):
        dP = _spmm(Aabs, dT)
        front = (S @ front.astype(np.float64)) > 0
        P = Ps[l][:, None, :]
        near = (np.abs(P) <= 2.0 * dP + gamma(kP[l]) * Pabs[l][:, None, :]) & front[:, :, None]
        crossing += int((((P > 0) != (P + dPs[l] > 0)) & front[:, :, None]).sum())
        taint = (((S @ taint.astype(np.float64)) > 0) | near.any(axis=-1)) & front
        dT = _matmul(dP, np.abs(m.W[l + 1]) if l + 1 < L else np.abs(m.Wlin.T))
    p = np.exp(O)[:, None, :]
    cabs = (p * np.expm1(dT)).sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        dl = dT - np.log1p(-np.minimum(cabs, 1.0))
    D = dl if output == "log_posteriors" else p * np.expm1(dl)
    M = np.sqrt((D * D).sum(axis=-1)).T / abs(m.delta)           # [v, u]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (p * np.abs(np.expm1(dZ))).sum(axis=-1, keepdims=True)
        c = c / (1.0 - np.minimum(c, 1.0))
    if output == "log_posteriors":
        Dp = np.repeat(c, nc, axis=-1)
    else:
        dl_true = dZ - np.log1p((p * np.expm1(dZ)).sum(axis=-1, keepdims=True))
        Dp = np.abs(p * np.expm1(dl_true)) + p * c
    Mp = np.sqrt((Dp * Dp).sum(axis=-1)).T / abs(m.delta)         # [v, u]
    noise = 64.0 * 2.0 ** -53 * (Zabs + 1.0) / abs(m.delta)      # the float64 truth's own cancellation: two forwards subtracted
    total = np.where(front.T, gamma(k_chain) * M + 1.01 * e_O[None, :] * Mp + noise[None, :], 0.0)
    ktot = k_chain + e_O / U
    return {"bound": total, "M": M, "excluded": taint.T.copy(), "reach": front.T.copy(), "crossing": crossing,
            "k": float(ktot.max())}


def auc(scores, labels):
    """The AUC of the unordered pairs a > b, ties 1/2: (pairs won + ties / 2) / (P N).  NaN without both classes."""
    a, b = np.tril_indices(scores.shape[0], -1)
    s, y = scores[a, b], labels[a, b] > 0
    pos, neg = np.sort(s[y]), np.sort(s[~y])
    if not len(pos) or not len(neg):
        return float("nan")
    less = np.searchsorted(neg, pos, "left")
    ties = np.searchsorted(neg, pos, "right") - less
    return float((less.sum() + 0.5 * ties.sum()) / (len(pos) * len(neg)))


def close_pair_share(scores, bounds, labels):
    """The share of (edge, non-edge) pairs of pairs whose truth scores lie closer than the sum of their bounds: what a scoring within
    its bounds can move the AUC by at most."""
    a, b = np.tril_indices(scores.shape[0], -1)
    s, e, y = scores[a, b], bounds[a, b], labels[a, b] > 0
    if not y.any() or y.all():
        return 0.0
    sp_, ep, sn, en = s[y], e[y], s[~y], e[~y]
    close = 0
    for i in range(0, len(sp_), 256):
        close += int((np.abs(sp_[i:i + 256, None] - sn[None, :]) < ep[i:i + 256, None] + en[None, :]).sum())
    return close / (len(sp_) * len(sn))
