"""Shared test helpers: load golden fixtures, build oracle objects from them."""
import contextlib
import functools
import glob
import os

import numpy as np

os.environ.setdefault("MCGRA_KEEP_GSYM", "1")     # the parity tests read each step's mirrored gradient ("G_sym")
os.environ.setdefault("MCGRA_AB", "1")            # ... and the engine honours such switches only beside MCGRA_AB=1 (attack_plan.hip: ab_env)

from oracle import mcgra_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def attack_cases():
    return sorted(os.path.basename(p)[len("attack_"):-4] for p in glob.glob(os.path.join(GOLDEN, "attack_*.npz")))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, f"attack_{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def weights_from(z):
    L = int(z["nlayer"]) if "nlayer" in z else 2
    Ws = [z[f"Ws{l}"] for l in range(L)] if "Ws0" in z else None
    return O.GCNWeights([z[f"W{l}"] for l in range(L)], [z[f"b{l}"] for l in range(L)], z["Wlin"], z["blin"], Ws,
                        str(z["act"]) if "act" in z else "relu", str(z["head_act"]) if "head_act" in z else "none")


def cfg_from(z):
    return O.AttackConfig(measure=str(z["measure"]), weight_sup=float(z["weight_sup"]),
                          weight_param=tuple(float(x) for x in z["weight_param"]), lr=float(z["lr"]),
                          num_edges=float(z["num_edges"]), eps=float(z["eps"]) if "eps" in z else 0.0,
                          emb_nlayer=int(z["emb_nlayer"]) if "emb_nlayer" in z else 2,
                          fin_layers=tuple(int(x) for x in z["fin_layers"]) if "fin_layers" in z else (1, 2))


def init_adj_changes(n, seed, scale):
    """Same generator as tests/golden/make_golden.py:init_adj_changes."""
    return (np.random.RandomState(int(seed)).rand(n * (n - 1) // 2) * float(scale)).astype(np.float32)


def a0_of(z):
    if "a0_seed" in z:
        a = init_adj_changes(z["adj"].shape[0], z["a0_seed"], z["a0_scale"])
        if "a0_keep" in z:      # a sparse start: that fraction of the entries, the rest zero (synthetic_case)
            a = a * (np.random.RandomState(int(z["a0_seed"]) + 1).rand(a.size) < float(z["a0_keep"])).astype(np.float32)
        return a
    return None


def seeded_noise(seed, t, shape):
    """Step t's noise of a seeded eps != 0 run (same generator as tests/golden/make_golden.py:seeded_noise: numpy's legacy
    RandomState, bit-reproducible across platforms by its compatibility policy)."""
    return np.random.RandomState(int(seed) + int(t)).standard_normal(shape).astype(np.float32)


def noise_of(z, t):
    """Noise the reference drew at step t, or None when eps == 0: the recorded torch.randn_like matrices (`noise`), or -- on
    large graphs -- the seeded stream the reference was handed (`noise_seed`), checked against the digest the generating
    run kept of it (sum, sum of squares, three entries: float64)."""
    if "noise" in z:
        return z["noise"][t]
    if "noise_seed" in z:
        n = len(z["labels"])
        zn = seeded_noise(z["noise_seed"], t, (n, n))
        z8 = zn.astype(np.float64)
        dig = np.array([z8.sum(), (z8 ** 2).sum(), z8[0, 0], z8[-1, -1], z8[n // 2, n // 3]])
        assert np.allclose(dig, z["noise_digest"][t], rtol=1e-12, atol=1e-9), "the seeded noise stream is not the fixture's"
        return zn
    return None


def oracle_from(z):
    n = z["adj"].shape[0]
    ori = z["ori_adj"] if "ori_adj" in z else np.zeros((n, n), np.float32)
    orc = O.PGDAttackOracle(weights_from(z), z["features"], z["adj"], ori,
                            z["feature_adj"], z["labels"], z["idx_attack"], cfg_from(z))
    if a0_of(z) is not None:
        orc.set_adj_changes(a0_of(z))
    return orc


def load_cora(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    nfeat = int(z["nfeat"])
    feats = np.unpackbits(z["features_bits"], axis=1)[:, :nfeat].astype(np.float32)
    n = feats.shape[0]
    adj = np.zeros((n, n), np.float32)
    e = z["adj_edges"]
    adj[e[:, 0], e[:, 1]] = 1
    adj[e[:, 1], e[:, 0]] = 1
    z["features"], z["adj"] = feats, adj
    return z


def readme_cases():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "readme_*.npz"))
                  if not p.endswith("_fp64.npz") and not p.endswith("_graph.npz"))


def main_feature_adj(feats, dataset):
    """main.dot_product_decode (main.py:44-55): sigmoid(relu(X X^T - I)) for cora / citeseer / AIDS, relu(Xn Xn^T - I) on
    row-normalised attributes for the other datasets."""
    X = np.asarray(feats, np.float32)
    if dataset in ("cora", "citeseer", "AIDS"):
        return cora_feature_adj(X)
    nrm = np.maximum(np.sqrt((X.astype(np.float64) ** 2).sum(1, keepdims=True)), 1e-12)
    Xn = (X / nrm).astype(np.float32)
    return np.maximum(Xn @ Xn.T - np.eye(X.shape[0], dtype=np.float32), 0).astype(np.float32)


_README_GRAPHS = {}


def load_readme_graph(dataset):
    """readme_<dataset>_graph.npz of tests/golden/make_golden.py:gen_readme: the graph rebuilt from its edges and diagonal,
    attributes from bits / the identity flag / float32, feature_adj by the dataset's rule, the trained weights (cached)."""
    key = str(dataset).lower()
    if key not in _README_GRAPHS:
        g = np.load(os.path.join(GOLDEN, f"readme_{key}_graph.npz"), allow_pickle=False)
        g = {k: g[k] for k in g.files}
        n = len(g["labels"])
        adj = np.zeros((n, n), np.float32)
        e = g["adj_edges"]
        adj[e[:, 0], e[:, 1]] = 1
        adj[e[:, 1], e[:, 0]] = 1
        adj[np.arange(n), np.arange(n)] = g["adj_diag"].astype(np.float32)
        g["adj"] = adj
        if int(g["features_identity"]):
            g["features"] = np.eye(n, dtype=np.float32)
        elif "features_bits" in g:
            g["features"] = np.unpackbits(g["features_bits"], axis=1)[:, :int(g["nfeat"])].astype(np.float32)
        else:
            g["features"] = g["features_f32"]
        g["feature_adj"] = main_feature_adj(g["features"], str(g["dataset"]))
        _README_GRAPHS[key] = g
    return _README_GRAPHS[key]


def load_readme(name):
    """A README-line fixture in the layout of load_case: its dataset's graph file merged with the line's own results."""
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    return {**load_readme_graph(str(z["dataset"])), **z}


def tril_pos(p):
    """packed position (torch.tril_indices(n, n, -1) order, topology_attack.py:369) -> (row, col)"""
    p = np.asarray(p, dtype=np.int64)
    i = ((1.0 + np.sqrt(1.0 + 8.0 * p.astype(np.float64))) / 2.0).astype(np.int64)
    i = np.where(i * (i - 1) // 2 > p, i - 1, i)
    i = np.where((i + 1) * i // 2 <= p, i + 1, i)
    return i, p - i * (i - 1) // 2


def decode_slices(n, rows=None):
    """Column slices of the fused MSELoss / KL step's per-pair passes (k_decode_stats, k_decode_fly<.., 1|2>) over `rows` rows of
    an n-node graph (None: all of them, the monolithic engine): a mirror of fl_decode_slabs(n, rows, alone=true) and of the
    slice width of fl_decode_fly / fl_decode_stats (mc-gra_amd/csrc/fused_lowrank.hip), rounded up to a multiple of 4 for the
    16-byte loads of M.  Returns (js, jper, [(j0, j1) per slice]); a slice with j0 >= n is empty."""
    rows = n if rows is None else rows
    nb = (rows + 255) // 256
    js = max(1, min((1024 + nb - 1) // nb, 64, n // 64))
    jper = ((n + js - 1) // js + 3) & ~3
    return js, jper, [(s * jper, min(n, s * jper + jper)) for s in range(js)]


def empty_decode_slices(n, rows=None):
    return sum(j0 >= n for j0, _ in decode_slices(n, rows)[2])


# n of the fused MSELoss / KL oracle cases that are there for a property of the decode's slicing (tests/test_gpu_parity.py):
# each must keep it (tests/test_cabi_symbols.py::test_fused_decode_edge_cases_keep_their_property)
DECODE_EDGE_N = {1155: "odd n, padded ld, empty last decode slice",
                 4200: "n >= 4096 (small-operand terms on their own stream), empty last decode slice, also on world-3 row blocks"}


def cora_feature_adj(feats):
    """main.dot_product_decode for cora (main.py:44-48)."""
    Z = feats @ feats.T
    Z = np.maximum(Z - np.eye(Z.shape[0], dtype=np.float32), 0)
    return (1.0 / (1.0 + np.exp(-Z.astype(np.float64)))).astype(np.float32)


def synthetic_case(n, nfeat, widths, nclass, seed, measure="HSIC", weight_param=(0.01, 0.01, 0, 0, 0, 10, 10, 0, 10, 1000),
                   emb_nlayer=None, gain=1.0, a0_keep=None, a0_scale=0.05, lr=0.01):
    """A seeded random problem.  emb_nlayer: depth of the embedding (default min(2, layers), as main.py leaves it); gain scales
    every W_l and Wlin (the biases stay): at 1.0 the priors Y_A / output2, which come from the UNNORMALISED adjacency, saturate
    their softmax on deep or narrow victims and the c10 / c9 gradient is exactly zero (tests/test_term_cases_cpu.py).  The
    random draws do not depend on either, so the defaults keep every earlier case's bits.  a0_keep: the seeded start keeps that
    fraction of its entries and zeroes the rest (a0_of); a0_scale, lr: the start's scale and Adam's step (SPARSE_START)."""
    rng = np.random.RandomState(seed)
    dims = [nfeat] + list(widths)
    z = {"measure": np.array(measure), "weight_sup": np.array(1.0), "weight_param": np.array(weight_param, np.float64),
         "lr": np.array(float(lr)), "num_edges": np.array(1e30), "nlayer": np.array(len(widths)),
         "emb_nlayer": np.array(min(2, len(widths)) if emb_nlayer is None else int(emb_nlayer)),
         "a0_seed": np.array(7), "a0_scale": np.array(float(a0_scale))}
    g = np.float32(gain)
    for l in range(len(widths)):
        s = 1.0 / np.sqrt(dims[l + 1])
        z[f"W{l}"] = rng.uniform(-s, s, (dims[l], dims[l + 1])).astype(np.float32) * g
        z[f"b{l}"] = rng.uniform(0, s, dims[l + 1]).astype(np.float32)
    s = 1.0 / np.sqrt(widths[-1])
    z["Wlin"] = rng.uniform(-s, s, (nclass, widths[-1])).astype(np.float32) * g
    z["blin"] = rng.uniform(-s, s, nclass).astype(np.float32)
    z["features"] = (rng.rand(n, nfeat) < 0.3).astype(np.float32)
    a = (rng.rand(n, n) < 0.08).astype(np.float32)
    a = np.triu(a, 1); z["adj"] = a + a.T
    z["feature_adj"] = cora_feature_adj(z["features"])
    z["labels"] = rng.randint(0, nclass, n)
    z["idx_attack"] = rng.permutation(n)[: n - 5]
    if a0_keep is not None:
        z["a0_keep"] = np.array(float(a0_keep))
    return z


def masked_weights(z):
    """Weights of a golden / synthetic case whose embedding-layer bias kills about half of em (the bias minus the median
    of the relu output at the first step): the decode then masks pairs (S_ij <= 0), which voids the low-rank forms."""
    w = weights_from(z)
    le = cfg_from(z).emb_nlayer - 1
    probe = oracle_from(z)
    probe.step()
    w.b = [b.copy() for b in w.b]
    w.b[le] = (w.b[le] - np.quantile(probe.last["em"], 0.5, axis=0)).astype(np.float32)
    return w


# ---------------------------------------------------------------- one loss term at a time, against the float64 oracle
@contextlib.contextmanager
def oracle_precision(dtype):
    """The numpy oracle evaluates in the module global O.F32: switch it for the block only (construction and every step() of
    a float64 oracle), so the float32 oracle tests of the same process never see it."""
    old = O.F32
    O.F32 = dtype
    try:
        yield
    finally:
        O.F32 = old


class Oracle64:
    """PGDAttackOracle evaluated in float64 on a case's own (float32) inputs, as tests/golden/make_truth64.py runs it.  Between
    steps its state is rounded to float32: that is the state an engine (and the float32 oracle) can be handed exactly."""

    def __init__(self, z, weight_sup=None, weight_param=None):
        f8 = lambda x: np.asarray(x).astype(np.float64)
        w0 = weights_from(z)
        w = O.GCNWeights([f8(x) for x in w0.W], [f8(x) for x in w0.b], f8(w0.Wlin), f8(w0.blin),
                         None if w0.Ws is None else [f8(x) for x in w0.Ws], w0.act, w0.head_act)
        cfg = cfg_from(z)
        if weight_sup is not None:
            cfg.weight_sup = float(weight_sup)
        if weight_param is not None:
            cfg.weight_param = tuple(float(x) for x in weight_param)
        n = z["adj"].shape[0]
        with oracle_precision(np.float64):
            ori = f8(z["ori_adj"]) if "ori_adj" in z else np.zeros((n, n))
            self.orc = O.PGDAttackOracle(w, f8(z["features"]), f8(z["adj"]), ori, f8(z["feature_adj"]), z["labels"],
                                         z["idx_attack"], cfg)
            self.orc.w = w
            if a0_of(z) is not None:
                self.orc.set_adj_changes(f8(a0_of(z)))
        assert self.orc.HA.dtype == np.float64 and self.orc.M.dtype == np.float64

    def step(self, noise=None):
        with oracle_precision(np.float64):
            out = self.orc.step(noise=None if noise is None else np.asarray(noise, np.float64))
            assert self.orc.last["G_sym"].dtype == np.float64
            self.orc.M = self.orc.M.astype(np.float32).astype(np.float64)
        return out

    @property
    def last(self):
        return self.orc.last

    @property
    def adj_changes(self):
        """packed state, float32 (exact: step() rounds the state)"""
        r, c = O.tril_indices(self.orc.n)
        return np.ascontiguousarray(self.orc.M[r, c]).astype(np.float32)


def oracle64_from(z, weight_sup=None, weight_param=None):
    return Oracle64(z, weight_sup, weight_param)


ALL_TERMS = (0.01, 0.01, 0, 0, 0, 10, 10, 0, 10, 1000)       # synthetic_case's default weight_param
_SLOT = {"c1": 0, "c2": 1, "c6": 5, "c7": 6, "c9": 8, "c10": 9}


def _only(term):
    return tuple(ALL_TERMS[i] if i == _SLOT[term] else 0.0 for i in range(10))


# (weight_sup, weight_param) with one term switched on; "all" is the default set of every synthetic case
TERM_SETS = {"nll": (1.0, (0.0,) * 10), **{t: (0.0, _only(t)) for t in _SLOT}}
TERMS = ("nll", "c1", "c2", "c6", "c7", "c9", "c10")
FLOOR = 3e-5                                                  # the suite's path-to-path allowance
CAPS = {"HSIC": 3e-4, "CKA": 3e-4, "DP": 3e-4, "KDE": 3e-4, "MSELoss": 1e-4, "KL": 1e-4}      # the suite's oracle bounds


def term_weights(term, tiny=0.0, factor=1.0):
    """(weight_sup, weight_param) of a term set.  tiny: w1 = w2 of the sets that have no N x N HSIC term of their own (the
    fused HSIC step exists only with one: attack.hip `fused_ok`); factor scales the term's OWN weights and not `tiny` (the
    resolving-power guard hands the engine factor = 1 + 4 bound)."""
    if term == "all":
        return factor, tuple(x * factor for x in ALL_TERMS)
    ws, wp = TERM_SETS[term]
    wp = [x * factor for x in wp]
    if term not in ("c1", "c2") and tiny:
        wp[0] = wp[1] = float(tiny)
    return ws * factor, tuple(wp)


def term_bound(yardstick, measure):
    """bound = min(cap, max(float32-oracle distance, floor)): every number is the suite's own or the reference's behaviour."""
    return min(CAPS[measure], max(float(yardstick), FLOOR))


def _values(orc):
    return {"nll": float(orc.last["nll"]), **{k: float(orc.last["terms"].get(k, 0.0)) for k in _SLOT}}


def _near_clamp(o):
    """How many entries sit within 1e-6 (relative to the bound) of one of Info_entropy's clamp bounds: adj_norm (c6), and the
    off-diagonal entries of modified_adj1 (c7).  The terms' gradients jump there, so float32 and float64 may disagree on a whole
    entry's share -- one such pair of 490 000 costs 4e-5 of the c7 gradient at n = 700."""
    def near(v):
        return int(sum((np.abs(v - b) <= 1e-6 * b).sum() for b in (1e-4, 1 - 1e-4)))
    A1 = o.last["A1"]
    return near(o.last["adj_norm"]), near(A1[~np.eye(A1.shape[0], dtype=bool)])


def oracle_trajectory(z, weight_sup, weight_param, steps=2):
    """`steps` teacher-forced steps of the float64 oracle and, from the same state, of the float32 oracle.  Per step:
    a (the packed float32 state the step starts from), G64 (mirrored gradient, float64), gmax = max|G64|, d32 = max|G32 - G64| /
    gmax (0 when gmax is 0), v64 / v32 (nll and the terms' values), dead (embedding rows that are all zero) and masked
    (off-diagonal pairs the decode's relu masks: S_ij <= 0), near6 / near7 (_near_clamp), all from the float64 run."""
    o64 = Oracle64(z, weight_sup, weight_param)
    z32 = dict(z)
    z32["weight_sup"], z32["weight_param"] = np.array(float(weight_sup)), np.array(weight_param, np.float64)
    o32 = oracle_from(z32)
    out = []
    for t in range(steps):
        a = o64.adj_changes
        o32.set_adj_changes(a)
        o64.step(); o32.step()
        G64, G32 = o64.last["G_sym"], o32.last["G_sym"]
        gmax = float(np.abs(G64).max())
        em, S = o64.last["em"], o64.last["S"]
        off = ~np.eye(S.shape[0], dtype=bool)
        near6, near7 = _near_clamp(o64)
        out.append(dict(near6=near6, near7=near7, a=a, G64=G64, gmax=gmax, d32=float(np.abs(G32 - G64).max() / gmax) if gmax > 0 else 0.0,
                        finite=bool(np.isfinite(G64).all() and np.isfinite(G32).all()),
                        v64=_values(o64), v32=_values(o32), dead=int((np.abs(em).sum(1) == 0).sum()),
                        masked=int(((S <= 0) & off).sum()) // 2))
    return out


@functools.lru_cache(maxsize=64)
def _nxn_unit_gmax(spec, unit):
    """max|G_64| of the first step with w1 = w2 = unit and nothing else on (linear in unit)."""
    o = Oracle64(case_from(spec), 0.0, (unit, unit) + (0.0,) * 8)
    o.step()
    return float(np.abs(o.last["G_sym"]).max())


def is_degenerate(spec, term):
    """The (case, term) pairs whose reference gradient is exactly zero on purpose: c10 on a victim with ONE class (its softmax is
    the constant 1).  They assert exact zeros / finiteness instead of a relative error."""
    return spec[0] == "syn" and spec[4] == 1 and term == "c10"


def term_conditions(spec, term, with_tiny, unit=1e-12):
    """The conditions a term case must meet, from the float64 oracle's first step alone:
      g_term  max|G_64| with ONLY the term on: non-zero and finite, exactly zero on is_degenerate pairs          (a)
      T       w1 = w2 of the sets without an N x N term of their own when with_tiny (the fused HSIC step exists only with one:
              attack.hip `fused_ok`): the largest of 1e-12, 1e-15, ... whose N x N contribution g_tiny is at most 1e-2 of g_term.
              The oracle carries the same T, so only the engine's ERROR on that contribution (<= 3e-4 of it) reaches a comparison:
              a tenth of the floor                                                                                   (b)
      dead, masked   embedding rows that are all zero, off-diagonal pairs the decode's relu masks (S_ij <= 0)              (c)
      near6, near7   entries of adj_norm / modified_adj1 on one of Info_entropy's clamp bounds (_near_clamp): none where c6 / c7
              is the term                                                                                                (e)"""
    z = case_from(spec)
    o = Oracle64(z, *term_weights(term))
    o.step()
    G = o.last["G_sym"]
    em, S = o.last["em"], o.last["S"]
    off = ~np.eye(S.shape[0], dtype=bool)
    c = dict(g_term=float(np.abs(G).max()), finite=bool(np.isfinite(G).all()), dead=int((np.abs(em).sum(1) == 0).sum()),
             masked=int(((S <= 0) & off).sum()) // 2, T=0.0, g_tiny=0.0)
    c["near6"], c["near7"] = _near_clamp(o)
    if with_tiny and term not in ("c1", "c2", "all"):
        g_unit = _nxn_unit_gmax(spec, unit) / unit
        T = unit
        while c["g_term"] > 0 and T * g_unit > 1e-2 * c["g_term"] and T > 1e-30:
            T *= 1e-3
        c["T"], c["g_tiny"] = T, T * g_unit
    return c


def assert_term_conditions(spec, term, c, fused_subject):
    assert c["finite"], (spec, term)
    if is_degenerate(spec, term):
        assert c["g_term"] == 0.0, (spec, term, c)
    else:
        assert c["g_term"] > 0.0, ("the isolated term's reference gradient is zero: the case checks nothing", spec, term)
        assert c["g_tiny"] <= 1e-2 * c["g_term"], (spec, term, c)
    if spec[0] == "syn":
        assert c["dead"] == 0, (spec, term, c)
        if fused_subject:
            assert c["masked"] == 0, (spec, term, c)
    assert_clear_of_the_clamp(term, c)


def assert_clear_of_the_clamp(term, c):
    if term in ("c6", "c7"):
        assert c["near" + term[1]] == 0, ("an entry sits on Info_entropy's clamp bound: the term's gradient jumps there", term, c["near" + term[1]])


# the victim-shape matrix: (nfeat, widths, nclass, emb_nlayer) and what each row crosses
def victim_shapes():
    return [
        ((11, (13, 16), 5, 2), "odd first width, padded leading dimensions"),
        ((1, (5, 8), 2, 2), "nfeat = 1, narrowest decode"),
        ((1, (5, 8), 1, 2), "one class: zero supervised and c10 gradients, nothing non-finite"),
        ((7, (31, 16), 32, 2), "HSIC fc = 63 -> 64, the last fused width; C = 32, the last fused head"),
        ((7, (32, 16), 33, 2), "HSIC fc = 65: leaves the fused step; MSELoss / KL fc = 64, FP_ROWS * w = 256; C = 33: separate head kernels"),
        ((11, (16, 32), 3, 2), "he = 32"),
        ((11, (24, 8), 6, 2), "he = 8"),
        ((11, (16, 16, 16, 16), 4, 2), "summed width 64 = kmax, four backward levels"),
        ((11, (16, 16, 16, 16, 8), 4, 2), "summed width 72: not fused; general tail in three rounds of 32 columns"),
        ((11, (16, 24), 4, 1), "embedding = first layer"),
        ((11, (8, 8, 16), 4, 3), "embedding = last of three layers"),
    ]


# the general step's rank-k tail: widths rounded up to 4 and summed give 32 / 36 / 64 / 68 / 128 / 132 columns
GENERAL_WIDTHS = [(16, 16), (17, 16), (32, 32), (33, 32), (64, 64), (65, 64)]
TERM_GAIN = 0.25       # synthetic_case(gain=...) of the term cases: keeps nll, c9 and c10 alive on every shape (test_term_cases_cpu.py)


# The start of the cases of c2 and c7, the terms that go through the decode (modified_adj1 = relu(Zn Zn^T)).  From the dense start
# of the other cases every embedding row is within 1e-4 of parallel to every other (smallest off-diagonal modified_adj1 0.99997
# at n = 700, 0.999995 at n = 1100, whatever the seed or the weight scale): all of modified_adj1 sits above Info_entropy's clamp
# at 1 - 1e-4, so c7 has NO gradient, and the decode backward of c2 projects out all but 1e-3 of what it is handed (the float32
# oracle itself is 5e-4 of the term away under MSELoss).  1 % of the entries at ten times the scale spreads modified_adj1 over
# [0.58, 0.9998], clear of the clamp's bounds (a pair that crosses one between float32 and float64 flips its whole share of a
# gradient that is not continuous there), and Adam's step of 1e-4 keeps the second step's state clear of them too.
SPARSE_START = dict(a0_keep=0.01, a0_scale=0.5, lr=1e-4)


def syn_spec(n, shape, measure, gain=TERM_GAIN, start=None):
    """Hashable description of a synthetic term case: shape = (nfeat, widths, nclass, emb_nlayer), seed = n; start "sparse":
    SPARSE_START."""
    nfeat, widths, nclass, emb = shape
    assert start in (None, "sparse")
    return ("syn", int(n), int(nfeat), tuple(widths), int(nclass), int(emb), str(measure), float(gain), start)


def golden_spec(name, term):
    return ("golden", name, "sparse" if term in ("c2", "c7") else None)


def case_from(spec):
    """Inputs of a term case: ("syn", ...) from syn_spec, or ("golden", name, start) from golden_spec: the inputs of a committed
    attack fixture (the general-only victims: elu / GAT head, GraphSAGE self weights, three layers below n = 256)."""
    if spec[0] == "golden":
        z = load_case(spec[1])
        if "a0_seed" not in z:      # a fixture that starts at the origin (adj_norm = I: the entropy terms sit on their clamp): a seeded start
            z["a0_seed"], z["a0_scale"] = np.array(7), np.array(0.05)
        if spec[2] == "sparse":     # (48 and 80 nodes: 30 % of the entries)
            z["a0_keep"], z["a0_scale"], z["lr"] = np.array(0.3), np.array(SPARSE_START["a0_scale"]), np.array(SPARSE_START["lr"])
        return z
    _, n, nfeat, widths, nclass, emb, measure, gain, start = spec
    return synthetic_case(n, nfeat, widths, nclass, seed=n, measure=measure, emb_nlayer=emb, gain=gain,
                          **(SPARSE_START if start == "sparse" else {}))


def step_case(measure, n, term):
    """The case of the step-implementation tests: synthetic_case as the other oracle tests use it (11 features, widths (16, 16),
    4 classes, weight scale 1); c2 and c7, the terms that go through the decode, from SPARSE_START."""
    return syn_spec(n, (11, (16, 16), 4, 2), measure, gain=1.0, start="sparse" if term in ("c2", "c7") else None)


@functools.lru_cache(maxsize=4)
def term_case(spec, term, with_tiny, steps=2):
    """(z, conditions, (weight_sup, weight_param), trajectory) of one term set on one case (term_conditions, oracle_trajectory).
    Cached: the paths of one (case, term) share the oracle's work."""
    c = term_conditions(spec, term, with_tiny)
    ws, wp = term_weights(term, c["T"])
    return case_from(spec), c, (ws, wp), oracle_trajectory(case_from(spec), ws, wp, steps)


# ---------------------------------------------------------------- the edge-budget projection against its exact root
def exact_projection_root(a_packed, num_edges):
    """(miu*, K): the float64 root of f(x) = sum(clip(a - x, 0, 1)) = num_edges and K, the number of entries with
    0 < a - miu* < 1 (f's slope at the root is -K).  f is piecewise linear and non-increasing: float64 bisection to 1e-15 finds the
    linear piece, the piece's own equation  sum_{active} a - K x + #{a - x >= 1} = num_edges  gives the root.  The budget must
    bind (f(0) > num_edges > 0): PGDAttack.projection does not search otherwise."""
    a = np.asarray(a_packed, np.float64).ravel()
    ne = float(num_edges)
    f = lambda x: float(np.clip(a - x, 0.0, 1.0).sum())
    assert 0.0 < ne < f(0.0), ("the budget does not bind", ne, f(0.0))
    lo, hi = float(a.min()) - 1.0, float(a.max())          # f(lo) = a.size > ne, f(hi) = 0 < ne
    while hi - lo > 1e-15:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:                        # (the bracket is down to neighbouring doubles)
            break
        if f(mid) > ne:
            lo = mid
        else:
            hi = mid
    x = 0.5 * (lo + hi)
    act = (a - x > 0.0) & (a - x < 1.0)
    K = int(act.sum())
    if K == 0:                                            # a flat piece: every point of it is a root
        return x, 0
    miu = (float(a[act].sum()) + float((a - x >= 1.0).sum()) - ne) / K
    assert abs(miu - x) <= 1e-12 and abs(f(miu) - ne) <= 1e-9 * max(1.0, ne), (miu, x, f(miu), ne)
    return miu, int(((a - miu > 0.0) & (a - miu < 1.0)).sum())


def pre_projection_state(M_before, adam_m, adam_v, t, lr):
    """What Adam's step t left of the state BEFORE projection and clamp: p - step_size * (m / denom) in float32, operation by
    operation as oracle.AdamState.step ends, from the moments AFTER that step (an engine's buffer("adam_m") / buffer("adam_v")).
    M_before is the state the step started from; t counts from 1.  Every argument is packed (strict lower triangle, O.pack_tril):
    the fused step does not write the mirrored halves of the moments (fl_tail_adam: mirror_moments = 0), so only that triangle
    is Adam's state.  Returns float32."""
    f4 = np.float32
    p, m, v = (np.asarray(x, f4) for x in (M_before, adam_m, adam_v))
    assert p.ndim == m.ndim == v.ndim == 1 and p.shape == m.shape == v.shape
    bc1 = 1 - 0.9 ** int(t)
    bc2 = 1 - 0.999 ** int(t)
    step_size = float(lr) / bc1
    denom = (np.sqrt(v) / f4(np.sqrt(bc2)) + f4(1e-8)).astype(f4)
    return (p - f4(step_size) * (m / denom)).astype(f4)


# The projection cases (tests/test_gpu_projection.py; their properties: tests/test_projection_cases_cpu.py).  The start is
# uniform on [0, 1.05): about 4 % of the entries sit above 1 + lr and are above 1 after any Adam step, so a premature clamp in an
# Adam kernel -- clip(clip(a, 0, 1) - miu, 0, 1) in place of clip(a - miu, 0, 1) -- moves them by up to 0.05.
PROJ_A0_SCALE = 1.05
PROJ_BUDGETS = {"tight": 0.4, "loose": 0.95}              # num_edges = factor * sum(clip(a0, 0, 1)), float64


def projection_case(n, measure, ori=False):
    """synthetic_case as the other oracle tests use it (11 features, widths (16, 16), 4 classes, seed = n) from the start above;
    ori: ori_adj = adj, the graph itself, so that the step runs clamp(M + ori) with its gradient gate."""
    z = synthetic_case(n, 11, (16, 16), 4, seed=n, measure=measure, a0_scale=PROJ_A0_SCALE)
    if ori:
        z["ori_adj"] = z["adj"].copy()
    return z


def projection_budget(z, which):
    return PROJ_BUDGETS[which] * float(np.clip(a0_of(z).astype(np.float64), 0.0, 1.0).sum())


# id -> (n, measure, ori_adj = adj, switches): one case per Adam kernel that can run in front of the projection, at the smallest
# n that takes it (HSIC: the fused step from n = 1024, where the split product starts; 515: a ragged last 64-tile)
PROJ_CASES = {
    "fused_mse_300": (300, "MSELoss", False, {}),
    "fused_kl_300": (300, "KL", False, {}),
    "fused_hsic_1100": (1100, "HSIC", False, {}),
    "rankk_adam_hsic_300": (300, "HSIC", False, {"MCGRA_NO_FUSED_LR": "1"}),
    "rankk_adam_mse_515": (515, "MSELoss", False, {"MCGRA_NO_FUSED_LR": "1"}),
    "rankk_nt_adam_sym_300": (300, "HSIC", False, {"MCGRA_NO_FUSED_LR": "1", "MCGRA_NO_FUSED_TAIL": "1"}),
    # (below n = 256.  Not the smallest ragged size, 97: its 4656 pairs hold about 4656 * lr / 1.05 = 44 entries within lr of 0, so
    #  no step can leave the 100 entries below 0 that test_projection_cases_cpu.py asks of every MSELoss case; 161 = 2 * 64 + 33 can)
    "adam_sym_161": (161, "MSELoss", False, {}),
    "adam_sym_gate_161": (161, "MSELoss", True, {}),
}


@functools.lru_cache(maxsize=None)
def projection_oracle_pre(n, measure, ori):
    """(a0, a_pre) of a projection case on the numpy oracle: the packed start and the packed state its first Adam step leaves
    before projection and clamp (which no budget changes)."""
    z = projection_case(n, measure, ori)
    orc = oracle_from(z)
    orc.step()
    a0 = a0_of(z)
    return a0, pre_projection_state(a0, O.pack_tril(orc.adam.m), O.pack_tril(orc.adam.v), 1, float(z["lr"]))


# ---------------------------------------------------------------- the sharding rule, stated independently of the engine
def shard_rule(measure, eps, ori_np, Ws, act, head_act, loss_type, n, dims, w1, w2, num_edges, emb_nlayer=None, projection=True):
    """None when a row-block rank may run this configuration (include/mcgra.h: mcgra_attack_shard_*: a fused step covers it and
    the projection budget cannot bind), else why not.  The suite's own statement of the engine's documented create-time rule
    (csrc/attack_plan.hip: plan_attack decides; PGDAttack._replicated_reason asks it): the two are compared, never derived from
    one another.  projection=False: the rule of the fused step alone."""
    if measure not in ("HSIC", "MSELoss", "KL"):
        return f"measure {measure} (the fused HSIC, MSELoss and KL steps are the sharded ones)"
    if loss_type != "CE":
        return "loss_type 'CW' takes no step"
    if eps != 0:
        return "eps != 0 (adding_noise makes modified_adj asymmetric: general step)"
    if ori_np is not None:
        return "a non-zero ori_adj (general step)"
    if Ws is not None or act != "relu" or head_act != "none":
        return "a GAT / GraphSAGE victim (Gram evaluation of linear_HSIC)"
    split = os.environ.get("MCGRA_SPLIT_BF16", "")[:1]            # (the first character decides; 1, 2 and 3 are the split modes)
    if measure == "HSIC" and split not in ("", "1", "2", "3"):
        return f"MCGRA_SPLIT_BF16={split} (the product runs on the fp32 kernel: nothing to shard)"
    if measure == "HSIC" and n < 1024 and split == "":
        return f"n = {n} < 1024 (the product runs on the fp32 kernel: nothing to shard)"
    if n < 256:
        return f"n = {n} < 256"
    widths = [int(w) for w in dims[1:]]
    le = min(2, len(widths)) if emb_nlayer is None else int(emb_nlayer)
    he = widths[le - 1]
    if max(widths) > 32:
        return f"hidden width {max(widths)} > 32"
    if he not in (8, 16, 32):                                  # lr_decode_supported: the per-pair decode's register tiles
        return f"embedding width {he} (the per-pair decode is built for widths 8, 16 and 32)"
    hsum = sum((w + 3) & ~3 for w in widths)                   # the concatenated node buffers: rank-k depth of the tail
    if max(hsum, 2 * he) > 64:                                 # fl_tail_supported: kmax <= 64
        return (f"summed layer widths {hsum} / twice the embedding width {2 * he} > 64 (rank-k depth of the tail's "
                f"panels: e.g. more than four 16-wide layers)")
    if measure == "HSIC":
        fc = max([2 * he + 1 + widths[-1]] + [2 * w + 1 for w in widths])
    else:
        fc = max(2 * w for w in widths)
    if ((fc + 3) & ~3) > 64:
        return f"skinny products of {fc} columns > 64"
    if measure == "HSIC" and w1 == 0 and w2 == 0:
        return "w1 == w2 == 0 (no N x N HSIC term)"
    if projection and num_edges < 0.5 * float(n) * float(n):
        return "a projection budget that can bind (host-driven bisection)"
    return None


# ---------------------------------------------------------------- GPU-side helpers
def engine_from(pkg, z, device="cuda:0", measure=None, weight_param=None, **kw):
    """AttackEngine (C-ABI handle) set up from a golden attack case."""
    import torch  # noqa: F401
    cfg = cfg_from(z)
    w = weights_from(z)
    dims = [w.W[0].shape[0]] + [x.shape[1] for x in w.W]
    eng = pkg.AttackEngine(z["adj"].shape[0], dims, w.Wlin.shape[0], cfg.emb_nlayer, measure or cfg.measure,
                           cfg.weight_sup, weight_param or cfg.weight_param, cfg.lr, cfg.num_edges,
                           len(z["idx_attack"]), eps=cfg.eps, device=device, act=w.act, head_act=w.head_act,
                           has_self=w.Ws is not None, fin_layers=cfg.fin_layers, **kw)
    eng.set_model(w.W, w.b, w.Wlin, w.blin, w.Ws)
    eng.set_graph(z["features"], z["adj"], z["ori_adj"] if "ori_adj" in z else None, z["feature_adj"], z["labels"], z["idx_attack"])
    if a0_of(z) is not None:
        eng.set_adj_changes(a0_of(z))
    return eng


def shard_engines(pkg, z, world, joint=False, **kw):
    """The row-block ranks of one attack inside this process: (plans, HipShardBackends) for sharded.run_lockstep."""
    from mc_gra_amd.sharded import RowBlockPlan, HipShardBackend, lockstep_backends
    n = z["adj"].shape[0]
    plans = [RowBlockPlan(n, world, r) for r in range(world)]
    if joint:      # arenas as rows of one tensor: run_lockstep's collectives become single strided copies
        return plans, lockstep_backends([engine_from(pkg, z, plan=p, **kw) for p in plans], plans)
    return plans, [HipShardBackend(engine_from(pkg, z, plan=p, **kw), p) for p in plans]


class _Layer:
    def __init__(self, W, b):
        import torch
        self.weight = torch.tensor(np.asarray(W, np.float32))
        self.bias = torch.tensor(np.asarray(b, np.float32))


class _Lin:
    def __init__(self, W, b):
        import torch
        self.weight = torch.tensor(np.asarray(W, np.float32))
        self.bias = torch.tensor(np.asarray(b, np.float32))


class FakeGCN:
    """Duck-typed stand-in for models/gcn.py GCN / embedding_GCN: the attributes
    PGDAttack reads (gc[l].weight/.bias, linear1, nclass, nfeat, hidden_sizes, nlayer)."""

    def __init__(self, w: O.GCNWeights):
        self.gc = [_Layer(W, b) for W, b in zip(w.W, w.b)]
        self.linear1 = _Lin(w.Wlin, w.blin)
        self.nclass = w.Wlin.shape[0]
        self.nfeat = w.W[0].shape[0]
        self.hidden_sizes = [w.W[0].shape[1]]
        self.nlayer = 2

    def eval(self):
        return self

    def set_layers(self, n):
        self.nlayer = n


class _Att:
    def __init__(self, W):
        import torch
        self.W = torch.tensor(np.asarray(W, np.float32))


class FakeGAT:
    """Duck-typed models/gat.py GAT / embedding_gat: attentions[l][head].W, out_att, nlayer."""

    def __init__(self, w: O.GCNWeights, nhid=16):
        self.attentions = [[_Att(W[:, k:k + nhid]) for k in range(0, W.shape[1], nhid)] for W in w.W]
        self.out_att = _Lin(w.Wlin, w.blin)
        self.nclass, self.nfeat, self.hidden_sizes, self.nlayer = w.Wlin.shape[0], w.W[0].shape[0], [nhid], len(w.W)

    def eval(self):
        return self

    def set_layers(self, n):
        self.nlayer = n


class _SageLayer:
    def __init__(self, Ws, Wn):
        import torch
        self.weight = torch.tensor(np.vstack([Ws, Wn]).astype(np.float32))      # graphsage.py:20, [2*in, out]
        self.bias = None


class FakeSAGE:
    """Duck-typed models/graphsage.py graphsage / embedding_graphsage."""

    def __init__(self, w: O.GCNWeights):
        self.gc = [_SageLayer(a, b) for a, b in zip(w.Ws, w.W)]
        self.linear1 = _Lin(w.Wlin, w.blin)
        self.linear1.bias = None
        self.nclass, self.nfeat, self.hidden_sizes, self.nlayer = w.Wlin.shape[0], w.W[0].shape[0], [w.W[0].shape[1]], 2

    def eval(self):
        return self

    def set_layers(self, n):
        self.nlayer = n
