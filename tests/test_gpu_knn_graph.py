"""The k-nearest-neighbour graph of the scores on the device (mcgra_knn_graph, engine.knn_graph, main.py --knn / --save_knn)
against tests/knn_truth.py: every integer of the header, of the seven columns, of the lists and of the edge list compared for
equality, every double of `stats` bit for bit -- at the selection sizes where the kernels change behaviour (one word and its two
sides, 256 positions a step, each side of every row-length class), k from 1 to m - 1 and at the capacity of 1024, all-tie,
two-valued, hub, signed-zero, negative and subnormal matrices, layouts (a subset, the subset permuted, junk outside the selection,
a padded leading dimension), labels given and NULL, the capacity.  Run with -m gpu.

tests/test_knn_cases_cpu.py checks, without a GPU, that these inputs (tests/knn_cases.py) have the properties the cases are there
for and that they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import knn_cases as KC
from tests import knn_truth as T

pytestmark = pytest.mark.gpu

CASES = KC.cases()


@functools.lru_cache(maxsize=None)
def truth(name, k, labelled=True):
    """The truth of a case at one k, computed once and shared (read-only)."""
    real, pred, idx, _ = CASES[name]
    return T.ints(real if labelled else None, pred, k, idx)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda:0")                    # a copy: the cases are read-only


def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


def _same_stats(s, want, what):
    assert sorted(s) == sorted(want), what
    for key, v in want.items():
        if isinstance(v, dict):
            assert sorted(s[key]) == sorted(v) and all(_same(s[key][q], v[q]) for q in v), (what, key, s[key], v)
        else:
            assert _same(s[key], v), (what, key, s[key], v)
    for g in ("directed", "union", "mutual"):
        assert all(isinstance(s[g][q], float) for q in T.GRAPH_DOUBLES), what
    assert isinstance(s["hubness"]["skewness"], float)


def _check(got, ints, what):
    """Every integer and every double of one engine.knn_graph result (lists=True, edges=True)."""
    s = got["stats"]
    print(f"{what}: header {[got[q] for q in T.HEADER]} union f1={s['union']['f1']} mutual f1={s['mutual']['f1']} "
          f"skewness={s['hubness']['skewness']}")
    assert got["nodes"] == len(ints["in"]) and got["k"] == ints["k"]
    for q in T.HEADER:
        assert isinstance(got[q], int) and got[q] == ints[q], (what, q, got[q], ints[q])
    for q in T.COLUMNS:
        assert str(got[q].dtype) == "torch.int64" and got[q].is_cuda and got[q].tolist() == ints[q], (what, q)
    _same_stats(s, T.stats(ints), what)
    assert str(got["lists"].dtype) == "torch.int32" and np.array_equal(got["lists"].cpu().numpy(), ints["lists"]), what
    pairs, scores, kind, hits = ints["edges"]
    assert str(got["pairs_list"].dtype) == "torch.int64" and np.array_equal(got["pairs_list"].cpu().numpy(), pairs), what
    assert np.array_equal(got["scores"].cpu().numpy().view(np.uint32), scores.view(np.uint32)), what      # the bits as stored
    assert str(got["kind"].dtype) == "torch.uint8" and np.array_equal(got["kind"].cpu().numpy(), kind), what
    if hits is None:
        assert got["hits"] is None
    else:
        assert str(got["hits"].dtype) == "torch.bool" and np.array_equal(got["hits"].cpu().numpy(), hits), what
    T.check_identities({**ints, **{q: got[q] for q in T.HEADER}, **{q: got[q].tolist() for q in T.COLUMNS}})


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_knn_graph_against_the_truth(pkg, name):
    """Every integer of the entry and every double the engine forms from them, at each k, with labels; without them at one k."""
    from mc_gra_amd import engine as E
    real, pred, idx, ks = CASES[name]
    r, p, ix = _dev(real), _dev(pred), None if idx is None else _dev(idx)
    for k in ks:
        _check(E.knn_graph(p, k, ix, r, lists=True, edges=True), truth(name, k), (name, k))
    k = ks[len(ks) // 2]
    if len(pred) > 1025:                                                 # (the label-free path does not depend on the size)
        return
    bare = E.knn_graph(p, k, ix, lists=True, edges=True)
    _check(bare, truth(name, k, False), (name, k, "bare"))
    assert [bare[q] for q in T.HEADER[4:]] == [-1] * 4 and all(set(bare[q].tolist()) == {-1} for q in T.COLUMNS[3:])
    lean = E.knn_graph(p, k, ix, r)                                      # header and columns alone
    assert "lists" not in lean and "pairs_list" not in lean and all(lean[q] == truth(name, k)[q] for q in T.HEADER)
    assert all(lean[q].tolist() == truth(name, k)[q] for q in T.COLUMNS)


def test_closed_forms(pkg):
    """All ties: L_k(a) is the first k positions other than a.  A hub column: in = m - 1.  m = 2: each node lists the other."""
    from mc_gra_amd import engine as E
    real, pred, _, ks = CASES["constant"]
    m = len(pred)
    for k in ks:
        g = E.knn_graph(_dev(pred), k, None, _dev(real), lists=True)
        assert g["lists"].tolist() == [[b for b in range(m) if b != a][:k] for a in range(m)], k
    real, pred, _, _ = CASES["hub"]
    g = E.knn_graph(_dev(pred), 1, None, _dev(real), lists=True)
    m = len(pred)
    assert g["in"][17].item() == m - 1 and g["stats"]["hubness"]["max_in"] == m - 1 and g["d_U"][17].item() == m - 1
    assert all(row == [17] for a, row in enumerate(g["lists"].tolist()) if a != 17) and g["stats"]["hubness"]["skewness"] > 5
    real, pred, _, _ = CASES["q2"]
    g = E.knn_graph(_dev(pred), 1, None, _dev(real), lists=True, edges=True)
    assert g["lists"].tolist() == [[1], [0]] and (g["E_U"], g["E_M"]) == (1, 1) and g["kind"].tolist() == [3]
    assert g["pairs_list"].tolist() == [[1, 0]] and math.isnan(g["stats"]["hubness"]["skewness"])
    real, pred, _, _ = CASES["signed_zeros"]
    a = E.knn_graph(_dev(pred), 33, lists=True)["lists"]
    b = E.knn_graph(_dev(np.where(pred == 0, np.float32(0.0), pred)), 33, lists=True)["lists"]     # every zero +0.0
    assert a.tolist() == b.tolist()


def test_a_permuted_selection_permutes_the_result(pkg):
    """On tie-free scores the result for idx[perm] is the result for idx under that permutation of the positions."""
    from mc_gra_amd import engine as E
    real, pred, idx, (k,) = CASES["subset_distinct"]
    pidx = CASES["subset_distinct_permuted"][2]
    one = E.knn_graph(_dev(pred), k, _dev(idx), _dev(real), lists=True, edges=True)
    two = E.knn_graph(_dev(pred), k, _dev(pidx), _dev(real), lists=True, edges=True)
    where = {int(v): a for a, v in enumerate(idx)}
    to_one = np.array([where[int(v)] for v in pidx])                     # position in two -> position in one
    assert sorted(pidx.tolist()) == sorted(idx.tolist()) and not np.array_equal(pidx, idx)
    assert all(one[q] == two[q] for q in T.HEADER)
    for q in T.COLUMNS:
        assert np.array_equal(two[q].cpu().numpy(), one[q].cpu().numpy()[to_one]), q
    assert np.array_equal(to_one[two["lists"].cpu().numpy()], one["lists"].cpu().numpy()[to_one])
    und = lambda g: sorted(tuple(sorted(p)) for p in g["pairs_list"].tolist())
    assert und(one) == und(two)


def test_two_calls_give_identical_bits(pkg):
    from mc_gra_amd import engine as E
    for name, k in (("q129", 7), ("subset_permuted", 7), ("q1025", 64), ("two_valued", 7)):
        real, pred, idx, _ = CASES[name]
        r, p, ix = _dev(real), _dev(pred), None if idx is None else _dev(idx)
        one, two = (E.knn_graph(p, k, ix, r, lists=True, edges=True) for _ in range(2))
        assert all(one[q] == two[q] for q in T.HEADER) and all(one[q].tolist() == two[q].tolist() for q in T.COLUMNS)
        assert all(bool((one[q] == two[q]).all()) for q in ("lists", "pairs_list", "kind", "hits"))
        assert np.array_equal(one["scores"].cpu().numpy().view(np.uint32), two["scores"].cpu().numpy().view(np.uint32))
        _same_stats(one["stats"], two["stats"], name)


def test_other_dtypes_and_padded_rows(pkg):
    """float64 / bool operands and host node ids are converted as the neighbours convert them; a padded leading dimension is kept."""
    import torch
    from mc_gra_amd import engine as E
    real, pred, idx, _ = CASES["subset_permuted"]
    clean = np.nan_to_num(real, nan=0, posinf=0)
    got = E.knn_graph(_dev(pred).double(), 7, idx.tolist(), _dev(clean).bool(), lists=True, edges=True)
    _check(got, truth("subset_permuted", 7), "dtypes")
    real, pred, _, _ = CASES["q129"]
    buf = torch.full((129, 160), float("nan"), device="cuda:0")             # the padding is never read
    buf[:, :129] = _dev(pred)
    p = buf[:, :129]
    assert p.stride(0) == 160
    _check(E.knn_graph(p, 7, None, _dev(real), lists=True, edges=True), truth("q129", 7), "ld 160")


def test_knn_graph_capacity(pkg):
    """m = MCGRA_KNN_MAX_NIDX, k = 8, every node selected, tie-free rows built on the device (KC.capacity_row): 64 sampled rows of
    the lists and the first and the last against np.argpartition and a sort of the k; the other integers are recomputed on the
    host from the device's lists.  One node more: MCGRA_ENOSUP before any device work."""
    import torch
    from mc_gra_amd import engine as E
    n, k = KC.MAX_NIDX, 8
    b = torch.arange(n, device="cuda:0", dtype=torch.int64)
    pred = ((7919 * b[None, :] + 104729 * b[:, None]) % 16411).to(torch.float32)
    g = E.knn_graph(pred, k, lists=True)
    L = g["lists"].cpu().numpy()
    rows = sorted(set([0, n - 1] + np.random.RandomState(1).randint(0, n, 64).tolist()))
    for a in rows:
        s = KC.capacity_row(a).astype(np.float32)
        assert len(np.unique(np.delete(s, a))) == n - 1
        s[a] = -1.0                                                      # below every candidate
        top = np.argpartition(-s, k - 1)[:k]
        assert L[a].tolist() == top[np.argsort(-s[top])].tolist(), a
    want = T.ints_from_lists(L, n)
    assert (g["pairs"], g["k"], g["E_U"], g["E_M"]) == (n * (n - 1) // 2, k, want["E_U"], want["E_M"])
    assert [g[q] for q in T.HEADER[4:]] == [-1] * 4
    for q in ("in", "d_U", "d_M"):
        assert g[q].tolist() == want[q], q
    T.check_identities({**{q: g[q] for q in T.HEADER}, **{q: g[q].tolist() for q in T.COLUMNS}})
    with pytest.raises(pkg._lib.McgraNotSupported, match=str(n)):
        E.knn_graph(torch.zeros(1, 1, device="cuda:0").expand(n + 1, n + 1), k)


# ------------------------------------------------------------------------------------------------ 2. the edge list, refusals
def _raw(pkg, real, pa, k, idx=None, cap=None, lists=True, mark=-7):
    """The C entry with every output pre-filled with `mark`: (rc, error text, header, out, lists, pairs, scores, kind, hits)."""
    import torch
    L = pkg._lib.lib
    n = len(pa)
    r, a = None if real is None else _dev(real), _dev(pa)
    ix = None if idx is None else _dev(np.asarray(idx, np.int64))
    rows = n if idx is None else len(idx)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    cap = rows * k if cap is None else cap
    hd = (ctypes.c_int64 * 8)(*([mark] * 8))
    out = torch.full((rows, 7), mark, device="cuda:0", dtype=torch.int64)
    nn = torch.full((rows, k), mark, device="cuda:0", dtype=torch.int32) if lists else None
    pairs = torch.full((max(cap, 1), 2), mark, device="cuda:0", dtype=torch.int64)
    scores = torch.full((max(cap, 1),), float(mark), device="cuda:0", dtype=torch.float32)
    kind = torch.full((max(cap, 1),), 200, device="cuda:0", dtype=torch.uint8)
    hits = torch.full((max(cap, 1),), 200, device="cuda:0", dtype=torch.uint8) if real is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mcgra_knn_graph(stream, n, p(a), n, p(r), n, p(ix), rows, k, hd, p(out), p(nn), cap, p(pairs), p(scores), p(kind),
                           p(hits))
    return rc, L.mcgra_last_error().decode(), list(hd), out, nn, pairs, scores, kind, hits


def _untouched(res, mark=-7):
    _, _, hd, out, nn, pairs, scores, kind, hits = res
    return (hd == [mark] * 8 and bool((out == mark).all()) and (nn is None or bool((nn == mark).all()))
            and _buffers_untouched(res, mark))


def _buffers_untouched(res, mark=-7):
    _, _, _, _, _, pairs, scores, kind, hits = res
    return (bool((pairs == mark).all()) and bool((scores == mark).all()) and bool((kind == 200).all())
            and (hits is None or bool((hits == 200).all())))


def test_edge_list_capacity(pkg):
    """cap = E_U exactly: the list; one below: MCGRA_ENOMEM, the header written, nothing in the buffers; cap == 0 with a buffer
    the same; cap == 0 with pairs NULL: no list, rc 0."""
    real, pred, _, _ = CASES["q65"]
    want = truth("q65", 7)
    E_U = want["E_U"]
    res = _raw(pkg, real, pred, 7, cap=E_U)
    assert res[0] == 0 and res[2] == [want[q] for q in T.HEADER]
    assert np.array_equal(res[5].cpu().numpy(), want["edges"][0]) and np.array_equal(res[7].cpu().numpy(), want["edges"][2])
    assert np.array_equal(res[8].cpu().numpy().astype(bool), want["edges"][3])
    assert np.array_equal(res[4].cpu().numpy(), want["lists"]) and res[3].t().tolist() == [want[q] for q in T.COLUMNS]
    for cap in (E_U - 1, 0):
        res = _raw(pkg, real, pred, 7, cap=cap)
        assert res[0] == -4 and str(E_U) in res[1] and "knn_graph" in res[1], res[:2]
        assert res[2] == [want[q] for q in T.HEADER] and _buffers_untouched(res)
    L = pkg._lib.lib
    import torch
    hd = (ctypes.c_int64 * 8)()
    out = torch.zeros(65, 7, device="cuda:0", dtype=torch.int64)
    p = _dev(pred)
    rc = L.mcgra_knn_graph(None, 65, ctypes.c_void_p(p.data_ptr()), 65, None, 0, None, 65, 7, hd, ctypes.c_void_p(out.data_ptr()),
                           None, 0, None, None, None, None)
    assert rc == 0 and list(hd)[:4] == [want[q] for q in T.HEADER[:4]] and out[:, 0].tolist() == want["in"]


def test_device_refusals_leave_the_outputs_untouched(pkg):
    """A NaN or infinite candidate score, a label of 0.5, a repeated id, an id out of range: MCGRA_EINVAL, the cause named, and
    not one word of any output written; the same entries on the diagonal and in unselected rows and columns are not looked at."""
    rng = np.random.RandomState(5)
    n = 70
    real, pa = KC.graph(rng, n, 0.2), rng.rand(n, n).astype(np.float32)

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    ok = _raw(pkg, real, pa, 5)
    assert ok[0] == 0 and -7 not in ok[2] and not bool((ok[3] == -7).any()) and not bool((ok[4] == -7).any())
    for value in (np.nan, np.inf, -np.inf):
        for where in ((40, 7), (7, 40)):                                  # a row is ranked whole: both triangles are candidates
            res = _raw(pkg, real, bad(pa, value, where), 5)
            assert res[0] == -1 and "NaN or infinite" in res[1] and "knn_graph" in res[1] and _untouched(res), (value, where)
        res = _raw(pkg, None, bad(pa, value), 5)
        assert res[0] == -1 and "NaN or infinite" in res[1] and _untouched(res)
    for value in (0.5, np.nan, 2.0):
        res = _raw(pkg, bad(real, value), pa, 5)
        assert res[0] == -1 and "label" in res[1] and _untouched(res)
    assert _raw(pkg, bad(real, 0.5, (7, 40)), pa, 5)[0] == 0                # G reads the strict lower triangle
    assert _raw(pkg, bad(real, 0.5, (9, 9)), bad(pa, np.nan, (9, 9)), 5)[0] == 0     # the diagonal is not looked at
    res = _raw(pkg, bad(real, 0.5), bad(pa, np.nan), 3, [3, 41, 7, 12, 60])          # an unselected row
    assert res[0] == 0 and res[2][0] == 10
    res = _raw(pkg, real, bad(pa, np.nan), 3, [3, 7, 40, 12, 60])
    assert res[0] == -1 and "NaN or infinite" in res[1] and _untouched(res)
    res = _raw(pkg, real, pa, 3, [3, 9, 4, 9, 12])
    assert res[0] == -1 and "twice" in res[1] and _untouched(res)
    for ids in ([3, 9, n], [3, -1, 5]):
        res = _raw(pkg, real, pa, 2, ids)
        assert res[0] == -1 and "outside" in res[1] and _untouched(res)


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = KC.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.knn_graph(_dev(nan), 3, None, _dev(real))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.knn_graph(_dev(pa), 1, [1, 2, 1])
    for k in (0, -1, n):
        with pytest.raises(pkg._lib.McgraError, match="k = "):
            E.knn_graph(_dev(pa), k, edges=True, lists=True)
    with pytest.raises(pkg._lib.McgraError):
        E.knn_graph(_dev(pa), 1, [4])                                     # fewer than two nodes


# ------------------------------------------------------------------------------------------------------ 3. main.py
def test_main_evaluate_knn_and_save_knn(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --knn 0 adds the knn_* dicts,
    each the truth on the matrices that were scored at the set's own mean true degree; global_f1_* is engine.topk_metrics called
    directly; --save_knn writes the columns of each set and the whole graph's union; a run without the flags returns and logs
    what it did before the flags existed."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt", "--save_scores", str(tmp_path / "plain.npy")])
    assert not any(hasattr(plain_args, q) for q in ("knn", "save_knn"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.knn_graph

    def record(pred, k, idx=None, real=None, lists=False, edges=False):
        v = orig(pred, k, idx, real, lists=lists, edges=edges)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx), k, v))
        return v

    monkeypatch.setattr(M.engine, "knn_graph", record)
    path = str(tmp_path / "knn.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "knn.txt", "--knn", "0", "--save_knn", path, "--save_scores",
                                                    str(tmp_path / "knn.npy")]))
    out = capsys.readouterr().out
    sets = ("attack", "train", "all")
    assert sorted(res) == sorted(list(plain) + [f"knn_{s}" for s in sets]) and len(seen) == 4      # three sets and the save
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    assert np.array_equal(np.load(tmp_path / "plain.npy").view(np.uint32), np.load(tmp_path / "knn.npy").view(np.uint32))
    saved = np.load(path)
    assert sorted(saved.files) == sorted([f"{q}_{s}" for q in ("nodes", "k") + T.COLUMNS for s in sets]
                                         + ["pairs", "scores", "kind", "hits"])
    for (real, pred, idx, k, v), name in zip(seen, sets):
        d = res[f"knn_{name}"]
        m = 1190 if idx is None else len(idx)
        ints = T.ints(real, pred, k, idx)
        assert sorted(d) == sorted(["stats", "k", "nodes", "pairs", "positives", "global_f1_union", "global_f1_mutual", "columns"])
        assert d["positives"] == ints["E_G"] > 0 and k == T.k_of_mean_degree(m, ints["E_G"]) == d["k"] and d["nodes"] == m
        assert d["pairs"] == m * (m - 1) // 2 and all(v[q] == ints[q] for q in T.HEADER)
        _same_stats(d["stats"], T.stats(ints), name)
        for which, E_X in (("union", ints["E_U"]), ("mutual", ints["E_M"])):
            direct = M.engine.topk_metrics(_dev(real), _dev(pred), E_X, idx)["f1"]
            assert _same(d[f"global_f1_{which}"], direct) and E_X > 0, (name, which)
        assert np.array_equal(saved[f"nodes_{name}"], np.arange(1190) if idx is None else idx) and int(saved[f"k_{name}"]) == k
        for q in T.COLUMNS:
            assert saved[f"{q}_{name}"].dtype == np.int64 and saved[f"{q}_{name}"].tolist() == ints[q], (q, name)
    real, pred, idx, k, v = seen[3]
    pairs, scores, kind, hits = T.ints(real, pred, k, None)["edges"]
    assert idx is None and k == res["knn_all"]["k"] and np.array_equal(saved["pairs"], pairs) and np.array_equal(saved["kind"], kind)
    assert np.array_equal(saved["scores"].view(np.uint32), scores.view(np.uint32)) and np.array_equal(saved["hits"], hits)
    d = res["knn_all"]
    q = d["stats"]
    u, mu, hub = q["union"], q["mutual"], q["hubness"]
    line = (f"k={d['k']} union f1={u['f1']} (edges={u['edges']}, isolated={u['isolated']}; global f1={d['global_f1_union']}) "
            f"mutual f1={mu['f1']} (edges={mu['edges']}, isolated={mu['isolated']}; global f1={d['global_f1_mutual']}) "
            f"max_in={hub['max_in']} orphans={hub['orphans']} skew={hub['skewness']}")
    assert f"current auc={res['auc_all']}\ncurrent knn {line}\n" in out and "current knn" not in out_plain
    log = open(tmp_path / "results" / "knn.txt").read().split("\n")
    for i, (title, name) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        assert log[2 + i] == R._knn_log(res, None)[i] and log[2 + i].startswith(f"In {title}: knn k={res[f'knn_{name}']['k']} union f1=")
    assert log[2 + 2].startswith(f"In Whole Graph: knn {line} | nodes=1190 positives=")
    assert log[5].startswith("current density:") and "knn=0" in log[0] and "save_knn=" in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert " knn=" not in old and "save_knn=" not in old and ": knn " not in old and old.count("\n") == 3 and old.split("\n")[1:] == log[1:2] + log[5:]
    # K >= 1 is used as given, clamped to the set's size less one
    seen.clear()
    M.run(M.build_parser().parse_args(argv + ["--log_name", "k5.txt", "--knn", "5"]))
    capsys.readouterr()
    assert [s[3] for s in seen] == [5, 5, 5]
