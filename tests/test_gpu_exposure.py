"""The exposure of the true edges on the device (mcgra_edge_exposure, engine.edge_exposure, main.py --exposure / --exposure_cut /
--save_exposure) against tests/exposure_truth.py: the header, all 768 table integers, every per-edge column and every double
compared for equality, twice with the same bits, and again under a permuted idx -- at the smallest selections where the kernels
change behaviour (one word, two words, the diagonal tile, the pad bits, one row more than the grid of the row passes, more
edges than the waves of the edge pass and than the staged samples), graphs (empty, complete, one edge, a star, cliques of 17 and
18, two cliques and a bridge, a path), scores (all equal, two values, signed zeros and subnormals, negative), layouts (n > m
with a permuted idx and padded rows), the capacities of the columns, the refusals, and the capacity.  Run with -m gpu.

tests/test_exposure_cases_cpu.py checks, without a GPU, that these inputs (tests/exposure_cases.py) have the properties the
cases are there for and that they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import lzma
import os

import numpy as np
import pytest

from tests import exposure_cases as XC
from tests import exposure_truth as T
from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = XC.cases()


@functools.lru_cache(maxsize=None)
def truth(name, thr):
    """The truth of one run of a case, computed once (read-only)."""
    real, pred, idx, _, _ = CASES[name]
    return T.ints(real, pred, idx, thr)


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x, pad=0):
    """A device copy (the cases are read-only); pad > 0: the rows of a buffer that many columns wider, the padding NaN."""
    import torch
    t = torch.as_tensor(np.array(x), device="cuda:0")
    if not pad:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda:0", dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    view = buf[:, :t.shape[1]]
    assert view.stride(0) == t.shape[1] + pad
    return view


def _circulant_on_device(n):
    """tests/exposure_cases.py's circulant(n) built on the device in row blocks."""
    import torch
    both = torch.empty(n, n, device="cuda:0", dtype=torch.float32)
    cols = torch.arange(n, device="cuda:0", dtype=torch.int32)[None, :]
    for r0 in range(0, n, 4096):
        rows = torch.arange(r0, min(n, r0 + 4096), device="cuda:0", dtype=torch.int32)[:, None]
        d = (rows - cols) % n
        both[r0:r0 + 4096] = ((d == 1) | (d == 2) | (d == n - 1) | (d == n - 2)).to(torch.float32)
    return both


def _mirrored(mat, idx):
    """mat with the selected strict lower triangle copied above the diagonal: what any order of the same nodes reads."""
    out = np.array(mat)
    ix = np.arange(len(out)) if idx is None else np.asarray(idx, np.int64)
    a, b = np.tril_indices(len(ix), -1)
    out[ix[b], ix[a]] = out[ix[a], ix[b]]
    return out


def _columns(d):
    return {q: d[q].cpu().numpy() for q in T.COLUMNS}


def _rows(cols):
    """The edge list as a sorted list of rows, each with its smaller node id first (and that node's degree first)."""
    out = []
    for (u, v), s, p, c, (du, dv) in zip(cols["pairs_list"].tolist(), cols["scores"].view(np.uint32).tolist(), cols["placement"].tolist(),
                                         cols["common"].tolist(), cols["deg"].tolist()):
        out.append((u, v, s, p, c, du, dv) if u < v else (v, u, s, p, c, dv, du))
    return sorted(out)


def _check(got, want, what):
    """One result of engine.edge_exposure (edges=True) against the truth's dict: integers, columns, doubles."""
    assert got["ints"] == want["header"] and got["table"] == T.as_tuples(want["table"]), what
    assert [got[k] for k in T.HEADER] == want["header"]
    for q, col in _columns(got).items():
        assert col.dtype == want[q].dtype and col.shape == want[q].shape, (what, q, col.dtype, col.shape)
        assert np.array_equal(col.view(np.uint32) if q == "scores" else col, want[q].view(np.uint32) if q == "scores" else want[q]), (what, q)
    assert T.same(got["stats"], T.stats(want["header"], want["table"])), what


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_exposure_against_the_truth(pkg, name):
    """Every integer of the entry, every column and every double the engine forms from them, at each threshold of the case, on
    two calls; then the same nodes in another order: the same header and table, the same set of rows."""
    from mc_gra_amd import engine as E
    real, pred, idx, pad, thresholds = CASES[name]
    r, p, ix = _dev(real, pad), _dev(pred, pad), None if idx is None else _dev(idx)
    for thr in thresholds:
        want = truth(name, thr)
        one, two = E.edge_exposure(r, p, ix, thr, edges=True), E.edge_exposure(r, p, ix, thr, edges=True)
        print(f"{name} threshold={thr}: {one['ints']} pooled={one['stats']['auc_pooled']} "
              f"by common neighbours={[c for c in one['stats']['by_embeddedness']['count']]}")
        assert one["threshold"] == (None if thr is None else float(thr))
        _check(one, want, (name, thr))
        assert two["ints"] == one["ints"] and two["table"] == one["table"] and T.same(two["stats"], one["stats"])
        for q, col in _columns(two).items():
            assert np.array_equal(col.view(np.uint32) if q == "scores" else col,
                                  one[q].cpu().numpy().view(np.uint32) if q == "scores" else one[q].cpu().numpy()), (name, q)
        plain = E.edge_exposure(r, p, ix, thr)                                     # the integers alone
        assert plain["ints"] == one["ints"] and plain["table"] == one["table"] and not set(T.COLUMNS) & set(plain)
    thr = thresholds[0]
    want = truth(name, thr)
    rng = np.random.RandomState(len(name))
    nodes = np.arange(len(real)) if idx is None else idx
    rs, ps = _dev(_mirrored(real, idx), pad), _dev(_mirrored(pred, idx), pad)
    for _ in range(2):
        got = E.edge_exposure(rs, ps, _dev(rng.permutation(nodes)), thr, edges=True)
        assert got["ints"] == want["header"] and got["table"] == T.as_tuples(want["table"]), name
        assert _rows(_columns(got)) == _rows({q: want[q] for q in T.COLUMNS}), name


@pytest.mark.parametrize("name", ["m129", "sub65", "two_cliques_bridge", "sparse_sub1025", "dense_n200"])
def test_the_sums_are_delongs_and_the_cut_is_threshold_pairs(pkg, name):
    """{m, P, N, T} are mcgra_auc_delong's on the same input and auc_pooled its auc bit for bit; above_* are
    mcgra_threshold_pairs' pairs by label; the pooled AUC is the mean of the class AUCs weighted by their shares."""
    from mc_gra_amd import engine as E
    real, pred, idx, pad, thresholds = CASES[name]
    r, p, ix = _dev(real, pad), _dev(pred, pad), None if idx is None else _dev(idx)
    dl = E.auc_delong(r, p, ix)
    d = E.edge_exposure(r, p, ix, thresholds[0])
    assert d["ints"][:4] == [dl["pairs"], dl["positives"], dl["negatives"], dl["ints"]["T"]] and d["stats"]["auc_pooled"] == dl["auc"]
    _, _, hits = E.threshold_pairs(p, thresholds[0], ix, r)
    assert (d["above_pos"], d["above_neg"]) == (int(hits.sum()), int((~hits).sum()))
    for mg in (d["stats"]["by_embeddedness"], d["stats"]["by_degree"]):
        assert abs(sum(a * w for a, w in zip(mg["auc"], mg["share"]) if w > 0) - dl["auc"]) < 1e-12
    none = E.edge_exposure(r, p, ix)
    assert none["threshold"] is None and (none["above_pos"], none["above_neg"]) == (0, 0) and none["ints"][:4] == d["ints"][:4]


def test_other_dtypes_and_host_node_ids(pkg):
    """float64 / bool operands and a list of node ids are converted as the neighbours convert them."""
    from mc_gra_amd import engine as E
    real, pred, idx, _, _ = CASES["sub65"]
    got = E.edge_exposure(_dev(np.nan_to_num(real, nan=0)).bool(), _dev(np.nan_to_num(pred, nan=0)).double(), idx.tolist(), -1.25, edges=True)
    _check(got, truth("sub65", -1.25), "sub65")


# ------------------------------------------------------------------------------------- 2. the capacity of the columns
def test_cap_zero_short_exact_and_long(pkg):
    """cap = 0: the integers alone; cap = P - 1: MCGRA_ENOMEM, header and table filled, not one word of the columns written;
    cap = P: the rows; cap = P + 3: the rows, the tail untouched."""
    import torch
    L = pkg._lib.lib
    real, pred, idx, pad, thresholds = CASES["sub129"]
    want = truth("sub129", thresholds[0])
    P = want["header"][1]
    assert P > 8
    r, p, ix = _dev(real, pad), _dev(pred, pad), _dev(idx)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    mark = -7

    def run(cap, with_columns=True):
        rows = max(cap, 1)
        cols = [torch.full((rows, 2), mark, device="cuda:0", dtype=torch.int64), torch.full((rows,), float(mark), device="cuda:0"),
                torch.full((rows,), mark, device="cuda:0", dtype=torch.int64), torch.full((rows,), mark, device="cuda:0", dtype=torch.int32),
                torch.full((rows, 2), mark, device="cuda:0", dtype=torch.int32)] if with_columns else [None] * 5
        hd, tb = (ctypes.c_int64 * 6)(*([mark] * 6)), (ctypes.c_int64 * 768)(*([mark] * 768))
        rc = L.mcgra_edge_exposure(stream, len(real), ptr(r), r.stride(0), ptr(p), p.stride(0), ptr(ix), len(idx), thresholds[0], cap,
                                   *(ptr(c) for c in cols), hd, tb)
        return rc, L.mcgra_last_error().decode(), list(hd), list(tb), [None if c is None else c.cpu().numpy() for c in cols]

    flat = [v for row in want["table"] for cell in row for v in cell]
    rc, _, hd, tb, _ = run(0, False)
    assert rc == 0 and hd == want["header"] and tb == flat
    rc, e, hd, tb, cols = run(P - 1)
    assert rc == -4 and "edge_exposure" in e and str(P) in e and f"cap = {P - 1}" in e and hd == want["header"] and tb == flat
    assert all((c == mark).all() for c in cols)
    for cap in (P, P + 3):
        rc, _, hd, tb, cols = run(cap)
        assert rc == 0 and hd == want["header"] and tb == flat
        for c, q in zip(cols, T.COLUMNS):
            assert np.array_equal(c[:P], want[q]) and (c[P:] == mark).all() and len(c) == cap, (cap, q)
    only = [torch.full((P, 2), mark, device="cuda:0", dtype=torch.int64)]
    hd2, tb2 = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 768)()                  # pairs alone: the other columns may be NULL
    assert L.mcgra_edge_exposure(stream, len(real), ptr(r), r.stride(0), ptr(p), p.stride(0), ptr(ix), len(idx), thresholds[0], P,
                                 ptr(only[0]), None, None, None, None, hd2, tb2) == 0
    assert np.array_equal(only[0].cpu().numpy(), want["pairs_list"]) and list(hd2) == hd and list(tb2) == tb


# ------------------------------------------------------------------------------------------------ 3. the refusals
def test_device_refusals_leave_every_output_untouched(pkg):
    """A NaN or infinite score, a label of 0.5, a repeated id, an id out of range: MCGRA_EINVAL, the cause named, and not one
    word of header, table or the columns written; the same entries outside the selected triangle are not looked at."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n = 70
    real, pa = XC.graph(rng, n, 0.05), rng.rand(n, n).astype(np.float32)
    mark = -7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cap = n * (n - 1) // 2

    def run(real, pa, idx=None, thr=0.5):
        r, a = _dev(real), _dev(pa)
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        rows = n if idx is None else len(idx)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        cols = [torch.full((cap, 2), mark, device="cuda:0", dtype=torch.int64), torch.full((cap,), float(mark), device="cuda:0"),
                torch.full((cap,), mark, device="cuda:0", dtype=torch.int64), torch.full((cap,), mark, device="cuda:0", dtype=torch.int32),
                torch.full((cap, 2), mark, device="cuda:0", dtype=torch.int32)]
        hd, tb = (ctypes.c_int64 * 6)(*([mark] * 6)), (ctypes.c_int64 * 768)(*([mark] * 768))
        rc = L.mcgra_edge_exposure(stream, n, p(r), n, p(a), n, p(ix), rows, thr, cap, *(p(c) for c in cols), hd, tb)
        clean = list(hd) == [mark] * 6 and list(tb) == [mark] * 768 and all(bool((c == mark).all()) for c in cols)
        return rc, L.mcgra_last_error().decode(), clean, list(hd)

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    rc, _, clean, hd = run(real, pa)
    assert rc == 0 and not clean and hd[0] == n * (n - 1) // 2 and hd[1] > 0
    for value in (np.nan, np.inf, -np.inf):
        for thr in (0.5, float("inf"), -float("inf")):                       # whatever the threshold decides about the entry
            rc, e, clean, _ = run(real, bad(pa, value), None, thr)
            assert rc == -1 and "NaN or infinite" in e and "edge_exposure" in e and clean
    for value in (0.5, np.nan, 2.0):
        rc, e, clean, _ = run(bad(real, value), pa)
        assert rc == -1 and "label" in e and clean
    # the same invalid entries above the diagonal, on it, and in unselected rows and columns are not looked at
    assert run(bad(real, 0.5, (7, 40)), bad(pa, np.nan, (7, 40)))[0] == 0
    assert run(bad(real, 0.5, (9, 9)), bad(pa, np.inf, (9, 9)))[0] == 0
    rc, _, _, hd = run(bad(real, 0.5), bad(pa, np.nan), [3, 41, 7, 12, 60])
    assert rc == 0 and hd[0] == 10
    rc, e, clean, _ = run(real, bad(pa, np.nan), [3, 7, 40, 12, 60])          # node 40 at position 2, node 7 at 1: [40][7] is read
    assert rc == -1 and "NaN or infinite" in e and clean
    assert run(real, bad(pa, np.nan), [3, 40, 7, 12, 60])[0] == 0             # node 7 at position 2, node 40 at 1: [7][40] is read
    rc, e, clean, _ = run(real, pa, [3, 9, 4, 9, 12])
    assert rc == -1 and "twice" in e and clean
    for ids in ([3, 9, n], [3, -1, 5]):
        rc, e, clean, _ = run(real, pa, ids)
        assert rc == -1 and "outside" in e and clean
    rc, e, clean, _ = run(real, pa, None, float("nan"))
    assert rc == -1 and "NaN" in e and clean


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = XC.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.edge_exposure(_dev(real), _dev(nan))
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.edge_exposure(_dev(real), _dev(pa), None, float("nan"))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.edge_exposure(_dev(real), _dev(pa), [1, 2, 1], edges=True)
    with pytest.raises(pkg._lib.McgraError):
        E.edge_exposure(_dev(real), _dev(pa), [4])                            # fewer than two nodes


# ------------------------------------------------------------------------------------------------ 4. the capacity
def _closed_form(n, what):
    from mc_gra_amd import engine as E
    both = _circulant_on_device(n)
    one, two = E.edge_exposure(both, both, None, 0.5, edges=True), E.edge_exposure(both, both, None, 0.5)
    header, table = T.circulant_ints(n)
    print(f"{what}: {one['ints']}")
    assert one["ints"] == header and one["table"] == T.as_tuples(table) and T.same(one["stats"], T.stats(header, table))
    assert two["ints"] == one["ints"] and two["table"] == one["table"]
    N, cols = header[2], _columns(one)
    a, b = cols["pairs_list"][:, 0], cols["pairs_list"][:, 1]
    off = np.minimum(a - b, n - (a - b))
    assert (a > b).all() and set(off.tolist()) == {1, 2} and len(a) == 2 * n
    packed = a * (a - 1) // 2 + b
    assert (np.diff(packed) > 0).all()                                           # ascending packed position
    assert (cols["placement"] == 2 * N).all() and (cols["deg"] == 4).all() and (cols["scores"] == 1).all()
    assert np.array_equal(cols["common"], np.where(off == 1, 2, 1))
    assert one["stats"]["auc_pooled"] == 1.0 and one["stats"]["by_embeddedness"]["auc"][1:3] == (1.0, 1.0)


def test_several_words_a_lane(pkg):
    """n_idx = 64 * 130 + 1: 131 words per row, three for some lanes of a wave.  The circulant graph of the capacity case and its
    closed form (held to the numpy truth at small n by the CPU tests)."""
    _closed_form(64 * 130 + 1, "W = 131")


def test_edge_exposure_capacity(pkg):
    """n_idx = 65 535, every node selected, built on the device in row blocks: the circulant graph of offsets +-1, +-2 as scores
    and labels at once, threshold 0.5.  1024 words per row, 524 800 tiles, matrix offsets up to 2^32, T up to 2^49."""
    import torch
    n = XC.MAX_NIDX
    need = 4 * n * n + 8 * n * ((n + 63) // 64) + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the capacity case needs {need / 2 ** 30:.1f} GiB of device memory (a 17 GB matrix and a 0.5 GB bit matrix); "
                    f"{free / 2 ** 30:.1f} GiB are free")
    assert n * n > 2 ** 31
    _closed_form(n, "capacity")


# ------------------------------------------------------------------------------------------------------ 5. main.py
def test_main_evaluate_exposure_and_save_exposure(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed cora file, 6 epochs of its README line with --ci: --exposure adds the exposure_*
    dicts, each the truth on the matrices that were scored, cut at the score of the set's P-th best pair; auc_pooled is --ci's
    auc; --save_exposure writes the tables and the whole graph's edges, the arrays of a second direct call; a run without the
    flags returns and logs what it did before the flags existed."""
    from mc_gra_amd import main as M
    monkeypatch.chdir(tmp_path)
    root = tmp_path / "dataset"                     # cora.npz is committed as an xz archive of the reference's file
    root.mkdir()
    with lzma.open(os.path.join(H.GOLDEN, "dataset", "cora.npz.xz")) as src:
        (root / "cora.npz").write_bytes(src.read())
    argv = ["--dataset", "cora", "--dataset_root", str(root), "--epochs", "6", "--w1", "0.01", "--w6", "10", "--w7", "10", "--w9", "10",
            "--w10", "1000", "--lr", "-2", "--useH_A", "--useY_A", "--useY", "--measure", "MSELoss", "--ci"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt", "--save_scores", str(tmp_path / "plain.npy")])
    assert not any(hasattr(plain_args, k) for k in ("exposure", "exposure_cut", "save_exposure"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    seen = []
    orig = M.engine.edge_exposure

    def record(real, pred, idx=None, threshold=None, edges=False):
        v = orig(real, pred, idx, threshold, edges)
        if not edges:
            seen.append((real, pred, None if idx is None else np.asarray(idx), threshold, v))
        return v

    monkeypatch.setattr(M.engine, "edge_exposure", record)
    path = str(tmp_path / "exposure.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "exp.txt", "--exposure", "--save_exposure", path,
                                                    "--save_scores", str(tmp_path / "exp.npy")]))
    out = capsys.readouterr().out
    sets = ("attack", "train", "all")
    assert sorted(res) == sorted(list(plain) + [f"exposure_{s}" for s in sets]) and len(seen) == 3
    for key in plain:
        if key != "path":
            assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    assert np.array_equal(np.load(tmp_path / "plain.npy"), np.load(tmp_path / "exp.npy"))          # modified_adj too
    saved = np.load(path)
    assert sorted(saved.files) == sorted([f"{k}_{s}" for k in ("nodes", "table", "threshold") for s in sets] +
                                         ["pairs", "scores", "placement", "common", "deg"])
    real_h, pred_h = seen[0][0].cpu().numpy(), seen[0][1].cpu().numpy()
    for (real, pred, idx, thr, v), name in zip(seen, sets):
        assert res[f"exposure_{name}"] is v
        want = T.ints(real_h, pred_h, idx, thr)
        assert v["ints"] == want["header"] and v["table"] == T.as_tuples(want["table"]), name
        assert T.same(v["stats"], T.stats(want["header"], want["table"])), name
        s = np.sort(pred_h[np.tril_indices(len(pred_h), -1)] if idx is None else pred_h[idx][:, idx][np.tril_indices(len(idx), -1)])[::-1]
        assert v["positives"] > 0 and thr == float(s[v["positives"] - 1])               # --exposure_cut defaults to `edges`
        assert v["stats"]["auc_pooled"] == res[f"ci_{name}"]["auc"]                      # auc_pairs of --ci
        assert saved[f"table_{name}"].dtype == np.int64 and saved[f"table_{name}"].tolist() == [[list(c) for c in row] for row in v["table"]]
        assert saved[f"threshold_{name}"].dtype == np.float32 and float(saved[f"threshold_{name}"]) == thr
        assert np.array_equal(saved[f"nodes_{name}"], np.arange(len(pred_h)) if idx is None else idx)
    again = orig(seen[2][0], seen[2][1], None, seen[2][3], edges=True)                    # a second direct call
    want = T.ints(real_h, pred_h, None, seen[2][3])
    for k, q in (("pairs", "pairs_list"), ("scores", "scores"), ("placement", "placement"), ("common", "common"), ("deg", "deg")):
        assert np.array_equal(saved[k], again[q].cpu().numpy()) and np.array_equal(saved[k], want[q]) and saved[k].dtype == want[q].dtype, k
    d = res["exposure_all"]
    q = d["stats"]
    by = lambda mg: " ".join(f"{k}:{a}" for k, c, a in zip(mg["names"], mg["count"], mg["auc"]) if c)
    line = f"current exposure by common neighbours {by(q['by_embeddedness'])} (pooled {q['auc_pooled']}) | by min degree {by(q['by_degree'])}\n"
    assert line in out and out.index("current auc_pairs=") < out.index(line) and "exposure" not in out_plain
    print(line)
    log = open(tmp_path / "results" / "exp.txt").read().split("\n")
    for i, (title, key) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        d = res[f"exposure_{key}"]
        assert log[5 + i].startswith(f"In {title}: exposure at {d['threshold']}: edges={d['positives']} recall={d['stats']['recall']} "
                                     f"precision={d['stats']['precision']} by common neighbours 0: count=")
    assert log[8].startswith("current density:") and "exposure=True" in log[0] and "save_exposure=" in log[0] and "exposure_cut" not in log[0]
    old = open(tmp_path / "results" / "plain.txt").read().split("\n")
    assert "exposure=" not in old[0] and "exposure" not in "\n".join(old[1:]) and old[1:] == log[1:5] + log[8:]      # (the path has the word)
