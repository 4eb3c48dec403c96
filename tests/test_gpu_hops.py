"""The AUC by true-graph distance on the device (mcgra_hop_auc, engine.hop_auc, main.py --hops / --hops_cut / --save_hops)
against tests/hop_truth.py: every integer and every double compared for equality, twice with the same bits -- at the smallest
selections where the kernels change behaviour (one word, two words, the diagonal tile, the pad bits, a row of AUC_THREADS
columns, more rows than the grid of the row passes, more edges than one sort tile, a lane of the expansion that owns a second
word), graphs (a path, two components, a star, the complete and the empty graph, cycles, a hub), scores (four levels, negative,
signed zeros, subnormals), hops 1, 3 and 8, thresholds -inf, +inf, a stored score and -0.0 against +0.0, layouts (n > m with a
permuted idx and padded rows), the refusals, and the capacity.  Run with -m gpu.

tests/test_hop_cases_cpu.py checks, without a GPU, that these inputs (tests/hop_cases.py) have the properties the cases are
there for and that they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import hop_cases as HC
from tests import hop_truth as T
from tests import two_means_truth as TM

pytestmark = pytest.mark.gpu

CASES = HC.cases()


@functools.lru_cache(maxsize=None)
def prep(name):
    """What the truth of a case shares over its runs, computed once (read-only)."""
    real, pred, idx, _, _ = CASES[name]
    return T.prepare(real, pred, idx)


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
    """tests/hop_cases.py's circulant(n) built on the device in row blocks."""
    import torch
    both = torch.empty(n, n, device="cuda:0", dtype=torch.float32)
    cols = torch.arange(n, device="cuda:0", dtype=torch.int32)[None, :]
    for r0 in range(0, n, 4096):
        rows = torch.arange(r0, min(n, r0 + 4096), device="cuda:0", dtype=torch.int32)[:, None]
        d = (rows - cols) % n
        both[r0:r0 + 4096] = ((d == 1) | (d == 2) | (d == n - 1) | (d == n - 2)).to(torch.float32)
    return both


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_hop_auc_against_the_truth(pkg, name):
    """Every integer of the entry and every double the engine forms from them, at each (hops, threshold) of the case, on two
    calls."""
    from mc_gra_amd import engine as E
    real, pred, idx, pad, runs = CASES[name]
    r, p, ix = _dev(real, pad), _dev(pred, pad), None if idx is None else _dev(idx)
    for hops, thr in runs:
        want = T.stats(T.rows_of(prep(name), hops, thr), hops, thr)
        one, two = E.hop_auc(r, p, ix, hops, thr), E.hop_auc(r, p, ix, hops, thr)
        print(f"{name} hops={hops} threshold={thr}: {one['ints']} auc={one['auc']} pooled={one['auc_pooled']}")
        assert T.same(one, want) and T.same(two, one), (name, hops, thr)


@pytest.mark.parametrize("name", ["m129", "sub257", "two_components", "sparse_sub1054"])
def test_pooled_auc_is_delongs_and_the_weighted_mean(pkg, name):
    """hops = 1 is {P, N, T} of mcgra_auc_delong on the same input; auc_pooled is its auc bit for bit at every hops, and the
    mean of the class AUCs weighted by their shares; the false positives are mcgra_threshold_pairs' pairs that are no edges."""
    from mc_gra_amd import engine as E
    real, pred, idx, pad, runs = CASES[name]
    r, p, ix = _dev(real, pad), _dev(pred, pad), None if idx is None else _dev(idx)
    dl = E.auc_delong(r, p, ix)
    one = E.hop_auc(r, p, ix, 1, 0.5)
    assert one["ints"] == [(dl["positives"], dl["ints"]["T"], one["above"][0]), (dl["negatives"], dl["ints"]["T"], one["above"][1])]
    _, _, hits = E.threshold_pairs(p, 0.5, ix, r)
    assert (one["above"][0], one["above"][1]) == (int(hits.sum()), int((~hits).sum()))
    for hops in (1, 3, 8):
        d = E.hop_auc(r, p, ix, hops)
        assert d["auc_pooled"] == dl["auc"] and d["T"][0] == dl["ints"]["T"] and "above" not in d
        mean = sum(a * w for a, w in zip(d["auc"][1:], d["share"][1:]) if w > 0)
        assert abs(mean - d["auc_pooled"]) < 1e-12


def test_any_permutation_of_idx_gives_the_same_integers(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(3)
    n = 150
    g = HC.graph(rng, n, 0.03)
    s = HC.scores(rng, g, "levels4")                                     # symmetric: a permutation keeps every candidate's score
    sel = rng.permutation(n)[:101]
    want = T.ints(g, s, sel, 3, 0.5)
    for _ in range(3):
        got = E.hop_auc(_dev(g), _dev(s), _dev(rng.permutation(sel)), 3, 0.5)
        assert got["ints"] == [tuple(c) for c in want]


def test_other_dtypes_and_host_node_ids(pkg):
    """float64 / bool operands and a list of node ids are converted as the neighbours convert them."""
    from mc_gra_amd import engine as E
    real, pred, idx, _, _ = CASES["sub65"]
    got = E.hop_auc(_dev(np.nan_to_num(real, nan=0)).bool(), _dev(np.nan_to_num(pred, nan=0)).double(), idx.tolist(), 3, -1.25)
    assert T.same(got, T.stats(T.rows_of(prep("sub65"), 3, -1.25), 3, -1.25))


def _closed_form(n, hops, what):
    from mc_gra_amd import engine as E
    both = _circulant_on_device(n)
    one, two = E.hop_auc(both, both, None, hops, 0.5), E.hop_auc(both, both, None, hops, 0.5)
    want = T.stats(T.circulant_rows(n, hops), hops, 0.5)
    print(f"{what}: {one['ints']}")
    assert T.same(one, want) and T.same(two, one)
    assert one["count"][:hops] == (2 * n,) * hops and one["above"] == (2 * n,) + (0,) * hops and one["auc"][1:] == (1.0,) * hops


def test_a_lane_of_the_expansion_owns_a_second_word(pkg):
    """n_idx = 64 * 256 + 63: 257 words per row.  The circulant graph of the capacity case and its closed form (held to the
    numpy truth at small n by the CPU tests)."""
    _closed_form(HC.SECOND_WORD_N, 3, "W = 257")


def test_hop_auc_capacity(pkg):
    """n_idx = 65 535, every node selected, built on the device in row blocks: the circulant graph of offsets +-1, +-2 as scores
    and labels at once, hops = 3, threshold 0.5.  1024 words per row, 524 800 tiles, matrix offsets up to 2^32, four words per
    lane of the expansion, T_c up to 2^49."""
    import torch
    n = HC.MAX_NIDX
    need = 4 * n * n + 3 * 8 * n * HC.words(n) + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the capacity case needs {need / 2 ** 30:.1f} GiB of device memory (a 17 GB matrix and 1.6 GB of bit "
                    f"matrices); {free / 2 ** 30:.1f} GiB are free")
    assert n * n > 2 ** 31
    _closed_form(n, 3, "capacity")


# ------------------------------------------------------------------------------------------------ 2. the refusals
def test_device_refusals_leave_out_untouched(pkg):
    """A NaN or infinite score, a label of 0.5, a repeated id, an id out of range: MCGRA_EINVAL, the cause named, and not one
    word of out written; the same entries outside the selected triangle are not looked at."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n = 70
    real, pa = HC.graph(rng, n, 0.05), rng.rand(n, n).astype(np.float32)
    mark = -7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(real, pa, idx=None, thr=0.5, hops=3):
        r, a = _dev(real), _dev(pa)
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        rows = n if idx is None else len(idx)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        out = (ctypes.c_int64 * 27)(*([mark] * 27))
        rc = L.mcgra_hop_auc(stream, n, p(r), n, p(a), n, p(ix), rows, hops, thr, out)
        return rc, L.mcgra_last_error().decode(), list(out)

    def bad(m, value, where=(40, 7)):
        m = m.copy()
        m[where] = value
        return m

    rc, _, out = run(real, pa)
    assert rc == 0 and mark not in out[:12] and out[12:] == [mark] * 15 and sum(out[0:12:3]) == n * (n - 1) // 2
    for value in (np.nan, np.inf, -np.inf):
        for thr in (0.5, float("inf"), -float("inf")):                       # whatever the threshold decides about the entry
            rc, e, out = run(real, bad(pa, value), None, thr)
            assert rc == -1 and "NaN or infinite" in e and "hop_auc" in e and out == [mark] * 27
    for value in (0.5, np.nan, 2.0):
        rc, e, out = run(bad(real, value), pa)
        assert rc == -1 and "label" in e and out == [mark] * 27
    # the same invalid entries above the diagonal, on it, and in unselected rows and columns are not looked at
    assert run(bad(real, 0.5, (7, 40)), bad(pa, np.nan, (7, 40)))[0] == 0
    assert run(bad(real, 0.5, (9, 9)), bad(pa, np.inf, (9, 9)))[0] == 0
    rc, _, out = run(bad(real, 0.5), bad(pa, np.nan), [3, 41, 7, 12, 60])
    assert rc == 0 and sum(out[0:12:3]) == 10
    rc, e, out = run(real, bad(pa, np.nan), [3, 7, 40, 12, 60])               # node 40 at position 2, node 7 at 1: [40][7] is read
    assert rc == -1 and "NaN or infinite" in e and out == [mark] * 27
    assert run(real, bad(pa, np.nan), [3, 40, 7, 12, 60])[0] == 0             # node 7 at position 2, node 40 at 1: [7][40] is read
    rc, e, out = run(real, pa, [3, 9, 4, 9, 12])
    assert rc == -1 and "twice" in e and out == [mark] * 27
    for ids in ([3, 9, n], [3, -1, 5]):
        rc, e, out = run(real, pa, ids)
        assert rc == -1 and "outside" in e and out == [mark] * 27
    rc, e, out = run(real, pa, None, float("nan"))
    assert rc == -1 and "NaN" in e and out == [mark] * 27
    rc, e, out = run(real, pa, None, 0.5, 9)
    assert rc == -1 and "hops" in e and out == [mark] * 27


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, pa = HC.graph(rng, n, 0.3), rng.rand(n, n).astype(np.float32)
    nan = pa.copy()
    nan[5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.hop_auc(_dev(real), _dev(nan))
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.hop_auc(_dev(real), _dev(pa), None, 3, float("nan"))
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.hop_auc(_dev(real), _dev(pa), [1, 2, 1])
    with pytest.raises(pkg._lib.McgraError):
        E.hop_auc(_dev(real), _dev(pa), [4])                                  # fewer than two nodes
    with pytest.raises(ValueError, match="hops"):
        E.hop_auc(_dev(real), _dev(pa), None, 9)


# ------------------------------------------------------------------------------------------------------ 3. main.py
def test_main_evaluate_hops_and_save_hops(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed usair files (n = 1190), 3 epochs of its README line: --hops 3 adds the hops_*
    dicts, each the truth on the matrices that were scored, its false positives counted at the score of the set's P-th best
    pair; --save_hops writes the classes of each set; a run without the flags returns and logs what it did before the flags
    existed."""
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "usair", "--dataset_root", root, "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--w7", "10000", "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt"])
    assert not any(hasattr(plain_args, k) for k in ("hops", "hops_cut", "save_hops"))
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.hop_auc

    def record(real, pred, idx=None, hops=3, threshold=None):
        v = orig(real, pred, idx, hops, threshold)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx), hops, threshold, v))
        return v

    monkeypatch.setattr(M.engine, "hop_auc", record)
    path = str(tmp_path / "hops.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "hops.txt", "--hops", "3", "--save_hops", path, "--ci"]))
    out = capsys.readouterr().out
    new = [f"{k}_{s}" for k in ("hops", "ci") for s in ("attack", "train", "all")]
    assert sorted(res) == sorted(list(plain) + new) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flags, bit for bit
    saved = np.load(path)
    keys = ("distance", "count", "T", "above", "auc", "threshold")
    assert sorted(saved.files) == sorted(f"{k}_{s}" for k in keys for s in ("attack", "train", "all"))
    for (real, pred, idx, hops, thr, v), name in zip(seen, ("attack", "train", "all")):
        assert res[f"hops_{name}"] is v and hops == 3
        s = np.sort(TM.K.packed(real, pred, idx)[0])[::-1]
        assert v["positives"] > 0 and thr == float(s[v["positives"] - 1])               # --hops_cut defaults to `edges`
        want = T.stats(T.rows_of(T.prepare(real, pred, idx, brute=False), 3, thr), 3, thr)
        assert T.same(v, want), name
        assert v["auc_pooled"] == res[f"ci_{name}"]["auc"]                              # auc_pairs of --ci
        assert abs(sum(a * w for a, w in zip(v["auc"][1:], v["share"][1:]) if w > 0) - v["auc_pooled"]) < 1e-12
        assert saved[f"distance_{name}"].tolist() == [1, 2, 3, 0]
        for k in ("count", "T", "above"):
            assert saved[f"{k}_{name}"].dtype == np.int64 and saved[f"{k}_{name}"].tolist() == list(v[k]), (k, name)
        assert saved[f"auc_{name}"].dtype == np.float64 and np.array_equal(saved[f"auc_{name}"], np.asarray(v["auc"]), equal_nan=True)
        assert saved[f"threshold_{name}"].dtype == np.float32 and float(saved[f"threshold_{name}"]) == thr
    d = res["hops_all"]
    line = (f"current auc_by_distance 2:{d['auc'][1]} 3:{d['auc'][2]} beyond:{d['auc'][3]} (pooled {d['auc_pooled']}) "
            f"false positives at distance 2: {d['above'][1]}/{sum(d['above'][1:])}\n")
    assert line in out and out.index("current auc_pairs=") < out.index(line) and "auc_by_distance" not in out_plain
    log = open(tmp_path / "results" / "hops.txt").read().split("\n")
    for i, (title, key) in enumerate((("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))):
        d = res[f"hops_{key}"]
        by = " ".join(f"{k}: count={c} AUC={a} above={x}" for k, c, a, x in zip(d["distance"], d["count"], d["auc"], d["above"]))
        assert log[5 + i] == f"In {title}: by true-graph distance at {d['threshold']}: {by} pooled AUC={d['auc_pooled']}"
    assert log[8].startswith("current density:") and "hops=3" in log[0] and "save_hops=" in log[0] and "hops_cut" not in log[0]
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "hops" not in old and old.count("\n") == 3 and old.split("\n")[1:] == log[1:2] + log[8:]
    # --hops_cut: a float is itself, `split` the threshold of the set's own 2-means split
    seen.clear()
    M.run(M.build_parser().parse_args(argv + ["--log_name", "cut.txt", "--hops", "1", "--hops_cut", "0.25"]))
    capsys.readouterr()
    assert [(s[3], s[4]) for s in seen] == [(1, 0.25)] * 3 and all(len(s[5]["count"]) == 2 for s in seen)
