"""Per-node ranking counts on the device (mcgra_node_rank_metrics, engine.node_rank_metrics, main.py --per_node) against
tests/node_rank_truth.py: the five integers and the four rates of every compared row, element for element, over row lengths
from one candidate to the capacity (around the wave, around the workgroup's lane count, on both sides of every row-length
class), score families with ties, row kinds, selections, refusals that leave `out` untouched, bit-level determinism and
main.py end to end.  Every expected value is exact: every comparison is equality.  Run with -m gpu.

tests/test_node_rank_cases_cpu.py checks, without a GPU, that the named inputs have the properties the cases are there for."""
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import node_rank_truth as T

pytestmark = pytest.mark.gpu

# mirrored by engine.NODE_RANK_* (tests/test_node_rank_cases_cpu.py holds the two equal without a GPU)
THREADS = 512
CLASSES = (1024, 2048, 4096, 8192, 16384)
MAX_NIDX = 16384


def _graph(rng, n, p):
    a = np.triu(rng.rand(n, n) < p, 1)
    return (a | a.T).astype(np.float32)


def _cases():
    """name -> (real, pred, idx, pad): pad > 0 puts pred's rows into a buffer that many columns wider."""
    rng = np.random.RandomState(41)
    out = {}
    tiny = np.array([-1.5, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 3e-39, 1e-38, 2.0], np.float32)
    n = 150
    real = _graph(rng, n, 0.15)
    out["equal"] = (real, np.full((n, n), 0.5, np.float32), None, 0)
    out["levels4_ties"] = (real, (rng.randint(0, 4, (n, n)) * 0.25).astype(np.float32), None, 0)
    out["signed_zeros"] = (real, np.array([-0.0, 0.0], np.float32)[rng.randint(0, 2, (n, n))], None, 0)
    out["subnormals"] = (real, tiny[rng.randint(1, 8, (n, n))], None, 0)
    out["negative"] = (real, (-rng.rand(n, n) - 0.5).astype(np.float32), None, 0)
    distinct = rng.permutation(n * n).reshape(n, n).astype(np.float32)
    out["distinct_asym"] = ((rng.rand(n, n) < 0.15).astype(np.float32), distinct - np.float32(n * n / 2), None, 0)
    kinds = (rng.rand(n, n) < 0.5).astype(np.float32)            # a dense truth: half the entries positive
    kinds[3, :] = 0.0                                            # P = 0
    kinds[5, :] = 1.0                                            # P = n_idx - 1
    out["row_kinds_dense"] = (kinds, (rng.randint(0, 6, (n, n)) * 0.25 + kinds * 0.25).astype(np.float32), None, 0)
    n = 300
    real = _graph(rng, n, 0.05)
    lev = (rng.randint(0, 3, (n, n)) * 0.5 + real * 0.5).astype(np.float32)
    out["permuted_idx"] = (real, lev, rng.permutation(n), 0)
    out["subset_idx"] = (real, lev, rng.permutation(n)[:170].copy(), 0)
    out["padded_rows"] = (real, (rng.randn(n, n) + real).astype(np.float32), None, 3)
    sub = np.sort(rng.permutation(n)[:200])
    junk = real.copy()
    off = np.ones(n, bool); off[sub] = False
    junk[off, :] = 2.0                                           # unselected rows and columns, and the diagonal: never read
    junk[:, off] = np.nan
    junk[np.arange(n), np.arange(n)] = np.where(np.arange(n) % 2 == 0, 2.0, np.nan)
    out["junk_outside_selection"] = (junk, lev, sub, 0)
    return out


CASES = _cases()
# candidates per row: 1, 2, around a wave, around the workgroup's lane count, the last length of every class and the first of
# the next (the last class ends at the capacity: test_capacity...)
LENGTHS = sorted({1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1} |
                 {c + d for c in CLASSES[:-1] for d in (0, 1)})
SMALL = 600                                                      # up to here every row is compared, and the inputs are numpy's


def tie_rows(real, pred, idx=None):
    """Rows whose P-th and (P + 1)-th ranked candidates have one key: the tie group straddles the cut of `hits`."""
    rows = []
    n_idx = len(pred) if idx is None else len(idx)
    for a in range(n_idx):
        k, lab, _ = T.candidates(real, pred, a, idx)
        P = int(lab.sum())
        ks = np.sort(k)[::-1]
        if 0 < P < len(ks) and ks[P - 1] == ks[P]:
            rows.append(a)
    return rows


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def _dev(x, pad=0):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    if pad:
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda:0")      # the padding is never read
        buf[:, :t.shape[1]] = t
        t = buf[:, :t.shape[1]]
    return t


def _same(a, b):
    """Equal float64 values element for element, NaN in the same places."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _check(got, want_cols, n_idx, rows, what):
    """got: the wrapper's dict; want_cols: the truth's counts of `rows` (None: every row)."""
    import torch
    sel = slice(None) if rows is None else np.asarray(rows)
    cols = np.stack([got[k].cpu().numpy() for k in T.COLUMNS], 1)
    for k in T.COLUMNS:
        assert got[k].dtype == torch.int64 and got[k].is_cuda and got[k].numel() == n_idx, (what, k)
    print(f"{what}: rows {n_idx}, compared {len(want_cols)}, P sum {int(want_cols[:, 0].sum())}, wins sum "
          f"{int(want_cols[:, 1].sum())}, ties sum {int(want_cols[:, 2].sum())}")
    bad = np.flatnonzero((cols[sel] != want_cols).any(1))
    assert bad.size == 0, (what, bad[:5], cols[sel][bad[:5]], want_cols[bad[:5]])
    want = T.rates(want_cols, n_idx)
    for r in T.RATES:
        assert got[r].dtype == np.float64 and len(got[r]) == n_idx and _same(got[r][sel], want[r]), (what, r)


# ------------------------------------------------------------------------------------ 1. families, kinds, selections
@pytest.mark.parametrize("name", sorted(CASES))
def test_node_rank_cases_against_the_truth(pkg, name):
    from mc_gra_amd import engine as E
    real, pred, idx, pad = CASES[name]
    r, p = _dev(real), _dev(pred, pad)
    if pad:
        assert p.stride(0) == pred.shape[1] + pad and (p.stride(0) * 4) % 16 != 0
    got = E.node_rank_metrics(r, p, idx)
    n_idx = len(pred) if idx is None else len(idx)
    want = T.per_node(real, pred, idx)
    _check(got, want, n_idx, None, name)
    assert np.array_equal(got["nodes"].cpu().numpy(), np.arange(n_idx) if idx is None else np.asarray(idx))
    s, ws = got["summary"], T.summary(want, n_idx)
    assert sorted(s) == sorted(ws) and s["scored"] == ws["scored"] and len(s["by_degree"]) == 7
    for k in ("macro_auc", "mrr", "hits_at_1", "r_precision"):
        assert _same(s[k], ws[k]), (name, k, s[k], ws[k])
    for a, b in zip(s["by_degree"], ws["by_degree"]):
        assert a[:3] == b[:3] and _same(a[3:], b[3:]), (name, a, b)


# --------------------------------------------------------------------------------------------------- 2. row lengths
def _random_on_device(n, seed, p):
    """A 4-level asymmetric score matrix (ties in every row) lifted where the label is 1, and a truth of density p."""
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    real = (torch.rand(n, n, device="cuda:0", generator=g) < p).to(torch.float32)
    pred = torch.randint(0, 4, (n, n), device="cuda:0", generator=g).to(torch.float32) * 0.25 + real * 0.25
    return real, pred


def _spread(n, count):
    return sorted(set(np.linspace(0, n - 1, count).astype(int).tolist()))


@pytest.mark.parametrize("c", LENGTHS)
def test_node_rank_row_lengths(pkg, c):
    """n = c + 1 nodes, every node selected: c candidates per row.  Up to SMALL every row is compared; beyond, 24 rows spread
    over the range (the first and the last among them), from the rows copied back."""
    from mc_gra_amd import engine as E
    n = c + 1
    if n <= SMALL:
        rng = np.random.RandomState(c)
        real = (rng.rand(n, n) < 0.3).astype(np.float32)
        pred = (rng.randint(0, 4, (n, n)) * 0.25 + real * 0.25).astype(np.float32)
        got = E.node_rank_metrics(_dev(real), _dev(pred))
        _check(got, T.per_node(real, pred), n, None, f"c={c}")
        return
    real, pred = _random_on_device(n, c, 0.02)
    got = E.node_rank_metrics(real, pred)
    rows = _spread(n, 24)
    rr, pr = real[rows].cpu().numpy(), pred[rows].cpu().numpy()
    want = np.array([T.row_of_vectors(rr[i], pr[i], a) for i, a in enumerate(rows)], np.int64)
    _check(got, want, n, rows, f"c={c}")


def test_node_rank_capacity(pkg):
    """n = NODE_RANK_MAX_NIDX, every node selected, distinct-ish random scores, a 0.2 % truth: all rows are computed, 48 of
    them compared, and the positives of all rows add up to the truth's off-diagonal count."""
    import torch
    from mc_gra_amd import engine as E
    n = E.NODE_RANK_MAX_NIDX
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    real = (torch.rand(n, n, device="cuda:0", generator=g) < 0.002).to(torch.float32)
    pred = torch.rand(n, n, device="cuda:0", generator=g) + real * 0.3
    got = E.node_rank_metrics(real, pred)
    rows = _spread(n, 48)
    rr, pr = real[rows].cpu().numpy(), pred[rows].cpu().numpy()
    want = np.array([T.row_of_vectors(rr[i], pr[i], a) for i, a in enumerate(rows)], np.int64)
    _check(got, want, n, rows, "capacity")
    lab = real.to(torch.uint8).cpu().numpy()
    total = int(np.count_nonzero(lab)) - int(np.count_nonzero(np.diagonal(lab)))
    assert int(got["positives"].sum()) == total and total > 0
    with pytest.raises(pkg._lib.McgraNotSupported, match=str(n)):
        E.node_rank_metrics(torch.zeros(n + 1, n + 1, device="cuda:0"), torch.zeros(n + 1, n + 1, device="cuda:0"))


# ------------------------------------------------------------------------------------------------- 3. determinism
def test_node_rank_two_calls_give_identical_bits(pkg):
    import torch
    from mc_gra_amd import engine as E
    real, pred, idx, _ = CASES["permuted_idx"]
    r, p = _dev(real), _dev(pred)
    a, b = E.node_rank_metrics(r, p, idx), E.node_rank_metrics(r, p, idx)
    for k in T.COLUMNS + ("nodes",):
        assert torch.equal(a[k], b[k]), k
    for k in T.RATES:
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert repr(a["summary"]) == repr(b["summary"])


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_node_rank_device_refusals_leave_out_untouched(pkg):
    """What only the device can decide: a repeated id, an id out of range, a NaN / inf candidate score, a candidate label 0.5.
    The C entry is called on a poisoned `out`: MCGRA_EINVAL, and no element of it has changed."""
    import ctypes
    import torch
    from mc_gra_amd import engine as E
    real, pred, _, _ = CASES["distinct_asym"]
    n = len(real)
    L = pkg._lib.lib
    poison = -0x0123456789ABCDEF

    def call(rl, pd, idx):
        r, p = _dev(rl), _dev(pd)
        ix = None if idx is None else torch.as_tensor(np.asarray(idx, np.int64), device="cuda:0")
        rows = n if ix is None else ix.numel()
        out = torch.full((rows, 5), poison, device="cuda:0", dtype=torch.int64)
        rc = L.mcgra_node_rank_metrics(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), n, r.data_ptr(), r.stride(0),
                                       p.data_ptr(), p.stride(0), None if ix is None else ix.data_ptr(), rows, out.data_ptr())
        torch.cuda.synchronize()
        return rc, out, L.mcgra_last_error()

    sub = np.arange(10, 90)
    rc, out, _ = call(real, pred, sub)
    assert rc == 0 and np.array_equal(out.cpu().numpy(), T.per_node(real, pred, sub))       # the harness itself works
    refused = []
    for idx in ([4, 9, 4], [7, 7], list(range(40)) + [39]):
        refused.append(call(real, pred, idx) + (b"twice",))
    for idx in ([0, n], [-1, 2], [3, 2 ** 40]):
        refused.append(call(real, pred, idx) + (b"outside",))
    for v in (np.nan, np.inf, -np.inf):
        bad = pred.copy(); bad[7, 3] = v
        refused.append(call(real, bad, None) + (b"NaN or infinite",))
        bad = pred.copy(); bad[20, 60] = v                               # row and column both selected by sub
        refused.append(call(real, bad, sub) + (b"NaN or infinite",))
    bad = real.copy(); bad[9, 2] = 0.5
    refused.append(call(bad, pred, None) + (b"neither 0 nor 1",))
    bad = real.copy(); bad[88, 11] = 0.5
    refused.append(call(bad, pred, sub) + (b"neither 0 nor 1",))
    for rc, out, msg, word in refused:
        assert rc == -1 and word in msg and b"node_rank_metrics" in msg, (rc, msg, word)
        assert bool((out == poison).all()), (msg, "out was written")
    # what is no candidate is not inspected: the diagonal, and rows and columns outside the selection
    want = T.per_node(real, pred, sub)
    for i, j in ((5, 5), (20, 20), (3, 50), (50, 3), (95, 95)):
        ok = pred.copy(); ok[i, j] = np.nan
        lab = real.copy(); lab[i, j] = 0.5
        rc, out, msg = call(lab, ok, sub)
        assert rc == 0 and np.array_equal(out.cpu().numpy(), want), (i, j, msg)
    with pytest.raises(pkg._lib.McgraError):
        E.node_rank_metrics(_dev(real), _dev(pred), [5])                 # fewer than two nodes
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.node_rank_metrics(_dev(real), _dev(pred), [5, 6, 5])


# ------------------------------------------------------------------------------------------------------ 5. main.py
def test_main_evaluate_per_node(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed brazil files (n = 131), 6 epochs: the file's arrays are the truth applied to
    the modified_adj the run scored, the summaries come back under per_node_<set>, and a run without the flag returns and logs
    what it did before the flag existed."""
    from mc_gra_amd import main as M
    root = os.path.join(H.GOLDEN, "dataset")
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "brazil", "--dataset_root", root, "--epochs", "6", "--measure", "MSELoss", "--w2", "100", "--w6", "100",
            "--weight_sup", "0", "--lr", "-3", "--useH_A"]
    plain = M.run(M.build_parser().parse_args(argv + ["--log_name", "plain.txt"]))
    out_plain = capsys.readouterr().out
    assert sorted(plain) == ["auc_all", "auc_attack", "auc_train", "density", "path"]
    seen = []
    orig = M.engine.node_rank_metrics

    def record(real, pred, idx=None):
        v = orig(real, pred, idx)
        seen.append((real.cpu().numpy(), pred.cpu().numpy(), None if idx is None else np.asarray(idx), v))
        return v

    monkeypatch.setattr(M.engine, "node_rank_metrics", record)
    path = str(tmp_path / "nodes.npz")
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "nodes.txt", "--per_node", path]))
    out = capsys.readouterr().out
    assert sorted(res) == sorted(list(plain) + ["per_node_attack", "per_node_train", "per_node_all"]) and len(seen) == 3
    for key in ("auc_attack", "auc_train", "auc_all", "density"):
        assert res[key] == plain[key], key                              # the run without the flag, bit for bit
    z = np.load(path)
    names = ("nodes", "positives", "wins", "ties", "hits", "first_rank", "auc")
    assert sorted(z.files) == sorted(f"{k}_{s}" for k in names for s in ("attack", "train", "all"))
    for (real, pred, idx, v), name in zip(seen, ("attack", "train", "all")):
        n_idx = 131 if idx is None else len(idx)
        want = T.per_node(real, pred, idx)
        assert np.array_equal(np.stack([z[f"{k}_{name}"] for k in T.COLUMNS], 1), want), name
        assert np.array_equal(z[f"nodes_{name}"], np.arange(131) if idx is None else idx) and z[f"wins_{name}"].dtype == np.int64
        assert _same(z[f"auc_{name}"], T.rates(want, n_idx)["auc"]) and z[f"auc_{name}"].dtype == np.float64
        assert res[f"per_node_{name}"] is v["summary"]
        ws = T.summary(want, n_idx)
        assert v["summary"]["scored"] == ws["scored"] > 0 and _same(v["summary"]["macro_auc"], ws["macro_auc"])
        assert _same(v["summary"]["mrr"], ws["mrr"]) and _same(v["summary"]["hits_at_1"], ws["hits_at_1"])
    assert seen[2][2] is None and int(z["positives_all"].sum()) == int((seen[2][0] == 1).sum() - (np.diagonal(seen[2][0]) == 1).sum())
    d = res["per_node_all"]
    assert f"current auc={res['auc_all']}\ncurrent macro_auc={d['macro_auc']} mrr={d['mrr']} hits@1={d['hits_at_1']}\n" in out
    assert "macro_auc" not in out_plain
    log = open(tmp_path / "results" / "nodes.txt").read().split("\n")
    assert "per_node=" in log[0] and log[2].startswith("In attack graph: scored nodes=") and log[3].startswith("In train graph:")
    assert log[4] == (f"In Whole Graph: scored nodes={d['scored']} macro AUC={d['macro_auc']} MRR={d['mrr']} "
                      f"Hits@1={d['hits_at_1']} R-precision={d['r_precision']}")
    assert log[5].startswith("current density:")
    old = open(tmp_path / "results" / "plain.txt").read()
    assert "per_node" not in old and "macro" not in old and old.count("\n") == 3
    assert old.split("\n")[1:] == log[1:2] + log[5:]
    assert math.isfinite(d["macro_auc"]) and 0 < d["mrr"] <= 1
