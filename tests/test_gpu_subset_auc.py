"""The one-run ensemble ablation on the device (mcgra_subset_auc, engine.subset_auc, mcgra_attack_finalize_components,
main.py --ablate / --save_ablation) against tests/subset_auc_truth.py: every integer compared for equality, twice with the same
bits, and for every mask against engine.auc_delong's T on the sum materialised in torch in the same order -- at the selections,
component counts and mask lists of tests/subset_auc_cases.py; the refusals; the capacity; finalize_components bit for bit against
finalize; and one end-to-end run.  Run with -m gpu.

tests/test_subset_auc_cases_cpu.py checks, without a GPU, that these inputs have the properties the cases are there for and that
they tell the wrong readings of the definition from the right one."""
import ctypes
import functools
import lzma
import math
import os
import time

import numpy as np
import pytest

from tests import helpers as H
from tests import subset_auc_cases as SC
from tests import subset_auc_truth as T
from tests.test_gpu_hops import _circulant_on_device, _dev

pytestmark = pytest.mark.gpu

CASES = SC.cases()


@functools.lru_cache(maxsize=None)
def truth(name, which):
    """The truth of one mask list of a case, computed once (read-only)."""
    real, comps, idx, _, lists = CASES[name]
    return T.stats(T.ints(real, comps, lists[which], idx), lists[which])


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def materialised(comps, mask):
    """The sum of the mask's components on the device, in ascending k, one float32 add each."""
    ks = [k for k in range(len(comps)) if mask >> k & 1]
    s = comps[ks[0]].clone()
    for k in ks[1:]:
        s = s + comps[k]
    return s


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("name", sorted(CASES))
def test_subset_auc_against_the_truth(pkg, name):
    """Every integer of the entry and every double the engine forms from them, for each mask list of the case, on two calls;
    and every mask's T against engine.auc_delong on the materialised sum."""
    from mc_gra_amd import engine as E
    real, comps, idx, pad, lists = CASES[name]
    r, ix = _dev(real, pad), None if idx is None else _dev(idx)
    cs = [_dev(c, pad) for c in comps]
    delong = {}
    for which, masks in enumerate(lists):
        want = truth(name, which)
        one, two = E.subset_auc(r, cs, masks, ix), E.subset_auc(r, cs, masks, ix)
        print(f"{name} K={len(cs)} masks={len(masks)}: m={one['pairs']} P={one['positives']} T={one['T'][:4]} ...")
        assert T.same(one, want) and T.same(two, one), (name, which)
        for q, t in zip(masks, one["T"]):
            if q not in delong:
                d = E.auc_delong(r, materialised(cs, q), ix)
                delong[q] = (d["ints"]["T"], d["positives"], d["negatives"])
            assert delong[q] == (t, one["positives"], one["negatives"]), (name, q)


def test_a_stacked_tensor_and_a_list_are_the_same_call(pkg):
    import torch
    from mc_gra_amd import engine as E
    real, comps, idx, _, lists = CASES["ints129_k8"]
    want = truth("ints129_k8", 1)
    stack = torch.as_tensor(comps, device="cuda:0")
    assert T.same(E.subset_auc(_dev(real), stack, lists[1]), want)
    assert T.same(E.subset_auc(_dev(real), [stack[k].double() for k in range(8)], lists[1]), want)      # converted to float32
    assert T.same(E.subset_auc(_dev(real), [stack[k] if k % 2 else _dev(comps[k], 4) for k in range(8)], lists[1]), want)


def test_known_answers_on_the_device(pkg):
    from mc_gra_amd import engine as E
    for name, T7 in (("cancellation", 0), ("cancellation_descending", 0)):
        real, comps, _, _, _ = CASES[name]
        d = E.subset_auc(_dev(real), [_dev(c) for c in comps], [7])
        assert d["T"] == [T7] and d["auc"] == [0.0] and d["positives"] > 0
    real, comps, _, _, _ = CASES["cancellation"]
    d = E.subset_auc(_dev(real), [_dev(comps[0]), _dev(comps[2]), _dev(comps[1])], [7])          # (1e8 - 1e8) + 1
    assert d["T"] == [2 * d["positives"] * d["negatives"]] and d["auc"] == [1.0]
    for name in ("no_edge", "complete"):
        real, comps, _, _, lists = CASES[name]
        d = E.subset_auc(_dev(real), [_dev(c) for c in comps], lists[0])
        assert d["T"] == [0] * 7 and all(np.isnan(a) for a in d["auc"]) and 0 in (d["positives"], d["negatives"])


def test_subset_auc_capacity(pkg):
    """n_idx = 65 535, every node selected, built on the device in row blocks: the circulant graph of offsets +-1, +-2 as labels
    and as both components, masks 1, 2, 3: every edge above every non-edge under each.  Matrix offsets up to 2^32."""
    import torch
    from mc_gra_amd import engine as E
    n = SC.MAX_NIDX
    need = 4 * n * n + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the capacity case needs {need / 2 ** 30:.1f} GiB of device memory (a 17 GB matrix); "
                    f"{free / 2 ** 30:.1f} GiB are free")
    both = _circulant_on_device(n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = E.subset_auc(both, [both, both], [1, 2, 3])
    print(f"capacity: {time.perf_counter() - t0:.3f} s, P={d['positives']} T={d['T']}")
    P, N = 2 * n, n * (n - 1) // 2 - 2 * n
    assert (d["pairs"], d["positives"], d["negatives"]) == (P + N, P, N) and d["T"] == [2 * P * N] * 3 and d["auc"] == [1.0] * 3


# ------------------------------------------------------------------------------------------------ 2. the refusals
def test_device_refusals_leave_out_untouched(pkg):
    """A NaN or infinite component value, a subset sum that overflows, a label of 0.5, a repeated id, an id out of range:
    MCGRA_EINVAL, the cause named, and not one word of out written; the same entries outside the selected triangle are not
    looked at."""
    import torch
    L = pkg._lib.lib
    rng = np.random.RandomState(5)
    n, K = 70, 3
    real, comps = SC.graph(rng, n, 0.05), rng.rand(K, n, n).astype(np.float32)
    real[40, 7] = real[7, 40] = 0                                         # a non-edge: the stream reads it
    real[41, 8] = real[8, 41] = 1                                         # an edge: the emit pass reads it
    masks, mark, words = [7, 1, 6], 2 ** 64 - 7, 10
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(real, comps, idx=None, masks=masks):
        r, cs = _dev(real), [_dev(c) for c in comps]
        ix = None if idx is None else _dev(np.asarray(idx, np.int64))
        ptrs = (ctypes.c_void_p * K)(*[c.data_ptr() for c in cs])
        out = (ctypes.c_uint64 * words)(*([mark] * words))
        rc = L.mcgra_subset_auc(stream, n, ctypes.c_void_p(r.data_ptr()), n, ptrs, K, n, None if ix is None else ctypes.c_void_p(ix.data_ptr()),
                                n if idx is None else len(idx), (ctypes.c_uint32 * len(masks))(*masks), len(masks), out)
        return rc, L.mcgra_last_error().decode(), list(out)

    def bad(m, value, where=(40, 7), k=None):
        m = m.copy()
        if k is None:
            m[where] = value
        else:
            m[k][where] = value
        return m

    untouched = [mark] * words
    rc, _, out = run(real, comps)
    assert rc == 0 and out[0] == n * (n - 1) // 2 and mark not in out[:6] and out[6:] == [mark] * 4
    for where in ((40, 7), (41, 8)):                                      # a non-edge and an edge
        for k in range(K):
            for value in (np.nan, np.inf, -np.inf):
                rc, e, out = run(real, bad(comps, value, where, k))
                assert rc == -1 and "NaN or infinite" in e and "subset_auc" in e and out == untouched, (where, k, value)
        # finite values whose sum is not: 3e38 + 3e38 under masks 7 and 6 (components 1 and 2)
        rc, e, out = run(real, bad(bad(comps, 3e38, where, 1), 3e38, where, 2))
        assert rc == -1 and "NaN or infinite" in e and out == untouched
        assert run(real, bad(bad(comps, 3e38, where, 1), 3e38, where, 2), None, [1, 2, 4, 5, 3])[0] == 0       # no mask adds them
        # a component that no mask selects is checked all the same
        rc, e, out = run(real, bad(comps, np.nan, where, 2), None, [1, 3])
        assert rc == -1 and "NaN or infinite" in e and out == untouched
    for value in (0.5, np.nan, 2.0):
        rc, e, out = run(bad(real, value), comps)
        assert rc == -1 and "label" in e and out == untouched
    # the same invalid entries above the diagonal, on it, and in unselected rows and columns are not looked at
    assert run(bad(real, 0.5, (7, 40)), bad(comps, np.nan, (7, 40), 1))[0] == 0
    assert run(bad(real, 0.5, (9, 9)), bad(comps, np.inf, (9, 9), 0))[0] == 0
    rc, _, out = run(bad(real, 0.5), bad(comps, np.nan, (40, 7), 2), [3, 41, 7, 12, 60])
    assert rc == 0 and out[0] == 10
    rc, e, out = run(real, bad(comps, np.nan, (40, 7), 1), [3, 7, 40, 12, 60])       # node 40 at position 2, node 7 at 1: [40][7] is read
    assert rc == -1 and "NaN or infinite" in e and out == untouched
    assert run(real, bad(comps, np.nan, (40, 7), 1), [3, 40, 7, 12, 60])[0] == 0     # node 7 at position 2: [7][40] is read
    rc, e, out = run(real, comps, [3, 9, 4, 9, 12])
    assert rc == -1 and "twice" in e and out == untouched
    for ids in ([3, 9, n], [3, -1, 5]):
        rc, e, out = run(real, comps, ids)
        assert rc == -1 and "outside" in e and out == untouched


def test_engine_raises_what_the_entry_refuses(pkg):
    from mc_gra_amd import engine as E
    rng = np.random.RandomState(6)
    n = 20
    real, comps = SC.graph(rng, n, 0.3), rng.rand(2, n, n).astype(np.float32)
    nan = comps.copy()
    nan[1, 5, 2] = np.nan
    with pytest.raises(pkg._lib.McgraError, match="NaN"):
        E.subset_auc(_dev(real), _dev(nan), [1])
    with pytest.raises(pkg._lib.McgraError, match="twice"):
        E.subset_auc(_dev(real), _dev(comps), [3], [1, 2, 1])
    with pytest.raises(pkg._lib.McgraError):
        E.subset_auc(_dev(real), _dev(comps), [3], [4])                  # fewer than two nodes
    with pytest.raises(ValueError, match="mask"):
        E.subset_auc(_dev(real), _dev(comps), [4])
    assert E.subset_auc(_dev(real), _dev(nan), [1, 3, 2], list(range(6, 20)))["pairs"] == 14 * 13 // 2      # [5][2] is not selected


# ------------------------------------------------------------------------------------ 3. finalize with its summands
PRIORS = {"all": (1, 1, 1), "no_HA": (0, 1, 1), "no_YA": (1, 0, 1), "no_label": (1, 1, 0), "none": (0, 0, 0)}


@pytest.mark.parametrize("mode", [0, 3, 4])
@pytest.mark.parametrize("case", ["s48_mse", "s48_mse_ori"])
def test_finalize_components_are_the_bits_finalize_adds(pkg, case, mode):
    """After the same two steps: out of finalize_components = out of finalize bit for bit, the stack summed in torch in
    ascending order = out, M afterwards = finalize's M, present as given; a smaller out_mask = finalize without those priors."""
    import torch
    z = H.load_case(case)
    lab = z["labels"]
    label_adj = (lab[:, None] == lab[None, :]).astype(np.float32)

    def after_steps():
        eng = H.engine_from(pkg, z)
        for _ in range(2):
            eng.step()
        return eng

    for name, use in PRIORS.items():
        given = (z["H_A2"] if use[0] else None, z["Y_A"] if use[1] else None, label_adj if use[2] else None)
        a, b = after_steps(), after_steps()
        ref = a.finalize(mode, *given)
        out, comps, present = b.finalize_components(mode, *given)
        want = 0x1f | use[0] << 5 | use[1] << 6 | use[2] << 7
        assert present == want, (name, present)
        assert torch.equal(out, ref), (name, float((out - ref).abs().max()))
        assert torch.equal(a.buffer("M"), b.buffer("M")), name
        ks = [k for k in range(8) if present >> k & 1]
        s = comps[ks[0]].clone()
        for k in ks[1:]:
            s = s + comps[k]
        assert torch.equal(s, out), name
        assert all(float(comps[k].abs().max()) == 0 for k in range(8) if not present >> k & 1)
        assert all(float(comps[k].abs().max()) > 0 for k in ks)
        a.close(); b.close()
    # every prior given, the base five summed: finalize without priors; no out at all: the same stack
    a, b, c = after_steps(), after_steps(), after_steps()
    ref = a.finalize(mode, None, None, None)
    out, comps, present = b.finalize_components(mode, z["H_A2"], z["Y_A"], label_adj, out_mask=0x1f)
    none, comps2, present2 = c.finalize_components(mode, z["H_A2"], z["Y_A"], label_adj, want_out=False)
    assert present == present2 == 0xff and torch.equal(out, ref) and none is None and torch.equal(comps, comps2)
    # the refusals, each before anything is touched: M stays what it is
    M = b.buffer("M")
    for kw in (dict(H_A=None, out_mask=0x3f), dict(out_mask=0), dict(out_mask=0x100)):
        args = dict(H_A=z["H_A2"], Y_A=z["Y_A"], label_adj=label_adj)
        args.update(kw)
        with pytest.raises(pkg._lib.McgraError):
            b.finalize_components(mode, **args)
    L = pkg._lib.lib
    assert L.mcgra_attack_finalize_components(b._h, None, mode, None, None, None, 0x1f, None, None, None) == -1      # NULL comps
    assert L.mcgra_attack_finalize_components(b._h, None, 7, None, None, None, 0x1f, None, ctypes.c_void_p(comps.data_ptr()), None) == -1
    assert torch.equal(b.buffer("M"), M)
    for e in (a, b, c):
        e.close()


# ------------------------------------------------------------------------------------------------------ 4. main.py
def test_main_evaluate_ablate_shapley_and_save_ablation(pkg, tmp_path, monkeypatch, capsys):
    """main.py --mode evaluate on the committed cora file, 6 epochs of its README line with --ci: --ablate shapley adds the
    ablation_* dicts -- the sum in use is modified_adj (auc_used and its T are --ci's), the shares sum to auc_used - 1/2, the
    file holds the dict's arrays -- and the same command without --ablate returns and logs what it did before the flag existed."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    monkeypatch.chdir(tmp_path)
    root = tmp_path / "dataset"                     # cora.npz is committed as an xz archive of the reference's file
    root.mkdir()
    with lzma.open(os.path.join(H.GOLDEN, "dataset", "cora.npz.xz")) as src:
        (root / "cora.npz").write_bytes(src.read())
    argv = ["--dataset", "cora", "--dataset_root", str(root), "--epochs", "6", "--w1", "0.01", "--w6", "10", "--w7", "10", "--w9", "10",
            "--w10", "1000", "--lr", "-2", "--useH_A", "--useY_A", "--useY", "--measure", "MSELoss", "--ci"]
    plain_args = M.build_parser().parse_args(argv + ["--log_name", "plain.txt"])
    assert not hasattr(plain_args, "ablate") and not hasattr(plain_args, "save_ablation")
    plain = M.run(plain_args)
    out_plain = capsys.readouterr().out
    path = str(tmp_path / "ablation.npz")
    t0 = time.perf_counter()
    res = M.run(M.build_parser().parse_args(argv + ["--log_name", "abl.txt", "--ablate", "shapley", "--save_ablation", path]))
    print(f"the run with --ablate shapley: {time.perf_counter() - t0:.2f} s")
    out = capsys.readouterr().out
    sets = ("attack", "train", "all")
    assert sorted(res) == sorted(list(plain) + [f"ablation_{s}" for s in sets])
    for key in plain:
        if key != "path":
            assert res[key] == plain[key], key                          # the run without the flag, bit for bit
    saved = np.load(path)
    assert sorted(saved.files) == sorted(["masks", "names"] + [f"{k}_{s}" for k in ("T", "auc", "counts", "shapley") for s in sets])
    assert saved["names"].tolist() == list(T.NAMES) and saved["masks"].dtype == np.uint32 and saved["masks"].tolist() == list(range(1, 256))
    for s in sets:
        d, ci = res[f"ablation_{s}"], res[f"ci_{s}"]
        assert (d["present"], d["used"], d["decode_mode"], d["components"]) == (0xff, 0xff, 0, T.NAMES)
        assert (d["pairs"], d["positives"], d["negatives"]) == (ci["pairs"], ci["positives"], ci["negatives"])
        by_mask = {r["mask"]: r for r in d["subsets"]}
        print(f"{s}: auc_used={d['auc_used']} ci auc={ci['auc']} T={by_mask[0xff]['T']} ci T={ci['ints']['T']}")
        assert d["auc_used"] == ci["auc"] and by_mask[0xff]["T"] == ci["ints"]["T"]
        assert [r["mask"] for r in d["subsets"]] == list(range(1, 256)) and by_mask[0x21]["names"] == ("learned", "ori_HA")
        assert d["alone"] == {nm: by_mask[1 << k]["auc"] for k, nm in enumerate(T.NAMES)}
        assert d["without"] == {nm: by_mask[0xff ^ 1 << k]["auc"] for k, nm in enumerate(T.NAMES)}
        assert [(r["useH_A"], r["useY_A"], r["useY"], r["auc"]) for r in d["flag_table"]] == \
            [(bool(q & 1), bool(q & 2), bool(q & 4), by_mask[0x1f | q << 5]["auc"]) for q in range(8)]
        P, N = d["positives"], d["negatives"]
        assert all(r["auc"] == float(T.Fraction(r["T"], 2 * P * N)) for r in d["subsets"])
        shares = [d["shapley"][nm] for nm in T.NAMES]
        total = math.fsum(shares)                                        # the float sum of the floats, rounded once
        print(f"{s}: shapley {d['shapley']} sum={total} auc_used - 0.5 = {d['auc_used'] - 0.5}")
        assert abs(total - (d["auc_used"] - 0.5)) <= np.spacing(abs(total)) and d["shapley_sum"] == float(T.Fraction(by_mask[0xff]["T"], 2 * P * N) - T.Fraction(1, 2))
        assert saved[f"T_{s}"].dtype == np.int64 and saved[f"T_{s}"].tolist() == [r["T"] for r in d["subsets"]]
        assert saved[f"auc_{s}"].dtype == np.float64 and saved[f"auc_{s}"].tolist() == [r["auc"] for r in d["subsets"]]
        assert saved[f"counts_{s}"].tolist() == [d["pairs"], P, N] and saved[f"shapley_{s}"].tolist() == shares
    lines = R._ablation_console(res, None)
    assert len(lines) == 2 and lines[0].startswith("current ablation used=learned+feature+H_A1+H_A2+Y_A2+ori_HA+ori_YA+label auc=")
    assert " | alone: learned=" in lines[0] and " | without: learned=" in lines[0] and lines[1].startswith("current shapley learned=")
    assert "\n".join(lines) + "\n" in out and out.index("current auc_pairs=") < out.index(lines[0]) and "ablation" not in out_plain
    log = open(tmp_path / "results" / "abl.txt").read().split("\n")
    old = open(tmp_path / "results" / "plain.txt").read().split("\n")
    mine = [i for i, line in enumerate(log) if ": ablation (decode mode 0) used=" in line]
    assert len(mine) == 3 and mine == list(range(mine[0], mine[0] + 3)) and log[mine[0] + 3].startswith("current density:")
    assert [line for i, line in enumerate(log) if i not in mine][1:] == old[1:]
    assert "ablate='shapley'" in log[0] and "save_ablation=" in log[0] and "ablate=" not in old[0] and "save_ablation" not in old[0]
