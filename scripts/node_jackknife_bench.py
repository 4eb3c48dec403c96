"""Times engine.auc_node_jackknife against (a) engine.auc_delong on the same input and (b) the same five integers per node
composed from torch on the device (a tril_indices gather, torch.sort of each class, torch.searchsorted both ways, index_add_ of
the placements to both endpoints, and for C_v a sort of every node's row of negatives with a batched searchsorted of its
positives), on a bench-shaped modified_adj at n = 2 708 and N = 10 000 with every node selected.  Everything is int64 on both
routes: the integers are compared for equality.  The device entry alone (the integers, as Python lists) and the whole call
(with the host's one rational per node) are timed apart.

    python scripts/node_jackknife_bench.py [OUT]        # OUT defaults to profiles/auc_node_jackknife.txt"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcgra_loader  # noqa: E402

mcgra_loader.load()
from mc_gra_amd import engine as E  # noqa: E402

dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench_graph(n, seed):
    """(real, pred): 0.1 % of the pairs are edges (0.05 % of all pairs flipped), scored near 0.8; the rest |N(0, 0.01)|: the
    first scoring of scripts/delong_bench.py."""
    g = torch.Generator(device=dev).manual_seed(seed)
    hi = torch.tril(torch.rand(n, n, device=dev, generator=g) < 0.001, -1)
    flip = torch.tril(torch.rand(n, n, device=dev, generator=g) < 0.0005, -1)
    real = (hi ^ flip)
    real = (real | real.t()).float().contiguous()
    s = torch.randn(n, n, device=dev, generator=g).abs_() * 0.01
    s = torch.where(hi, 0.8 + 0.05 * torch.randn(n, n, device=dev, generator=g), s)
    s = torch.tril(s, -1)
    return real, (s + s.t()).contiguous()


def timed(fn, reps):
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return out, ts[len(ts) // 2], ts[0], ts[-1]


def torch_ints(real, pred):
    """The header and the five columns from torch, int64 throughout."""
    n = real.shape[0]
    i, j = torch.tril_indices(n, n, -1, device=dev)
    lab = real[i, j] == 1
    s = pred[i, j]
    pos, neg = s[lab], s[~lab]
    sp, sn = torch.sort(pos).values, torch.sort(neg).values
    ap = torch.searchsorted(sn, pos) + torch.searchsorted(sn, pos, right=True)
    bq = 2 * pos.numel() - torch.searchsorted(sp, neg) - torch.searchsorted(sp, neg, right=True)
    cols = torch.zeros(5, n, device=dev, dtype=torch.int64)
    for end in (i, j):
        cols[0].index_add_(0, end[lab], torch.ones_like(ap))
        cols[2].index_add_(0, end[lab], ap)
        cols[3].index_add_(0, end[~lab], bq)
    cols[1] = n - 1 - cols[0]
    # C_v: row v of the symmetric matrix of the lower triangle, its negatives sorted, its positives searched among them
    sym = torch.tril(pred, -1)
    sym = sym + sym.t()
    lsym = torch.tril(real, -1) == 1
    lsym = lsym | lsym.t()
    inf = torch.full_like(sym, float("inf"))
    negs = torch.where(lsym, inf, sym)
    negs.fill_diagonal_(float("inf"))
    negs = torch.sort(negs, dim=1).values                                    # the N_v negatives of the row, then +inf
    both = torch.searchsorted(negs, sym) + torch.searchsorted(negs, sym, right=True)
    cols[4] = torch.where(lsym, both, torch.zeros_like(both)).sum(1)
    return [int(lab.sum()), int(ap.sum())] + cols.tolist()


say("ms per call, host clock around work that ends in a device synchronise (the wrappers' own synchronisations, allocations and "
    "host arithmetic included); 2 warm-up calls of every route, then two passes of 10 calls per route, the routes alternating")
for n in (2708, 10000):
    real, pred = bench_graph(n, n)
    m = n * (n - 1) // 2
    routes = (("hip_nodes_ints", lambda: E._node_jackknife_ints(real, pred, None)),
              ("hip_nodes_full", lambda: E.auc_node_jackknife(real, pred)),
              ("hip_delong", lambda: E.auc_delong(real, pred)),
              ("torch_nodes_ints", lambda: torch_ints(real, pred)))
    for _ in range(2):                                      # warm-up of every shape that is timed
        for _, fn in routes:
            fn()
    reps = 10
    res = {}
    for _ in range(2):                                      # two alternating passes: the spread between them is the noise
        for name, fn in routes:
            out, med, lo, hi = timed(fn, reps)
            res.setdefault(name, []).append((med, lo, hi))
            res[name + "_out"] = out
    d, dl, g, t = res["hip_nodes_full_out"], res["hip_delong_out"], res["hip_nodes_ints_out"], res["torch_nodes_ints_out"]
    same = [t[0] == g["positives"], t[1] == g["T"]] + [t[2 + q] == g[k] for q, k in enumerate(E.NODE_JACKKNIFE_COLUMNS)]
    header = all(g[k] == dl["ints"][k] for k in ("pairs", "positives", "negatives", "T")) and g == d["ints"]
    say(f"n = {n}, m = {m} pairs, every node selected, P = {d['positives']}, N = {d['negatives']}; bench-shaped modified_adj "
        f"(edges near 0.8, the rest |N(0, 0.01)|)")
    say(f"  auc_node_jackknife: auc = {d['auc']!r}, auc_jackknife = {d['auc_jackknife']!r}, se_nodes = {d['se']!r}, "
        f"95 % CI = [{d['ci_low']!r}, {d['ci_high']!r}], undefined_nodes = {d['undefined_nodes']}")
    say(f"  auc_delong:         auc = {dl['auc']!r}, se = {dl['se']!r}; se_nodes / se = {d['se'] / dl['se']!r}")
    for name, _ in routes:
        a, b = res[name]
        say(f"  {name:16s} median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:8.3f} ms "
            f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, host clock around a device synchronise]")
    say(f"  the torch composition returns the same integers (P, T, P_v, N_v, A_v, B_v, C_v): {same}; the header is "
        f"auc_delong's: {header}")
    del real, pred, res
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "auc_node_jackknife.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
