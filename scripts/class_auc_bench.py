"""Times engine.class_auc against the same integers composed from torch on the device -- a tril_indices gather of the scores,
the labels and the two ends' classes, a stratum id per pair from the table, one sort of the edges by (stratum, score), two
searchsorted of every non-edge among the edges of its stratum (sort and searches run on the combined key stratum * 2^32 + the
score's order-preserving 32-bit key, so one call serves every stratum), and bincount / index_add_ per stratum -- and beside engine.auc_delong on the same input: a bench-shaped modified_adj at n = 2 708 and N = 10 000 with every
node selected, at the `edges` threshold (the score of the P-th best pair), for C = 7 random classes with the strata `same` and
`blocks` and for C = 16 with `blocks` (136 strata).  The integers are compared for equality and the script fails when they
differ.

    python scripts/class_auc_bench.py [OUT]        # OUT defaults to profiles/class_auc.txt"""
import os
import signal
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcgra_loader  # noqa: E402

mcgra_loader.load()
from mc_gra_amd import engine as E  # noqa: E402

signal.alarm(int(os.environ.get("CLASS_AUC_BENCH_TIMEOUT", "540")))      # a time limit of its own: the default action ends the script
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench_graph(n, seed):
    """(real, pred): 0.1 % of the pairs are edges (0.05 % of all pairs flipped), scored near 0.8; the rest |N(0, 0.01)|: the
    first scoring of scripts/delong_bench.py, scripts/hop_auc_bench.py's input."""
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


def order_key(s):
    """The order-preserving unsigned 32-bit key of a float32 score as an int64 (-0.0 and +0.0 one value)."""
    u = (s + 0.0).view(torch.int32).to(torch.int64) & 0xffffffff                 # -0.0 + 0.0 = +0.0
    return torch.where(u >= 0x80000000, 0xffffffff - u, u | 0x80000000)


def torch_ints(real, pred, cl, table, G, thr):
    """The G rows (pairs_g, P_g, T_g, above_g, hits_g) from torch."""
    n = real.shape[0]
    i, j = torch.tril_indices(n, n, -1, device=real.device)
    s, lab = pred[i, j], real[i, j] == 1
    g = table[cl[i], cl[j]]
    key = (g << 32) | order_key(s)                                               # (stratum, score) as one sortable integer
    edges = torch.sort(key[lab]).values                                          # stratum-major, ascending inside a stratum
    P = torch.bincount(g[lab], minlength=G)
    start = torch.cumsum(P, 0) - P
    lb = torch.searchsorted(edges, key) - start[g]
    ub = torch.searchsorted(edges, key, right=True) - start[g]
    b = torch.where(lab, torch.zeros_like(lb), 2 * P[g] - lb - ub)
    T = torch.zeros(G, dtype=torch.int64, device=real.device).index_add_(0, g, b)
    up = s >= thr
    rows = torch.stack((torch.bincount(g, minlength=G), P, T, torch.bincount(g[up], minlength=G),
                        torch.bincount(g[up & lab], minlength=G)), 1)
    return [tuple(r) for r in rows.tolist()]


say("ms per call, host clock around work that ends in a device synchronise (the wrapper's own synchronisations, allocations, "
    "the classes' copy to the device and host arithmetic included); 2 warm-up calls of every route, then two passes of 10 calls "
    "per route, the routes alternating")
ok = True
for n in (2708, 10000):
    real, pred = bench_graph(n, n)
    m = n * (n - 1) // 2
    thr = E.topk_metrics(real, pred, 0)["threshold"]
    for C, how in ((7, "same"), (7, "blocks"), (16, "blocks")):
        cl = torch.randint(0, C, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(C))
        cl_host = cl.cpu().numpy()
        strata = E.class_strata(C, how)
        table, G = torch.as_tensor(strata[0], device=dev).to(torch.int64), len(strata[1])
        routes = (("hip_class_auc", lambda: E.class_auc(real, pred, cl_host, None, strata, thr)),
                  ("hip_auc_delong", lambda: E.auc_delong(real, pred)),
                  ("torch_ints", lambda: torch_ints(real, pred, cl, table, G, thr)))
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
        d, t, dl = res["hip_class_auc_out"], res["torch_ints_out"], res["hip_auc_delong_out"]
        same = d["ints"] == t
        ok = ok and same
        say(f"n = {n}, m = {m} pairs, every node selected, C = {C} random classes, strata `{how}` (G = {G}), threshold {thr!r} "
            f"(the score of the P-th best pair); bench-shaped modified_adj (edges near 0.8, the rest |N(0, 0.01)|)")
        say(f"  P {sum(d['positives'])}, auc_within {d['auc_within']!r}, auc_adjusted {d['auc_adjusted']!r}, pooled (auc_delong) "
            f"{dl['auc']!r}; first strata {d['ints'][:2]}")
        for name, _ in routes:
            a, b = res[name]
            say(f"  {name:15s} median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:8.3f} ms "
                f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, host clock around a device synchronise]")
        say(f"  the torch composition returns the same integers (pairs, P, T, above, hits of every stratum): {same}")
        del res
    del real, pred
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "class_auc.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "the torch composition and the entry disagree"
