"""Times engine.hop_auc against the same integers composed from torch on the device -- the tril mask of the labels symmetrised,
reach_h+1 = reach_h | (reach_h @ G > 0) as an fp16 product (a count that is positive stays positive in any rounding: exact),
a tril_indices gather of the scores and of the H reach matrices, one torch.sort of the edges' scores, two searchsorted of every
non-edge, and bincount / index_add_ per class -- on a bench-shaped modified_adj at n = 2 708 and N = 10 000 with every node
selected, hops = 3, at the `edges` threshold (the score of the P-th best pair), and the same with one node joined to every
node (a hub: one row of the expansion that reads the whole matrix in a single workgroup).  The integers are compared for
equality and the script fails when they differ.

    python scripts/hop_auc_bench.py [OUT]        # OUT defaults to profiles/hop_auc.txt"""
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

signal.alarm(int(os.environ.get("HOP_AUC_BENCH_TIMEOUT", "540")))      # a time limit of its own: the default action ends the script
dev = torch.device("cuda:0")
HOPS = 3
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


def torch_ints(real, pred, thr, hops):
    """The hops + 1 rows (pairs_c, T_c, above_c) from torch."""
    n = real.shape[0]
    low = torch.tril(torch.ones_like(real, dtype=torch.bool), -1)
    G = (real == 1) & low
    G = G | G.t()
    g16 = G.half()
    i, j = torch.tril_indices(n, n, -1, device=real.device)
    reach = G
    cls = torch.full((i.numel(),), hops, dtype=torch.int64, device=real.device)
    for h in range(hops):
        if h:
            reach = reach | ((reach.half() @ g16) > 0)
        cls -= reach[i, j].to(torch.int64)
    s = pred[i, j]
    pos = torch.sort(s[cls == 0]).values
    b = 2 * pos.numel() - torch.searchsorted(pos, s) - torch.searchsorted(pos, s, right=True)
    b = torch.where(cls == 0, torch.zeros_like(b), b)
    count = torch.bincount(cls, minlength=hops + 1)
    T = torch.zeros(hops + 1, dtype=torch.int64, device=real.device).index_add_(0, cls, b)
    above = torch.bincount(cls[s >= thr], minlength=hops + 1)
    T[0] = T[1:].sum()
    return [tuple(r) for r in torch.stack((count, T, above), 1).tolist()]


torch.backends.cuda.matmul.allow_tf32 = False
say("ms per call, host clock around work that ends in a device synchronise (the wrapper's own synchronisations, allocations and "
    "host arithmetic included); 2 warm-up calls of every route, then two passes of 10 calls per route, the routes alternating")
ok = True
for n in (2708, 10000):
    real, pred = bench_graph(n, n)
    m = n * (n - 1) // 2
    hub_real, hub_pred = real.clone(), pred.clone()          # the same graph with node 0 joined to every node: one long row
    hub_real[0, 1:] = hub_real[1:, 0] = 1.0
    hub_pred[0, 1:] = hub_pred[1:, 0] = 0.8
    plain = (real, pred)
    for what in ("bench-shaped modified_adj (edges near 0.8, the rest |N(0, 0.01)|)",
                 "a hub: the same with node 0 joined to every node, scored 0.8, in the graph and in the scores"):
        real, pred = (hub_real, hub_pred) if what.startswith("a hub") else plain
        thr = E.topk_metrics(real, pred, 0)["threshold"]
        routes = (("hip_hop_auc", lambda: E.hop_auc(real, pred, None, HOPS, thr)),
                  ("hip_auc_delong", lambda: E.auc_delong(real, pred)),
                  ("torch_ints", lambda: torch_ints(real, pred, thr, HOPS)))
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
        d, t, dl = res["hip_hop_auc_out"], res["torch_ints_out"], res["hip_auc_delong_out"]
        same = d["ints"] == t
        ok = ok and same and d["auc_pooled"] == dl["auc"]
        say(f"n = {n}, m = {m} pairs, every node selected, hops = {HOPS}, threshold {thr!r} (the score of the P-th best pair); {what}")
        say(f"  distance {d['distance']}: count {d['count']}, T {d['T']}, above {d['above']}")
        say(f"  auc {d['auc']}, pooled {d['auc_pooled']!r} (auc_delong: {dl['auc']!r}), fp_share {d['fp_share']}")
        for name, _ in routes:
            a, b = res[name]
            say(f"  {name:15s} median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:8.3f} ms "
                f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, host clock around a device synchronise]")
        say(f"  the torch composition returns the same integers (pairs, T, above of every class): {same}")
        del res
    del real, pred, plain, hub_real, hub_pred
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hop_auc.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "the torch composition and the entry disagree"
