"""Times engine.two_means_split / engine.threshold_pairs against the same answer composed from torch on the device (a
tril_indices gather, a float32 Lloyd of the same number of rounds; a comparison plus nonzero on the gathered tril), on a
bench-shaped modified_adj at n = 2 708 and N = 10 000 with every node selected.

    python scripts/two_means_bench.py [OUT]        # OUT defaults to profiles/two_means.txt"""
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


def bench_adj(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.randn(n, n, device=dev, generator=g).abs_() * 0.01
    hi = torch.rand(n, n, device=dev, generator=g) < 0.001
    s = torch.where(hi, 0.8 + 0.05 * torch.randn(n, n, device=dev, generator=g), s)
    s = torch.tril(s, -1)
    return (s + s.t()).contiguous()


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


def torch_split(adj, rounds):
    n = adj.shape[0]
    i, j = torch.tril_indices(n, n, -1, device=dev)
    s = adj[i, j]
    c_lo, c_hi = s.min(), s.max()
    for _ in range(rounds):
        high = (s - c_hi).abs() < (s - c_lo).abs()
        c_lo, c_hi = s[~high].mean(), s[high].mean()
    return high, s, i, j


def torch_pairs(adj, thr):
    n = adj.shape[0]
    i, j = torch.tril_indices(n, n, -1, device=dev)
    s = adj[i, j]
    at = (s >= thr).nonzero().reshape(-1)
    return torch.stack([i[at], j[at]], 1), s[at]


say("ms per call, host clock around work that ends in a device synchronise (the wrappers' own synchronisations, allocations and "
    "host arithmetic included); 2 warm-up calls of every route, then two passes of 10 calls per route, the routes alternating")
for n in (2708, 10000):
    adj = bench_adj(n, n)
    m = n * (n - 1) // 2
    for _ in range(2):                                      # warm-up of every shape that is timed
        r = E.two_means_split(adj)
        E.threshold_pairs(adj, r["threshold"])
        torch_split(adj, r["iterations"])
        torch_pairs(adj, r["threshold"])
    reps = 10
    res = {}
    for _ in range(2):                                      # two alternating passes: the spread between them is the noise
        for name, fn in (("hip_split", lambda: E.two_means_split(adj)),
                         ("torch_split", lambda: torch_split(adj, r["iterations"])),
                         ("hip_pairs", lambda: E.threshold_pairs(adj, r["threshold"])),
                         ("torch_pairs", lambda: torch_pairs(adj, r["threshold"]))):
            out, med, lo, hi = timed(fn, reps)
            res.setdefault(name, []).append((med, lo, hi))
            res[name + "_out"] = out
    high, s, _, _ = res["torch_split_out"]
    agree = bool(torch.equal(high, s >= r["threshold"]))
    tp = res["torch_pairs_out"]
    hp = res["hip_pairs_out"]
    same_pairs = bool(torch.equal(tp[0], hp[0]) and torch.equal(tp[1], hp[1]))
    say(f"n = {n}, m = {m} pairs, every node selected, bench-shaped modified_adj (0.1 % of pairs near 0.8, the rest |N(0, 0.01)|)")
    say(f"  two_means_split: rounds = {r['iterations']}, converged = {r['converged']}, edges = {r['edges']}, "
        f"threshold = {r['threshold']!r}, threshold_low = {r['threshold_low']!r}")
    for name in ("hip_split", "torch_split", "hip_pairs", "torch_pairs"):
        a, b = res[name]
        say(f"  {name:12s} median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:8.3f} ms "
            f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, host clock around a device synchronise]")
    say(f"  torch float32 Lloyd ({r['iterations']} rounds, same start and tie rule) partition agrees with the split: {agree}; "
        f"torch nonzero pairs equal threshold_pairs element for element: {same_pairs}")
    del adj, res, high, s, tp, hp
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "two_means.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
