"""Times engine.subset_auc -- every subset sum ranked in ONE pass over the pairs -- against the obvious alternative on the same
commit: per mask, the torch sum of the components in the same ascending order (one float32 add each) and engine.auc_delong on
that sum.  Input: the bench-shaped graph and modified_adj of the other report benches at n = 2 708 and N = 10 000, every node
selected, as the `learned` summand of an eight-component stack (a second scoring as `feature`, five decode-shaped summands
0.5 + sigmoid noise around a weak signal, and a 0 / 1 label adjacency of 7 random classes); the 21 distinct masks of
engine.ablation_masks(0xff, 0xff) and all 255 masks.  The integers T are compared for equality and the script fails when they
differ.  Both times are written down, whichever is lower.

    python scripts/ablation_bench.py [OUT]        # OUT defaults to profiles/ablation.txt"""
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

signal.alarm(int(os.environ.get("ABLATION_BENCH_TIMEOUT", "540")))      # a time limit of its own: the default action ends the script
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench_graph(n, seed):
    """(real, pred, hi): scripts/class_auc_bench.py's input -- 0.1 % of the pairs are edges (0.05 % of all pairs flipped), scored
    near 0.8; the rest |N(0, 0.01)| -- and the pairs that were scored high."""
    g = torch.Generator(device=dev).manual_seed(seed)
    hi = torch.tril(torch.rand(n, n, device=dev, generator=g) < 0.001, -1)
    flip = torch.tril(torch.rand(n, n, device=dev, generator=g) < 0.0005, -1)
    real = (hi ^ flip)
    real = (real | real.t()).float().contiguous()
    s = torch.randn(n, n, device=dev, generator=g).abs_() * 0.01
    s = torch.where(hi, 0.8 + 0.05 * torch.randn(n, n, device=dev, generator=g), s)
    s = torch.tril(s, -1)
    return real, (s + s.t()).contiguous(), hi | hi.t()


def stack_of(n, pred, hi):
    """The eight summands: pred; a second scoring of the same kind; five times sigmoid(relu(.)) of a weak signal; the label
    adjacency of 7 random classes."""
    g = torch.Generator(device=dev).manual_seed(7 * n)
    comps = torch.empty(8, n, n, device=dev)
    comps[0] = pred
    comps[1] = torch.randn(n, n, device=dev, generator=g).abs_() * 0.01 + 0.4 * hi
    for k in range(2, 7):
        comps[k] = torch.sigmoid(torch.relu(0.3 * torch.randn(n, n, device=dev, generator=g) + 0.2 * hi))
    cl = torch.randint(0, 7, (n,), device=dev, generator=g)
    comps[7] = (cl[:, None] == cl[None, :]).float()
    return comps


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


def one_by_one(real, comps, masks):
    """Per mask: the sum in ascending k, then engine.auc_delong's T."""
    T = []
    for q in masks:
        ks = [k for k in range(8) if q >> k & 1]
        s = comps[ks[0]]
        for k in ks[1:]:
            s = s + comps[k]
        T.append(E.auc_delong(real, s)["ints"]["T"])
    return T


say("ms per call, host clock around work that ends in a device synchronise (the wrappers' own synchronisations, allocations and "
    "host arithmetic included); 1 warm-up call of every route, then two passes of 5 calls per route, the routes alternating")
ok = True
for n in (2708, 10000):
    real, pred, hi = bench_graph(n, n)
    comps = stack_of(n, pred, hi)
    del hi
    m = n * (n - 1) // 2
    for what, masks in (("the table of engine.ablation_masks(0xff, 0xff)", E.ablation_masks(0xff, 0xff)), ("all masks", list(range(1, 256)))):
        routes = (("hip_subset_auc", lambda: E.subset_auc(real, comps, masks)["T"]),
                  ("sum_then_delong", lambda: one_by_one(real, comps, masks)))
        for _, fn in routes:
            fn()
        reps, res = 5, {}
        for _ in range(2):                                      # two alternating passes: the spread between them is the noise
            for name, fn in routes:
                out, med, lo, top = timed(fn, reps)
                res.setdefault(name, []).append((med, lo, top))
                res[name + "_out"] = out
        same = res["hip_subset_auc_out"] == res["sum_then_delong_out"]
        ok = ok and same
        d = E.subset_auc(real, comps, [0xff, 1])
        say(f"n = {n}, m = {m} pairs, every node selected, K = 8 components, {len(masks)} masks ({what}); P {d['positives']}, "
            f"AUC of the full sum {d['auc'][0]!r}, of `learned` alone {d['auc'][1]!r}")
        for name, _ in routes:
            a, b = res[name]
            say(f"  {name:16s} median {a[0]:9.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:9.3f} ms "
                f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, {a[0] / len(masks):.3f} ms per mask]")
        say(f"  the two routes return the same T for every mask: {same}")
        del res
    del real, pred, comps
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ablation.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "the two routes disagree"
