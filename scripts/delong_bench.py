"""Times engine.auc_delong / engine.auc_delong_paired against the same sums composed from torch on the device (a tril_indices
gather, torch.sort of each class, torch.searchsorted both ways, float64 sums of the placements, their squares and products),
on a bench-shaped modified_adj and a second, noisier scoring of the same graph, at n = 2 708 and N = 10 000 with every node
selected.  The torch sums are float64, so the two routes are compared to a relative 1e-12, not for equality.

    python scripts/delong_bench.py [OUT]        # OUT defaults to profiles/auc_delong.txt"""
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
    """(real, pred_a, pred_b): 0.1 % of the pairs are edges (0.05 % of all pairs flipped), scored near 0.8 by both scorings;
    the rest |N(0, 0.01)| under A and |N(0, 0.3)| under B."""
    g = torch.Generator(device=dev).manual_seed(seed)
    hi = torch.tril(torch.rand(n, n, device=dev, generator=g) < 0.001, -1)
    flip = torch.tril(torch.rand(n, n, device=dev, generator=g) < 0.0005, -1)
    real = (hi ^ flip)
    real = (real | real.t()).float().contiguous()

    def scoring(noise):
        s = torch.randn(n, n, device=dev, generator=g).abs_() * noise
        s = torch.where(hi, 0.8 + 0.05 * torch.randn(n, n, device=dev, generator=g), s)
        s = torch.tril(s, -1)
        return (s + s.t()).contiguous()

    return real, scoring(0.01), scoring(0.3)


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


def torch_placements(lab, s):
    pos, neg = s[lab], s[~lab]
    sp, sn = torch.sort(pos).values, torch.sort(neg).values
    a = torch.searchsorted(sn, pos) + torch.searchsorted(sn, pos, right=True)
    b = 2 * pos.numel() - torch.searchsorted(sp, neg) - torch.searchsorted(sp, neg, right=True)
    return a.double(), b.double()


def torch_single(real, pred):
    n = real.shape[0]
    i, j = torch.tril_indices(n, n, -1, device=dev)
    lab = real[i, j] == 1
    a, b = torch_placements(lab, pred[i, j])
    return [float(x) for x in (lab.sum(), a.sum(), (a * a).sum(), (b * b).sum())]


def torch_paired(real, pa, pb):
    n = real.shape[0]
    i, j = torch.tril_indices(n, n, -1, device=dev)
    lab = real[i, j] == 1
    aa, ba = torch_placements(lab, pa[i, j])
    ab, bb = torch_placements(lab, pb[i, j])
    return [float(x) for x in (lab.sum(), aa.sum(), ab.sum(), (aa * aa).sum(), (ba * ba).sum(), (ab * ab).sum(), (bb * bb).sum(),
                               (aa * ab).sum(), (ba * bb).sum())]


def close(x, y):
    return abs(float(x) - float(y)) <= 1e-12 * max(abs(float(x)), abs(float(y)), 1.0)


say("ms per call, host clock around work that ends in a device synchronise (the wrappers' own synchronisations, allocations and "
    "host arithmetic included); 2 warm-up calls of every route, then two passes of 10 calls per route, the routes alternating")
for n in (2708, 10000):
    real, pa, pb = bench_graph(n, n)
    m = n * (n - 1) // 2
    for _ in range(2):                                      # warm-up of every shape that is timed
        E.auc_delong(real, pa)
        E.auc_delong_paired(real, pa, pb)
        torch_single(real, pa)
        torch_paired(real, pa, pb)
    reps = 10
    res = {}
    for _ in range(2):                                      # two alternating passes: the spread between them is the noise
        for name, fn in (("hip_single", lambda: E.auc_delong(real, pa)),
                         ("torch_single", lambda: torch_single(real, pa)),
                         ("hip_paired", lambda: E.auc_delong_paired(real, pa, pb)),
                         ("torch_paired", lambda: torch_paired(real, pa, pb))):
            out, med, lo, hi = timed(fn, reps)
            res.setdefault(name, []).append((med, lo, hi))
            res[name + "_out"] = out
    d, p = res["hip_single_out"], res["hip_paired_out"]
    g = p["ints"]
    ok_single = all(close(x, y) for x, y in zip(res["torch_single_out"], (d["positives"], d["ints"]["T"], d["ints"]["A2"], d["ints"]["B2"])))
    ok_paired = all(close(x, y) for x, y in zip(res["torch_paired_out"], (g["positives"], g["T_a"], g["T_b"], g["A2_a"], g["B2_a"], g["A2_b"],
                                                                          g["B2_b"], g["A_ab"], g["B_ab"])))
    say(f"n = {n}, m = {m} pairs, every node selected, P = {d['positives']}, N = {d['negatives']}; bench-shaped modified_adj "
        f"(edges near 0.8, the rest |N(0, 0.01)|) against a second scoring (the rest |N(0, 0.3)|)")
    say(f"  auc_delong: auc = {d['auc']!r}, se = {d['se']!r}, 95 % CI = [{d['ci_low']!r}, {d['ci_high']!r}]")
    say(f"  auc_delong_paired: auc_b = {p['b']['auc']!r}, delta = {p['delta']!r}, se_delta = {p['se_delta']!r}, z = {p['z']!r}, "
        f"p = {p['p_value']!r}")
    for name in ("hip_single", "torch_single", "hip_paired", "torch_paired"):
        a, b = res[name]
        say(f"  {name:12s} median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:8.3f} ms "
            f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, host clock around a device synchronise]")
    say(f"  torch float64 sums agree with the integers to a relative 1e-12: single {ok_single}, paired {ok_paired}")
    del real, pa, pb, res
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "auc_delong.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
