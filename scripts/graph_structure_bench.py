"""Times engine.graph_structure against the same integers composed from torch on the device -- the tril mask of score >=
threshold symmetrised, an fp16 R @ R with fp32 accumulation and fp32 output (every entry is a count below 2^24: exact), * R,
row sums in float64, for R, G and C = R & G -- on a bench-shaped modified_adj at n = 2 708 and N = 10 000 with every node
selected, at the `edges` threshold (the score of the P-th best pair: a sparse graph), at the median score (half the pairs
are edges: the dense case the bit-matrix intersection was NOT built for) and, at 0.5, with one node joined to every node (a
hub: one row that is a single workgroup's work).  The integers are compared for equality and the
script fails when they differ.  The device entry alone and the whole call (with the host's rationals) are timed apart.

    python scripts/graph_structure_bench.py [OUT]        # OUT defaults to profiles/graph_structure.txt"""
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

signal.alarm(int(os.environ.get("GRAPH_STRUCTURE_BENCH_TIMEOUT", "540")))      # a time limit of its own: the default action ends the script
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


def product_f32(a):
    """a @ a of a 0 / 1 fp16 matrix with fp32 accumulation, as fp32 (counts below 2^24: exact)."""
    global PRODUCT
    if PRODUCT != "fp32 operands":
        try:
            out = torch.mm(a, a, out_dtype=torch.float32)
            PRODUCT = "fp16 operands, fp32 accumulation and output (torch.mm out_dtype)"
            return out
        except (TypeError, NotImplementedError, RuntimeError):       # no out_dtype here: fp32 operands, the same exact counts
            PRODUCT = "fp32 operands"
    b = a.float()
    return b @ b


PRODUCT = ""


def torch_ints(real, pred, thr):
    """The header without `pairs` and the six columns from torch."""
    low = torch.tril(torch.ones_like(pred, dtype=torch.bool), -1)
    R = (pred >= thr) & low
    G = (real == 1) & low
    R, G = R | R.t(), G | G.t()
    header, cols = [], []
    for X in (R, G, R & G):
        a = X.half()
        d = X.sum(1, dtype=torch.int64)
        t = ((product_f32(a) * a).sum(1, dtype=torch.float64) / 2).to(torch.int64)
        header += [int(d.sum()) // 2, int(t.sum()) // 3, int((d * (d - 1) // 2).sum())]
        cols += [d, t]
    return header[:8], torch.stack(cols)


torch.backends.cuda.matmul.allow_tf32 = False
say("ms per call, host clock around work that ends in a device synchronise (the wrappers' own synchronisations, allocations and "
    "host arithmetic included); 2 warm-up calls of every route, then two passes of 10 calls per route, the routes alternating")
ok = True
for n in (2708, 10000):
    real, pred = bench_graph(n, n)
    m = n * (n - 1) // 2
    i, j = torch.tril_indices(n, n, -1, device=dev)
    half = float(torch.sort(pred[i, j]).values[m // 2])
    del i, j
    hub_real, hub_pred = real.clone(), pred.clone()          # the same graph with node 0 joined to every node: one long row
    hub_real[0, 1:] = hub_real[1:, 0] = 1.0
    hub_pred[0, 1:] = hub_pred[1:, 0] = 0.8
    plain = (real, pred)
    for what, thr in (("edges: the score of the P-th best pair", E.topk_metrics(real, pred, 0)["threshold"]),
                      ("the median score: half the pairs are edges", half),
                      ("a hub: node 0 joined to every node, scored 0.8, in the graph and in the scores", 0.5)):
        real, pred = (hub_real, hub_pred) if what.startswith("a hub") else plain
        routes = (("hip_ints", lambda: E._graph_structure_ints(pred, thr, None, real)),
                  ("hip_full", lambda: E.graph_structure(pred, thr, None, real)),
                  ("hip_ints_no_labels", lambda: E._graph_structure_ints(pred, thr, None, None)),
                  ("torch_ints", lambda: torch_ints(real, pred, thr)))
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
        (gh, gc), (th, tc), d = res["hip_ints_out"], res["torch_ints_out"], res["hip_full_out"]
        same = gh[1:] == th and bool((gc == tc).all()) and [d[k] for k in E.GRAPH_STRUCTURE_HEADER] == gh
        ok = ok and same
        q = d["stats"]
        say(f"n = {n}, m = {m} pairs, every node selected, threshold {thr!r} ({what}); bench-shaped modified_adj (edges near 0.8, "
            f"the rest |N(0, 0.01)|)")
        say(f"  E_R = {d['E_R']} (density {q['recovered']['density']!r}), T_R = {d['T_R']}, W_R = {d['W_R']}, max degree "
            f"{q['recovered']['max_degree']}; E_G = {d['E_G']}, T_G = {d['T_G']}; E_C = {d['E_C']}, T_C = {d['T_C']}; transitivity "
            f"{q['recovered']['transitivity']!r} (true {q['true']['transitivity']!r}), degree_corr {q['degree_corr']!r}")
        for name, _ in routes:
            a, b = res[name]
            say(f"  {name:18s} median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:8.3f} ms "
                f"(min {b[1]:.3f}, max {b[2]:.3f})   [{reps} calls each, host clock around a device synchronise]")
        say(f"  the torch composition ({PRODUCT}) returns the same integers (E, T, W of R and G, E, T of C, and the six "
            f"columns): {same}")
        del res
    del real, pred, plain, hub_real, hub_pred
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "graph_structure.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "the torch composition and the entry disagree"
