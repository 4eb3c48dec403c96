"""Times engine.topk_metrics / engine.top_pairs against the torch route (tril_indices gather + stable descending sort + label
gather) at N = 10 000 on the modified_adj of a short bench-shaped attack, k = P, and checks that both routes return the
same pairs.  python scripts/topk_select_bench.py [OUT.txt]  ->  profiles/topk_select.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import mcgra_loader

pkg = mcgra_loader.load()
from mc_gra_amd import engine as E

dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


eng, inp, adj = bench.build_engine(pkg, torch, dev, "synthetic-10k-hsic", 0)
for _ in range(10):
    eng.step()
lab = torch.as_tensor(inp["labels"], device=dev)
label_adj = (lab[:, None] == lab[None, :]).float()
final = eng.finalize(0, eng.buffer("HA"), eng.buffer("YA"), label_adj)
del label_adj, eng
torch.cuda.synchronize()
n = final.shape[0]
say(f"N = {n}, modified_adj after 10 steps of synthetic-10k-hsic + finalize; distinct scores in the lower triangle: "
    f"{int(torch.unique(final[torch.tril(torch.ones(n, n, dtype=torch.bool, device=dev), -1)]).numel())}")


def ours_metrics():
    return E.topk_metrics(adj, final, 0)


P = ours_metrics()["positives"]


def ours_pairs():
    return E.top_pairs(final, P, None, adj)


def torch_route(keep_index):
    ij = keep_index if keep_index is not None else torch.tril_indices(n, n, -1, device=dev)
    s = final[ij[0], ij[1]]
    vals, order = torch.sort(s, stable=True, descending=True)
    top = order[:P]
    pairs = torch.stack([ij[0][top], ij[1][top]], 1)
    hits = adj[pairs[:, 0], pairs[:, 1]] == 1
    tp = int(hits.sum())
    return pairs, vals[:P], hits, tp


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


ij = torch.tril_indices(n, n, -1, device=dev)
routes = {"engine.topk_metrics (k = P)": ours_metrics, "engine.top_pairs (k = P, with hits)": ours_pairs,
          "torch: tril_indices + gather + stable sort + label gather": lambda: torch_route(None),
          "torch: the same, index tensors prebuilt": lambda: torch_route(ij)}
for f in routes.values():                     # warm-up of every shape
    f(); f()
times = {k: [] for k in routes}
for rep in range(7):                          # interleaved
    for k, f in routes.items():
        times[k].append(timed(f)[0])
m = ours_metrics()
pairs, scores, hits = ours_pairs()
tp_pairs, tp_scores, tp_hits, tp = torch_route(ij)
say(f"k = P = {P}, TP = {m['hits']}, F1 = {m['f1']:.6f}, threshold = {m['threshold']!r}; torch route TP = {tp}")
say(f"same pairs as the torch route: {bool(torch.equal(pairs, tp_pairs))}, same scores: {bool(torch.equal(scores, tp_scores))}, "
    f"same hits: {bool(torch.equal(hits, tp_hits))}")
say("wall ms per call (host clock around a call that ends in a device synchronise; 2 warm-up calls, 7 interleaved repeats):")
for k, v in times.items():
    say(f"  {k:62s} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
say(f"peak torch allocation during the run: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
