"""Times engine.rank_curves (both curves, drop_intermediate on, best F1) against engine.rank_metrics (AUC + average precision:
the same classify, emit and sorts) on the modified_adj of a short bench-shaped attack, at N = 10 000 (synthetic-10k-hsic; and the same graph under uniform random scores,
where nearly every entry is a level of its own) and at n = 2 708 (cora-shape-hsic): device events around each call, both routes in one process, alternating, median of 9.  At
n = 2 708 also sklearn's roc_curve + precision_recall_curve on the host, for context, and a check that both give the same
points.  python scripts/curves_bench.py [OUT.txt]  ->  profiles/curves.txt"""
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


def modified_adj(workload):
    eng, inp, adj = bench.build_engine(pkg, torch, dev, workload, 0)
    for _ in range(10):
        eng.step()
    lab = torch.as_tensor(inp["labels"], device=dev)
    label_adj = (lab[:, None] == lab[None, :]).float()
    final = eng.finalize(0, eng.buffer("HA"), eng.buffer("YA"), label_adj).clone()
    del label_adj, eng
    torch.cuda.synchronize()
    return adj, final


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


say("ms per call between device events (the calls synchronise inside: host gaps are included); 2 warm-up calls, then 9 "
    "repeats alternating the routes")
say(f"{'workload':20s} {'n':>6s} {'rank_metrics':>13s} {'rank_curves':>12s} {'ratio':>6s}   P, N, levels, ROC points, PR points")
for workload in ("synthetic-10k-hsic", "10k-uniform-scores", "cora-shape-hsic"):
    if workload == "10k-uniform-scores":      # the graph of synthetic-10k-hsic under scores with no large tie: 2^24 values
        adj = torch.as_tensor(bench.make_inputs(*bench.WORKLOADS["synthetic-10k-hsic"][:5], 0)["adj"], device=dev)
        final = torch.rand(adj.shape, device=dev, generator=torch.Generator(dev).manual_seed(0)) * 0.7 + 0.3 * adj
    else:
        adj, final = modified_adj(workload)
    n = final.shape[0]
    routes = {"metrics": lambda: E.rank_metrics(adj, final), "curves": lambda: E.rank_curves(adj, final)}
    for f in routes.values():
        f(); f()
    times = {k: [] for k in routes}
    for rep in range(9):
        for k, f in routes.items():
            times[k].append(event_ms(f)[0])
    c = routes["curves"]()
    auc, ap = routes["metrics"]()
    tm, tc = statistics.median(times["metrics"]), statistics.median(times["curves"])
    say(f"{workload:20s} {n:6d} {tm:13.2f} {tc:12.2f} {tc / tm:6.2f}   {c['positives']}, {c['negatives']}, {c['levels']}, "
        f"{c['roc_points']}, {c['pr_points']}")
    say(f"  rank_metrics min {min(times['metrics']):.2f} max {max(times['metrics']):.2f}; rank_curves min {min(times['curves']):.2f} "
        f"max {max(times['curves']):.2f}; AUC {auc!r} AP {ap!r} best F1 {c['best_f1']['f1']!r} at {c['best_f1']['threshold']!r}")
    fpr, tpr, _ = (t.cpu().numpy() for t in c["roc"])
    say(f"  trapezoid area of the returned ROC - AUC = {float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) * 0.5)) - auc:.3e}")
    if n <= 3000:
        from sklearn.metrics import precision_recall_curve, roc_curve
        y, s = adj.cpu().numpy().reshape(-1), final.cpu().numpy().reshape(-1)
        t0 = time.perf_counter()
        sk_roc = roc_curve(y, s)
        t1 = time.perf_counter()
        sk_pr = precision_recall_curve(y, s, drop_intermediate=True)
        t2 = time.perf_counter()
        same = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(c["roc"] + c["pr"], sk_roc + sk_pr))
        say(f"  sklearn on the host for the same input: roc_curve {(t1 - t0) * 1e3:.0f} ms, precision_recall_curve "
            f"{(t2 - t1) * 1e3:.0f} ms (wall); same arrays as the device curves, bit for bit: {same}")
    del adj, final
say(f"peak torch allocation during the run: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
