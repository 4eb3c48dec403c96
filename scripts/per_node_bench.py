"""Times engine.node_rank_metrics (one workgroup per row, ranked in LDS) against the same five integers per node computed with
torch on the device in the same process -- a per-row stable torch.sort plus cumulative sums -- on the modified_adj of a short
bench-shaped attack at N = 10 000 (synthetic-10k-hsic) and at n = 2 708 (cora-shape-hsic): device events around each call, the
two routes alternating, median of 9 with min - max, and a check that both give the same integers.
python scripts/per_node_bench.py [OUT.txt]  ->  profiles/per_node.txt"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def torch_route(real, pred):
    """[n, 5] int64 on the device: P, wins, ties, hits, first_rank of every row, every node selected."""
    n = pred.shape[0]
    c = n - 1
    s = pred.clone()
    s.fill_diagonal_(float("-inf"))                        # the diagonal sorts last and is cut off
    vals, order = torch.sort(s, dim=1, descending=True, stable=True)
    lab = (real.gather(1, order)[:, :c] == 1).to(torch.int64)
    vals = vals[:, :c]
    del s, order
    P = lab.sum(1)
    N = c - P
    neg = torch.cumsum(1 - lab, 1)                         # negatives up to and including each rank
    last = torch.ones(n, c, dtype=torch.bool, device=pred.device)
    last[:, :-1] = vals[:, :-1] != vals[:, 1:]             # a tie group ends here
    head = torch.ones(n, c, dtype=torch.bool, device=pred.device)
    head[:, 1:] = last[:, :-1]
    # negatives down to the end of each rank's group (the nearest end behind it: neg only grows) and before its head
    neg_end = torch.where(last, neg, torch.full_like(neg, c)).flip(1).cummin(1).values.flip(1)
    neg_head = torch.where(head, neg - (1 - lab), torch.zeros_like(neg)).cummax(1).values
    wins = (lab * (N[:, None] - neg_end)).sum(1)
    ties = (lab * (neg_end - neg_head)).sum(1)
    rank = torch.arange(c, device=pred.device)
    hits = (lab * (rank[None, :] < P[:, None])).sum(1)
    head_rank = torch.where(head, rank[None, :].expand(n, c), torch.zeros_like(neg)).cummax(1).values
    first = torch.where(P > 0, 1 + head_rank.gather(1, lab.argmax(1, keepdim=True))[:, 0], torch.zeros_like(P))
    return torch.stack((P, wins, ties, hits, first), 1)


def kernel_route(real, pred):
    m = E.node_rank_metrics(real, pred)
    return torch.stack([m[k] for k in ("positives", "wins", "ties", "hits", "first_rank")], 1), m["summary"]


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


say("ms per call between device events (node_rank_metrics synchronises inside and computes its rates on the host: both are "
    "included); 2 warm-up calls, then 9 repeats alternating the routes")
say(f"{'workload':20s} {'n':>6s} {'torch sort+cumsum':>18s} {'node_rank_metrics':>18s} {'ratio':>6s}")
for workload in ("synthetic-10k-hsic", "cora-shape-hsic"):
    adj, final = modified_adj(workload)
    n = final.shape[0]
    routes = {"torch": lambda: torch_route(adj, final), "kernel": lambda: kernel_route(adj, final)}
    for f in routes.values():
        f(); f()
    times = {k: [] for k in routes}
    for rep in range(9):
        for k, f in routes.items():
            times[k].append(event_ms(f)[0])
    want = routes["torch"]()
    got, summary = routes["kernel"]()
    tt, tk = statistics.median(times["torch"]), statistics.median(times["kernel"])
    say(f"{workload:20s} {n:6d} {tt:18.2f} {tk:18.2f} {tt / tk:6.2f}")
    say(f"  torch min {min(times['torch']):.2f} max {max(times['torch']):.2f}; node_rank_metrics min {min(times['kernel']):.2f} "
        f"max {max(times['kernel']):.2f}; same integers from both routes: {bool(torch.equal(want, got))}")
    say(f"  scored nodes {summary['scored']}, macro AUC {summary['macro_auc']!r}, MRR {summary['mrr']!r}, Hits@1 "
        f"{summary['hits_at_1']!r}, R-precision {summary['r_precision']!r}")
    del adj, final, want, got
say(f"peak torch allocation during the run: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
