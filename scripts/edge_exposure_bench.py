"""Times engine.edge_exposure (a bit matrix of the true graph, AND + popcount per edge, a search among the sorted edges) -- the
header and the table alone, then with the per-edge columns -- against the same integers computed with torch on the device in the
same process (a tril_indices gather of labels and scores, a sort of the non-edges and two searchsorted for the placements, an
fp16 G @ G read at the edges for the common neighbours, row sums for the degrees, index_add_ for the table) and against
engine.auc_delong on the same input, on the modified_adj of a short bench-shaped attack at N = 10 000 (synthetic-10k-hsic) and at
n = 2 708 (cora-shape-hsic), every node selected, cut at the score of the P-th best pair: device events around each call, the
routes alternating, median of 9 with min - max.  The packed indices of the torch route are built once, outside its timing.
python scripts/edge_exposure_bench.py [OUT.txt]  ->  profiles/edge_exposure.txt"""
import ctypes as C
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


POWERS = None


def torch_route(real, pred, a, b, thr):
    """(header [6], table [16, 16, 3], placement, common, deg) as int64 tensors on the device, every node selected."""
    global POWERS
    if POWERS is None:
        POWERS = torch.tensor([1 << k for k in range(32)], device=real.device, dtype=torch.int64)
    lab = real[a, b] == 1
    s = pred[a, b]
    pos, neg = s[lab], torch.sort(s[~lab]).values
    place = torch.searchsorted(neg, pos, right=False) + torch.searchsorted(neg, pos, right=True)
    low = torch.tril(real == 1, -1)
    G = low | low.t()
    Gh = G.to(torch.float16)
    ea, eb = a[lab], b[lab]
    common = (Gh @ Gh)[ea, eb].to(torch.int64)                # exact: a count below 2048, accumulated in float32
    degree = G.sum(1)
    deg = torch.stack([degree[ea], degree[eb]], 1)
    d = deg.min(1).values
    ec = common.clamp(max=15)
    dc = torch.bucketize(d, POWERS, right=True).clamp(max=15)          # bit_length
    cell = ec * 16 + dc
    above = pos >= thr
    table = torch.zeros(256, 3, device=real.device, dtype=torch.int64)
    table[:, 0] = torch.bincount(cell, minlength=256)
    table[:, 1].index_add_(0, cell, place)
    table[:, 2].index_add_(0, cell, above.to(torch.int64))
    P = pos.numel()
    header = torch.stack([torch.tensor(s.numel(), device=real.device), torch.tensor(P, device=real.device),
                          torch.tensor(neg.numel(), device=real.device), place.sum(), above.sum(), (neg >= thr).sum()])
    return header, table.reshape(16, 16, 3), place, common, deg


def entry_alone(real, pred, thr, header, table):
    """mcgra_edge_exposure itself, header and table: no wrapper, no host arithmetic."""
    n = pred.shape[0]
    p = lambda t: C.c_void_p(t.data_ptr())
    pkg._lib.check(pkg._lib.lib.mcgra_edge_exposure(C.c_void_p(torch.cuda.current_stream().cuda_stream), n, p(real), real.stride(0),
                                                    p(pred), pred.stride(0), None, n, thr, 0, None, None, None, None, None, header, table))
    return list(header)


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


say("ms per call between device events (edge_exposure synchronises inside and forms its stats on the host: both are included; the "
    "torch route ends in one copy of its header to the host); 2 warm-up calls, then 9 repeats alternating the routes; median (min - max)")
for workload in ("synthetic-10k-hsic", "cora-shape-hsic"):
    adj, final = modified_adj(workload)
    n = final.shape[0]
    a, b = torch.tril_indices(n, n, -1, device=dev)
    thr = E.topk_metrics(adj, final, 0)["threshold"]
    header, table = (C.c_int64 * 6)(), (C.c_int64 * 768)()
    routes = {"torch gather, sort, fp16 G @ G": lambda: torch_route(adj, final, a, b, thr)[0].tolist(),
              "mcgra_edge_exposure alone": lambda: entry_alone(adj, final, thr, header, table),
              "edge_exposure (header, table)": lambda: E.edge_exposure(adj, final, None, thr),
              "edge_exposure + columns": lambda: E.edge_exposure(adj, final, None, thr, edges=True),
              "auc_delong": lambda: E.auc_delong(adj, final)}
    for f in routes.values():
        f(); f()
    times = {q: [] for q in routes}
    for rep in range(9):
        for q, f in routes.items():
            times[q].append(event_ms(f)[0])
    say(f"{workload} n = {n}, threshold {thr!r}")
    for q, t in times.items():
        say(f"  {q:32s} {statistics.median(t):9.3f} ms ({min(t):.3f} - {max(t):.3f})")
    th, tt, tplace, tcommon, tdeg = torch_route(adj, final, a, b, thr)
    g = E.edge_exposure(adj, final, None, thr, edges=True)
    same = {"header": th.tolist() == g["ints"], "table": tt.tolist() == [[list(c) for c in row] for row in g["table"]],
            "placement": bool(torch.equal(tplace, g["placement"])), "common": bool(torch.equal(tcommon, g["common"].to(torch.int64))),
            "deg": bool(torch.equal(tdeg, g["deg"].to(torch.int64))),
            "pairs": bool(torch.equal(torch.stack([a, b], 1)[adj[a, b] == 1], g["pairs_list"]))}
    say("  the torch integers equal the kernel's: " + " ".join(f"{k}: {v}" for k, v in same.items()))
    assert all(same.values())
    q = g["stats"]
    e, d = q["by_embeddedness"], q["by_degree"]
    say(f"  m {g['pairs']} P {g['positives']} N {g['negatives']} T {g['T']} above {g['above_pos']} / {g['above_neg']}; pooled AUC "
        f"{q['auc_pooled']!r} (auc_delong {E.auc_delong(adj, final)['auc']!r})")
    say("  by common neighbours (count, AUC): " + " ".join(f"{k}: {c}, {x:.4f}" for k, c, x in zip(e["names"], e["count"], e["auc"]) if c))
    say("  by min degree (count, AUC): " + " ".join(f"{k}: {c}, {x:.4f}" for k, c, x in zip(d["names"], d["count"], d["auc"]) if c))
    del adj, final, a, b, th, tt, tplace, tcommon, tdeg, g
say(f"peak torch allocation during the run: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
