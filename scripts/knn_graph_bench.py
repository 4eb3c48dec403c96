"""Times engine.knn_graph (a radix select of each row in LDS, bit matrices, popcounts) -- the header and the seven columns alone,
then with the union's edge list, then with the lists -- against the same integers computed with torch on the device in the same
process (torch.topk per row with the diagonal masked, a scatter into a bool matrix, | and & with its transpose, row sums) and
against engine.node_rank_metrics on the same input, which sorts whole rows, on the modified_adj of a short bench-shaped attack at
N = 10 000 (synthetic-10k-hsic) and at n = 2 708 (cora-shape-hsic), for k = 8 and k = 64: device events around each call, the
routes alternating, median of 9 with min - max.  modified_adj has ties, which torch.topk breaks as it likes, so the lists are
compared as sets on a tie-free matrix of the same size (every row a permutation), and on modified_adj the rows whose sets differ
are counted beside the rows whose k-th and (k + 1)-th scores tie.
python scripts/knn_graph_bench.py [OUT.txt]  ->  profiles/knn_graph.txt"""
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


def torch_route(real, pred, k):
    """(D as a bool matrix, [n, 7] int64 on the device: in, d_U, d_M, d_G, h_D, h_U, h_M), every node selected."""
    n = pred.shape[0]
    s = pred.clone()
    s.fill_diagonal_(float("-inf"))
    nn = torch.topk(s, k, dim=1).indices
    D = torch.zeros(n, n, dtype=torch.bool, device=pred.device)
    D.scatter_(1, nn, True)
    Dt = D.t()
    U, Mu = D | Dt, D & Dt
    low = torch.tril(real == 1, -1)
    G = low | low.t()
    cols = (Dt.sum(1), U.sum(1), Mu.sum(1), G.sum(1), (D & G).sum(1), (U & G).sum(1), (Mu & G).sum(1))
    return D, torch.stack(cols, 1)


def kernel_cols(g):
    return torch.stack([g[q] for q in E.KNN_COLUMNS], 1)


def entry_alone(real, pred, k, out):
    """mcgra_knn_graph itself, header and columns, into a buffer allocated once: no wrapper, no host arithmetic."""
    import ctypes as C
    n = pred.shape[0]
    header = (C.c_int64 * 8)()
    p = lambda t: C.c_void_p(t.data_ptr())
    pkg._lib.check(pkg._lib.lib.mcgra_knn_graph(C.c_void_p(torch.cuda.current_stream().cuda_stream), n, p(pred), pred.stride(0),
                                                p(real), real.stride(0), None, n, k, header, p(out), None, 0, None, None, None, None))
    return list(header)


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def lists_as_matrix(nn, n):
    D = torch.zeros(n, n, dtype=torch.bool, device=nn.device)
    D.scatter_(1, nn.to(torch.int64), True)
    return D


say("ms per call between device events (knn_graph synchronises inside and forms its stats on the host: both are included); "
    "2 warm-up calls, then 9 repeats alternating the routes; median (min - max)")
for workload in ("synthetic-10k-hsic", "cora-shape-hsic"):
    adj, final = modified_adj(workload)
    n = final.shape[0]
    free = torch.rand(n, n, device=dev).argsort(1).to(torch.float32)          # every row a permutation: no ties within a row
    for k in (8, 64):
        out = torch.empty(n, 7, device=dev, dtype=torch.int64)
        routes = {"torch topk + bool matrices": lambda: torch_route(adj, final, k),
                  "mcgra_knn_graph alone": lambda: entry_alone(adj, final, k, out),
                  "knn_graph (header, columns)": lambda: E.knn_graph(final, k, None, adj),
                  "knn_graph + edge list": lambda: E.knn_graph(final, k, None, adj, edges=True),
                  "knn_graph + lists": lambda: E.knn_graph(final, k, None, adj, lists=True),
                  "node_rank_metrics (sorts rows)": lambda: E.node_rank_metrics(adj, final)}
        for f in routes.values():
            f(); f()
        times = {q: [] for q in routes}
        for rep in range(9):
            for q, f in routes.items():
                times[q].append(event_ms(f)[0])
        say(f"{workload} n = {n}, k = {k}")
        for q, t in times.items():
            say(f"  {q:32s} {statistics.median(t):9.3f} ms ({min(t):.3f} - {max(t):.3f})")
        Dt_, want = torch_route(adj, final, k)
        g = E.knn_graph(final, k, None, adj, lists=True)
        Dk = lists_as_matrix(g["lists"], n)
        s = final.clone()
        s.fill_diagonal_(float("-inf"))
        top = torch.topk(s, k + 1, dim=1).values
        tied = int((top[:, k - 1] == top[:, k]).sum())
        differ = int((Dk != Dt_).any(1).sum())
        say(f"  modified_adj: rows whose k-th and (k + 1)-th scores tie: {tied}; rows whose list differs from torch.topk's as a "
            f"set: {differ}; the seven columns equal: {bool(torch.equal(want, kernel_cols(g)))}")
        Df, wantf = torch_route(adj, free, k)
        gf = E.knn_graph(free, k, None, adj, lists=True)
        same_sets = bool(torch.equal(lists_as_matrix(gf["lists"], n), Df))
        say(f"  tie-free matrix of the same size: the lists are the same sets: {same_sets}; the seven columns equal: "
            f"{bool(torch.equal(wantf, kernel_cols(gf)))}")
        assert same_sets and torch.equal(wantf, kernel_cols(gf))
        q = g["stats"]
        say(f"  E_U {g['E_U']} E_M {g['E_M']} E_G {g['E_G']}; union f1 {q['union']['f1']!r} mutual f1 {q['mutual']['f1']!r}; "
            f"max_in {q['hubness']['max_in']} orphans {q['hubness']['orphans']} skewness {q['hubness']['skewness']!r}")
        del Dt_, want, g, Dk, s, top, Df, wantf, gf
    del adj, final, free
say(f"peak torch allocation during the run: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
