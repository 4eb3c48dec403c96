"""Times engine.influence_scores, the whole call, on a graph of the bench's shape (about 8 expected neighbours, normalised with
self-loops) at N = 10 000 and n = 2 708 for a 2-layer victim of width 16 with 7 classes, against the paper's procedure in torch on
the device -- one perturbed forward per source through the dense A, in batches of sources, differenced -- and against the same with
torch.sparse; and at one point of the dense regime, the n = 2 708 graph under EdgeRand at eps = 1 (about 27 % of the pairs become
edges, so every frontier is every node).  The torch routes subtract two float32 forwards: the same quantity with u |O| / Delta of
cancellation noise, not the same bits.  Device events around each call, 2 warm-up calls, median of 5 with min - max.
python scripts/influence_bench.py [OUT.txt]  ->  profiles/influence.txt"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcgra_loader  # noqa: E402

mcgra_loader.load()
from mc_gra_amd import engine as E  # noqa: E402

OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
lines = []
DELTA = 1e-4


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return f"{statistics.median(ts):10.3f} ms ({min(ts):.3f} - {max(ts):.3f})"


def graph(n, seed=0):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    low = torch.tril(torch.rand(n, n, device="cuda:0", generator=g) < 8.0 / n, -1)
    return (low | low.T).float()


def victim(nfeat, h, nclass, seed=1):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    u = lambda *shape, s: (torch.rand(*shape, device="cuda:0", generator=g) * 2 - 1) * s
    W = [u(nfeat, h, s=h ** -0.5), u(h, h, s=h ** -0.5)]
    b = [u(h, s=h ** -0.5), u(h, s=h ** -0.5)]
    return W, b, u(nclass, h, s=h ** -0.5), u(nclass, s=h ** -0.5)


def forward(T0, A, W, b, Wlin, blin, sparse):
    """The victim behind T0 = X W_0 for a batch of sources: T0 [n, s, h]."""
    n, s, h = T0.shape
    mm = (lambda T: torch.sparse.mm(A, T.reshape(n, -1)).reshape(n, s, -1)) if sparse else (lambda T: (A @ T.reshape(n, -1)).reshape(n, s, -1))
    H = torch.relu(mm(T0) + b[0])
    H = torch.relu(mm(H @ W[1]) + b[1])
    return torch.log_softmax(H @ Wlin.T + blin, dim=-1)


def paper(X, A, W, b, Wlin, blin, sparse, batch):
    """One perturbed forward per source, `batch` sources at a time, minus the base forward; posteriors; max of the two directions."""
    n = X.shape[0]
    As = A.to_sparse_csr() if sparse else A
    T0 = X @ W[0]
    base = torch.exp(forward(T0[:, None, :], As, W, b, Wlin, blin, sparse))[:, 0, :]
    out = torch.empty(n, n, device=X.device)
    for v0 in range(0, n, batch):
        v1 = min(n, v0 + batch)
        T = T0[:, None, :].repeat(1, v1 - v0, 1)
        idx = torch.arange(v0, v1, device=X.device)
        T[idx, idx - v0, :] = (1 + DELTA) * T0[v0:v1]
        P = torch.exp(forward(T, As, W, b, Wlin, blin, sparse))
        out[v0:v1] = ((P - base[:, None, :]).norm(dim=-1) / DELTA).T
    return torch.maximum(out, out.T)


def measure(n, A, nfeat, what, batch):
    W, b, Wlin, blin = victim(nfeat, 16, 7)
    g = torch.Generator(device="cuda:0").manual_seed(2)
    X = (torch.rand(n, nfeat, device="cuda:0", generator=g) < 5.0 / nfeat).float()
    X = X / X.sum(1, keepdim=True).clamp(min=1)
    An = E.normalize_adj_tensor(A)
    S, info = E.influence_scores((W, b, Wlin, blin), X, An, DELTA, "posteriors", "max")
    say(f"n = {n}, nfeat = {nfeat}, {what}: nnz = {info['nnz']}, reached = {info['reached']} ({info['reached'] / n:.1f} a source), "
        f"max_reach = {info['max_reach']}")
    say(f"  engine.influence_scores posteriors max (whole call)        {timed(lambda: E.influence_scores((W, b, Wlin, blin), X, An, DELTA, 'posteriors', 'max'))}")
    say(f"  engine.influence_scores log_posteriors directed            {timed(lambda: E.influence_scores((W, b, Wlin, blin), X, An, DELTA, 'log_posteriors', 'directed'))}")
    ref = paper(X, An, W, b, Wlin, blin, False, batch)
    scale = float(ref.abs().max())
    say(f"  largest |engine - torch| = {float((S - ref).abs().max()):.3e} of a largest score {scale:.3e} (torch subtracts two float32 forwards)")
    del ref
    say(f"  torch, dense A, {batch} sources a batch                         {timed(lambda: paper(X, An, W, b, Wlin, blin, False, batch), warm=1, reps=3)}")
    say(f"  torch.sparse (CSR), {batch} sources a batch                     {timed(lambda: paper(X, An, W, b, Wlin, blin, True, batch), warm=1, reps=3)}")


if __name__ == "__main__":
    say("ms per call between device events (the call synchronises inside and fetches its counts: included); 2 warm-up calls, "
        "5 repeats (torch: 1 and 3); median (min - max).  L = 2, h = 16, 7 classes, delta = 1e-4")
    measure(10000, graph(10000), 1433, "bench-shaped graph", 250)
    measure(2708, graph(2708), 1433, "bench-shaped graph", 677)
    dense, dp = E.dp_perturb_graph(graph(2708), "edgerand", 1.0, 15)
    measure(2708, dense, 1433, f"EdgeRand eps = 1 ({dp['edges_out']} edges: the dense regime)", 677)
    say(f"peak torch allocation: {torch.cuda.max_memory_allocated() >> 20} MiB")
