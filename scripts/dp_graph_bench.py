"""Times engine.dp_perturb_graph, the whole call, for EdgeRand and LapGraph at eps = 4 on a graph of the bench's shape (about 8
expected neighbours) at N = 10 000 and n = 2 708, against the same result's torch-on-device counterpart -- torch.rand / compare
for EdgeRand; a Laplace sample plus torch.topk over the tril_indices gather for LapGraph, the indices built outside the timing --
and against numpy on the host.  The other routes draw other bits: the same distribution, not the same graph.  Device events around
each call, 2 warm-up calls, median of 9 with min - max (numpy: a host clock, median of 3).
With `cora`: the privacy-utility sweep of DESIGN.md 3r instead -- the README's HSIC command line on Cora (tests/golden/dataset),
undefended and under both mechanisms at eps = 1, 4, 8, with --ci --exposure.
python scripts/dp_graph_bench.py [measure|cora|all] [OUT.txt]  ->  profiles/dp_graph.txt"""
import json
import lzma
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcgra_loader  # noqa: E402

mcgra_loader.load()
from mc_gra_amd import engine as E  # noqa: E402
from mc_gra_amd import main as M  # noqa: E402

OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, warm=2, reps=9):
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
    return f"{statistics.median(ts):9.3f} ms ({min(ts):.3f} - {max(ts):.3f})"


def host_timed(fn, reps=3):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return f"{statistics.median(ts):9.1f} ms ({min(ts):.1f} - {max(ts):.1f})"


def graph(n, seed=0):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    low = torch.tril(torch.rand(n, n, device="cuda:0", generator=g) < 8.0 / n, -1)
    return (low | low.T).float()


def measure(n, eps):
    A = graph(n)
    m = n * (n - 1) // 2
    Edges = int(A.sum().item()) // 2
    say(f"n = {n}, m = {m}, E = {Edges}, eps = {eps}")
    out = torch.empty(n, n, device="cuda:0")
    _, info = E.dp_perturb_graph(A, "edgerand", eps, 15, out=out)
    say(f"  edgerand: {json.dumps({k: v for k, v in info.items()})}")
    t = timed(lambda: E.dp_perturb_graph(A, "edgerand", eps, 15, out=out))
    moved = (2 * n * n + 4 * n * n) / 1e9
    say(f"  engine.dp_perturb_graph edgerand (whole call)     {t}   [{moved:.3f} GB by design]")
    q = info["flip_probability"]

    def torch_edgerand():
        flip = torch.tril(torch.rand(n, n, device="cuda:0") < q, -1)
        flip = flip | flip.T
        return (A.bool() ^ flip).float()

    say(f"  torch.rand / compare / mirror on the device       {timed(torch_edgerand)}")
    _, info = E.dp_perturb_graph(A, "lapgraph", eps, 15, out=out)
    say(f"  lapgraph: {json.dumps({k: v for k, v in info.items()})}")
    say(f"  engine.dp_perturb_graph lapgraph (whole call)     {timed(lambda: E.dp_perturb_graph(A, 'lapgraph', eps, 15, out=out))}")
    say(f"  engine.dp_perturb_graph lapgraph, want_noisy      {timed(lambda: E.dp_perturb_graph(A, 'lapgraph', eps, 15, want_noisy=True, out=out))}")
    ii, jj = torch.tril_indices(n, n, -1, device="cuda:0")      # (kept outside the timed call: 16 bytes per pair)
    target = max(info["target"], 1)
    lap = torch.distributions.Laplace(torch.tensor(0.0, device="cuda:0"), torch.tensor(1.0 / (0.99 * eps), device="cuda:0"))

    def torch_lapgraph():
        v = A[ii, jj] + lap.sample((m,))
        top = torch.topk(v, target).indices
        o = torch.zeros(n, n, device="cuda:0")
        o[ii[top], jj[top]] = 1.0
        o[jj[top], ii[top]] = 1.0
        return o

    say(f"  torch Laplace sample + topk over the tril gather   {timed(torch_lapgraph, reps=5)}")
    del ii, jj
    Ah = A.cpu().numpy()
    a, b = np.tril_indices(n, -1)
    lab = Ah[a, b]

    def numpy_edgerand():
        flip = np.random.rand(m) < q
        o = np.zeros((n, n), np.float32)
        bits = (lab != 0) ^ flip
        o[a, b] = bits
        o[b, a] = bits
        return o

    def numpy_lapgraph():
        v = lab + np.random.laplace(0.0, 1.0 / (0.99 * eps), m)
        top = np.argpartition(-v, target)[:target]
        o = np.zeros((n, n), np.float32)
        o[a[top], b[top]] = 1.0
        o[b[top], a[top]] = 1.0
        return o

    say(f"  numpy on the host, edgerand (indices prepared)    {host_timed(numpy_edgerand)}")
    say(f"  numpy on the host, lapgraph (indices prepared)    {host_timed(numpy_lapgraph)}")


def cora_sweep():
    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, "dataset")
    os.makedirs(root)
    with lzma.open(os.path.join(ROOT, "tests", "golden", "dataset", "cora.npz.xz")) as src:
        open(os.path.join(root, "cora.npz"), "wb").write(src.read())
    os.chdir(tmp)
    argv = ["--dataset", "cora", "--dataset_root", root, "--measure", "HSIC", "--w1", "0.01", "--w2", "0.01", "--w6", "10", "--w7", "10",
            "--w9", "10", "--w10", "1000", "--lr", "-2", "--useH_A", "--useY_A", "--useY", "--ci", "--exposure"]
    say("Cora, the HSIC command line, 100 epochs, every node selected: mechanism eps | test_accuracy | auc_all | auc_perturbed_all | "
        "exposure AUC of the edges with 0 common neighbours | with >= 2 | edges -> edges_out (kept, added, removed)")
    for mech, eps in [(None, None)] + [(mch, e) for mch in ("edgerand", "lapgraph") for e in (1.0, 4.0, 8.0)]:
        extra = [] if mech is None else ["--dp_defense", mech, "--dp_eps", str(eps)]
        t = time.perf_counter()
        res = M.run(M.build_parser().parse_args(argv + extra))
        emb = res["exposure_all"]["stats"]["by_embeddedness"]
        c, auc = np.array(emb["count"], float), np.array([x if x == x else 0.0 for x in emb["auc"]], float)
        hi = float((c[2:] * auc[2:]).sum() / c[2:].sum()) if c[2:].sum() else float("nan")
        d = res.get("defense", {})
        say(f"  {mech or 'none'} {eps} | {d.get('test_accuracy')} | {res['auc_all']:.4f} | {res.get('auc_perturbed_all', float('nan')):.4f} | "
            f"{auc[0]:.4f} (n={int(c[0])}) | {hi:.4f} (n={int(c[2:].sum())}) | {d.get('edges')} -> {d.get('edges_out')} "
            f"({d.get('kept')}, {d.get('added')}, {d.get('removed')}) | {time.perf_counter() - t:.1f} s")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    say("ms per call between device events (the call synchronises inside and fetches its counts: included); 2 warm-up calls, "
        "9 repeats; median (min - max).  The torch and numpy routes draw other bits: the same distribution, not the same graph")
    if what in ("all", "measure"):
        measure(10000, 4.0)
        measure(2708, 4.0)
        say(f"peak torch allocation: {torch.cuda.max_memory_allocated() >> 20} MiB")
    if what in ("all", "cora"):
        cora_sweep()
