"""Times the link-stealing pair distances -- engine.pair_distance_rank_metrics (scores never stored) and
engine.pair_distance_scores (the n x n matrix) -- against the same result from torch on the device: torch.cdist where it applies
(euclidean, sqeuclidean as its square, cityblock, chebyshev), a normalised product for cosine and correlation, chunked
broadcasting for braycurtis and canberra, then engine.auc_delong on that matrix.  Sizes: N = 10 000 with d = 16 and d = 128,
n = 2 708 with d = 7 (softmax rows) and d = 1 433, every node selected, per metric.  The torch route's integers are compared
with the entry's where its float32 scores are the same bits as pair_distance_scores'; where they are not, the number of
differing entries is reported beside both AUCs.

    python scripts/pair_distance_bench.py [OUT]        # OUT defaults to profiles/pair_distance.txt"""
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcgra_loader  # noqa: E402

mcgra_loader.load()
from mc_gra_amd import engine as E  # noqa: E402

signal.alarm(int(os.environ.get("PAIR_DISTANCE_BENCH_TIMEOUT", "540")))      # a time limit of its own: the default action ends the script
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench_input(n, d, softmax, seed):
    """(real, Z): four planted groups, about 12 % edges (36 % inside a group, 4 % across); rows = group centre + noise."""
    g = torch.Generator(device=dev).manual_seed(seed)
    grp = torch.randint(0, 4, (n,), device=dev, generator=g)
    prob = torch.where(grp[:, None] == grp[None, :], 0.36, 0.04)
    up = torch.triu(torch.rand(n, n, device=dev, generator=g) < prob, 1)
    real = (up | up.t()).float().contiguous()
    Z = torch.randn(n, d, device=dev, generator=g) + torch.randn(4, d, device=dev, generator=g)[grp]
    return real, (torch.softmax(1.5 * Z, 1) if softmax else 0.8 * Z).contiguous()


CDIST = {"euclidean": 2.0, "sqeuclidean": 2.0, "cityblock": 1.0, "chebyshev": float("inf")}


def torch_scores(Z, metric, cdist=True):
    """0 - dist as torch computes it (not the entry's chains: cdist and the product sum in another order).  cdist=False: the
    four cdist metrics by chunked broadcasting too."""
    n, d = Z.shape
    if metric in CDIST and cdist:
        D = torch.cdist(Z, Z, p=CDIST[metric], compute_mode="donot_use_mm_for_euclid_dist")
        return 0.0 - (D * D if metric == "sqeuclidean" else D)
    if metric in ("cosine", "correlation"):
        C = Z - Z.mean(1, keepdim=True) if metric == "correlation" else Z
        Zn = C / C.norm(dim=1, keepdim=True).clamp_min(1e-12)
        return 0.0 - (1.0 - Zn @ Zn.t()).clamp_min(0.0)
    out = torch.empty(n, n, device=Z.device, dtype=Z.dtype)
    rows = max(1, (64 << 20) // (n * d))                                      # 256 MB of float32 per broadcast chunk
    for r0 in range(0, n, rows):
        a, b = Z[r0:r0 + rows, None, :], Z[None, :, :]
        num = (a - b).abs()
        if metric == "braycurtis":
            den = (a + b).abs().sum(2)
            out[r0:r0 + rows] = torch.where(den == 0, torch.zeros_like(den), num.sum(2) / den)
        elif metric == "canberra":
            den = a.abs() + b.abs()
            out[r0:r0 + rows] = torch.where(den == 0, torch.zeros_like(den), num / den).sum(2)
        elif metric == "chebyshev":
            out[r0:r0 + rows] = num.amax(2)
        elif metric == "cityblock":
            out[r0:r0 + rows] = num.sum(2)
        else:
            sq = (num * num).sum(2)
            out[r0:r0 + rows] = sq.sqrt() if metric == "euclidean" else sq
    return 0.0 - out


def sample_error(S, Z, metric):
    """max |S - float64| over the first and the last 32 rows of an n x n score matrix, relative to the largest |score| there
    (inf when S holds a NaN or an infinity there)."""
    k = torch.cat((torch.arange(32, device=dev), torch.arange(Z.shape[0] - 32, Z.shape[0], device=dev)))
    Zd = Z.double()
    if metric in ("cosine", "correlation"):
        C = Zd - Zd.mean(1, keepdim=True) if metric == "correlation" else Zd
        Zn = C / C.norm(dim=1, keepdim=True).clamp_min(1e-12)
        ref = (1.0 - Zn[k] @ Zn.t()).clamp_min(0.0)
    else:
        a, b = Zd[k][:, None, :], Zd[None, :, :]
        num = (a - b).abs()
        ref = {"braycurtis": lambda: num.sum(2) / (a + b).abs().sum(2).clamp_min(1e-300),
               "canberra": lambda: (num / (a.abs() + b.abs()).clamp_min(1e-300)).sum(2),
               "chebyshev": lambda: num.amax(2), "cityblock": lambda: num.sum(2),
               "euclidean": lambda: (num * num).sum(2).sqrt(), "sqeuclidean": lambda: (num * num).sum(2)}[metric]()
    err = (S[k].double() + ref).abs()                 # S = 0 - dist
    return float((err.max() / ref.max().clamp_min(1e-300)).item()) if bool(torch.isfinite(err).all()) else float("inf")


def timed(fn, reps):
    """(result, median, min, max) in ms by device events around each call."""
    ts = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    ts.sort()
    return out, ts[len(ts) // 2], ts[0], ts[-1]


say("ms per call by device events around the call (the wrappers' own synchronisations, allocations and host arithmetic included); "
    "1 warm-up call of every route, then two passes of 5 calls per route, the routes alternating")
ok = True
for n, d, softmax in ((10000, 16, False), (10000, 128, False), (2708, 7, True), (2708, 1433, False)):
    real, Z = bench_input(n, d, softmax, n + d)
    say(f"n = {n}, d = {d} ({'softmax rows' if softmax else 'group centre + noise'}), m = {n * (n - 1) // 2} pairs, every node selected, "
        f"{int(torch.tril(real, -1).sum().item())} edges")
    for metric in E.PAIR_METRICS:
        # torch.cdist is the baseline where it applies and is right: its values are checked against float64 on 64 rows first
        cdist = metric not in CDIST or sample_error(torch_scores(Z, metric), Z, metric) < 1e-4
        routes = (("hip_rank_metrics", lambda: E.pair_distance_rank_metrics(real, Z, metric)),
                  ("hip_scores", lambda: E.pair_distance_scores(Z, metric)),
                  ("hip_scores+delong", lambda: E.auc_delong(real, E.pair_distance_scores(Z, metric))),
                  ("torch_scores", lambda: torch_scores(Z, metric, cdist)),
                  ("torch_scores+delong", lambda: E.auc_delong(real, torch_scores(Z, metric, cdist))))
        for _, fn in routes:
            fn()
        res = {}
        for _ in range(2):
            for name, fn in routes:
                out, med, lo, hi = timed(fn, 5)
                res.setdefault(name, []).append((med, lo, hi))
                res[name + "_out"] = out
        r, dl, tdl = res["hip_rank_metrics_out"], res["hip_scores+delong_out"], res["torch_scores+delong_out"]
        own = (r["pairs"], r["positives"], r["negatives"], r["T"]) == (dl["pairs"], dl["positives"], dl["negatives"], dl["ints"]["T"])
        ok = ok and own and r["auc"] == dl["auc"]
        differ = int((res["hip_scores_out"].view(torch.int32) != (res["torch_scores_out"] + 0.0).view(torch.int32)).sum().item())
        same_ints = r["T"] == tdl["ints"]["T"]
        if differ == 0:
            ok = ok and same_ints
        say(f"  {metric}: auc {r['auc']!r}, ap {r['ap']!r}; ranked pair by pair == auc_delong on the materialised matrix: {own}")
        say(f"    against float64 on 64 rows, relative to the largest score: the entry {sample_error(res['hip_scores_out'], Z, metric):.2e}, "
            f"torch {sample_error(res['torch_scores_out'], Z, metric):.2e}"
            + ("" if cdist else "  [torch.cdist was wrong at this size on this build (checked on the same rows): the torch route is chunked broadcasting]"))
        for name, _ in routes:
            a, b = res[name]
            say(f"    {name:20s} median {a[0]:9.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | second pass median {b[0]:9.3f} ms "
                f"(min {b[1]:.3f}, max {b[2]:.3f})")
        say(f"    torch's float32 scores differ from the entry's in {differ} of {n * n} entries; its auc {tdl['auc']!r}, "
            f"T the same integer: {same_ints}")
        del res
    del real, Z
    torch.cuda.empty_cache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pair_distance.txt")
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "the entries disagree with auc_delong on the materialised matrix"
