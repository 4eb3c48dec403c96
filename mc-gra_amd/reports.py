"""The optional reports of `main.py --mode evaluate` (none is in the reference; main.py's docstring says what each flag asks):
per report the argument check, the computation on the device, the console lines, the --save_* file and the log lines, and at
the bottom the one ordered table of them that main.py's parser, run and log loop over: REPORT_TABLE, which is REPORTS, then
EVERY_REPORT's hops report, then ALL_REPORTS' by_class report, then the ablate report (four tuples that tests pin); what main.py
loops over is EVALUATE_REPORTS, which is REPORT_TABLE and then the knn report (a fifth pinned tuple), followed by LATER_REPORTS,
the reports added since.
To add a report, add an entry to LATER_REPORTS.

`sets` is always index set name -> node ids (None: every node); fail(message) does not return; a --save_* file is written at
exactly the path given.  engine functions are looked up as engine.<fn> at the call."""
import argparse
import collections
from fractions import Fraction

import numpy as np
import torch

from . import engine

SET_TITLES = (("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all"))
CI_LEVEL = 0.95


# what one evaluate run hands its reports: real is the true adjacency on the device of inference_adj (the attack's modified_adj),
# other the second n x n score matrix of --versus and versus the flag as given (both None without it), classes the int64 class
# of every node of --by_class (None without it)
Context = collections.namedtuple("Context", "real inference_adj sets n rank other versus args classes", defaults=(None,))
# Context (whose fields tests pin) and, last, components: what --ablate needs of the attack (None without it): {"stack" the
# [8, n, n] summands of modified_adj on the device, "present", "used" (masks over engine.ENSEMBLE_COMPONENTS), "decode_mode"}.
# What main.py builds; every report reads its fields by name, so either form serves the reports that came before --ablate.
RunContext = collections.namedtuple("RunContext", Context._fields + ("components",), defaults=(None, None))
# RunContext (pinned as well) and, last, defense: what --dp_defense did before the victim was trained (None without it):
# {"perturbed" the graph the victim saw, n x n on the device, "info" engine.dp_perturb_graph's info and "test_accuracy"}.
# real stays the TRUE graph: every report scores the attack against what the defence protects.
DefendedContext = collections.namedtuple("DefendedContext", RunContext._fields + ("defense",), defaults=(None, None, None))


class Report:
    """One optional report: check(args, fail) refuses a bad command line, wanted(args) says whether it is on, compute(ctx) runs
    on every rank and returns the keys to merge into the result, console(res, ctx) and log(res, ctx) return the lines rank 0
    prints and logs, save(res, ctx) writes rank 0's --save_* file when one was asked for."""
    def __init__(self, flags, check, wanted, compute, console, log, save=lambda res, ctx: None):
        self.flags = flags      # the namespace names it owns: hidden from the log's parameter line while it is off
        self.check, self.wanted, self.compute, self.console, self.log, self.save = check, wanted, compute, console, log, save


def _on(flag, given=False):
    """wanted(args) of a report: its flag is set or, with `given` (a flag whose 0 asks for something), there at all."""
    return lambda args: getattr(args, flag, None) is not None if given else bool(getattr(args, flag, None))


def _per_set(res, key):
    """(title, the report's dict) of each index set, in the log's order."""
    return [(title, res[f"{key}_{name}"]) for title, name in SET_TITLES]


def _save_npz(path, **arrays):
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def _save_per_set(path, res, key, ctx, columns):
    """One .npz with, per index set, nodes_<set> and every array of columns(res["<key>_<set>"]) as <name>_<set>."""
    arrays = {}
    for name, ix in ctx.sets.items():
        arrays[f"nodes_{name}"] = np.arange(ctx.n, dtype=np.int64) if ix is None else np.asarray(ix, dtype=np.int64)
        arrays.update({f"{k}_{name}": v for k, v in columns(res[f"{key}_{name}"]).items()})
    _save_npz(path, **arrays)


def check_topk_args(args, fail):
    topk, edges = getattr(args, "topk", None), getattr(args, "save_edges", None)
    if edges and topk is None:
        fail("--save_edges needs --topk")
    if topk is not None and topk < 0:
        fail("--topk takes K >= 0 (0: each index set's own true edge count)")
    if topk is not None and args.mode != "evaluate":
        fail(f"--topk scores the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def topk_report(real, inference_adj, sets, K):
    """--topk K: {"topk_<name>": engine.topk_metrics of the index set}, K clamped to its pair count (K = 0: its true edge count)."""
    out = {}
    for name, ix in sets.items():
        rows = inference_adj.shape[0] if ix is None else len(ix)
        out[f"topk_{name}"] = engine.topk_metrics(real, inference_adj, min(K, rows * (rows - 1) // 2), ix)
    return out


def save_edges(res, ctx):
    """--save_edges: the k best pairs of the whole graph in ranking order (engine.top_pairs)."""
    k = res["topk_all"]["k"]
    if k > 0:
        pairs, scores, hits = (t.cpu().numpy() for t in engine.top_pairs(ctx.inference_adj, k, None, ctx.real))
    else:
        pairs, scores, hits = np.zeros((0, 2), np.int64), np.zeros(0, np.float32), np.zeros(0, bool)
    _save_npz(ctx.args.save_edges, pairs=pairs, scores=scores, hits=hits)


def _topk_log(res, ctx):
    return ["\t".join(f"In {title}: k={d['k']} P={d['precision']} R={d['recall']} F1={d['f1']}" for title, d in _per_set(res, "topk"))]


def check_binarize_args(args, fail):
    binarize, graph = getattr(args, "binarize", False), getattr(args, "save_graph", None)
    if graph and not binarize:
        fail("--save_graph needs --binarize")
    if binarize and args.mode != "evaluate":
        fail(f"--binarize splits the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def save_graph(res, ctx):
    """--save_graph: every pair of the whole graph at or above its split's threshold; a degenerate split: no edges, a NaN threshold."""
    split = res["split_all"]
    if split["degenerate"]:
        pairs, scores, hits, thr = np.zeros((0, 2), np.int64), np.zeros(0, np.float32), np.zeros(0, bool), float("nan")
    else:
        thr = split["threshold"]
        pairs, scores, hits = (t.cpu().numpy() for t in engine.threshold_pairs(ctx.inference_adj, thr, None, ctx.real))
    _save_npz(ctx.args.save_graph, pairs=pairs, scores=scores, hits=hits, threshold=np.float32(thr),
              iterations=np.int64(split["iterations"]))


def _binarize_log(res, ctx):
    return [f"In {title}: split edges={d['edges']} threshold={d['threshold']} rounds={d['iterations']} "
            f"P={d['precision']} R={d['recall']} F1={d['f1']}" for title, d in _per_set(res, "split")]


def check_curves_args(args, fail):
    if getattr(args, "curves", None) and args.mode != "evaluate":
        fail(f"--curves draws the curves of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def curves_report(ctx):
    """--curves PATH: the ROC curve (drop_intermediate on, as the reference's roc_curve call) and the precision-recall curve (off,
    sklearn's default) of each index set, written by rank 0 as one .npz.  Returns {"curves_<name>": point counts and best F1}."""
    out, arrays = {}, {}
    for name, ix in ctx.sets.items():
        c = engine.rank_curves(ctx.real, ctx.inference_adj, ix)
        pr = engine.precision_recall_curve(ctx.real, ctx.inference_adj, ix)
        for k, t in zip(("fpr", "tpr", "thresholds"), c["roc"]):
            arrays[f"roc_{k}_{name}"] = t.cpu().numpy()
        for k, t in zip(("precision", "recall", "thresholds"), pr):
            arrays[f"pr_{k}_{name}"] = t.cpu().numpy()
        out[f"curves_{name}"] = {"roc_points": c["roc_points"], "pr_points": int(pr[2].numel()), "levels": c["levels"],
                                 "best_f1": c["best_f1"]["f1"], "best_threshold": c["best_f1"]["threshold"]}
    if ctx.rank == 0:
        _save_npz(ctx.args.curves, **arrays)
    return out


def _curves_log(res, ctx):
    return ["\t".join(f"In {title}: ROC points={d['roc_points']} PR points={d['pr_points']} levels={d['levels']} "
                      f"best F1={d['best_f1']} at {d['best_threshold']}" for title, d in _per_set(res, "curves"))]


def check_per_node_args(args, fail):
    if getattr(args, "per_node", None) and args.mode != "evaluate":
        fail(f"--per_node ranks each node's row of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def per_node_report(ctx):
    """--per_node PATH: engine.node_rank_metrics of each index set, the integer columns and the per-node AUC written by rank 0
    as one .npz at PATH while they are at hand.  Returns {"per_node_<name>": the set's summary dict}."""
    out, arrays = {}, {}
    for name, ix in ctx.sets.items():
        m = engine.node_rank_metrics(ctx.real, ctx.inference_adj, ix)
        for k in ("nodes", "positives", "wins", "ties", "hits", "first_rank"):
            arrays[f"{k}_{name}"] = m[k].cpu().numpy()
        arrays[f"auc_{name}"] = m["auc"]
        out[f"per_node_{name}"] = m["summary"]
    if ctx.rank == 0:
        _save_npz(ctx.args.per_node, **arrays)
    return out


def _per_node_log(res, ctx):
    return [f"In {title}: scored nodes={d['scored']} macro AUC={d['macro_auc']} MRR={d['mrr']} "
            f"Hits@1={d['hits_at_1']} R-precision={d['r_precision']}" for title, d in _per_set(res, "per_node")]


LINK_SOURCES = ("posteriors", "embedding", "features")      # what a link-stealing distance is taken between (main.py)


def versus_baseline(versus, fail):
    """--versus SOURCE:METRIC, a link-stealing baseline of the run itself, as (source, metric); None for any other value
    (`features`, or a path).  A value is read as the shortcut when its SOURCE is one of LINK_SOURCES or its METRIC one of
    engine.PAIR_METRICS; the other half is then refused by name when it is not one too."""
    source, sep, metric = (versus or "").partition(":")
    if not sep or (source not in LINK_SOURCES and metric not in engine.PAIR_METRICS):
        return None
    if source not in LINK_SOURCES:
        fail(f"--versus {versus}: source `{source}` is not one of {', '.join(LINK_SOURCES)}")
    if metric not in engine.PAIR_METRICS:
        fail(f"--versus {versus}: metric `{metric}` is not one of {', '.join(engine.PAIR_METRICS)}")
    return source, metric


LINKTELLER_MODE = "link_teller"
LINKTELLER_GRAPHS = ("normalised", "raw")       # --lt_graph: what the victim is queried on
LINKTELLER_DELTA = 1e-4                         # --lt_delta's default, the paper's
# the density beliefs of Wu et al. (IEEE S&P 2022, section VI): the attacker takes the k = belief x (true edge count) best pairs
LINKTELLER_BELIEFS = (0.25, 0.5, 1.0, 2.0, 4.0)
LINKTELLER_FLAGS = ("lt_graph", "lt_delta", "save_linkteller")


def versus_linkteller(versus, fail):
    """--versus linkteller:OUTPUT, the LinkTeller influence matrix of the run's own victim, as OUTPUT (one of
    engine.INFLUENCE_OUTPUTS); None for any other value, which versus_baseline then reads as it always did."""
    source, sep, output = (versus or "").partition(":")
    if not sep or source != "linkteller":
        return None
    if output not in engine.INFLUENCE_OUTPUTS:
        fail(f"--versus {versus}: output `{output}` is not one of {', '.join(engine.INFLUENCE_OUTPUTS)}")
    return output


def check_link_teller_args(args, fail):
    """--mode link_teller and its flags, and --versus linkteller:OUTPUT: what can be refused from the command line alone."""
    mode, arch = getattr(args, "mode", None), getattr(args, "arch", "gcn")
    for flag in LINKTELLER_FLAGS:
        if flag in vars(args) and mode != LINKTELLER_MODE:
            fail(f"--{flag} needs --mode {LINKTELLER_MODE}")
    if versus_linkteller(getattr(args, "versus", None), fail) is not None and arch != "gcn":
        fail(f"--versus {args.versus} queries a GCN victim (engine.influence_scores): --arch gcn only, not --arch {arch}")
    if mode != LINKTELLER_MODE:
        return
    if arch != "gcn":
        fail(f"--mode {LINKTELLER_MODE} queries a GCN victim (engine.influence_scores): --arch gcn only, not --arch {arch}")
    if getattr(args, "ap", False):
        fail(f"--ap adds the average precision of a ranking that is sorted: --mode evaluate, notrain_test and link_stealing only, "
             f"not --mode {mode}")
    if getattr(args, "lt_graph", LINKTELLER_GRAPHS[0]) not in LINKTELLER_GRAPHS:
        fail(f"--lt_graph takes one of {', '.join(LINKTELLER_GRAPHS)}, not {args.lt_graph!r}")
    delta = getattr(args, "lt_delta", LINKTELLER_DELTA)
    with np.errstate(over="ignore"):
        d32 = float(np.float32(delta))
    if not (np.isfinite(d32) and d32 != 0.0 and abs(d32) < 1.0):
        fail(f"--lt_delta takes a perturbation whose float32 is finite, not 0 and below 1 in magnitude, not {delta!r}")
    if getattr(args, "save_linkteller", None) == "":
        fail("--save_linkteller takes the path of the .npz to write")


def belief_k(belief, positives, pairs):
    """k of a density belief: belief x the true edge count, rounded half up, clamped to the pair count."""
    return min(int(Fraction(belief) * positives + Fraction(1, 2)), pairs)


def link_teller_metrics(real, matrix, sets):
    """One influence matrix scored against the true graph on every index set: {set: {"auc", "pairs", "positives" (engine.auc_delong's)
    and "beliefs": {belief: {"k", "hits", "precision", "recall", "f1"}} over LINKTELLER_BELIEFS (engine.topk_metrics at belief_k)}}."""
    out = {}
    for name, ix in sets.items():
        d = engine.auc_delong(real, matrix, ix)
        beliefs = {}
        for belief in LINKTELLER_BELIEFS:
            k = belief_k(belief, d["positives"], d["pairs"])
            if k > 0:
                t = engine.topk_metrics(real, matrix, k, ix)
                beliefs[belief] = {key: t[key] for key in ("k", "hits", "precision", "recall", "f1")}
            else:       # (k = 0 would ask engine.topk_metrics for the true edge count)
                none = float("nan") if d["positives"] == 0 else 0.0
                beliefs[belief] = {"k": 0, "hits": 0, "precision": float("nan"), "recall": none, "f1": none}
        out[name] = {"auc": d["auc"], "pairs": d["pairs"], "positives": d["positives"], "beliefs": beliefs}
    return out


def link_teller_lines(res):
    """Per output of link_teller_metrics' results: the AUC line, then one belief line per index set."""
    lines = []
    for output, by_set in res.items():
        lines.append(f"link teller {output}: " + " ".join(f"auc_{name}={d['auc']}" for name, d in by_set.items()))
        for name, d in by_set.items():
            lines.append(f"link teller {output} {name} beliefs: " + " ".join(
                f"{belief}:k={b['k']},P={b['precision']},R={b['recall']},F1={b['f1']}" for belief, b in d["beliefs"].items()))
    return lines


def save_linkteller(path, real, matrices, res, info):
    """--save_linkteller: per output the whole graph's P best pairs in ranking order, P its true edge count (engine.top_pairs:
    pairs_<output> [P, 2] int64, scores_<output>, hits_<output>), the AUC of the whole graph, and the run's parameters and counts."""
    arrays = {k: np.array(v) for k, v in info.items()}
    for output, matrix in matrices.items():
        d = res[output]["all"]
        if d["positives"] > 0:
            pairs, scores, hits = (t.cpu().numpy() for t in engine.top_pairs(matrix, d["positives"], None, real))
        else:
            pairs, scores, hits = np.zeros((0, 2), np.int64), np.zeros(0, np.float32), np.zeros(0, bool)
        arrays.update({f"pairs_{output}": pairs, f"scores_{output}": scores, f"hits_{output}": hits, f"auc_{output}": np.float64(d["auc"])})
    _save_npz(path, **arrays)


def check_ci_args(args, fail):
    ci, versus, scores = getattr(args, "ci", False), getattr(args, "versus", None), getattr(args, "save_scores", None)
    if versus is not None and not ci and not getattr(args, "ci_nodes", False):
        fail("--versus needs --ci or --ci_nodes")
    if versus is not None and versus == "":
        fail("--versus takes `features` or the path of an .npy score matrix")
    if versus is not None and versus_linkteller(versus, fail) is None:      # (read ahead of the SOURCE:METRIC shortcut)
        versus_baseline(versus, fail)
    if ci and args.mode != "evaluate":
        fail(f"--ci puts an interval on the AUC of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")
    if scores is not None and args.mode != "evaluate":
        fail(f"--save_scores writes the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")
    if scores is not None and scores == "":
        fail("--save_scores takes the path of the .npy to write")


def check_ci_nodes_args(args, fail):
    nodes, path = getattr(args, "ci_nodes", False), getattr(args, "save_influence", None)
    if nodes and args.mode != "evaluate":
        fail(f"--ci_nodes jackknifes the AUC of the attack's modified_adj over its nodes: --mode evaluate only, not --mode {args.mode}")
    if path is not None and not nodes:
        fail("--save_influence needs --ci_nodes")
    if path is not None and path == "":
        fail("--save_influence takes the path of the .npz to write")


def load_versus(path, n):
    """--versus PATH: the .npy at `path` as an n x n float32 matrix; anything else is refused by name."""
    try:
        other = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--versus {path}: not a readable .npy ({e})")
    if other.shape != (n, n):
        raise SystemExit(f"--versus {path}: a matrix of shape {tuple(other.shape)}; this graph's modified_adj is {n} x {n}")
    return torch.from_numpy(np.ascontiguousarray(other, dtype=np.float32))


def save_scores(path, inference_adj):
    """--save_scores: modified_adj as a float32 .npy (what --versus PATH reads)."""
    with open(path, "wb") as f:
        np.save(f, inference_adj.detach().to(torch.float32).cpu().numpy())


def interval_report(real, inference_adj, sets, other, single, paired, key, versus_key):
    """{"<key>_<name>": single(real, inference_adj, ix, CI_LEVEL)} over the index sets; with `other` (--versus: a second n x n
    score matrix) paired(real, inference_adj, other, ix, CI_LEVEL) instead, whose "a" is that dict, as "<versus_key>_<name>" too."""
    out = {}
    for name, ix in sets.items():
        if other is None:
            out[f"{key}_{name}"] = single(real, inference_adj, ix, CI_LEVEL)
        else:
            d = paired(real, inference_adj, other.to(inference_adj.device), ix, CI_LEVEL)
            out[f"{key}_{name}"] = d["a"]
            out[f"{versus_key}_{name}"] = d
    return out


def ci_report(real, inference_adj, sets, other=None):
    """--ci: DeLong's interval of each index set (engine.auc_delong / engine.auc_delong_paired): ci_<name>, versus_<name>."""
    return interval_report(real, inference_adj, sets, other, engine.auc_delong, engine.auc_delong_paired, "ci", "versus")


def _se_ratio(res, ctx, name):
    """` se_nodes/se=<the jackknife's standard error over DeLong's, NaN where that is zero>` of one index set: only beside --ci."""
    if not getattr(ctx.args, "ci", False):
        return ""
    nodes, pairs = res[f"ci_nodes_{name}"], res[f"ci_{name}"]
    return f" se_nodes/se={nodes['se'] / pairs['se'] if pairs['se'] > 0 else float('nan')}"


def _ci_console(res, ctx):
    d = res["ci_all"]
    lines = [f"current auc_pairs={d['auc']} se={d['se']} ci=[{d['ci_low']}, {d['ci_high']}]"]
    if ctx.other is not None:
        d = res["versus_all"]
        lines.append(f"current delta={d['delta']} z={d['z']} p={d['p_value']}")
    return lines


def _ci_log(res, ctx):
    lines = []
    for title, name in SET_TITLES:
        d = res[f"ci_{name}"]
        lines.append(f"In {title}: pairs={d['pairs']} positives={d['positives']} AUC of pairs={d['auc']} se={d['se']} "
                     f"{int(round(100 * d['level']))}% CI=[{d['ci_low']}, {d['ci_high']}]")
        if ctx.other is not None:
            d = res[f"versus_{name}"]
            lines.append(f"In {title}: versus {ctx.versus}: AUC={d['b']['auc']} delta={d['delta']} se={d['se_delta']} "
                         f"z={d['z']} p={d['p_value']}")
    return lines


def _ci_nodes_console(res, ctx):
    d = res["ci_nodes_all"]
    lines = [f"current auc_pairs={d['auc']} se_nodes={d['se']} ci_nodes=[{d['ci_low']}, {d['ci_high']}]{_se_ratio(res, ctx, 'all')}"]
    if ctx.other is not None:
        d = res["versus_nodes_all"]
        lines.append(f"current delta={d['delta']} se_nodes={d['se_delta']} z={d['z']} p={d['p_value']}")
    return lines


def _ci_nodes_log(res, ctx):
    lines = []
    for title, name in SET_TITLES:
        d = res[f"ci_nodes_{name}"]
        lines.append(f"In {title}: nodes={d['nodes']} pairs={d['pairs']} AUC of pairs={d['auc']} jackknife AUC={d['auc_jackknife']} "
                     f"se_nodes={d['se']} {int(round(100 * d['level']))}% CI_nodes=[{d['ci_low']}, {d['ci_high']}] "
                     f"undefined_nodes={d['undefined_nodes']}{_se_ratio(res, ctx, name)}")
        if ctx.other is not None:
            d = res[f"versus_nodes_{name}"]
            lines.append(f"In {title}: versus {ctx.versus} (nodes): AUC={d['b']['auc']} delta={d['delta']} "
                         f"se_nodes={d['se_delta']} z={d['z']} p={d['p_value']}")
    return lines


def save_influence(res, ctx):
    """--save_influence: the jackknife's five int64 columns and d_v = AUC - AUC_-v (float64, NaN where deleting v leaves no AUC)."""
    _save_per_set(ctx.args.save_influence, res, "ci_nodes", ctx, lambda d: {
        **{k: np.asarray(d["ints"][k], dtype=np.int64) for k in engine.NODE_JACKKNIFE_COLUMNS}, "influence": d["influence"].numpy()})


def structure_source(source):
    """--structure SOURCE as "split", "edges" or a finite float; None for anything else."""
    if source in ("split", "edges"):
        return source
    try:
        thr = float(source)
    except (TypeError, ValueError):
        return None
    return thr if np.isfinite(thr) else None


def check_structure_args(args, fail):
    source, path = getattr(args, "structure", None), getattr(args, "save_structure", None)
    if path is not None and source is None:
        fail("--save_structure needs --structure")
    if path is not None and path == "":
        fail("--save_structure takes the path of the .npz to write")
    if source is not None and args.mode != "evaluate":
        fail(f"--structure measures the graph cut out of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")
    if source is not None and structure_source(source) is None:
        fail(f"--structure takes `split`, `edges` or a finite threshold, not {source!r}")


def structure_threshold(source, real, inference_adj, ix):
    """The threshold of one index set for --structure SOURCE (structure_source's value); +inf, the empty graph, for a degenerate
    split or a set without true edges."""
    if source == "split":
        d = engine.two_means_split(inference_adj, ix)
        return float("inf") if d["degenerate"] else d["threshold"]
    if source == "edges":
        d = engine.topk_metrics(real, inference_adj, 0, ix)
        return d["threshold"] if d["k"] else float("inf")
    return float(source)


def structure_report(ctx):
    """--structure: {"structure_<name>": engine.graph_structure of the index set at its structure_threshold, beside the true graph}."""
    source, real, pred = structure_source(ctx.args.structure), ctx.real, ctx.inference_adj
    return {f"structure_{name}": engine.graph_structure(pred, structure_threshold(source, real, pred, ix), ix, real)
            for name, ix in ctx.sets.items()}


def _structure_console(res, ctx):
    d = res["structure_all"]
    q = d["stats"]
    return [f"current transitivity={q['recovered']['transitivity']} (true {q['true']['transitivity']}) "
            f"triangles={d['T_C']}/{d['T_G']} degree_corr={q['degree_corr']} degree_ks={q['degree_ks']}"]


def _structure_log(res, ctx):
    lines = []
    for title, d in _per_set(res, "structure"):
        q = d["stats"]
        lines.append(f"In {title}: structure at {d['threshold']}: edges={d['E_R']} (true {d['E_G']}, shared {d['E_C']}) "
                     f"triangles={d['T_R']} (true {d['T_G']}, shared {d['T_C']}) "
                     f"transitivity={q['recovered']['transitivity']} (true {q['true']['transitivity']}) "
                     f"clustering={q['recovered']['avg_clustering']} (true {q['true']['avg_clustering']}) "
                     f"degree_corr={q['degree_corr']} degree_ks={q['degree_ks']} degree_l1={q['degree_l1']}")
    return lines


def save_structure(res, ctx):
    """--save_structure: the six int64 columns of engine.graph_structure and the threshold (float32)."""
    _save_per_set(ctx.args.save_structure, res, "structure", ctx, lambda d: {
        **{k: d[k].cpu().numpy() for k in engine.GRAPH_STRUCTURE_COLUMNS}, "threshold": np.float32(d["threshold"])})


def check_hops_args(args, fail):
    hops, cut, path = getattr(args, "hops", None), getattr(args, "hops_cut", None), getattr(args, "save_hops", None)
    if cut is not None and hops is None:
        fail("--hops_cut needs --hops")
    if path is not None and hops is None:
        fail("--save_hops needs --hops")
    if path is not None and path == "":
        fail("--save_hops takes the path of the .npz to write")
    if hops is not None and args.mode != "evaluate":
        fail(f"--hops splits the AUC of the attack's modified_adj by true-graph distance: --mode evaluate only, not --mode {args.mode}")
    if hops is not None and not 1 <= hops <= engine.HOP_MAX:
        fail(f"--hops takes H in [1, {engine.HOP_MAX}], not {hops}")
    if cut is not None and structure_source(cut) is None:
        fail(f"--hops_cut takes `split`, `edges` or a finite threshold, not {cut!r}")


def hops_report(ctx):
    """--hops H: {"hops_<name>": engine.hop_auc of the index set, its false positives counted at the set's structure_threshold of
    --hops_cut (default `edges`)}."""
    source, real, pred = structure_source(getattr(ctx.args, "hops_cut", "edges")), ctx.real, ctx.inference_adj
    return {f"hops_{name}": engine.hop_auc(real, pred, ix, ctx.args.hops, structure_threshold(source, real, pred, ix))
            for name, ix in ctx.sets.items()}


def _hops_console(res, ctx):
    d = res["hops_all"]
    by = " ".join(f"{k}:{v}" for k, v in zip(d["distance"][1:], d["auc"][1:]))
    where = "at distance 2" if d["hops"] >= 2 else "beyond distance 1"
    return [f"current auc_by_distance {by} (pooled {d['auc_pooled']}) false positives {where}: {d['above'][1]}/{sum(d['above'][1:])}"]


def _hops_log(res, ctx):
    lines = []
    for title, d in _per_set(res, "hops"):
        by = " ".join(f"{k}: count={c} AUC={a} above={x}" for k, c, a, x in zip(d["distance"], d["count"], d["auc"], d["above"]))
        lines.append(f"In {title}: by true-graph distance at {d['threshold']}: {by} pooled AUC={d['auc_pooled']}")
    return lines


def save_hops(res, ctx):
    """--save_hops: per index set the classes' distance (beyond: 0), count, T, above (int64), AUC (float64) and the threshold."""
    arrays = {}
    for name in ctx.sets:
        d = res[f"hops_{name}"]
        arrays[f"distance_{name}"] = np.asarray([0 if k == "beyond" else k for k in d["distance"]], dtype=np.int64)
        arrays.update({f"{k}_{name}": np.asarray(d[k], dtype=np.int64) for k in ("count", "T", "above")})
        arrays[f"auc_{name}"] = np.asarray(d["auc"], dtype=np.float64)
        arrays[f"threshold_{name}"] = np.float32(d["threshold"])
    _save_npz(ctx.args.save_hops, **arrays)


def check_by_class_args(args, fail):
    source, cut, path = (getattr(args, k, None) for k in ("by_class", "by_class_cut", "save_by_class"))
    if cut is not None and source is None:
        fail("--by_class_cut needs --by_class")
    if path is not None and source is None:
        fail("--save_by_class needs --by_class")
    if path is not None and path == "":
        fail("--save_by_class takes the path of the .npz to write")
    if source is not None and args.mode != "evaluate":
        fail(f"--by_class splits the AUC of the attack's modified_adj by the classes of a pair's ends: --mode evaluate only, "
             f"not --mode {args.mode}")
    if source is not None and source == "":
        fail("--by_class takes `labels`, `degree` or the path of an integer .npy with one class per node")
    if cut is not None and structure_source(cut) is None:
        fail(f"--by_class_cut takes `split`, `edges` or a finite threshold, not {cut!r}")


def degree_classes(degrees):
    """--by_class degree: min(15, d.bit_length()) of each degree d -- 0, 1, 2-3, 4-7, ..., 16384 and more."""
    return np.asarray([min(engine.CLASS_MAX - 1, int(d).bit_length()) for d in degrees], dtype=np.int64)


def node_classes(source, labels, adj):
    """--by_class SOURCE as an int64 vector with one class in [0, 16) per node: `labels` the run's node labels, `degree`
    degree_classes of the degrees in the whole true graph adj, anything else the path of an integer .npy of length n.  What is
    no such vector is refused by name."""
    n = adj.shape[0]
    if source == "labels":
        cl = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    elif source == "degree":
        dense = adj.cpu() if isinstance(adj, torch.Tensor) else torch.as_tensor(np.asarray(adj))
        return degree_classes((dense != 0).sum(1).tolist())
    else:
        try:
            cl = np.load(source, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise SystemExit(f"--by_class {source}: not a readable .npy ({e})")
    if cl.dtype == bool or not np.issubdtype(cl.dtype, np.integer):
        raise SystemExit(f"--by_class {source}: classes of dtype {cl.dtype}; one integer class per node")
    if cl.shape != (n,):
        raise SystemExit(f"--by_class {source}: classes of shape {tuple(cl.shape)}; this graph has {n} nodes")
    cl = cl.astype(np.int64)
    if cl.min() < 0 or cl.max() >= engine.CLASS_MAX:
        raise SystemExit(f"--by_class {source}: classes from {int(cl.min())} to {int(cl.max())}; at most {engine.CLASS_MAX} "
                         f"classes, 0 to {engine.CLASS_MAX - 1}")
    return cl


def by_class_report(ctx):
    """--by_class SOURCE: {"by_class_<name>": per index set engine.class_auc of ctx.classes with the strata `same` and `blocks`
    at the set's structure_threshold of --by_class_cut (default `edges`), engine.auc_delong's auc as auc_pooled, and the shares
    of same-class pairs among the true edges, the pairs at or above the cut and all pairs}."""
    source, real, pred = structure_source(getattr(ctx.args, "by_class_cut", "edges")), ctx.real, ctx.inference_adj
    C = int(np.max(ctx.classes)) + 1
    ratio = lambda a, b: a / b if b else float("nan")
    out = {}
    for name, ix in ctx.sets.items():
        thr = structure_threshold(source, real, pred, ix)
        same = engine.class_auc(real, pred, ctx.classes, ix, engine.class_strata(C, "same"), thr)
        blocks = engine.class_auc(real, pred, ctx.classes, ix, engine.class_strata(C, "blocks"), thr)
        out[f"by_class_{name}"] = {
            "source": ctx.args.by_class, "classes": C, "threshold": thr,
            "auc_pooled": engine.auc_delong(real, pred, ix, CI_LEVEL)["auc"], "same": same, "blocks": blocks,
            "homophily": {"true": ratio(same["positives"][0], sum(same["positives"])),
                          "recovered": ratio(same["above"][0], sum(same["above"])), "pairs": ratio(same["count"][0], same["pairs"])}}
    return out


def _by_class_text(d):
    s, b, h = d["same"], d["blocks"], d["homophily"]
    return (f"same-class AUC={s['auc'][0]} different-class AUC={s['auc'][1]} within blocks={b['auc_within']} "
            f"adjusted={b['auc_adjusted']} (pooled {d['auc_pooled']}) same-class share: true edges={h['true']} "
            f"recovered={h['recovered']} pairs={h['pairs']}")


def _by_class_console(res, ctx):
    return [f"current auc_by_class {_by_class_text(res['by_class_all'])}"]


def _by_class_log(res, ctx):
    return [f"In {title}: by class ({d['source']}, {d['classes']} classes) at {d['threshold']}: {_by_class_text(d)}"
            for title, d in _per_set(res, "by_class")]


def save_by_class(res, ctx):
    """--save_by_class: per index set the blocks' two classes, count, positives, T, above, hits (int64) and AUC (float64), the
    five integers of the `same` split [2][5] and the threshold; once the class of every node."""
    arrays = {"classes": np.asarray(ctx.classes, dtype=np.int64)}
    for name in ctx.sets:
        d = res[f"by_class_{name}"]
        b, C = d["blocks"], d["classes"]
        arrays[f"class_i_{name}"] = np.asarray([i for i in range(C) for _ in range(i, C)], dtype=np.int64)
        arrays[f"class_j_{name}"] = np.asarray([j for i in range(C) for j in range(i, C)], dtype=np.int64)
        arrays.update({f"{k}_{name}": np.asarray(b[k], dtype=np.int64) for k in ("count", "positives", "T", "above", "hits")})
        arrays[f"auc_{name}"] = np.asarray(b["auc"], dtype=np.float64)
        arrays[f"same_ints_{name}"] = np.asarray(d["same"]["ints"], dtype=np.int64)
        arrays[f"threshold_{name}"] = np.float32(d["threshold"])
    _save_npz(ctx.args.save_by_class, **arrays)


ABLATE_HOW = ("table", "shapley")


def check_ablate_args(args, fail):
    how, path = getattr(args, "ablate", None), getattr(args, "save_ablation", None)
    if path is not None and how is None:
        fail("--save_ablation needs --ablate")
    if path is not None and path == "":
        fail("--save_ablation takes the path of the .npz to write")
    if how is not None and how not in ABLATE_HOW:
        fail(f"--ablate takes {' or '.join(ABLATE_HOW)}, not {how!r}")
    if how is not None and args.mode != "evaluate":
        fail(f"--ablate ranks the subsets of the summands of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def _mask_names(mask):
    return tuple(nm for k, nm in enumerate(engine.ENSEMBLE_COMPONENTS) if mask >> k & 1)


def ablation_masks(present, used, how):
    """The masks --ablate HOW ranks: engine.ablation_masks' table, or with `shapley` every non-empty subset of the present
    components, the subset q of the present components in ascending order at place q - 1 (the table's masks are among them)."""
    if how != "shapley":
        return engine.ablation_masks(present, used)
    bits = [k for k in range(len(engine.ENSEMBLE_COMPONENTS)) if present >> k & 1]
    return [sum(1 << k for j, k in enumerate(bits) if q >> j & 1) for q in range(1, 1 << len(bits))]


def ablation_stats(d, present, used, decode_mode, how):
    """One index set's dict of --ablate from engine.subset_auc's dict d over ablation_masks(present, used, how).  No device."""
    names = engine.ENSEMBLE_COMPONENTS
    bits = [k for k in range(len(names)) if present >> k & 1]
    auc, P, N = dict(zip(d["masks"], d["auc"])), d["positives"], d["negatives"]
    res = {"components": names, "present": present, "used": used, "decode_mode": decode_mode,
           "pairs": d["pairs"], "positives": P, "negatives": N,
           "subsets": [{"mask": q, "names": _mask_names(q), "T": t, "auc": a} for q, t, a in zip(d["masks"], d["T"], d["auc"])],
           "auc_used": auc[used], "alone": {names[k]: auc[1 << k] for k in bits},
           "without": {names[k]: auc[used & ~(1 << k)] for k in bits if used >> k & 1 and used != 1 << k},
           "flag_table": [{"useH_A": bool(q >> 5 & 1), "useY_A": bool(q >> 6 & 1), "useY": bool(q >> 7 & 1), "mask": q, "auc": auc[q]}
                          for q in engine.flag_table_masks(present)]}
    if how == "shapley":
        nan = float("nan")
        res["shapley"], res["shapley_sum"] = {names[k]: nan for k in bits}, nan
        if P and N:           # the game on the present components: player j is component bits[j]
            T = dict(zip(d["masks"], d["T"]))
            value = {q: Fraction(T[sum(1 << k for j, k in enumerate(bits) if q >> j & 1)], 2 * P * N)
                     for q in range(1, 1 << len(bits))}
            shares = engine.shapley_shares(len(bits), value)
            res["shapley"] = {names[k]: float(s) for k, s in zip(bits, shares)}
            res["shapley_sum"] = float(sum(shares))
    return res


def ablation_report(ctx):
    """--ablate: {"ablation_<name>": ablation_stats of engine.subset_auc over the index set}: every subset in one pass."""
    c, how = ctx.components, ctx.args.ablate
    masks = ablation_masks(c["present"], c["used"], how)
    return {f"ablation_{name}": ablation_stats(engine.subset_auc(ctx.real, c["stack"], masks, ix), c["present"], c["used"],
                                               c["decode_mode"], how) for name, ix in ctx.sets.items()}


def _ablation_text(d):
    pairs = lambda m: " ".join(f"{k}={v}" for k, v in m.items())
    flags = " ".join(f"{int(r['useH_A'])}{int(r['useY_A'])}{int(r['useY'])}={r['auc']}" for r in d["flag_table"])
    return (f"used={'+'.join(_mask_names(d['used']))} auc={d['auc_used']} | alone: {pairs(d['alone'])} | "
            f"without: {pairs(d['without'])}"), flags


def _ablation_console(res, ctx):
    d = res["ablation_all"]
    lines = [f"current ablation {_ablation_text(d)[0]}"]
    if "shapley" in d:
        lines.append("current shapley " + " ".join(f"{k}={v}" for k, v in d["shapley"].items()))
    return lines


def _ablation_log(res, ctx):
    lines = []
    for title, d in _per_set(res, "ablation"):
        text, flags = _ablation_text(d)
        shapley = " | shapley: " + " ".join(f"{k}={v}" for k, v in d["shapley"].items()) if "shapley" in d else ""
        lines.append(f"In {title}: ablation (decode mode {d['decode_mode']}) {text} | flags HA,YA,Y: {flags}{shapley}")
    return lines


def save_ablation(res, ctx):
    """--save_ablation: masks (uint32) and names once; per index set T (int64) and auc (float64) of every mask, counts =
    {pairs, positives, negatives} (int64) and shapley (float64 per component; NaN for an absent one or without `shapley`)."""
    first = res["ablation_all"]
    arrays = {"masks": np.asarray([r["mask"] for r in first["subsets"]], dtype=np.uint32), "names": np.asarray(first["components"])}
    for name in ctx.sets:
        d = res[f"ablation_{name}"]
        arrays[f"T_{name}"] = np.asarray([r["T"] for r in d["subsets"]], dtype=np.int64)
        arrays[f"auc_{name}"] = np.asarray([r["auc"] for r in d["subsets"]], dtype=np.float64)
        arrays[f"counts_{name}"] = np.asarray([d["pairs"], d["positives"], d["negatives"]], dtype=np.int64)
        arrays[f"shapley_{name}"] = np.asarray([d.get("shapley", {}).get(nm, float("nan")) for nm in d["components"]], dtype=np.float64)
    _save_npz(ctx.args.save_ablation, **arrays)


def check_knn_args(args, fail):
    knn, path = getattr(args, "knn", None), getattr(args, "save_knn", None)
    if path is not None and knn is None:
        fail("--save_knn needs --knn")
    if path is not None and path == "":
        fail("--save_knn takes the path of the .npz to write")
    if knn is not None and knn < 0:
        fail("--knn takes K >= 0 (0: each index set's own mean true degree)")
    if knn is not None and args.mode != "evaluate":
        fail(f"--knn keeps each node's own k best partners in the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def knn_k(K, m, P):
    """The k of one index set of m nodes and P true edges for --knn K: K >= 1 as given; K = 0 the set's mean true degree 2 P / m
    rounded half up, in integers, at least 1; either clamped to min(m - 1, engine.KNN_MAX_K)."""
    k = K if K >= 1 else max(1, (4 * P + m) // (2 * m))
    return min(k, m - 1, engine.KNN_MAX_K)


def knn_report(ctx):
    """--knn K: {"knn_<name>": per index set the stats of engine.knn_graph at knn_k, with k, nodes, pairs, positives, the seven
    columns (numpy int64, for --save_knn) and global_f1_union / global_f1_mutual, the F1 of engine.topk_metrics -- the global
    cut -- at exactly the union's and the mutual graph's edge counts (NaN at 0 edges)}."""
    real, pred, out = ctx.real, ctx.inference_adj, {}
    for name, ix in ctx.sets.items():
        m = ctx.n if ix is None else len(ix)
        if m > engine.KNN_MAX_NIDX:
            raise SystemExit(f"--knn: the index set `{name}` has {m} nodes; engine.knn_graph takes at most {engine.KNN_MAX_NIDX}")
        P = engine.topk_metrics(real, pred, 0, ix)["positives"]
        g = engine.knn_graph(pred, knn_k(ctx.args.knn, m, P), ix, real)
        f1_at = lambda E: engine.topk_metrics(real, pred, E, ix)["f1"] if E else float("nan")
        out[f"knn_{name}"] = {"stats": g["stats"], "k": g["k"], "nodes": m, "pairs": g["pairs"], "positives": P,
                              "global_f1_union": f1_at(g["E_U"]), "global_f1_mutual": f1_at(g["E_M"]),
                              "columns": {q: g[q].cpu().numpy() for q in engine.KNN_COLUMNS}}
    return out


def _knn_text(d):
    q = d["stats"]
    u, mu, hub = q["union"], q["mutual"], q["hubness"]
    return (f"k={d['k']} union f1={u['f1']} (edges={u['edges']}, isolated={u['isolated']}; global f1={d['global_f1_union']}) "
            f"mutual f1={mu['f1']} (edges={mu['edges']}, isolated={mu['isolated']}; global f1={d['global_f1_mutual']}) "
            f"max_in={hub['max_in']} orphans={hub['orphans']} skew={hub['skewness']}")


def _knn_log(res, ctx):
    lines = []
    for title, d in _per_set(res, "knn"):
        q = d["stats"]
        lines.append(f"In {title}: knn {_knn_text(d)} | nodes={d['nodes']} positives={d['positives']} "
                     f"lists P={q['directed']['precision']} R={q['directed']['recall']} "
                     f"union P={q['union']['precision']} R={q['union']['recall']} "
                     f"mutual P={q['mutual']['precision']} R={q['mutual']['recall']}")
    return lines


def save_knn(res, ctx):
    """--save_knn: per index set nodes, k and the seven int64 columns of engine.knn_graph; for the whole graph the union's edge
    list in packed order: pairs, scores, kind (bit 0 a -> b, bit 1 b -> a) and hits."""
    arrays = {}
    for name, ix in ctx.sets.items():
        d = res[f"knn_{name}"]
        arrays[f"nodes_{name}"] = np.arange(ctx.n, dtype=np.int64) if ix is None else np.asarray(ix, dtype=np.int64)
        arrays[f"k_{name}"] = np.int64(d["k"])
        arrays.update({f"{q}_{name}": np.asarray(d["columns"][q], dtype=np.int64) for q in engine.KNN_COLUMNS})
    g = engine.knn_graph(ctx.inference_adj, res["knn_all"]["k"], None, ctx.real, edges=True)
    arrays.update({"pairs": g["pairs_list"].cpu().numpy(), "scores": g["scores"].cpu().numpy(), "kind": g["kind"].cpu().numpy(),
                   "hits": g["hits"].cpu().numpy()})
    _save_npz(ctx.args.save_knn, **arrays)


def check_exposure_args(args, fail):
    on, cut, path = "exposure" in vars(args), getattr(args, "exposure_cut", None), getattr(args, "save_exposure", None)
    if cut is not None and not on:
        fail("--exposure_cut needs --exposure")
    if path is not None and not on:
        fail("--save_exposure needs --exposure")
    if path is not None and path == "":
        fail("--save_exposure takes the path of the .npz to write")
    if on and args.mode != "evaluate":
        fail(f"--exposure splits the true edges of the attack's modified_adj by where they sit in the true graph: "
             f"--mode evaluate only, not --mode {args.mode}")
    if cut is not None and structure_source(cut) is None:
        fail(f"--exposure_cut takes `split`, `edges` or a finite threshold, not {cut!r}")


def exposure_report(ctx):
    """--exposure: {"exposure_<name>": engine.edge_exposure of the index set, its true edges at or above the set's
    structure_threshold of --exposure_cut (default `edges`) counted class by class}."""
    source, real, pred = structure_source(getattr(ctx.args, "exposure_cut", "edges")), ctx.real, ctx.inference_adj
    return {f"exposure_{name}": engine.edge_exposure(real, pred, ix, structure_threshold(source, real, pred, ix))
            for name, ix in ctx.sets.items()}


def _exposure_text(d, auc_only):
    """`by common neighbours ... (pooled ...) | by min degree ...` over the classes that hold edges."""
    q = d["stats"]

    def by(mg):
        if auc_only:
            return " ".join(f"{k}:{a}" for k, c, a in zip(mg["names"], mg["count"], mg["auc"]) if c)
        return " ".join(f"{k}: count={c} AUC={a} recall={r}" for k, c, a, r in zip(mg["names"], mg["count"], mg["auc"], mg["recall"]) if c)

    return f"by common neighbours {by(q['by_embeddedness'])} (pooled {q['auc_pooled']}) | by min degree {by(q['by_degree'])}"


def _exposure_log(res, ctx):
    return [f"In {title}: exposure at {d['threshold']}: edges={d['positives']} recall={d['stats']['recall']} "
            f"precision={d['stats']['precision']} {_exposure_text(d, False)}" for title, d in _per_set(res, "exposure")]


def save_exposure(res, ctx):
    """--save_exposure: per index set nodes, the 16 x 16 x 3 table (int64) and the threshold (float32); for the whole graph the
    true edges in packed order: pairs, scores, placement, common and deg."""
    arrays = {}
    for name, ix in ctx.sets.items():
        d = res[f"exposure_{name}"]
        arrays[f"nodes_{name}"] = np.arange(ctx.n, dtype=np.int64) if ix is None else np.asarray(ix, dtype=np.int64)
        arrays[f"table_{name}"] = np.asarray(d["table"], dtype=np.int64)
        arrays[f"threshold_{name}"] = np.float32(d["threshold"])
    g = engine.edge_exposure(ctx.real, ctx.inference_adj, None, res["exposure_all"]["threshold"], edges=True)
    arrays.update({"pairs": g["pairs_list"].cpu().numpy(), "scores": g["scores"].cpu().numpy(),
                   "placement": g["placement"].cpu().numpy(), "common": g["common"].cpu().numpy(), "deg": g["deg"].cpu().numpy()})
    _save_npz(ctx.args.save_exposure, **arrays)


DEFENSE_MODES = ("evaluate", "notrain_test", "link_stealing")      # the modes that have a victim to defend
DEFENSE_SCALARS = ("mechanism", "eps", "seed", "replicate", "pairs", "edges", "target", "edges_out", "kept", "added", "removed",
                   "flip_probability", "eps_realised", "count_noise", "test_accuracy")


def check_defense_args(args, fail):
    on, eps = "dp_defense" in vars(args), getattr(args, "dp_eps", None)
    for flag in ("dp_eps", "dp_seed", "save_defense"):
        if getattr(args, flag, None) is not None and not on:
            fail(f"--{flag} needs --dp_defense")
    if not on:
        return
    if args.dp_defense not in engine.DP_MECHANISMS:
        fail(f"--dp_defense takes one of {', '.join(engine.DP_MECHANISMS)}, not {args.dp_defense!r}")
    if eps is None:
        fail("--dp_defense needs --dp_eps, the edge-level privacy budget")
    if not (eps > 0 and eps < float("inf")):
        fail(f"--dp_eps takes a finite privacy budget above 0, not {eps!r}")
    if not 0 <= defense_seed(args) < 1 << 64:
        fail(f"--dp_seed takes an integer in [0, 2^64), not {defense_seed(args)!r} (it defaults to --seed)")
    if getattr(args, "save_defense", None) == "":
        fail("--save_defense takes the path of the .npz to write")
    if args.mode not in DEFENSE_MODES + (LINKTELLER_MODE,):      # (DEFENSE_MODES is pinned as it was before --mode link_teller)
        fail(f"--dp_defense perturbs the graph the victim is trained on: --mode {', '.join(DEFENSE_MODES + (LINKTELLER_MODE,))} only, "
             f"not --mode {args.mode}")


def defense_seed(args):
    """--dp_seed, or --seed without it."""
    seed = getattr(args, "dp_seed", None)
    return int(args.seed if seed is None else seed)


def defense_line(d):
    """The one line that says what the defence did to the graph and what it cost the victim."""
    return (f"defense {d['mechanism']} eps={d['eps']} edges {d['edges']}->{d['edges_out']} (kept {d['kept']}, added {d['added']}, "
            f"removed {d['removed']}) test_accuracy={d['test_accuracy']}")


def defense_report(ctx):
    """--dp_defense in --mode evaluate: {"defense": what the mechanism did (engine.dp_perturb_graph's info) and the defended
    victim's test accuracy, "auc_perturbed_<name>": metric_pool of modified_adj against the PERTURBED graph on the index set --
    beside auc_<name>, which is against the true one: which of the two graphs did the attack recover}."""
    res = {"defense": dict(ctx.defense["info"])}
    res.update({f"auc_perturbed_{name}": float(engine.roc_auc(ctx.defense["perturbed"], ctx.inference_adj, ix))
                for name, ix in ctx.sets.items()})
    return res


def _defense_log(res, ctx):
    return [defense_line(res["defense"]) + " " + " ".join(f"auc_perturbed_{name}={res[f'auc_perturbed_{name}']}" for _, name in SET_TITLES)]


def save_defense(path, real, perturbed, d):
    """--save_defense: the perturbed graph's edges in packed order (edge_list [edges_out, 2] int64, rows (a, b) with a > b), the
    pairs the mechanism added and removed (added_list, removed_list, packed order too) and every scalar of DEFENSE_SCALARS."""
    pairs, _, true = engine.threshold_pairs(perturbed, 0.5, None, real)
    gone, _, still = engine.threshold_pairs(real, 0.5, None, perturbed)
    arrays = {"edge_list": pairs.cpu().numpy(), "added_list": pairs[~true].cpu().numpy(), "removed_list": gone[~still].cpu().numpy()}
    for k in DEFENSE_SCALARS:
        arrays[k] = np.array(d[k], dtype=np.uint64 if k == "seed" else None)
    _save_npz(path, **arrays)


def _saver(flag, write):
    """write(res, ctx) when the --save_* flag names a file."""
    return lambda res, ctx: write(res, ctx) if getattr(ctx.args, flag, None) else None


# in the order in which the reports are computed, printed and logged
REPORTS = (
    Report(flags=("topk", "save_edges"), check=check_topk_args, wanted=_on("topk", given=True),
           compute=lambda ctx: topk_report(ctx.real, ctx.inference_adj, ctx.sets, ctx.args.topk),
           console=lambda res, ctx: [f"current f1={res['topk_all']['f1']} (k={res['topk_all']['k']})"],
           log=_topk_log, save=_saver("save_edges", save_edges)),
    Report(flags=("binarize", "save_graph"), check=check_binarize_args, wanted=_on("binarize"),    # split_<set>: the 2-means split
           compute=lambda ctx: {f"split_{s}": engine.two_means_split(ctx.inference_adj, ix, ctx.real) for s, ix in ctx.sets.items()},
           console=lambda res, ctx: ["current split_f1={f1} (edges={edges}, threshold={threshold})".format(**res["split_all"])],
           log=_binarize_log, save=_saver("save_graph", save_graph)),
    Report(flags=("curves",), check=check_curves_args, wanted=_on("curves"), compute=curves_report,
           console=lambda res, ctx: ["current best_f1={best_f1} (threshold={best_threshold})".format(**res["curves_all"])],
           log=_curves_log),
    Report(flags=("per_node",), check=check_per_node_args, wanted=_on("per_node"), compute=per_node_report,
           console=lambda res, ctx: ["current macro_auc={macro_auc} mrr={mrr} hits@1={hits_at_1}".format(**res["per_node_all"])],
           log=_per_node_log),
    Report(flags=("ci",), check=check_ci_args, wanted=_on("ci"),
           compute=lambda ctx: ci_report(ctx.real, ctx.inference_adj, ctx.sets, ctx.other), console=_ci_console, log=_ci_log),
    Report(flags=("ci_nodes", "save_influence"), check=check_ci_nodes_args, wanted=_on("ci_nodes"),
           compute=lambda ctx: interval_report(ctx.real, ctx.inference_adj, ctx.sets, ctx.other, engine.auc_node_jackknife,
                                               engine.auc_node_jackknife_paired, "ci_nodes", "versus_nodes"),
           console=_ci_nodes_console, log=_ci_nodes_log, save=_saver("save_influence", save_influence)),
    Report(flags=("structure", "save_structure"), check=check_structure_args, wanted=_on("structure", given=True),
           compute=structure_report, console=_structure_console, log=_structure_log, save=_saver("save_structure", save_structure)),
)
# REPORTS holds the reports of the recorded run with every flag on (tests/golden/evaluate_all_flags.json), whose tests pin its
# entries; the hops report, added since then, follows here.
EVERY_REPORT = REPORTS + (
    Report(flags=("hops", "hops_cut", "save_hops"), check=check_hops_args, wanted=_on("hops", given=True), compute=hops_report,
           console=_hops_console, log=_hops_log, save=_saver("save_hops", save_hops)),
)
# EVERY_REPORT ends with the hops report, as its tests pin it; the by_class report follows.
ALL_REPORTS = EVERY_REPORT + (
    Report(flags=("by_class", "by_class_cut", "save_by_class"), check=check_by_class_args, wanted=_on("by_class", given=True),
           compute=by_class_report, console=_by_class_console, log=_by_class_log, save=_saver("save_by_class", save_by_class)),
)
# ALL_REPORTS ends with the by_class report, as its tests pin it; the ablate report follows.
REPORT_TABLE = ALL_REPORTS + (
    Report(flags=("ablate", "save_ablation"), check=check_ablate_args, wanted=_on("ablate"), compute=ablation_report,
           console=_ablation_console, log=_ablation_log, save=_saver("save_ablation", save_ablation)),
)
# REPORT_TABLE ends with the ablate report, as its tests pin it; EVALUATE_REPORTS is what main.py's parser, run and log loop over.
EVALUATE_REPORTS = REPORT_TABLE + (
    Report(flags=("knn", "save_knn"), check=check_knn_args, wanted=_on("knn", given=True), compute=knn_report,
           console=lambda res, ctx: [f"current knn {_knn_text(res['knn_all'])}"], log=_knn_log, save=_saver("save_knn", save_knn)),
)
# EVALUATE_REPORTS ends with the knn report, as its tests pin it; the reports added since follow here, and main.py loops over both.
LATER_REPORTS = (
    Report(flags=("exposure", "exposure_cut", "save_exposure"), check=check_exposure_args, wanted=lambda args: "exposure" in vars(args),
           compute=exposure_report, console=lambda res, ctx: [f"current exposure {_exposure_text(res['exposure_all'], True)}"],
           log=_exposure_log, save=_saver("save_exposure", save_exposure)),
    # --dp_defense: main.py perturbs the graph before the victim is trained, prints defense_line and writes --save_defense in every
    # mode that has a victim; what is left for --mode evaluate is here
    Report(flags=("dp_defense", "dp_eps", "dp_seed", "save_defense"), check=check_defense_args,
           wanted=lambda args: "dp_defense" in vars(args), compute=defense_report,
           console=lambda res, ctx: [f"current auc_perturbed={res['auc_perturbed_all']}"], log=_defense_log),
)


def shown_parameters(args):
    """The namespace that the log's parameter line prints: args without `ap` while --ap is off and without the flags of every
    report that is off, so that a run without a flag logs what it logged before the flag existed."""
    hidden = set() if getattr(args, "ap", False) else {"ap"}
    for r in EVALUATE_REPORTS + LATER_REPORTS:
        if not r.wanted(args):
            hidden.update(r.flags)
    return argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in hidden})
