"""main.py entry with the reference's command line (/root/reference/MC-GRA/main.py:78-139) and its
``--mode evaluate`` flow (:141-324, :392-409): load the graph, train the victim GCN, compute the priors
H_A / Y_A, run PGDAttack on the MI355X hot path, report the recovered-adjacency AUC.

    python -m mc_gra_amd.main --dataset cora --w1 0.01 --w6 10 --w7 10 --w9 10 --w10 1000 --lr -2 \
        --useH_A --useY_A --useY --measure MSELoss            (after mcgra_loader.load())
    python mc-gra_amd/main.py ...                             (stand-alone; bootstraps the loader itself)

--arch gcn | sage | gat select the victim family as main.py:175-231 does.  Also provided: --mode prepare (main.py:440-450,
writes the label adjacency under --saved_data) and --mode notrain_test (main.py:412-437: no attack; the AUC of each prior's
own decode -- features, H_A1, H_A2, Y_A, label adjacency -- against the true graph, the three thin priors pair by pair on
the GPU without an n x n score matrix).  --ap (not in the reference; off by default, and then nothing changes) adds the
average precision of every ranking that is scored beside its AUC, from the same sort (engine.rank_metrics).
--topk K (not in the reference; --mode evaluate only; absent by default, and then nothing changes) reports the recovered
graph itself: of the K best-scored unordered node pairs of modified_adj within each index set (attack, train, all), how many
are true edges -- precision, recall and F1 at K (engine.topk_metrics; ties by packed position, so the answer is defined).
K = 0 takes each set's own true edge count; a K above a set's pair count is clamped to it, and the printed k says so.
--save_edges PATH (needs --topk) writes the whole-graph selection as an .npz of pairs, scores and hits in ranking order
(engine.top_pairs).
--curves PATH (not in the reference; --mode evaluate only; absent by default, and then nothing changes) writes what the
reference's roc_curve call returns, and the precision-recall curve beside it, for each of the three index sets as an .npz at
PATH (roc_fpr_<set>, roc_tpr_<set>, roc_thresholds_<set>, pr_precision_<set>, pr_recall_<set>, pr_thresholds_<set>; sklearn's
conventions and defaults: drop_intermediate on for the ROC curve, off for the PR curve), computed on the GPU
(engine.rank_curves, engine.precision_recall_curve), and reports the best F1 over all thresholds.
--per_node PATH (not in the reference; --mode evaluate only; absent by default, and then nothing changes) asks whose
neighbourhood leaked: for each node of each of the three index sets, how its true neighbours rank among the set's other nodes
by its row of modified_adj (engine.node_rank_metrics) -- written as an .npz at PATH (nodes_<set>, positives_<set>, wins_<set>,
ties_<set>, hits_<set>, first_rank_<set>, auc_<set>), with the macro AUC, the MRR and Hits@1 of each set reported.
--binarize (not in the reference's main.py; --mode evaluate only; absent by default, and then nothing changes) answers "which
graph did the attack recover" without the truth: the entries of modified_adj within each index set are split into two
clusters by an exact integer 2-means (engine.two_means_split; the defined form of PGDAttack.kmeans, baseline.py:88-109), the
upper cluster is the recovered edge set, and its precision, recall and F1 against the true graph are reported.  The scores
must lie in [0, 16): every decode branch but brazil's unbounded relu(Z Z^T - I), whose modified_adj is refused when it holds more.
--save_graph PATH (needs --binarize) writes the whole graph's recovered edges as an .npz of pairs, scores and hits in packed
order with the threshold and the round count (engine.threshold_pairs).
--ci (not in the reference; --mode evaluate only; absent by default, and then nothing changes) says how far the attack's AUC
can be trusted: DeLong's standard error and 95 % confidence interval of the AUC of the unordered node pairs of each index set
(engine.auc_delong; integer counts on the GPU, exact rationals on the host).  Pairs that share a node are not independent, so
the interval is a lower bound on the real uncertainty.
--versus features|PATH (needs --ci or --ci_nodes) asks whether the attack beats another scoring of the same pairs: DeLong's paired test
(engine.auc_delong_paired) of modified_adj against the run's own feature_adj -- the prior the attacker already holds -- or
against an n x n float32 matrix stored as an .npy at PATH; delta, z and the two-sided p-value of each index set are reported.
--save_scores PATH (--mode evaluate only) writes modified_adj as that .npy, so that one run can be compared with another.
--ci_nodes (not in the reference; --mode evaluate only; absent by default, and then nothing changes) puts the conservative
bracket beside --ci's optimistic one: the delete-one-node jackknife standard error and 95 % interval of the same AUC
(engine.auc_node_jackknife; five exact integers per node on the GPU, one exact rational per node on the host).  With --ci the
ratio se_nodes / se of the two standard errors is reported; with --versus the jackknife of the difference of the two scorings'
AUCs (engine.auc_node_jackknife_paired).
--save_influence PATH (needs --ci_nodes) writes, as an .npz at PATH, which nodes carry the attack's AUC: for each index set
nodes_<set>, the integers P_v_<set>, N_v_<set>, A_v_<set>, B_v_<set>, C_v_<set> and influence_<set> = AUC - AUC without the node.
--structure split|edges|THRESHOLD (not in the reference; --mode evaluate only; absent by default, and then nothing changes) asks
whether the recovered graph LOOKS like the real one: modified_adj within each index set is cut at a threshold -- `split`: that
of the set's own 2-means split (engine.two_means_split; a degenerate split is the empty graph), `edges`: the score of the P-th
best pair, P the set's true edge count (engine.topk_metrics(k=0); ties at that score may add edges, the real count is reported),
or a float -- and the degrees, triangles, wedges, transitivity and clustering of that graph are reported beside the true
graph's, with the triangles both share and the distance between the two degree sequences (engine.graph_structure: bit
matrices and popcounts on the GPU, exact integers, exact rationals on the host).
--save_structure PATH (needs --structure) writes, as an .npz at PATH, for each index set nodes_<set>, the six integer columns
d_R_<set>, t_R_<set>, d_G_<set>, t_G_<set>, d_C_<set>, t_C_<set> (degree and triangles per node in the recovered graph, the true
graph and their intersection) and threshold_<set>.
Not provided (each exits with a message naming the reference line): --mode search/baseline/gaussian/gcn_attack.

Several GPUs of one node -- one process per GPU, RCCL over xGMI:
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 mc-gra_amd/main.py --dataset ... --measure HSIC ...
Every rank loads the graph and trains the victim on the same seed (rank 0's weights are then broadcast), and
PGDAttack.attack (main.py:298-307) runs ONE attack row-block sharded over the ranks when the configuration allows it
(mc-gra_amd/topology_attack.py); rank 0 prints and logs the result.  MCGRA_SHARED_GPU=1 puts every rank on cuda:0 over
gloo with host-staged exchanges: the test mode of a 1-GPU box.
"""
import argparse
import os
import random
import sys
from copy import deepcopy

import numpy as np

if __package__ in (None, ""):          # run as a script: load the hyphenated directory as package mc_gra_amd
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mcgra_loader
    mcgra_loader.load()
    from mc_gra_amd import engine, utils
    from mc_gra_amd.dataset import Dataset
    from mc_gra_amd.models.gcn import GCN, embedding_GCN
    from mc_gra_amd.models.gat import GAT, embedding_gat
    from mc_gra_amd.models.graphsage import graphsage, embedding_graphsage
    from mc_gra_amd.topology_attack import PGDAttack
else:
    from . import engine, utils
    from .dataset import Dataset
    from .models.gcn import GCN, embedding_GCN
    from .models.gat import GAT, embedding_gat
    from .models.graphsage import graphsage, embedding_graphsage
    from .topology_attack import PGDAttack

import torch
import torch.nn.functional as F


def check_topk_args(args, fail):
    """--topk / --save_edges against the rest of the command line; fail(message) does not return."""
    topk, edges = getattr(args, "topk", None), getattr(args, "save_edges", None)
    if edges and topk is None:
        fail("--save_edges needs --topk")
    if topk is not None and topk < 0:
        fail("--topk takes K >= 0 (0: each index set's own true edge count)")
    if topk is not None and args.mode != "evaluate":
        fail(f"--topk scores the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def check_binarize_args(args, fail):
    """--binarize / --save_graph against the rest of the command line; fail(message) does not return."""
    binarize, graph = getattr(args, "binarize", False), getattr(args, "save_graph", None)
    if graph and not binarize:
        fail("--save_graph needs --binarize")
    if binarize and args.mode != "evaluate":
        fail(f"--binarize splits the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def check_curves_args(args, fail):
    """--curves against the rest of the command line; fail(message) does not return."""
    if getattr(args, "curves", None) and args.mode != "evaluate":
        fail(f"--curves draws the curves of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def check_per_node_args(args, fail):
    """--per_node against the rest of the command line; fail(message) does not return."""
    if getattr(args, "per_node", None) and args.mode != "evaluate":
        fail(f"--per_node ranks each node's row of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")


def check_ci_args(args, fail):
    """--ci / --versus / --save_scores against the rest of the command line; fail(message) does not return."""
    ci, versus, scores = getattr(args, "ci", False), getattr(args, "versus", None), getattr(args, "save_scores", None)
    if versus is not None and not ci and not getattr(args, "ci_nodes", False):
        fail("--versus needs --ci or --ci_nodes")
    if versus is not None and versus == "":
        fail("--versus takes `features` or the path of an .npy score matrix")
    if ci and args.mode != "evaluate":
        fail(f"--ci puts an interval on the AUC of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")
    if scores is not None and args.mode != "evaluate":
        fail(f"--save_scores writes the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")
    if scores is not None and scores == "":
        fail("--save_scores takes the path of the .npy to write")


def check_ci_nodes_args(args, fail):
    """--ci_nodes / --save_influence against the rest of the command line; fail(message) does not return."""
    nodes, path = getattr(args, "ci_nodes", False), getattr(args, "save_influence", None)
    if nodes and args.mode != "evaluate":
        fail(f"--ci_nodes jackknifes the AUC of the attack's modified_adj over its nodes: --mode evaluate only, not --mode {args.mode}")
    if path is not None and not nodes:
        fail("--save_influence needs --ci_nodes")
    if path is not None and path == "":
        fail("--save_influence takes the path of the .npz to write")


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
    """--structure / --save_structure against the rest of the command line; fail(message) does not return."""
    source, path = getattr(args, "structure", None), getattr(args, "save_structure", None)
    if path is not None and source is None:
        fail("--save_structure needs --structure")
    if path is not None and path == "":
        fail("--save_structure takes the path of the .npz to write")
    if source is not None and args.mode != "evaluate":
        fail(f"--structure measures the graph cut out of the attack's modified_adj: --mode evaluate only, not --mode {args.mode}")
    if source is not None and structure_source(source) is None:
        fail(f"--structure takes `split`, `edges` or a finite threshold, not {source!r}")


class _Parser(argparse.ArgumentParser):
    def parse_args(self, *a, **k):
        args = super().parse_args(*a, **k)
        check_topk_args(args, self.error)
        check_binarize_args(args, self.error)
        check_curves_args(args, self.error)
        check_per_node_args(args, self.error)
        check_ci_args(args, self.error)
        check_ci_nodes_args(args, self.error)
        check_structure_args(args, self.error)
        return args


def build_parser():
    """Same flags and defaults as main.py:78-137 (+ --dataset_root, --saved_data for file locations)."""
    p = _Parser()
    p.add_argument('--seed', type=int, default=15)
    p.add_argument('--epochs', type=int, default=100)
    p.add_argument('--lr', type=float, default=0.01)
    p.add_argument('--weight_decay', type=float, default=5e-4)
    p.add_argument('--hidden', type=int, default=16)
    p.add_argument('--dropout', type=float, default=0.5)
    p.add_argument('--nlayers', type=int, default=2)
    p.add_argument('--arch', type=str, choices=["gcn", "gat", "sage"], default='gcn')
    p.add_argument('--dataset', type=str, default='cora',
                   choices=['cora', 'cora_ml', 'citeseer', 'polblogs', 'pubmed', 'AIDS', 'usair', 'brazil'])
    p.add_argument('--density', type=float, default=10000000.0)
    p.add_argument('--model', type=str, default='PGD', choices=['PGD', 'min-max'])
    p.add_argument('--nlabel', type=float, default=1.0)
    p.add_argument('--iter', type=int, default=1)
    p.add_argument('--max_eval', type=int, default=100)
    p.add_argument('--log_name', type=str, default="result.txt")
    p.add_argument("--mode", type=str, default="evaluate", choices=["evaluate", "prepare", "notrain_test"])
    p.add_argument("--measure", type=str, default="HSIC", choices=["HSIC", "MSELoss", "KL", "KDE", "CKA", "DP"])
    p.add_argument("--measure2", type=str, default="HSIC")
    p.add_argument("--nofeature", action='store_true')
    p.add_argument('--weight_aux', type=float, default=0)
    p.add_argument('--weight_sup', type=float, default=1)
    for i in range(1, 11):
        p.add_argument(f'--w{i}', type=float, default=0)
    p.add_argument('--eps', type=float, default=0)
    p.add_argument('--useH_A', action='store_true')
    p.add_argument('--useY_A', action='store_true')
    p.add_argument('--useY', action='store_true')
    p.add_argument('--ensemble', action='store_true')
    p.add_argument('--add_noise', action='store_true')
    p.add_argument('--defense', action='store_true')
    p.add_argument('--dataset_root', type=str, default='./dataset')
    p.add_argument('--saved_data', type=str, default='./saved_data')
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--ap', action='store_true')     # also report average precision (engine.rank_metrics)
    p.add_argument('--topk', type=int, default=None)        # also report the K best pairs' precision / recall / F1
    p.add_argument('--save_edges', type=str, default=None)  # with --topk: the whole-graph edge list as an .npz
    p.add_argument('--curves', type=str, default=None)      # also write the ROC and precision-recall curves as an .npz
    p.add_argument('--per_node', type=str, default=None)    # also write each node's own ranking counts as an .npz
    p.add_argument('--binarize', action='store_true')       # also split modified_adj into edges / no edges by 2-means
    p.add_argument('--save_graph', type=str, default=None)  # with --binarize: the whole graph's recovered edges as an .npz
    # absent from the namespace unless given: without them the parameter line of the log is what it was
    p.add_argument('--ci', action='store_true', default=argparse.SUPPRESS)      # also DeLong's se and interval of the AUC
    p.add_argument('--versus', type=str, default=argparse.SUPPRESS)            # with --ci: paired test against `features` or an .npy
    p.add_argument('--save_scores', type=str, default=argparse.SUPPRESS)       # write modified_adj as an .npy for a later --versus
    p.add_argument('--ci_nodes', action='store_true', default=argparse.SUPPRESS)   # also the node-jackknife se and interval of the AUC
    p.add_argument('--save_influence', type=str, default=argparse.SUPPRESS)    # with --ci_nodes: each node's influence as an .npz
    p.add_argument('--structure', type=str, default=argparse.SUPPRESS)         # also degrees, triangles and clustering of the cut graph
    p.add_argument('--save_structure', type=str, default=argparse.SUPPRESS)    # with --structure: the per-node columns as an .npz
    return p


def dot_product_decode(Z, dataset):
    """main.dot_product_decode (main.py:44-55): feature_adj."""
    if dataset in ('cora', 'citeseer', 'AIDS'):
        Z = torch.matmul(Z, Z.t())
        return torch.sigmoid(torch.relu(Z - torch.eye(Z.shape[0], device=Z.device)))
    Z = F.normalize(Z, p=2, dim=1)
    Z = torch.matmul(Z, Z.t())
    return torch.relu(Z - torch.eye(Z.shape[0], device=Z.device))


def decode_branch(dataset):
    """The branch of dot_product_decode above as a decode mode of mcgra.h: 0 sigmoid(relu(Z Z^T - I)) for cora / citeseer /
    AIDS, 4 relu(Zn Zn^T - I) on L2-normalised rows otherwise."""
    return 0 if dataset in ('cora', 'citeseer', 'AIDS') else 4


def metric_pool(ori_adj, inference_adj, idx):
    """main.metric_pool (main.py:66-75): roc_curve + auc of ori_adj[idx][:, idx] against inference_adj[idx][:, idx], on the
    device that holds inference_adj (engine.roc_auc: exact, no gathered submatrix, no host copy).  idx None: every node."""
    return engine.roc_auc(ori_adj.to(inference_adj.device), inference_adj, idx)


def label_adjacency(labels):
    """main.prepare (main.py:440-450): label_adj[i][j] = (labels[i] == labels[j])."""
    lab = np.asarray(labels)
    return (lab[:, None] == lab[None, :]).astype(np.float32)


def prior_aucs(adj, feature_adj, H_A1, H_A2, Y_A, label_adj, dataset):
    """main.notrain_test (main.py:412-437): metric_pool over all nodes of what each prior gives away on its own.  The two
    n x n matrices go through engine.roc_auc; H_A1, H_A2, Y_A are decoded pair by pair inside engine.decode_auc (no n x n
    score matrix), a prior wider than 128 columns through engine.decode_scores + engine.roc_auc (the same scores)."""
    dev, mode = H_A2.device, decode_branch(dataset)
    adj = adj.to(dev)

    def matrix(S):
        return engine.roc_auc(adj, torch.as_tensor(S).to(dev))

    def thin(Z):
        Z = Z.detach().to(dev)
        if Z.shape[1] > 128:
            return engine.roc_auc(adj, engine.decode_scores(Z, mode))
        return engine.decode_auc(adj, Z, mode)

    return {"feature": float(matrix(feature_adj)), "layer1": float(thin(H_A1)), "layer2": float(thin(H_A2)),
            "out": float(thin(Y_A)), "label": float(matrix(label_adj))}


def prior_rank_metrics(adj, feature_adj, H_A1, H_A2, Y_A, label_adj, dataset):
    """prior_aucs with the average precision of each ranking beside its AUC (--ap): (aucs, aps), two dicts with prior_aucs'
    keys.  Each pair comes from one sort: engine.rank_metrics for the matrices, engine.decode_rank_metrics for the thin
    priors, engine.decode_scores + engine.rank_metrics past 128 columns.  The AUCs are prior_aucs' bit for bit."""
    dev, mode = H_A2.device, decode_branch(dataset)
    adj = adj.to(dev)

    def matrix(S):
        return engine.rank_metrics(adj, torch.as_tensor(S).to(dev))

    def thin(Z):
        Z = Z.detach().to(dev)
        if Z.shape[1] > 128:
            return engine.rank_metrics(adj, engine.decode_scores(Z, mode))
        return engine.decode_rank_metrics(adj, Z, mode)

    both = {"feature": matrix(feature_adj), "layer1": thin(H_A1), "layer2": thin(H_A2), "out": thin(Y_A),
            "label": matrix(label_adj)}
    return {k: float(v[0]) for k, v in both.items()}, {k: float(v[1]) for k, v in both.items()}


def topk_report(ori_adj, inference_adj, sets, K):
    """--topk K: engine.topk_metrics of each index set of `sets` (name -> node ids, None: every node), K clamped to the
    set's pair count (K = 0: the set's own true edge count).  Returns {"topk_<name>": dict}."""
    real = ori_adj.to(inference_adj.device)
    out = {}
    for name, ix in sets.items():
        rows = inference_adj.shape[0] if ix is None else len(ix)
        out[f"topk_{name}"] = engine.topk_metrics(real, inference_adj, min(K, rows * (rows - 1) // 2), ix)
    return out


def save_edges(path, ori_adj, inference_adj, k):
    """--save_edges: the k best pairs of the whole graph in ranking order (engine.top_pairs) as an .npz at exactly `path`."""
    if k > 0:
        pairs, scores, hits = (t.cpu().numpy() for t in engine.top_pairs(inference_adj, k, None, ori_adj.to(inference_adj.device)))
    else:
        pairs, scores, hits = np.zeros((0, 2), np.int64), np.zeros(0, np.float32), np.zeros(0, bool)
    with open(path, "wb") as f:
        np.savez(f, pairs=pairs, scores=scores, hits=hits)


def binarize_report(ori_adj, inference_adj, sets):
    """--binarize: engine.two_means_split of each index set of `sets` (name -> node ids, None: every node) with the true graph
    beside it for precision, recall and F1.  Returns {"split_<name>": dict}."""
    real = ori_adj.to(inference_adj.device)
    return {f"split_{name}": engine.two_means_split(inference_adj, ix, real) for name, ix in sets.items()}


def save_graph(path, ori_adj, inference_adj, split):
    """--save_graph: the high cluster of the whole graph's split, every pair at or above its threshold in packed order
    (engine.threshold_pairs), as an .npz at exactly `path`; a degenerate split has no edges and a NaN threshold."""
    if split["degenerate"]:
        pairs, scores, hits, thr = np.zeros((0, 2), np.int64), np.zeros(0, np.float32), np.zeros(0, bool), float("nan")
    else:
        thr = split["threshold"]
        pairs, scores, hits = (t.cpu().numpy() for t in
                               engine.threshold_pairs(inference_adj, thr, None, ori_adj.to(inference_adj.device)))
    with open(path, "wb") as f:
        np.savez(f, pairs=pairs, scores=scores, hits=hits, threshold=np.float32(thr), iterations=np.int64(split["iterations"]))


CI_LEVEL = 0.95


def _se_ratio(nodes, pairs):
    """se_nodes / se of one index set: the node jackknife's standard error over DeLong's; NaN where either is undefined."""
    return nodes["se"] / pairs["se"] if pairs["se"] > 0 else float("nan")


def ci_report(ori_adj, inference_adj, sets, other=None):
    """--ci: engine.auc_delong of each index set of `sets` (name -> node ids, None: every node); with `other` (--versus: a second
    n x n score matrix) engine.auc_delong_paired of inference_adj against it instead, whose "a" is the same dict.  Returns
    {"ci_<name>": dict} and, with `other`, {"versus_<name>": dict}."""
    real = ori_adj.to(inference_adj.device)
    out = {}
    for name, ix in sets.items():
        if other is None:
            out[f"ci_{name}"] = engine.auc_delong(real, inference_adj, ix, CI_LEVEL)
        else:
            d = engine.auc_delong_paired(real, inference_adj, other.to(inference_adj.device), ix, CI_LEVEL)
            out[f"ci_{name}"] = d["a"]
            out[f"versus_{name}"] = d
    return out


def ci_nodes_report(ori_adj, inference_adj, sets, other=None):
    """--ci_nodes: engine.auc_node_jackknife of each index set of `sets` (name -> node ids, None: every node); with `other`
    (--versus) engine.auc_node_jackknife_paired of inference_adj against it instead, whose "a" is the same dict.  Returns
    {"ci_nodes_<name>": dict} and, with `other`, {"versus_nodes_<name>": dict}."""
    real = ori_adj.to(inference_adj.device)
    out = {}
    for name, ix in sets.items():
        if other is None:
            out[f"ci_nodes_{name}"] = engine.auc_node_jackknife(real, inference_adj, ix, CI_LEVEL)
        else:
            d = engine.auc_node_jackknife_paired(real, inference_adj, other.to(inference_adj.device), ix, CI_LEVEL)
            out[f"ci_nodes_{name}"] = d["a"]
            out[f"versus_nodes_{name}"] = d
    return out


def save_influence(path, res, sets, n):
    """--save_influence: per index set the node ids, the five integer columns of engine.auc_node_jackknife (int64) and the
    influence d_v = AUC - AUC_-v (float64, NaN where deleting the node leaves no AUC), as an .npz at exactly `path`."""
    arrays = {}
    for name, ix in sets.items():
        d = res[f"ci_nodes_{name}"]
        arrays[f"nodes_{name}"] = np.arange(n, dtype=np.int64) if ix is None else np.asarray(ix, dtype=np.int64)
        for k in engine.NODE_JACKKNIFE_COLUMNS:
            arrays[f"{k}_{name}"] = np.asarray(d["ints"][k], dtype=np.int64)
        arrays[f"influence_{name}"] = d["influence"].numpy()
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def structure_threshold(source, real, inference_adj, ix):
    """The threshold of one index set for --structure SOURCE (structure_source's value): `split`: the smallest score of the
    high cluster of the set's 2-means split; `edges`: the score of the P-th best pair, P the set's true edge count; +inf (the
    empty graph) for a degenerate split or P == 0; a float: itself."""
    if source == "split":
        d = engine.two_means_split(inference_adj, ix)
        return float("inf") if d["degenerate"] else d["threshold"]
    if source == "edges":
        d = engine.topk_metrics(real, inference_adj, 0, ix)
        return d["threshold"] if d["k"] else float("inf")
    return float(source)


def structure_report(ori_adj, inference_adj, sets, source):
    """--structure: engine.graph_structure of each index set of `sets` (name -> node ids, None: every node) at the threshold
    structure_threshold gives for it, with the true graph beside it.  Returns {"structure_<name>": dict}."""
    real = ori_adj.to(inference_adj.device)
    return {f"structure_{name}": engine.graph_structure(inference_adj, structure_threshold(source, real, inference_adj, ix), ix, real)
            for name, ix in sets.items()}


def save_structure(path, res, sets, n):
    """--save_structure: per index set the node ids, the six integer columns of engine.graph_structure (int64) and the threshold
    (float32), as an .npz at exactly `path`."""
    arrays = {}
    for name, ix in sets.items():
        d = res[f"structure_{name}"]
        arrays[f"nodes_{name}"] = np.arange(n, dtype=np.int64) if ix is None else np.asarray(ix, dtype=np.int64)
        for k in engine.GRAPH_STRUCTURE_COLUMNS:
            arrays[f"{k}_{name}"] = d[k].cpu().numpy()
        arrays[f"threshold_{name}"] = np.float32(d["threshold"])
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load_versus(path, n):
    """--versus PATH: the .npy at `path` as an n x n float32 matrix; anything else is refused by name."""
    try:
        other = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        _exit(f"--versus {path}: not a readable .npy ({e})")
    if other.shape != (n, n):
        _exit(f"--versus {path}: a matrix of shape {tuple(other.shape)}; this graph's modified_adj is {n} x {n}")
    return torch.from_numpy(np.ascontiguousarray(other, dtype=np.float32))


def save_scores(path, inference_adj):
    """--save_scores: modified_adj as a float32 .npy at exactly `path` (what --versus PATH reads)."""
    with open(path, "wb") as f:
        np.save(f, inference_adj.detach().to(torch.float32).cpu().numpy())


def curves_report(path, ori_adj, inference_adj, sets):
    """--curves PATH: the ROC curve (drop_intermediate on, as the reference's roc_curve call) and the precision-recall curve
    (drop_intermediate off, sklearn's default) of each index set of `sets` (name -> node ids, None: every node), written as
    one .npz at exactly `path` when it is given.  Returns {"curves_<name>": dict} with the point counts and the best F1."""
    real = ori_adj.to(inference_adj.device)
    out, arrays = {}, {}
    for name, ix in sets.items():
        c = engine.rank_curves(real, inference_adj, ix)
        pr = engine.precision_recall_curve(real, inference_adj, ix)
        for k, t in zip(("fpr", "tpr", "thresholds"), c["roc"]):
            arrays[f"roc_{k}_{name}"] = t.cpu().numpy()
        for k, t in zip(("precision", "recall", "thresholds"), pr):
            arrays[f"pr_{k}_{name}"] = t.cpu().numpy()
        out[f"curves_{name}"] = {"roc_points": c["roc_points"], "pr_points": int(pr[2].numel()), "levels": c["levels"],
                                 "best_f1": c["best_f1"]["f1"], "best_threshold": c["best_f1"]["threshold"]}
    if path:
        with open(path, "wb") as f:
            np.savez(f, **arrays)
    return out


def per_node_report(path, ori_adj, inference_adj, sets):
    """--per_node PATH: engine.node_rank_metrics of each index set of `sets` (name -> node ids, None: every node), the integer
    columns and the per-node AUC written as one .npz at exactly `path` when it is given.  Returns {"per_node_<name>": the
    set's summary dict}."""
    real = ori_adj.to(inference_adj.device)
    out, arrays = {}, {}
    for name, ix in sets.items():
        m = engine.node_rank_metrics(real, inference_adj, ix)
        for k in ("nodes", "positives", "wins", "ties", "hits", "first_rank"):
            arrays[f"{k}_{name}"] = m[k].cpu().numpy()
        arrays[f"auc_{name}"] = m["auc"]
        out[f"per_node_{name}"] = m["summary"]
    if path:
        with open(path, "wb") as f:
            np.savez(f, **arrays)
    return out


def victim_tensors(m):
    """Every parameter of a victim: the registered ones and those of the layers it keeps in plain lists (models/gcn.py:44,
    graphsage.py:50, gat.py:47 -- as the reference's classes do)."""
    mods = [m] + list(getattr(m, "gc", [])) + [a for heads in getattr(m, "attentions", []) for a in heads]
    seen, out = set(), []
    for mod in mods:
        for p_ in mod.parameters():
            if id(p_) not in seen:
                seen.add(id(p_))
                out.append(p_)
    return out


def init_distributed(args):
    """Under a launcher that set WORLD_SIZE > 1 (torchrun): join the process group BEFORE anything touches the GPU and take
    this rank's device.  Returns (rank, world); (0, 1) for a plain single-process run.  args._own_group says whether the group
    was created here (run() then destroys it on the way out; a caller's group is the caller's)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args._own_group = False
    if world < 2:
        return 0, 1
    import torch.distributed as dist
    if not dist.is_initialized():
        args._own_group = True
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("MCGRA_SHARED_GPU") == "1":
            dist.init_process_group("gloo")
            args.device = "cuda:0"
        else:
            local = int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
            args.device = f"cuda:{local}"
            dist.init_process_group("nccl", device_id=torch.device(args.device))
    torch.cuda.set_device(torch.device(args.device))
    return dist.get_rank(), dist.get_world_size()


def run(args):
    """main.py:78-324 for one configuration.  Under a launcher every rank calls this; the process group this call created is
    destroyed on the way out, also when the run fails (a rank that dies with the group alive leaves its peers in a collective)."""
    rank, world = init_distributed(args)
    try:
        return _run(args, rank, world)
    finally:
        if world > 1 and getattr(args, "_own_group", False):
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


def _exit(message):
    raise SystemExit(message)


def _run(args, rank, world):
    check_topk_args(args, _exit)
    check_binarize_args(args, _exit)
    check_curves_args(args, _exit)
    check_per_node_args(args, _exit)
    check_ci_args(args, _exit)
    check_ci_nodes_args(args, _exit)
    check_structure_args(args, _exit)
    device = torch.device(args.device)
    np.random.seed(args.seed); random.seed(args.seed); torch.manual_seed(args.seed)       # main.py:142-146
    data = Dataset(root=args.dataset_root, name=args.dataset, setting='GCN')
    adj, features, labels, init_adj = data.adj, data.features, data.labels, data.init_adj
    idx_train, idx_val, idx_test = data.idx_train, data.idx_val, data.idx_test
    random.sample(range(adj.shape[0]), int(adj.shape[0] * args.nlabel))                    # main.py:155 (consumes the RNG)
    adj, features, labels = utils.preprocess(adj, features, labels, preprocess_adj=False, onehot_feature=False)
    if args.mode == "prepare":
        if rank == 0:
            os.makedirs(args.saved_data, exist_ok=True)
            np.save(os.path.join(args.saved_data, args.dataset + ".npy"), label_adjacency(labels))
        if world > 1:      # the file is there when any rank returns (the next command of a script reads it)
            import torch.distributed as dist
            dist.barrier()
        return None
    feature_adj = dot_product_decode(features, args.dataset)
    if args.nofeature:
        feature_adj = torch.eye(*feature_adj.size())
    init_adj = torch.FloatTensor(init_adj.todense())

    nfeat, nclass = features.shape[1], labels.max().item() + 1
    if args.arch == "gcn":                                                                 # main.py:175-190
        victim_model = GCN(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5, weight_decay=5e-4,
                           device=device).to(device)
        victim_model.fit(features, adj, labels, idx_train, idx_val, verbose=False)
        embedding = embedding_GCN(nfeat=nfeat, nhid=16, nlayer=args.nlayers, device=device)
        embedding.gc = deepcopy(victim_model.gc)
    elif args.arch == "sage":                                                              # main.py:193-210
        victim_model = graphsage(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5,
                                 weight_decay=5e-4, device=device).to(device)
        for l in victim_model.gc:
            l.to(device)
        victim_model.fit(features, adj, labels, idx_train, idx_val, verbose=False)
        embedding = embedding_graphsage(nfeat=nfeat, nhid=16, nlayer=args.nlayers, device=device)
        embedding.gc = deepcopy(victim_model.gc)
    else:                                                                                  # main.py:213-231
        victim_model = GAT(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5, alpha=0.1, nheads=5,
                           device=device).to(device)
        victim_model.fit(features, adj, labels, idx_train, idx_val, train_iters=getattr(args, "gat_train_iters", 200))
        embedding = embedding_gat(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5, alpha=0.1,
                                  nheads=5, device=device)
        embedding.attentions = victim_model.attentions
    if world > 1:
        # one victim for all ranks: rank 0's parameters (training on the same seed is not guaranteed to be bit-reproducible
        # across processes); the embedding shares / copies them as main.py:190 / :210 / :231 do
        import torch.distributed as dist
        staged = str(dist.get_backend()).lower() != "nccl"
        with torch.no_grad():
            for p_ in victim_tensors(victim_model):
                t_ = p_.data.cpu() if staged else p_.data
                dist.broadcast(t_, 0)
                if staged:
                    p_.data.copy_(t_)
        if args.arch != "gat":
            embedding.gc = deepcopy(victim_model.gc)
    # main.py:233-241, call for call: the victim is in eval mode (fit() leaves it there), the freshly built embedding is
    # NOT -- embedding_gat.forward therefore applies F.dropout(0.5) and the reference's H_A priors of --arch gat carry
    # dropout noise (embedding_GCN / embedding_graphsage have no dropout); each call consumes the RNG as the reference's does
    embedding = embedding.to(device)
    with torch.no_grad():
        fd, ad = features.to(device), adj.to(device)
        embedding(fd, ad)                                                                  # H_A     main.py:235
        Y_A = victim_model(fd, ad)                                                         # main.py:236
        embedding.set_layers(1)
        H_A1 = embedding(fd, ad)                                                           # main.py:238-239
        embedding.set_layers(2)
        H_A2 = embedding(fd, ad)                                                           # main.py:240-241
        out = victim_model(fd, utils.normalize_adj_tensor(ad))
        print("Test set results:", "accuracy= {:.4f}".format(utils.accuracy(out[idx_test], labels.to(device)[idx_test]).item()))
    idx_attack = np.array(random.sample(range(adj.shape[0]), int(adj.shape[0] * args.nlabel)))   # main.py:244
    num_edges = int(0.5 * args.density * adj.sum() / adj.shape[0] ** 2 * len(idx_attack) ** 2)

    lab_path = os.path.join(args.saved_data, args.dataset + ".npy")
    label_adj = np.load(lab_path) if os.path.exists(lab_path) else label_adjacency(labels)
    if args.mode == "notrain_test":                                                        # main.py:412-437: no attack
        want_ap = getattr(args, "ap", False)
        if want_ap:
            res, aps = prior_rank_metrics(ad, feature_adj, H_A1, H_A2, Y_A, label_adj, args.dataset)
            res["ap"] = aps
        else:
            res = prior_aucs(ad, feature_adj, H_A1, H_A2, Y_A, label_adj, args.dataset)
        if rank == 0:
            print("feautre adj=", res["feature"])
            print("layer1 adj=", res["layer1"])
            print("layer2 adj=", res["layer2"])
            print("out adj=", res["out"])
            if want_ap:
                for k in ("feature", "layer1", "layer2", "out", "label"):
                    print(f"{k} ap=", res["ap"][k])
        return res
    want_ci, versus = bool(getattr(args, "ci", False)), getattr(args, "versus", None)
    want_ci_nodes = bool(getattr(args, "ci_nodes", False))
    other = None
    if versus is not None:  # refused before the attack runs, not after it
        other = feature_adj if versus == "features" else load_versus(versus, adj.shape[0])
    lr = 10 ** args.lr                                                                     # objective(): main.py:282-283
    weight_param = tuple(getattr(args, f"w{i}") for i in range(1, 11))
    model = PGDAttack(model=victim_model, embedding=embedding, H_A=H_A2, Y_A=Y_A, nnodes=adj.shape[0],
                      loss_type='CE', device=device)
    if getattr(args, "adj_changes_init", None) is not None:      # (tests: a seeded start; adj_changes is a public attribute, :77)
        model.adj_changes = args.adj_changes_init
    model.attack(args, None, lr, 0, args.weight_sup, weight_param, feature_adj, 0, 0, 0, idx_train, idx_val,
                 idx_test, adj, features, init_adj, labels, idx_attack, num_edges, 0, epochs=args.epochs,
                 label_adj=label_adj)
    inference_adj = model.modified_adj                     # stays on the device: the three AUCs run there (main.py:247-250)
    want_ap = getattr(args, "ap", False)
    if want_ap:             # AUC and average precision from one sort per index set; the AUCs are metric_pool's bit for bit
        sets = {"attack": idx_attack, "train": idx_train, "all": None}
        both = {k: engine.rank_metrics(ad.to(inference_adj.device), inference_adj, ix) for k, ix in sets.items()}
        res = {f"auc_{k}": float(both[k][0]) for k in sets}
        res["density"] = float(inference_adj.mean())
        res.update({f"ap_{k}": float(both[k][1]) for k in sets})
    else:
        res = {"auc_attack": float(metric_pool(ad, inference_adj, idx_attack)),
               "auc_train": float(metric_pool(ad, inference_adj, idx_train)),
               "auc_all": float(metric_pool(ad, inference_adj, None)),
               "density": float(inference_adj.mean())}
    want_topk = getattr(args, "topk", None) is not None
    if want_topk:           # every rank computes (as the AUCs); the keys exist only with the flag
        res.update(topk_report(ad, inference_adj, {"attack": idx_attack, "train": idx_train, "all": None}, args.topk))
    want_split = bool(getattr(args, "binarize", False))
    if want_split:          # every rank computes; the keys exist only with the flag
        res.update(binarize_report(ad, inference_adj, {"attack": idx_attack, "train": idx_train, "all": None}))
    want_curves = bool(getattr(args, "curves", None))
    if want_curves:         # every rank computes; rank 0 writes the file
        res.update(curves_report(args.curves if rank == 0 else None, ad, inference_adj,
                                 {"attack": idx_attack, "train": idx_train, "all": None}))
    want_per_node = bool(getattr(args, "per_node", None))
    if want_per_node:       # every rank computes; rank 0 writes the file
        res.update(per_node_report(args.per_node if rank == 0 else None, ad, inference_adj,
                                   {"attack": idx_attack, "train": idx_train, "all": None}))
    if want_ci:             # every rank computes; the keys exist only with the flag
        res.update(ci_report(ad, inference_adj, {"attack": idx_attack, "train": idx_train, "all": None}, other))
    if want_ci_nodes:       # every rank computes; the keys exist only with the flag
        res.update(ci_nodes_report(ad, inference_adj, {"attack": idx_attack, "train": idx_train, "all": None}, other))
    want_structure = getattr(args, "structure", None) is not None
    if want_structure:      # every rank computes; the keys exist only with the flag
        res.update(structure_report(ad, inference_adj, {"attack": idx_attack, "train": idx_train, "all": None},
                                    structure_source(args.structure)))
    res["path"] = dict(model.history.get("path", {}), world=world)
    if rank != 0:           # every rank holds the same modified_adj; rank 0 reports
        return res
    print(f"current auc={res['auc_all']}")
    if want_ap:
        print(f"current ap={res['ap_all']}")
    if want_topk:
        print(f"current f1={res['topk_all']['f1']} (k={res['topk_all']['k']})")
        if getattr(args, "save_edges", None):
            save_edges(args.save_edges, ad, inference_adj, res["topk_all"]["k"])
    if want_split:
        d = res["split_all"]
        print(f"current split_f1={d['f1']} (edges={d['edges']}, threshold={d['threshold']})")
        if getattr(args, "save_graph", None):
            save_graph(args.save_graph, ad, inference_adj, d)
    if want_curves:
        print(f"current best_f1={res['curves_all']['best_f1']} (threshold={res['curves_all']['best_threshold']})")
    if want_per_node:
        d = res["per_node_all"]
        print(f"current macro_auc={d['macro_auc']} mrr={d['mrr']} hits@1={d['hits_at_1']}")
    if want_ci:
        d = res["ci_all"]
        print(f"current auc_pairs={d['auc']} se={d['se']} ci=[{d['ci_low']}, {d['ci_high']}]")
        if other is not None:
            d = res["versus_all"]
            print(f"current delta={d['delta']} z={d['z']} p={d['p_value']}")
    if want_ci_nodes:
        d = res["ci_nodes_all"]
        ratio = f" se_nodes/se={_se_ratio(d, res['ci_all'])}" if want_ci else ""
        print(f"current auc_pairs={d['auc']} se_nodes={d['se']} ci_nodes=[{d['ci_low']}, {d['ci_high']}]{ratio}")
        if other is not None:
            d = res["versus_nodes_all"]
            print(f"current delta={d['delta']} se_nodes={d['se_delta']} z={d['z']} p={d['p_value']}")
        if getattr(args, "save_influence", None):
            save_influence(args.save_influence, res, {"attack": idx_attack, "train": idx_train, "all": None}, adj.shape[0])
    if want_structure:
        d = res["structure_all"]
        q = d["stats"]
        print(f"current transitivity={q['recovered']['transitivity']} (true {q['true']['transitivity']}) "
              f"triangles={d['T_C']}/{d['T_G']} degree_corr={q['degree_corr']} degree_ks={q['degree_ks']}")
        if getattr(args, "save_structure", None):
            save_structure(args.save_structure, res, {"attack": idx_attack, "train": idx_train, "all": None}, adj.shape[0])
    if getattr(args, "save_scores", None):
        save_scores(args.save_scores, inference_adj)
    os.makedirs("./results/", exist_ok=True)
    # the parameter line names --ap, --topk, --save_edges, --binarize, --save_graph, --curves and --per_node only when they are set:
    # without them the log is what it was before the flags existed
    hidden = (set() if want_ap else {"ap"}) | (set() if want_topk else {"topk", "save_edges"}) | \
        (set() if want_curves else {"curves"}) | (set() if want_per_node else {"per_node"}) | \
        (set() if want_split else {"binarize", "save_graph"})
    shown = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in hidden})
    with open(os.path.join("./results", args.log_name), "a") as f:                         # main.py:314-323
        f.write(f"current parameter: {shown}\n")
        f.write(f"In attack graph: AUC={res['auc_attack']}\tIn train graph: AUC={res['auc_train']}\t"
                f"In Whole Graph: AUC={res['auc_all']}\n")
        if want_ap:
            f.write(f"In attack graph: AP={res['ap_attack']}\tIn train graph: AP={res['ap_train']}\t"
                    f"In Whole Graph: AP={res['ap_all']}\n")
        if want_topk:
            f.write("\t".join(f"In {name}: k={d['k']} P={d['precision']} R={d['recall']} F1={d['f1']}" for name, d in
                              (("attack graph", res["topk_attack"]), ("train graph", res["topk_train"]),
                               ("Whole Graph", res["topk_all"]))) + "\n")
        if want_split:
            for name, d in (("attack graph", res["split_attack"]), ("train graph", res["split_train"]),
                            ("Whole Graph", res["split_all"])):
                f.write(f"In {name}: split edges={d['edges']} threshold={d['threshold']} rounds={d['iterations']} "
                        f"P={d['precision']} R={d['recall']} F1={d['f1']}\n")
        if want_curves:
            f.write("\t".join(f"In {name}: ROC points={d['roc_points']} PR points={d['pr_points']} levels={d['levels']} "
                              f"best F1={d['best_f1']} at {d['best_threshold']}" for name, d in
                              (("attack graph", res["curves_attack"]), ("train graph", res["curves_train"]),
                               ("Whole Graph", res["curves_all"]))) + "\n")
        if want_per_node:
            for name, d in (("attack graph", res["per_node_attack"]), ("train graph", res["per_node_train"]),
                            ("Whole Graph", res["per_node_all"])):
                f.write(f"In {name}: scored nodes={d['scored']} macro AUC={d['macro_auc']} MRR={d['mrr']} "
                        f"Hits@1={d['hits_at_1']} R-precision={d['r_precision']}\n")
        if want_ci:
            for name, key in (("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all")):
                d = res[f"ci_{key}"]
                f.write(f"In {name}: pairs={d['pairs']} positives={d['positives']} AUC of pairs={d['auc']} se={d['se']} "
                        f"{int(round(100 * d['level']))}% CI=[{d['ci_low']}, {d['ci_high']}]\n")
                if other is not None:
                    d = res[f"versus_{key}"]
                    f.write(f"In {name}: versus {versus}: AUC={d['b']['auc']} delta={d['delta']} se={d['se_delta']} "
                            f"z={d['z']} p={d['p_value']}\n")
        if want_ci_nodes:
            for name, key in (("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all")):
                d = res[f"ci_nodes_{key}"]
                ratio = f" se_nodes/se={_se_ratio(d, res[f'ci_{key}'])}" if want_ci else ""
                f.write(f"In {name}: nodes={d['nodes']} pairs={d['pairs']} AUC of pairs={d['auc']} "
                        f"jackknife AUC={d['auc_jackknife']} se_nodes={d['se']} "
                        f"{int(round(100 * d['level']))}% CI_nodes=[{d['ci_low']}, {d['ci_high']}] "
                        f"undefined_nodes={d['undefined_nodes']}{ratio}\n")
                if other is not None:
                    d = res[f"versus_nodes_{key}"]
                    f.write(f"In {name}: versus {versus} (nodes): AUC={d['b']['auc']} delta={d['delta']} se_nodes={d['se_delta']} "
                            f"z={d['z']} p={d['p_value']}\n")
        if want_structure:
            for name, key in (("attack graph", "attack"), ("train graph", "train"), ("Whole Graph", "all")):
                d = res[f"structure_{key}"]
                q = d["stats"]
                f.write(f"In {name}: structure at {d['threshold']}: edges={d['E_R']} (true {d['E_G']}, shared {d['E_C']}) "
                        f"triangles={d['T_R']} (true {d['T_G']}, shared {d['T_C']}) "
                        f"transitivity={q['recovered']['transitivity']} (true {q['true']['transitivity']}) "
                        f"clustering={q['recovered']['avg_clustering']} (true {q['true']['avg_clustering']}) "
                        f"degree_corr={q['degree_corr']} degree_ks={q['degree_ks']} degree_l1={q['degree_l1']}\n")
        f.write(f"current density: {res['density']}\n")
    return res


if __name__ == '__main__':
    run(build_parser().parse_args())
