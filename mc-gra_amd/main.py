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
The reports of mc-gra_amd/reports.py: none is in the reference, each is for --mode evaluate only and absent by default (and then
nothing changes), each looks at modified_adj within the index sets attack, train and all, and each --save_* flag needs its
report's flag and writes an .npz at PATH.  README.md lists the result keys, the printed lines and the arrays of every file.
--topk K: of the K best-scored unordered node pairs of a set, how many are true edges -- precision, recall and F1 at K
(engine.topk_metrics; ties by packed position).  K = 0 takes each set's own true edge count; a K above a set's pair count is
clamped, and the printed k says so.  --save_edges PATH: the whole graph's selection in ranking order (engine.top_pairs).
--curves PATH writes what the reference's roc_curve call returns and the precision-recall curve beside it (sklearn's conventions
and defaults; engine.rank_curves, engine.precision_recall_curve) and reports the best F1 over all thresholds.
--per_node PATH asks whose neighbourhood leaked: for each node of a set, how its true neighbours rank among the set's other nodes
by its row of modified_adj (engine.node_rank_metrics), written per node, with the macro AUC, the MRR and Hits@1 reported.
--binarize answers "which graph did the attack recover" without the truth: an exact integer 2-means splits a set's entries in two
(engine.two_means_split; the defined form of PGDAttack.kmeans, baseline.py:88-109) and the upper cluster, the recovered edge set,
is scored against the true graph.  The scores must lie in [0, 16): brazil's unbounded decode is refused when it holds more.
--save_graph PATH: the whole graph's recovered edges in packed order, the threshold and the round count (engine.threshold_pairs).
--ci: DeLong's standard error and 95 % interval of the AUC of a set's unordered node pairs (engine.auc_delong): a lower bound on the
uncertainty, since pairs that share a node are not independent.  --ci_nodes: the conservative bracket beside it, the delete-one-node
jackknife of the same AUC (engine.auc_node_jackknife); with --ci the ratio se_nodes / se.  --save_influence PATH: each node's share.
--versus features|PATH (needs --ci or --ci_nodes) asks whether the attack beats another scoring of the same pairs, the run's own
feature_adj or an n x n float32 .npy at PATH: DeLong's paired test (engine.auc_delong_paired) and the jackknife of the difference
(engine.auc_node_jackknife_paired).  --save_scores PATH (--mode evaluate only) writes modified_adj as that .npy.
--structure split|edges|THRESHOLD asks whether the recovered graph LOOKS like the real one: a set is cut at the threshold of its
own 2-means split, at the score of the P-th best pair, P its true edge count (ties may add edges), or at a float, and the degrees,
triangles, wedges, transitivity and clustering of that graph are reported beside the true graph's (engine.graph_structure).
--save_structure PATH: degree and triangles per node in the recovered graph, the true graph and their intersection.
--hops H (1 to 8) asks which non-edges the attack confuses with edges: the AUC of a set's true edges against its non-edges at
distance 2, 3, ..., H of the true graph on the set's nodes and against those beyond (engine.hop_auc); the pooled AUC of --ci is
their mean weighted by the classes' sizes.  --hops_cut split|edges|THRESHOLD (default edges; --structure's cuts) says where the
false positives are counted, class by class.  --save_hops PATH: the counts, the sums and the AUC of every class.
--by_class labels|degree|PATH asks what the attack knows beyond the node classes it was handed: the AUC of a set's true edges
against the non-edges of the SAME stratum of class pairs (engine.class_auc) -- same-class and different-class pairs, and every
unordered class pair as a block, with the blocks' pooled-within and covariate-adjusted AUC beside the pooled AUC of --ci, and
the share of same-class pairs among the true edges, the recovered pairs and all pairs.  The classes are the run's node labels,
min(15, bit_length) of a node's degree in the true graph, or an integer .npy with one class in [0, 16) per node.
--by_class_cut split|edges|THRESHOLD (default edges; --structure's cuts) says where the recovered pairs are counted.
--save_by_class PATH: the counts, the sums and the AUC of every block, and the class of every node.
--ablate [table|shapley] asks which summand of modified_adj carries it.  After the loop modified_adj is a sum of up to eight
matrices (engine.ENSEMBLE_COMPONENTS: the learned adjacency, feature_adj, the decodes of H_A1 / H_A2 / Y_A2 on the recovered graph,
the decodes of the priors H_A and Y_A, the label adjacency); the attack keeps them apart (every prior it holds is decoded, the
use flags only choose what modified_adj sums, so modified_adj is bit for bit what it is without the flag) and ONE pass over a
set's pairs ranks many subset sums (engine.subset_auc).  `table` (the default): the sum in use, every present summand alone, the
sum in use without each of its summands, and the base five with every combination of --useH_A --useY_A --useY -- the paper's
flag table from one run.  `shapley`: every non-empty subset of the present summands and each summand's exact Shapley share of
AUC - 1/2.  On polblogs / usair the decode branch itself depends on the use flags: there a subset's AUC is that of THIS run's
decode mode, not of a rerun with other flags; for cora, citeseer, AIDS and brazil the flag table is the rerun's.
--save_ablation PATH: every subset's mask, T and AUC per index set.
--knn K asks for the recovered graph as a LOCAL cut: every node of a set keeps its own K best-scored partners (its row of
modified_adj; engine.knn_graph), and the lists are symmetrised as the union (either end picks the other) and as the mutual graph
(both do).  Each is scored against the true graph, beside the F1 of --topk's global cut at exactly the same number of edges,
with the nodes either leaves without an edge and the hubness of the lists: the largest in-degree, the nodes in nobody's list and
the skewness of the in-degrees.  K = 0 takes each set's own mean true degree, rounded; K is clamped to the set's size less one
and to 1024.  --save_knn PATH: per node the in-degree, the degrees and the hits; the whole graph's union as an edge list.
--exposure asks which edges leak: every true edge of a set is placed among ALL the set's non-edges (engine.edge_exposure) and the
edges are classed by their embeddedness, the common neighbours of their two ends in the true graph on the set's nodes (0, 1, ...,
14, 15+), and by the smaller of the two degrees (1, 2-3, 4-7, ...); per class the count, the AUC of the class's edges against all
non-edges -- the pooled AUC of --ci is their mean weighted by the counts -- and the recall at a cut.  --exposure_cut
split|edges|THRESHOLD (default edges; --structure's cuts) says where.  --save_exposure PATH: every set's 16 x 16 table and the
whole graph's true edges one by one: placement, common neighbours, degrees.
--mode link_stealing (not in the reference) is the baseline every paper in this line compares with, Attack-0 of He et al.,
"Stealing Links from Graph Neural Networks" (USENIX Security 2021): notrain_test's flow up to the priors -- no attack, nothing
written -- then the AUC (with --ap the average precision too) of the unordered node pairs of attack, train and all scored by
minus a distance between the two nodes' rows of `posteriors` (exp(Y_A)), `embedding` (H_A2) or `features`, for each of cosine,
euclidean, correlation, chebyshev, braycurtis, canberra, cityblock and sqeuclidean (engine.pair_distance_rank_metrics: pair by
pair on the GPU, no n x n score matrix); one `link stealing <source> <metric>: auc_attack=... auc_train=... auc_all=...` line each.
--versus SOURCE:METRIC (--mode evaluate, with --ci or --ci_nodes) takes one of those 24 scorings as the other side of the paired
tests (engine.pair_distance_scores): does the attack beat this baseline on these pairs, with delta, se_delta, z and p_value.
--dp_defense edgerand|lapgraph --dp_eps EPS [--dp_seed S] (not in the reference, whose --defense only loads weight files it does not
ship; --defense and --add_noise stay parsed and unused, as there) defends the victim with one of the two edge-level differential-
privacy mechanisms of Wu et al., "LinkTeller" (IEEE S&P 2022): EdgeRand, randomised response on every node pair, or LapGraph,
Laplace noise on every pair and then the noisy top-E~ (engine.dp_perturb_graph: one Philox draw per pair keyed by the seed and the
pair, so every run, rank and device perturbs alike; S defaults to --seed).  The victim is trained on, and answers from, the
perturbed graph: the fit, the priors H_A / Y_A / H_A1 / H_A2, the test accuracy and the graph the attack is handed.  Every score --
the AUCs, every report above, the baselines of --mode link_stealing, the priors of --mode notrain_test -- stays against the TRUE
graph, so each becomes a report about a defended victim.  The result gains `defense` (what the mechanism kept, added and removed,
the realised flip probability or the count's noise, and the defended victim's test accuracy: the utility side of the trade) and
one `defense ...` line; --mode evaluate also reports auc_perturbed_*, the AUC of modified_adj against the perturbed graph: which of
the two graphs the attack recovered.  --save_defense PATH: the perturbed graph's edge list in packed order, the pairs added and
removed, and those scalars.  --mode evaluate, notrain_test, link_stealing and link_teller.
--mode link_teller (not in the reference) is the attack those two mechanisms were designed against, the influence attack of Wu et
al., "LinkTeller" (IEEE S&P 2022): link_stealing's flow up to the priors -- no attack, no engine object, nothing written -- then every
node's features are scaled by 1 + delta in turn (--lt_delta, default 1e-4) and every other node's posteriors are watched:
I[v -> u] = || O(X^(v))_u - O(X)_u ||_2 / delta, a pair's score max(I[a -> b], I[b -> a]) (engine.influence_scores: the differences are
carried along the graph's support on the GPU, one source costs its L-hop neighbourhood, not a forward pass).  The victim answers from
the graph it was trained and tested on, normalised (the perturbed graph under --dp_defense); --lt_graph raw queries the un-normalised
graph of the priors instead, without self-loops, where a 2-layer victim's influence follows walks of exactly two steps and neighbours
without a common neighbour score 0.  --arch gcn only.  For the outputs `log_posteriors` and `posteriors` and the sets attack, train and
all: the AUC (engine.auc_delong's, of the unordered pairs) and, for the paper's density beliefs 1/4, 1/2, 1, 2 and 4, the precision,
recall and F1 of the k = belief x (true edge count) best pairs (engine.topk_metrics); one `link teller <output>: auc_attack=...
auc_train=... auc_all=...` line per output and one belief line per output and set.  --save_linkteller PATH: the whole graph's best pairs
per output (as many as it has true edges, engine.top_pairs), the counts and the parameters as an .npz.  --ap and every report flag are
refused in this mode.  --versus linkteller:posteriors|log_posteriors (--mode evaluate, with --ci or --ci_nodes, --arch gcn) takes that
matrix (normalised graph, delta 1e-4) as the other side of the paired tests.
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
    from mc_gra_amd import engine, reports, topology_attack, utils
    from mc_gra_amd.dataset import Dataset
    from mc_gra_amd.models.gcn import GCN, embedding_GCN
    from mc_gra_amd.models.gat import GAT, embedding_gat
    from mc_gra_amd.models.graphsage import graphsage, embedding_graphsage
    from mc_gra_amd.topology_attack import PGDAttack
else:
    from . import engine, reports, topology_attack, utils
    from .dataset import Dataset
    from .models.gcn import GCN, embedding_GCN
    from .models.gat import GAT, embedding_gat
    from .models.graphsage import graphsage, embedding_graphsage
    from .topology_attack import PGDAttack

import torch
import torch.nn.functional as F


class _Parser(argparse.ArgumentParser):
    def parse_args(self, *a, **k):
        args = super().parse_args(*a, **k)
        for r in reports.EVALUATE_REPORTS + reports.LATER_REPORTS:
            r.check(args, self.error)
        reports.check_link_teller_args(args, self.error)
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
    p.add_argument("--mode", type=str, default="evaluate", choices=["evaluate", "prepare", "notrain_test", "link_stealing", reports.LINKTELLER_MODE])
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
    p.add_argument('--versus', type=str, default=argparse.SUPPRESS)            # with --ci: paired test against `features`, SOURCE:METRIC or an .npy
    p.add_argument('--save_scores', type=str, default=argparse.SUPPRESS)       # write modified_adj as an .npy for a later --versus
    p.add_argument('--ci_nodes', action='store_true', default=argparse.SUPPRESS)   # also the node-jackknife se and interval of the AUC
    p.add_argument('--save_influence', type=str, default=argparse.SUPPRESS)    # with --ci_nodes: each node's influence as an .npz
    p.add_argument('--structure', type=str, default=argparse.SUPPRESS)         # also degrees, triangles and clustering of the cut graph
    p.add_argument('--save_structure', type=str, default=argparse.SUPPRESS)    # with --structure: the per-node columns as an .npz
    p.add_argument('--hops', type=int, default=argparse.SUPPRESS)              # also the AUC by true-graph distance 2 .. H and beyond
    p.add_argument('--hops_cut', type=str, default=argparse.SUPPRESS)          # with --hops: where its false positives are counted
    p.add_argument('--save_hops', type=str, default=argparse.SUPPRESS)         # with --hops: the per-distance counts as an .npz
    p.add_argument('--by_class', type=str, default=argparse.SUPPRESS)          # also the AUC within the classes of labels | degree | an .npy
    p.add_argument('--by_class_cut', type=str, default=argparse.SUPPRESS)      # with --by_class: where its pairs above a cut are counted
    p.add_argument('--save_by_class', type=str, default=argparse.SUPPRESS)     # with --by_class: the per-block counts as an .npz
    p.add_argument('--ablate', type=str, nargs='?', const='table', default=argparse.SUPPRESS)   # also the AUC of subsets of modified_adj's summands
    p.add_argument('--save_ablation', type=str, default=argparse.SUPPRESS)     # with --ablate: every subset's T and AUC as an .npz
    p.add_argument('--knn', type=int, default=argparse.SUPPRESS)               # also the k-nearest-neighbour graphs of the scores
    p.add_argument('--save_knn', type=str, default=argparse.SUPPRESS)          # with --knn: the per-node columns and the union's edges as an .npz
    p.add_argument('--exposure', action='store_true', default=argparse.SUPPRESS)   # also the true edges' AUC by common neighbours and min degree
    p.add_argument('--exposure_cut', type=str, default=argparse.SUPPRESS)      # with --exposure: where the recovered true edges are counted
    p.add_argument('--save_exposure', type=str, default=argparse.SUPPRESS)     # with --exposure: the tables and the whole graph's edges as an .npz
    p.add_argument('--dp_defense', type=str, choices=list(engine.DP_MECHANISMS), default=argparse.SUPPRESS)   # train the victim on an edge-DP graph
    p.add_argument('--dp_eps', type=float, default=argparse.SUPPRESS)          # with --dp_defense: the edge-level privacy budget
    p.add_argument('--dp_seed', type=int, default=argparse.SUPPRESS)           # with --dp_defense: the mechanism's seed (default: --seed)
    p.add_argument('--save_defense', type=str, default=argparse.SUPPRESS)      # with --dp_defense: the perturbed graph and what changed as an .npz
    p.add_argument('--lt_graph', type=str, choices=list(reports.LINKTELLER_GRAPHS), default=argparse.SUPPRESS)   # --mode link_teller: the graph queried
    p.add_argument('--lt_delta', type=float, default=argparse.SUPPRESS)        # --mode link_teller: the relative feature perturbation (1e-4)
    p.add_argument('--save_linkteller', type=str, default=argparse.SUPPRESS)   # --mode link_teller: the best pairs, counts and parameters as an .npz
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


def link_sources(Y_A, H_A2, features, device):
    """What a link-stealing distance is taken between (reports.LINK_SOURCES), each n x d float32 on the device: the victim's
    posteriors exp(Y_A) (Y_A is the log-softmax the attack itself is given), the embedding H_A2, the preprocessed features."""
    feats = features.to_dense() if features.is_sparse else features
    return {"posteriors": torch.exp(Y_A.detach().to(device=device, dtype=torch.float32)),
            "embedding": H_A2.detach().to(device=device, dtype=torch.float32),
            "features": feats.detach().to(device=device, dtype=torch.float32)}


def link_stealing_metrics(real, sources, sets, want_ap):
    """--mode link_stealing: Attack-0 of He et al. (USENIX Security 2021) on this run's victim.  For every source, each of
    engine.PAIR_METRICS and every index set, the AUC (with want_ap the average precision too) of the unordered node pairs
    scored by minus the distance of their two rows (engine.pair_distance_rank_metrics: no n x n score matrix).
    out[source][metric][set] = {"auc", "pairs", "positives"} (+ "ap")."""
    keep = ("auc", "pairs", "positives") + (("ap",) if want_ap else ())
    out = {}
    for source, Z in sources.items():
        out[source] = {}
        for metric in engine.PAIR_METRICS:
            per_set = {name: engine.pair_distance_rank_metrics(real, Z, metric, ix) for name, ix in sets.items()}
            out[source][metric] = {name: {k: d[k] for k in keep} for name, d in per_set.items()}
    return out


def link_stealing_lines(res, want_ap):
    """One line per source and metric of link_stealing_metrics' result."""
    lines = []
    for source, by_metric in res.items():
        for metric, by_set in by_metric.items():
            line = f"link stealing {source} {metric}: " + " ".join(f"auc_{name}={d['auc']}" for name, d in by_set.items())
            if want_ap:
                line += " " + " ".join(f"ap_{name}={d['ap']}" for name, d in by_set.items())
            lines.append(line)
    return lines


def link_teller_scores(victim_model, features, victim_graph, graph, delta, outputs=None):
    """The LinkTeller pair scores of this run's victim: {output: n x n matrix} over `outputs` (default: engine.INFLUENCE_OUTPUTS)
    and the info of the call.  graph "normalised": the victim is queried on utils.normalize_adj_tensor(victim_graph), what it was
    trained and tested on; "raw": on victim_graph as it is, what the priors are computed from."""
    query = victim_graph if graph == "raw" else utils.normalize_adj_tensor(victim_graph)
    feats = features.to_dense() if features.is_sparse else features
    matrices, info = {}, None
    for output in outputs or engine.INFLUENCE_OUTPUTS:
        matrices[output], info = engine.influence_scores(victim_model, feats, query, delta, output, "max")
    return matrices, {"delta": info["delta"], "graph": graph, "nnz": info["nnz"], "reached": info["reached"],
                      "max_reach": info["max_reach"]}


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


def base_metrics(ctx, want_ap):
    """The three AUCs of main.py:247-250 and the density, on the device; with --ap the AUC and the average precision of each
    index set from one sort (engine.rank_metrics), the AUCs metric_pool's bit for bit.  Keys: auc_*, density, then ap_*."""
    if want_ap:
        both = {k: engine.rank_metrics(ctx.real, ctx.inference_adj, ix) for k, ix in ctx.sets.items()}
        res = {f"auc_{k}": float(v[0]) for k, v in both.items()}
    else:
        res = {f"auc_{k}": float(metric_pool(ctx.real, ctx.inference_adj, ix)) for k, ix in ctx.sets.items()}
    res["density"] = float(ctx.inference_adj.mean())
    if want_ap:
        res.update({f"ap_{k}": float(v[1]) for k, v in both.items()})
    return res


def log_lines(res, ctx):
    """What one run appends to the log (main.py:314-323), the lines of the reports that are on between the AUCs and the density."""
    lines = [f"current parameter: {reports.shown_parameters(ctx.args)}",
             f"In attack graph: AUC={res['auc_attack']}\tIn train graph: AUC={res['auc_train']}\t"
             f"In Whole Graph: AUC={res['auc_all']}"]
    if getattr(ctx.args, "ap", False):
        lines.append(f"In attack graph: AP={res['ap_attack']}\tIn train graph: AP={res['ap_train']}\t"
                     f"In Whole Graph: AP={res['ap_all']}")
    for r in reports.EVALUATE_REPORTS + reports.LATER_REPORTS:
        if r.wanted(ctx.args):
            lines += r.log(res, ctx)
    return lines + [f"current density: {res['density']}"]


def _run(args, rank, world):
    for r in reports.EVALUATE_REPORTS + reports.LATER_REPORTS:
        r.check(args, _exit)
    reports.check_link_teller_args(args, _exit)
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
    # --dp_defense: the victim is trained on, and answers from, the perturbed graph; everything that scores the attack keeps
    # the true one.  Every rank computes the same graph from the same seed (engine.dp_perturb_graph), so nothing is broadcast
    victim_adj, perturbed, defense = adj, None, None
    if "dp_defense" in vars(args):
        perturbed, dp_info = engine.dp_perturb_graph(adj.to(device), args.dp_defense, args.dp_eps, reports.defense_seed(args))
        victim_adj = perturbed.cpu()
    feature_adj = dot_product_decode(features, args.dataset)
    if args.nofeature:
        feature_adj = torch.eye(*feature_adj.size())
    init_adj = torch.FloatTensor(init_adj.todense())

    nfeat, nclass = features.shape[1], labels.max().item() + 1
    if args.arch == "gcn":                                                                 # main.py:175-190
        victim_model = GCN(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5, weight_decay=5e-4,
                           device=device).to(device)
        victim_model.fit(features, victim_adj, labels, idx_train, idx_val, verbose=False)
        embedding = embedding_GCN(nfeat=nfeat, nhid=16, nlayer=args.nlayers, device=device)
        embedding.gc = deepcopy(victim_model.gc)
    elif args.arch == "sage":                                                              # main.py:193-210
        victim_model = graphsage(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5,
                                 weight_decay=5e-4, device=device).to(device)
        for l in victim_model.gc:
            l.to(device)
        victim_model.fit(features, victim_adj, labels, idx_train, idx_val, verbose=False)
        embedding = embedding_graphsage(nfeat=nfeat, nhid=16, nlayer=args.nlayers, device=device)
        embedding.gc = deepcopy(victim_model.gc)
    else:                                                                                  # main.py:213-231
        victim_model = GAT(nfeat=nfeat, nclass=nclass, nhid=16, nlayer=args.nlayers, dropout=0.5, alpha=0.1, nheads=5,
                           device=device).to(device)
        victim_model.fit(features, victim_adj, labels, idx_train, idx_val, train_iters=getattr(args, "gat_train_iters", 200))
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
        vd = ad if perturbed is None else perturbed        # what the victim answers from; ad stays the truth of every score
        embedding(fd, vd)                                                                  # H_A     main.py:235
        Y_A = victim_model(fd, vd)                                                         # main.py:236
        embedding.set_layers(1)
        H_A1 = embedding(fd, vd)                                                           # main.py:238-239
        embedding.set_layers(2)
        H_A2 = embedding(fd, vd)                                                           # main.py:240-241
        out = victim_model(fd, utils.normalize_adj_tensor(vd))
        test_accuracy = utils.accuracy(out[idx_test], labels.to(device)[idx_test]).item()
        print("Test set results:", "accuracy= {:.4f}".format(test_accuracy))
    if perturbed is not None:
        defense = {"perturbed": perturbed, "info": dict(dp_info, test_accuracy=test_accuracy)}
        if rank == 0:
            print(reports.defense_line(defense["info"]))
            if getattr(args, "save_defense", None):
                reports.save_defense(args.save_defense, ad, perturbed, defense["info"])
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
        if defense is not None:
            res["defense"] = dict(defense["info"])
        if rank == 0:
            print("feautre adj=", res["feature"])
            print("layer1 adj=", res["layer1"])
            print("layer2 adj=", res["layer2"])
            print("out adj=", res["out"])
            if want_ap:
                for k in ("feature", "layer1", "layer2", "out", "label"):
                    print(f"{k} ap=", res["ap"][k])
        return res
    if args.mode == "link_stealing":                                                       # no attack either
        want_ap = getattr(args, "ap", False)
        sets = {"attack": idx_attack, "train": idx_train, "all": None}
        res = {"link_stealing": link_stealing_metrics(ad, link_sources(Y_A, H_A2, features, device), sets, want_ap)}
        if defense is not None:
            res["defense"] = dict(defense["info"])
        if rank == 0:
            print("\n".join(link_stealing_lines(res["link_stealing"], want_ap)))
        return res
    if args.mode == reports.LINKTELLER_MODE:                                               # no attack either
        sets = {"attack": idx_attack, "train": idx_train, "all": None}
        with torch.no_grad():
            matrices, lt_info = link_teller_scores(victim_model, fd, vd, getattr(args, "lt_graph", reports.LINKTELLER_GRAPHS[0]),
                                                   getattr(args, "lt_delta", reports.LINKTELLER_DELTA))
        res = {"link_teller": {output: reports.link_teller_metrics(ad, S, sets) for output, S in matrices.items()},
               "link_teller_info": lt_info}
        if defense is not None:
            res["defense"] = dict(defense["info"])
        if rank == 0:
            print("\n".join(reports.link_teller_lines(res["link_teller"])))
            if getattr(args, "save_linkteller", None):
                reports.save_linkteller(args.save_linkteller, ad, matrices, res["link_teller"], lt_info)
        return res
    versus = getattr(args, "versus", None)
    other = None
    if versus is not None:  # refused before the attack runs, not after it
        influence = reports.versus_linkteller(versus, _exit)      # read ahead of versus_baseline, which keeps every other value
        baseline = reports.versus_baseline(versus, _exit) if influence is None else None
        if influence is not None:
            with torch.no_grad():
                other = link_teller_scores(victim_model, fd, vd, reports.LINKTELLER_GRAPHS[0], reports.LINKTELLER_DELTA,
                                           (influence,))[0][influence]
        elif baseline is not None:
            other = engine.pair_distance_scores(link_sources(Y_A, H_A2, features, device)[baseline[0]], baseline[1])
        else:
            other = feature_adj if versus == "features" else reports.load_versus(versus, adj.shape[0])
    by_class = getattr(args, "by_class", None)
    classes = None if by_class is None else reports.node_classes(by_class, labels, adj)    # refused before the attack runs too
    lr = 10 ** args.lr                                                                     # objective(): main.py:282-283
    weight_param = tuple(getattr(args, f"w{i}") for i in range(1, 11))
    model = PGDAttack(model=victim_model, embedding=embedding, H_A=H_A2, Y_A=Y_A, nnodes=adj.shape[0],
                      loss_type='CE', device=device)
    if getattr(args, "adj_changes_init", None) is not None:      # (tests: a seeded start; adj_changes is a public attribute, :77)
        model.adj_changes = args.adj_changes_init
    model.attack(args, None, lr, 0, args.weight_sup, weight_param, feature_adj, 0, 0, 0, idx_train, idx_val,
                 idx_test, victim_adj, features, init_adj, labels, idx_attack, num_edges, 0, epochs=args.epochs,
                 label_adj=label_adj)
    inference_adj = model.modified_adj                     # stays on the device: the three AUCs run there (main.py:247-250)
    ctx = reports.DefendedContext(real=ad.to(inference_adj.device), inference_adj=inference_adj,
                                  sets={"attack": idx_attack, "train": idx_train, "all": None}, n=adj.shape[0], rank=rank,
                                  other=other, versus=versus, args=args, classes=classes,
                                  components=None if not getattr(args, "ablate", None) else {
                                      "stack": model.components, "present": model.components_present, "used": model.component_mask,
                                      "decode_mode": topology_attack._decode_mode(args)},
                                  defense=defense)
    want_ap = getattr(args, "ap", False)
    res = base_metrics(ctx, want_ap)
    wanted = [r for r in reports.EVALUATE_REPORTS + reports.LATER_REPORTS if r.wanted(args)]
    for r in wanted:        # every rank computes (as the AUCs); a report's keys exist only with its flag
        res.update(r.compute(ctx))
    res["path"] = dict(model.history.get("path", {}), world=world)
    if rank != 0:           # every rank holds the same modified_adj; rank 0 reports
        return res
    print(f"current auc={res['auc_all']}")
    if want_ap:
        print(f"current ap={res['ap_all']}")
    for r in wanted:
        print("\n".join(r.console(res, ctx)))
        r.save(res, ctx)
    if getattr(args, "save_scores", None):
        reports.save_scores(args.save_scores, inference_adj)
    os.makedirs("./results/", exist_ok=True)
    with open(os.path.join("./results", args.log_name), "a") as f:                         # main.py:314-323
        f.write("\n".join(log_lines(res, ctx)) + "\n")
    return res


if __name__ == '__main__':
    run(build_parser().parse_args())
