"""main.py --mode evaluate's optional reports as one table (mc-gra_amd/reports.py: REPORTS), without a GPU: the log's parameter
line over every combination of the flags against the rule it followed before the table existed, written out here; and the
console and log text that the table's functions make of a recorded result, byte for byte against what the commit before the
table printed and logged for it (tests/golden/evaluate_all_flags.json, scripts/record_evaluate_report.py)."""
import argparse
import itertools
import os

import pytest

from tests import evaluate_report_text as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mc-gra_amd", "libmcgra_hip.so")

FLAGS = {"ap": ["--ap"], "topk": ["--topk", "3", "--save_edges", "e.npz"], "binarize": ["--binarize", "--save_graph", "g.npz"],
         "curves": ["--curves", "c.npz"], "per_node": ["--per_node", "p.npz"], "ci": ["--ci"],
         "ci_nodes": ["--ci_nodes", "--save_influence", "i.npz"], "structure": ["--structure", "split", "--save_structure", "s.npz"]}


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import mcgra_loader
    return mcgra_loader.load()


def shown_before_the_table(args):
    """The parameter line's namespace as _run built it by hand: five flags in a `hidden` set expression, the newer ones absent
    from the namespace unless given."""
    want_ap = getattr(args, "ap", False)
    want_topk = getattr(args, "topk", None) is not None
    want_split = bool(getattr(args, "binarize", False))
    want_curves = bool(getattr(args, "curves", None))
    want_per_node = bool(getattr(args, "per_node", None))
    hidden = (set() if want_ap else {"ap"}) | (set() if want_topk else {"topk", "save_edges"}) | \
        (set() if want_curves else {"curves"}) | (set() if want_per_node else {"per_node"}) | \
        (set() if want_split else {"binarize", "save_graph"})
    return argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in hidden})


def test_the_parameter_line_over_every_combination_of_the_flags(pkg):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    assert [r.flags[0] for r in R.REPORTS] == [k for k in FLAGS if k != "ap"]
    seen = set()
    for on in itertools.product((False, True), repeat=len(FLAGS)):
        names = [k for k, o in zip(FLAGS, on) if o]
        args = M.build_parser().parse_args([w for k in names for w in FLAGS[k]])
        text = str(R.shown_parameters(args))
        assert text == str(shown_before_the_table(args)), names
        assert [k for k in FLAGS if f" {k}=" in text] == names
        assert [r.flags[0] for r in R.REPORTS if r.wanted(args)] == [k for k in names if k != "ap"]
        seen.add(text)
    assert len(seen) == 256
    for argv, name in ((["--versus", "features", "--ci_nodes"], "versus"), (["--save_scores", "s.npy"], "save_scores")):
        args = M.build_parser().parse_args(argv)
        text = str(R.shown_parameters(args))
        assert text == str(shown_before_the_table(args)) and f" {name}={argv[1]!r}" in text, argv
        assert " ci=" not in text


def test_console_and_log_text_of_the_recorded_run_byte_for_byte(pkg):
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    fx = X.fixture()
    args = X.recorded_args(M, fx)
    assert all(r.wanted(args) for r in R.REPORTS) and args.ap and args.versus == "features"
    ctx = R.Context(real=None, inference_adj=None, sets={"attack": None, "train": None, "all": None}, n=1190, rank=0,
                    other=object(), versus=args.versus, args=args)            # the text asks only whether there is an `other`
    console, log = X.texts(M, R, fx["res"], ctx)
    out = fx["stdout"]
    assert out.count("current auc=") == 1 and console == out[out.index("current auc="):]
    assert log == fx["log"]
    lines = fx["log"].split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(X.log_kinds()) == 27
    assert all(line.startswith(kind) for line, kind in zip(lines, X.log_kinds()))
    assert sorted(fx["npz"]) == sorted(["edges.npz", "graph.npz", "c.npz", "p.npz", "influence.npz", "structure.npz"])
