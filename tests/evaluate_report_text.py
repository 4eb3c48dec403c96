"""What tests/test_evaluate_reports_cpu.py and tests/test_gpu_evaluate_reports.py share: the fixture
tests/golden/evaluate_all_flags.json (recorded by scripts/record_evaluate_report.py: main.py --mode evaluate on usair with every
optional report on), the text that main.py and reports.py make of a result dict, and the kinds of line a log with every report
on holds, in order."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TITLES = ("attack graph", "train graph", "Whole Graph")


def fixture():
    """The recorded run.  json writes a float as its repr (NaN and inf by name), which reads back as the same double, so
    writing what was read gives the file back: asserted here."""
    with open(os.path.join(GOLDEN, "evaluate_all_flags.json")) as f:
        text = f.read()
    fx = json.loads(text)
    assert json.dumps(fx) + "\n" == text
    return fx


def recorded_args(M, fx):
    """The namespace of the recorded command line as _run sees it: run() sets _own_group before it calls _run."""
    args = M.build_parser().parse_args(fx["argv"])
    args._own_group = False
    return args


def texts(M, R, res, ctx):
    """(console, log): what rank 0 prints from `current auc=` on and what it appends to the log, from main.py's and
    reports.py's own functions."""
    console = [f"current auc={res['auc_all']}"]
    if getattr(ctx.args, "ap", False):
        console.append(f"current ap={res['ap_all']}")
    for r in R.REPORTS:
        if r.wanted(ctx.args):
            console += r.console(res, ctx)
    return "\n".join(console) + "\n", "\n".join(M.log_lines(res, ctx)) + "\n"


def log_kinds(versus="features"):
    """How each line of a log with every report on starts, in order: parameter, AUC, AP, topk, split x 3, curves,
    per_node x 3, ci / versus x 6, ci_nodes / versus x 6, structure x 3, density."""
    kinds = ["current parameter: Namespace(seed=", "In attack graph: AUC=", "In attack graph: AP=", "In attack graph: k="]
    kinds += [f"In {t}: split edges=" for t in TITLES] + ["In attack graph: ROC points="]
    kinds += [f"In {t}: scored nodes=" for t in TITLES]
    for t in TITLES:
        kinds += [f"In {t}: pairs=", f"In {t}: versus {versus}: AUC="]
    for t in TITLES:
        kinds += [f"In {t}: nodes=", f"In {t}: versus {versus} (nodes): AUC="]
    return kinds + [f"In {t}: structure at " for t in TITLES] + ["current density: "]
