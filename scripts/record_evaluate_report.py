"""Records what `main.py --mode evaluate` prints, logs and returns with every optional report on, as the fixture
tests/golden/evaluate_all_flags.json that tests/test_evaluate_reports_cpu.py and tests/test_gpu_evaluate_reports.py read.

It uses main.build_parser and main.run only, so the same file runs on the commit whose text is to be pinned and on any later
one.  The run is the usair line of the per-flag tests (n = 1190, 3 epochs) in a temporary working directory that holds a link
`dataset` to tests/golden/dataset, with relative file names throughout: nothing in the fixture names a place.  Needs the GPU.

    python scripts/record_evaluate_report.py [OUT]       # OUT defaults to tests/golden/evaluate_all_flags.json

The fixture holds `argv`, `stdout` (everything the run printed), `log` (the text of results/<log_name>), `res` (the returned
dict without its tensor and array leaves; floats as Python's json writes them, NaN and inf included, which load back to the
same doubles) and `npz` (file name -> the sorted names of its arrays)."""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcgra_loader  # noqa: E402

mcgra_loader.load()
from mc_gra_amd import main as M  # noqa: E402

ARGV = ["--dataset", "usair", "--epochs", "3", "--measure", "MSELoss", "--w2", "100", "--w6", "100", "--w7", "10000",
        "--w9", "100", "--weight_sup", "0", "--lr", "-3", "--useH_A", "--log_name", "all_flags.txt",
        "--ap", "--topk", "0", "--save_edges", "edges.npz", "--binarize", "--save_graph", "graph.npz", "--curves", "c.npz",
        "--per_node", "p.npz", "--ci", "--ci_nodes", "--versus", "features", "--save_scores", "scores.npy",
        "--save_influence", "influence.npz", "--structure", "split", "--save_structure", "structure.npz"]
NPZ = ("edges.npz", "graph.npz", "c.npz", "p.npz", "influence.npz", "structure.npz")


def plain(v):
    """v without its tensor and array leaves: dicts and lists walked, numbers, strings, bools and None kept."""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items() if not isinstance(x, (torch.Tensor, np.ndarray))}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v if not isinstance(x, (torch.Tensor, np.ndarray))]
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    raise TypeError(f"a leaf of type {type(v).__name__}")


def record():
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.symlink(os.path.join(ROOT, "tests", "golden", "dataset"), os.path.join(tmp, "dataset"))
        os.chdir(tmp)
        try:
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                res = M.run(M.build_parser().parse_args(ARGV))
            with open(os.path.join("results", "all_flags.txt")) as f:
                log = f.read()
            npz = {name: sorted(np.load(name).files) for name in NPZ}
            assert np.load("scores.npy").shape == (1190, 1190)
        finally:
            os.chdir(here)
    return {"argv": ARGV, "stdout": out.getvalue(), "log": log, "res": plain(res), "npz": npz}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "evaluate_all_flags.json")
    fixture = record()
    text = json.dumps(fixture)          # one line: the per-node integer lists of --ci_nodes make an indented file too large
    assert json.dumps(json.loads(text)) == text, "the fixture does not load back to itself"     # by text: NaN != NaN
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(f"wrote {path}: {len(text)} bytes, {len(fixture['stdout'].splitlines())} lines of stdout, "
          f"{len(fixture['log'].splitlines())} lines of log, res keys {sorted(fixture['res'])}")
