"""main.py --mode evaluate with every optional report on at once, on the device: the per-flag tests run each flag alone, so this
run pins the order of the console and log lines across reports, the keys of the result and the arrays of every file it
writes, against the run recorded before the reports became one table (tests/golden/evaluate_all_flags.json).  Run with -m gpu.
No float is compared with the recording: the attack is not asserted to be bit-repeatable across processes."""
import os

import numpy as np
import pytest

from tests import evaluate_report_text as X
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import mcgra_loader
    p = mcgra_loader.load()
    p._lib.require_device()
    return p


def test_main_evaluate_with_every_report_on(pkg, tmp_path, monkeypatch, capsys):
    """The recorded command line (usair, n = 1190, 3 epochs of its README line) run once, in a working directory that holds a
    link `dataset` to the committed files as the recording's did."""
    from mc_gra_amd import main as M
    from mc_gra_amd import reports as R
    fx = X.fixture()
    monkeypatch.chdir(tmp_path)
    os.symlink(os.path.join(H.GOLDEN, "dataset"), tmp_path / "dataset")
    args = M.build_parser().parse_args(fx["argv"])
    res = M.run(args)
    out = capsys.readouterr().out
    assert sorted(res) == sorted(fx["res"])
    ctx = R.Context(real=None, inference_adj=None, sets={"attack": None, "train": None, "all": None}, n=1190, rank=0,
                    other=object(), versus=args.versus, args=args)            # the text asks only whether there is an `other`
    console, log = X.texts(M, R, res, ctx)
    assert out.count("current auc=") == 1 and out[out.index("current auc="):] == console
    logged = open(tmp_path / "results" / "all_flags.txt").read()
    assert logged == log
    lines = logged.split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(X.log_kinds())
    for line, kind in zip(lines, X.log_kinds()):
        assert line.startswith(kind), (line[:60], kind)
    assert lines[0] == fx["log"].split("\n")[0]                              # the parameter line holds nothing the attack computed
    assert [l.split("=")[0] for l in console.split("\n")] == [l.split("=")[0] for l in fx["stdout"][fx["stdout"].index("current auc="):].split("\n")]
    for name, files in fx["npz"].items():
        assert sorted(np.load(tmp_path / name).files) == files, name
    assert np.load(tmp_path / "scores.npy").shape == (1190, 1190)
