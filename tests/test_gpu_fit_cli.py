"""`himut fit` as a child process on the hand-written files of tests/fit_cases.py: the files it writes are compared byte for
byte with what the writers of himut_amd/fit.py make of the plain model's exposures (tests/fit_model.py)."""
import os
import subprocess
import sys

import pytest

from himut_amd import fit
from tests import fit_cases as C, fit_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "himut_amd", "fit"] + args, cwd=str(cwd), env=env, capture_output=True,
                          text=True, timeout=300)


def _files(tmp_path, layout):
    (tmp_path / "spectrum.tsv").write_text(C.SPECTRA[layout])
    (tmp_path / "sigs.tsv").write_text(C.SIGNATURES)
    (tmp_path / "opp.tsv").write_text(C.OPPORTUNITIES)


def _want(tmp_path, select, opp, n_boot, seed, iters, min_fraction=0.05):
    """{file: text} from the model through the command's own loaders and writers."""
    prep = fit.load_inputs(str(tmp_path / "spectrum.tsv"), str(tmp_path / "sigs.tsv"), select,
                           str(tmp_path / opp) if opp not in (None, "normcounts") else opp)
    expo, _ = M.fit(prep.sig, prep.counts, n_boot=n_boot, seed=seed, iters=iters)
    res = fit.summarise(prep, expo, min_fraction)
    want = tmp_path / "want"
    want.mkdir()
    fit.write_exposures(prep, res, str(want / "exposures.tsv"))
    fit.write_recon(prep, res, str(want / "recon.tsv"))
    fit.write_boot(prep, expo, str(want / "boot.tsv"))
    return prep, {k: (want / k).read_text() for k in ("exposures.tsv", "recon.tsv", "boot.tsv")}


def test_select_recon_boot_and_log(tmp_path):
    _files(tmp_path, "simple")
    prep, want = _want(tmp_path, "SigA,SigB", None, 6, 3, 40, 0.3)
    r = _cli(["-i", "spectrum.tsv", "--signatures", "sigs.tsv", "-o", "exposures.tsv", "--select", "SigA,SigB", "--bootstrap", "6",
              "--seed", "3", "--iters", "40", "--min_fraction", "0.3", "--recon", "recon.tsv", "--boot", "boot.tsv"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, text in want.items():
        assert (tmp_path / k).read_text() == text, k
    head = want["exposures.tsv"].split("\n")
    assert head[:3] == ["# N\t100", "# fitted_N\t95", "# unexplained\t5"]
    assert head[5] == "signature\texposure\tfraction\texposure_genome\tlo\tmedian\thi\tpresence" and len(head) == 9
    assert (tmp_path / "himut_fit.log").read_text() == C.log_text(5, 1, 2, 95, 7, 40)


def test_opp_file(tmp_path):
    _files(tmp_path, "sbs96")
    prep, want = _want(tmp_path, None, "opp.tsv", 3, 1, 25)
    r = _cli(["-i", "spectrum.tsv", "--signatures", "sigs.tsv", "-o", "exposures.tsv", "--opp", "opp.tsv", "--bootstrap", "3",
              "--iters", "25"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "exposures.tsv").read_text() == want["exposures.tsv"]
    rows = [ln.split("\t") for ln in want["exposures.tsv"].split("\n")[6:9]]
    assert [x[0] for x in rows] == ["SigA", "SigB", "SigC"] and any(x[1] != x[3] for x in rows)      # the genome's differ
    assert not (tmp_path / "recon.tsv").exists() and not (tmp_path / "boot.tsv").exists()
    assert (tmp_path / "himut_fit.log").read_text() == C.log_text(6, 0, 3, 100, 4, 25)


def test_opp_normcounts(tmp_path):
    _files(tmp_path, "normcounts")
    prep, want = _want(tmp_path, "SigB,SigA", "normcounts", 2, 1, 30)
    assert prep.names == ["SigB", "SigA"] and prep.aside == [("T[T>G]T", 5)]
    r = _cli(["-i", "spectrum.tsv", "--signatures", "sigs.tsv", "-o", "exposures.tsv", "--select", "SigB,SigA", "--opp",
              "normcounts", "--bootstrap", "2", "--iters", "30", "--recon", "recon.tsv"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "exposures.tsv").read_text() == want["exposures.tsv"]
    assert (tmp_path / "recon.tsv").read_text() == want["recon.tsv"]
    # on a table without the ratios the word is an error
    (tmp_path / "spectrum.tsv").write_text(C.SPECTRUM_SBS96)
    r = _cli(["-i", "spectrum.tsv", "--signatures", "sigs.tsv", "-o", "e2.tsv", "--opp", "normcounts"], tmp_path)
    assert r.returncode == 1 and "is not a normcounts table" in r.stderr and not (tmp_path / "e2.tsv").exists()


def test_point_fit_alone(tmp_path):
    _files(tmp_path, "sbs1536")
    prep, want = _want(tmp_path, None, None, 0, 1, 50)
    r = _cli(["-i", "spectrum.tsv", "--signatures", "sigs.tsv", "-o", "exposures.tsv", "--bootstrap", "0", "--iters", "50",
              "--boot", "boot.tsv"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "exposures.tsv").read_text() == want["exposures.tsv"]
    assert (tmp_path / "boot.tsv").read_text() == want["boot.tsv"]
    assert want["exposures.tsv"].split("\n")[5] == "signature\texposure\tfraction\texposure_genome"
    assert (tmp_path / "himut_fit.log").read_text() == C.log_text(6, 0, 3, 100, 1, 50)


def test_failure_exits(tmp_path):
    _files(tmp_path, "simple")
    for name, text, word in (("missing.tsv", C.SIG_MISSING_ROW, "label A[C>T]G of the spectrum is not in the signature matrix"),
                             ("extra.tsv", C.SIG_EXTRA_ROW, "label G[T>A]G of the signature matrix is not in the spectrum"),
                             ("zero.tsv", C.SIG_ZERO_COLUMN, "signature SigZ sums to 0")):
        (tmp_path / name).write_text(text)
        r = _cli(["-i", "spectrum.tsv", "--signatures", name, "-o", "out.tsv", "--bootstrap", "0"], tmp_path)
        assert r.returncode == 1 and word in r.stderr, (name, r.stderr[-500:])
        assert not (tmp_path / "out.tsv").exists()
    r = _cli(["-i", "spectrum.tsv", "--signatures", "sigs.tsv", "-o", "out.tsv", "--bootstrap", "100001"], tmp_path)
    assert r.returncode == 1 and "--bootstrap must lie in 0..100000" in r.stderr
