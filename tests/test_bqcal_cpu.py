"""The bqcal run's contract on the CPU: the plain-Python model (tests/bqcal_model.py) against the counts the reference's
own worker gave (tests/golden/bqcal_*.json, made by tests/golden/make_golden_bqcal.py), the command line, the table."""
import math
import os

import numpy as np
import pytest

from tests import bqcal_model as M
from tests import util

GOLDENS = ["bqcal_basic", "bqcal_dense", "bqcal_softmask", "bqcal_insins", "bqcal_dense_md", "bqcal_basic_regions"]


def load_golden(case):
    """(golden, read batch, contig string) of a bqcal golden: the reads and the string are its norm fixture's."""
    from himut_amd.readbatch import ReadBatch
    g = util.load_json(case)
    with np.load(os.path.join(util.GOLDEN, g["fixture"] + ".npz")) as z:
        return g, ReadBatch.from_npz_dict(z), bytes(z["refseq"]).decode("ascii")


_MODEL = {}


def golden_model(case):
    """The model's (match, mismatch, log) of a golden, computed once per process and left unchanged."""
    if case not in _MODEL:
        g, b, seq = load_golden(case)
        _MODEL[case] = M.run(b, seq, g["regions"], g["germline_snv_prior"], min_gq=g["min_gq"], md_threshold=g["md_threshold"])
    return _MODEL[case]


@pytest.mark.parametrize("case", GOLDENS)
def test_model_reproduces_the_reference(case):
    g = util.load_json(case)
    match, mismatch, log = golden_model(case)
    assert [int(x) for x in match[1:94]] == g["match"] and [int(x) for x in mismatch[1:94]] == g["mismatch"]
    assert match[0] == mismatch[0] == 0 and match[94:].sum() == mismatch[94:].sum() == 0
    assert sum(g["mismatch"]) > 0 and sum(g["match"]) > 0
    assert log[0] == sum(e - s for s, e in g["regions"]) == sum(log[1:9]) and log[11] == 0
    assert log[9] + log[10] <= sum(log[5:9])
    if case == "bqcal_dense_md":
        assert log[2] > 0
    if case == "bqcal_softmask":
        assert log[1] > 0


def test_cli_parses_bqcal_and_reaches_the_driver(monkeypatch):
    from himut_amd import __main__ as cli
    from himut_amd import bqcal
    from himut_amd.parse_args import parse_args
    _parser, o = parse_args("x", ["bqcal", "-i", "in.bam", "--ref", "g.fa", "-o", "out.tsv"])
    assert (o.sub, o.bam, o.ref, o.output) == ("bqcal", "in.bam", "g.fa", "out.tsv")
    assert (o.min_mapq, o.min_gq, o.germline_snv_prior, o.threads, o.devices, o.cs_from_ref) == (0, 20, 1 / (10 ** 3), 1, "0", False)
    assert o.region is None and o.region_list is None
    with pytest.raises(SystemExit):
        parse_args("x", ["bqcal", "-i", "in.bam", "-o", "out.tsv"])             # --ref is required
    seen = []
    monkeypatch.setattr(bqcal, "dump_empirical_bq", lambda *a, **kw: seen.append((a, kw)))
    cli.main(["bqcal", "-i", "in.bam", "--ref", "g.fa", "--region", "chr2", "--min_mapq", "20", "--min_gq", "30",
              "--germline_snv_prior", "0.01", "-t", "4", "--devices", "0,1", "-o", "out.tsv"])
    assert seen == [(("in.bam", "g.fa", "chr2", None, 20, 30, 0.01, 4, "out.tsv"), dict(devices=[0, 1], cs_from_ref=False))]


def test_table_writer():
    from himut_amd import bqcal
    match, mismatch = np.zeros(256, np.int64), np.zeros(256, np.int64)
    match[93], mismatch[93] = 1167207, 281
    match[40] = 17                       # no mismatch: NA
    mismatch[7] = 3                      # no match: NA
    match[200], mismatch[200] = 5, 2     # above 93: a row of its own
    mismatch[255] = 1
    lines = bqcal.table_lines(match, mismatch)
    assert lines[0] == "bq\tmismatch\tmatch\tpq\n" and len(lines) == 1 + 93 + 2
    assert [int(line.split("\t")[0]) for line in lines[1:]] == list(range(1, 94)) + [200, 255]
    assert lines[93] == "93\t281\t1167207\t{}\n".format(-10 * math.log10(281 / float(1167207)))
    assert lines[40] == "40\t0\t17\tNA\n" and lines[7] == "7\t3\t0\tNA\n" and lines[1] == "1\t0\t0\tNA\n"
    assert lines[94] == "200\t2\t5\t{}\n".format(-10 * math.log10(2 / float(5))) and lines[95] == "255\t1\t0\tNA\n"
    assert "".join(lines) == M.table_text(match, mismatch)
    # nothing above 93: the script's 94 lines
    match[200] = mismatch[200] = mismatch[255] = 0
    assert len(bqcal.table_lines(match, mismatch)) == 94
