"""The haplotag run without a GPU: the plain-Python model of its contract against the rows written down by hand
(tests/haplotag_cases.py), the phased-VCF loader, the two TSV formatters and the command line."""
import numpy as np
import pytest

from tests import haplotag_cases as C
from tests import haplotag_model as M


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_model_gives_the_hand_computed_rows(case):
    rows, snp_rows, log = M.haplotag(case.batch, case.snps, **case.kw)
    C.check_expectations(case, rows, snp_rows)
    M.check_identities(case.snps, rows, snp_rows, log)
    assert list(rows["read"]) == list(range(case.batch.n))


def test_model_counters_by_hand():
    _rows, _snps, log = M.haplotag(C.BY_NAME["segments"].batch, C.BY_NAME["segments"].snps)
    # nine pile reads: six of haplotype 1, one of haplotype 0, two without a vote; 8 votes, 3 other, 3 del, 2 lowbq
    assert log == [9, 9, 1, 6, 0, 2, 0, 0, 0, 8, 3, 3, 2]
    _rows, _snps, log = M.haplotag(C.BY_NAME["sets"].batch, C.BY_NAME["sets"].snps)
    assert log[:9] == [7, 6, 3, 2, 0, 0, 0, 1, 6]              # six pile reads, each with votes in two sets or more


def test_model_rejects_broken_lists():
    c = C.BY_NAME["pile"]
    good = c.snps
    for bad in ([good[1], good[0]], [good[0], good[0]], [good[0][:2] + (good[0][1],) + good[0][3:]],
                [(good[0][0], "a", "C", 0, 0)], [good[0][:4] + (-1,)], [good[0][:3] + (2, 0)], [(0, "A", "C", 0, 0)]):
        with pytest.raises(ValueError):
            M.haplotag(c.batch, bad)
    for kw in (dict(min_snps=0), dict(min_agree_permille=500), dict(min_agree_permille=1001)):
        with pytest.raises(ValueError):
            M.haplotag(c.batch, good, **kw)


VCF = """##fileformat=VCFv4.2
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsyn
chrH\t100\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0|1:100
chrH\t200\t.\tG\tT\t.\tPASS\t.\tGT:PS\t1|0:200
chrH\t250\t.\tT\tC\t.\tPASS\t.\tGT:PS\t0|1:250
chrH\t300\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0|1:200
chrH\t300\t.\tA\tG\t.\tPASS\t.\tGT:PS\t1|0:100
chrH\t400\t.\tC\tA\t.\tPASS\t.\tGT:PS\t1|0:200
chrH\t400\t.\tC\tG\t.\tPASS\t.\tGT:PS\t0|1:200
chrH\t450\t.\tC\tCA\t.\tPASS\t.\tGT:PS\t1|0:200
chrH\t460\t.\tC\tT\t.\tPASS\t.\tGT\t0/1
chrH\t500\t.\tT\tG\t.\tPASS\t.\tGT:PS\t0|1:100
chrH\t500\t.\tT\tA\t.\tPASS\t.\tGT:PS\t1|0:250
chrOther\t7\t.\tT\tG\t.\tPASS\t.\tGT:PS\t0|1:7
chrOther\t9\t.\tT\tG\t.\tPASS\t.\tGT:PS\t1|0:7
chrUnphased\t9\t.\tT\tG\t.\tPASS\t.\tGT\t0/1
"""


@pytest.mark.parametrize("suffix", [".vcf", ".vcf.bgz"])
def test_load_phased(tmp_path, capsys, suffix):
    """A position-sorted file with interleaved sets.  Position 300 is listed by set 200 and then by set 100, which appears
    earlier in the file; 400 twice by set 200; 500 by set 100 and then by set 250: each time the record that stands first
    in the file stays."""
    import gzip
    from himut_amd import haplotag
    path = str(tmp_path / ("phased" + suffix))
    with (gzip.open(path, "wt") if suffix.endswith(".bgz") else open(path, "w")) as o:
        o.write(VCF)
    got, absent = haplotag.load_phased(path, ["chrH", "chrEmpty"], {"chrH": 6000, "chrEmpty": 100})
    assert sorted(got) == ["chrH"]
    assert absent == {"chrOther": 2}                             # in the file, not in the BAM: for the driver to report
    s = got["chrH"]
    # sets by first position: 100 -> 0, 200 -> 1, 250 -> 2; the insertion and the unphased record are no hetSNPs of the run
    assert s.names == ["100", "200", "250"] and s.duplicates == 3
    assert s.tuples() == [(100, "A", "C", 0, 0), (200, "G", "T", 1, 1), (250, "T", "C", 0, 2), (300, "A", "C", 0, 1),
                          (400, "C", "A", 1, 1), (500, "T", "G", 0, 0)]
    assert s.pos1.dtype == np.int32 and s.set.dtype == np.int32 and s.bit.dtype == np.uint8 and s.ref.dtype == np.uint8
    M.check_snps(s.tuples(), len(s.names))
    out = capsys.readouterr().out
    assert "3 positions" in out and "stands first in the file" in out


def test_phased_record_order(tmp_path):
    from himut_amd import vcflib
    path = tmp_path / "phased.vcf"
    path.write_text(VCF)
    order = vcflib.phased_record_order(str(path))
    assert sorted(order) == ["chrH", "chrOther"]
    assert order["chrH"][(300, "200")] == 4 and order["chrH"][(300, "100")] == 5
    assert order["chrH"][(400, "200")] == 6 and order["chrH"][(450, "200")] == 8 and order["chrOther"] == {(7, "7"): 12, (9, "7"): 13}


def test_formatters_by_hand_and_against_the_model():
    from himut_amd import _ffi, haplotag
    assert _ffi.HAPLOTAG_ROW_DTYPE == M.ROW_DTYPE and _ffi.HAPLOTAG_SNP_DTYPE == M.SNP_DTYPE
    assert _ffi.HAPLOTAG_STATUS_NAMES == M.STATUS_NAMES and _ffi.HAPLOTAG_LOG_NAMES == M.LOG_NAMES
    assert haplotag.READ_COLUMNS == M.READ_COLUMNS and haplotag.SNP_COLUMNS == M.SNP_COLUMNS
    c = C.BY_NAME["pile"]
    rows, snp_rows, log = M.haplotag(c.batch, c.snps, **c.kw)
    b = c.batch
    names = ["4001"]
    s = haplotag.PhasedSnps(*[[t[k] if k not in (1, 2) else ord(t[k]) for t in c.snps] for k in range(5)], names)
    info = (b.tstart, b.tend, b.flag, b.mapq)
    lines = haplotag.format_reads("chrH", rows, info, names, b.query_name)
    assert lines == M.read_lines("chrH", b, rows, names)
    assert lines[0] == "chrH\tccs/0\t3991\t4190\t+\t20\t4001\t1\tAssigned\t4\t0\t0\t0\t0\t1"
    assert lines[1] == "chrH\tccs/1\t3992\t4191\t+\t60\t.\t.\tNotInPile\t0\t0\t0\t0\t0\t0"
    assert lines[4] == "chrH\tccs/4\t3995\t4194\t-\t20\t4001\t.\tConflict\t3\t1\t0\t0\t0\t1"
    slines = haplotag.format_snps("chrH", s, snp_rows)
    assert slines == M.snp_lines("chrH", c.snps, snp_rows, names)
    ref, alt = c.snps[1][1], c.snps[1][2]
    assert slines[1] == "chrH\t4051\t{}\t{}\t1|0\t4001\t3\t1\t2\t0\t0\t0\t2\t0".format(ref, alt)
    assert haplotag.log_of(log, snp_rows) == log + [4, 4, 0]
    assert len(haplotag.LOG_ROWS) == 16


def _parse(*extra):
    from himut_amd.parse_args import parse_args
    return parse_args("test", ["haplotag", "-i", "in.bam", "--phased_vcf", "p.vcf", "-o", "out.tsv"] + list(extra))[1]


def test_command_line_defaults_and_the_permille():
    from himut_amd.parse_args import build_parser
    o = _parse()
    germline = build_parser("test").parse_args(["germline", "-i", "x", "-o", "y"])
    phase = build_parser("test").parse_args(["phase", "-i", "x", "--vcf", "v", "-o", "y"])
    assert o.min_mapq == germline.min_mapq == 0 and o.min_bq == phase.min_bq == 20
    assert o.min_snps == 1 and o.min_agree == 0.8 and o.min_agree_permille == 800
    assert o.snps is None and o.region is None and o.region_list is None and o.ref is None and not o.cs_from_ref
    assert o.devices == "0" and o.threads == 1
    assert _parse("--min_agree", "0.501").min_agree_permille == 501
    assert _parse("--min_agree", "1.0").min_agree_permille == 1000
    assert _parse("--min_agree", "0.8004").min_agree_permille == 800
    o = _parse("--snps", "s.tsv", "--min_snps", "3", "--min_mapq", "20", "--min_bq", "30", "--region", "chr1", "--devices", "0,1")
    assert (o.snps, o.min_snps, o.min_mapq, o.min_bq, o.region, o.devices) == ("s.tsv", 3, 20, 30, "chr1", "0,1")
    for bad in (["--min_agree", "0.5"], ["--min_agree", "1.01"], ["--min_snps", "0"], ["--cs_from_ref"]):
        with pytest.raises(SystemExit):
            _parse(*bad)


def test_agree_permille():
    from himut_amd.haplotag import agree_permille
    assert agree_permille(0.8) == 800 and agree_permille(0.501) == 501 and agree_permille(1.0) == 1000
    for bad in (0.5, 0.0, 1.001, -1):
        with pytest.raises(ValueError):
            agree_permille(bad)
