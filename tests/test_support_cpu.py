"""`himut support` without a GPU: the contract's Python model (tests/support_model.py) against what the reference
itself printed for the twelve golden fixtures, and the host parts of the command -- parser, site loader, TSV text."""
import gzip

import numpy as np
import pytest

from himut_amd import support
from himut_amd._ffi import SUPPORT_ROW_DTYPE
from himut_amd.parse_args import build_parser
from tests import support_model as M
from tests import util

CASES = util.WORKER_CASES + util.PHASE_CASES
ALT_COUNT = 8            # column of a fixture record: [tpos, ref, alt, status, gq, bq, depth, ref_count, alt_count, vaf, ps]


def fixture_sites(exp):
    """The fixture's bi-allelic records as a sorted site list, and per record its site (None: multi-allelic)."""
    recs = exp["records"]
    bi = [k for k, r in enumerate(recs) if len(r[2]) == 1]
    order = sorted(bi, key=lambda k: recs[k][0])
    site_of = {k: n for n, k in enumerate(order)}
    return [(recs[k][0], recs[k][1], recs[k][2]) for k in order], [site_of.get(k) for k in range(len(recs))]


def check_fixture(exp, rows, counts, site_of):
    """Checks (a) and (b) of one fixture; returns (records, records left out of (a))."""
    p = util.params_of(exp)
    starts = {c[0] for c in util.chunks_of(exp)}
    first = np.searchsorted(rows["site"], np.arange(counts.shape[0] + 1))
    left_out = 0
    for r, n in zip(exp["records"], site_of):
        if n is None:                                   # multi-allelic
            left_out += 1
            continue
        if r[0] in starts:                              # the reference's pile is short of the reads that end there
            left_out += 1
        else:
            assert counts[n, 1] == r[ALT_COUNT], (r, counts[n])
        assert any(M.could_propose(x, p) for x in rows[first[n]:first[n + 1]]), r
    return len(exp["records"]), left_out


def test_model_alt_counts_and_proposing_reads_match_the_reference():
    total = left_out = 0
    for case in CASES:
        batch, exp = util.load_case(case)
        sites, site_of = fixture_sites(exp)
        rows, counts = M.support(batch, sites, 0, util.params_of(exp)["mismatch_window_size"])
        n, out = check_fixture(exp, rows, counts, site_of)
        total += n
        left_out += out
    assert total == 5687
    assert left_out <= 6


def test_parser_flags_and_defaults():
    o = build_parser("x").parse_args(["support", "-i", "a.bam", "--sbs", "s.vcf", "-o", "t.tsv"])
    assert (o.sub, o.bam, o.sbs, o.output) == ("support", "a.bam", "s.vcf", "t.tsv")
    assert (o.min_mapq, o.mismatch_window_size, o.all_filters, o.cs_from_ref) == (0, 20, False, False)
    assert (o.region, o.region_list, o.ref, o.devices, o.threads) == (None, None, None, "0", 1)
    o = build_parser("x").parse_args(["support", "-i", "a.bam", "--sbs", "s.vcf.bgz", "-o", "t.tsv", "--all_filters",
                                      "--min_mapq", "60", "--mismatch_window_size", "5", "--region", "c", "--devices", "0,1"])
    assert (o.all_filters, o.min_mapq, o.mismatch_window_size, o.region, o.devices) == (True, 60, 5, "c", "0,1")


VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts",
    "c2\t30\t.\tA\tG\t.\tPASS\t.\tGT\t./.",
    "c1\t20\t.\tC\tT\t.\tPASS\t.\tGT\t./.",
    "c1\t10\t.\tA\tC,G\t.\tHetAltSite\t.\tGT\t./.",
    "c1\t20\t.\tC\tT\t.\tPASS\t.\tGT\t./.",
    "c1\t12\t.\tAC\tA\t.\tPASS\t.\tGT\t./.",
    "c1\t13\t.\tN\tA\t.\tPASS\t.\tGT\t./.",
    "c1\t14\t.\tA\tAT,N\t.\tLowBQ\t.\tGT\t./.",
    "c1\t15\t.\tT\tG\t.\tLowBQ\t.\tGT\t./.",
    "c1\t5\t.\tG\tT\t.\tPASS\t.\tGT\t./.",
]) + "\n"


def test_site_loader(tmp_path):
    plain = tmp_path / "s.vcf"
    plain.write_text(VCF)
    sites, skipped = support.load_sites(str(plain))
    assert sites == {"c1": [(5, "G", "T", "PASS"), (20, "C", "T", "PASS")], "c2": [(30, "A", "G", "PASS")]}
    assert skipped == 2                                                    # the indel and the N reference among the PASS lines
    sites, skipped = support.load_sites(str(plain), all_filters=True)
    assert sites["c1"] == [(5, "G", "T", "PASS"), (10, "A", "C", "HetAltSite"), (10, "A", "G", "HetAltSite"),
                           (15, "T", "G", "LowBQ"), (20, "C", "T", "PASS")]
    assert skipped == 3
    packed = tmp_path / "s.vcf.bgz"
    with gzip.open(str(packed), "wt") as fh:
        fh.write(VCF)
    assert support.load_sites(str(packed), all_filters=True) == (sites, skipped)
    with pytest.raises(ValueError):
        support.load_sites(str(tmp_path / "s.txt"))


def test_tsv_text_of_a_hand_made_row_array():
    sites = [(5, "G", "T", "PASS"), (9, "A", "C", "LowBQ"), (9, "A", "G", "LowBQ")]
    rows = np.zeros(3, SUPPORT_ROW_DTYPE)
    rows["site"] = [0, 0, 2]
    rows["read"] = [1, 4, 4]
    rows["qid"] = [1, 2, 2]
    rows["flag"] = [0, 16, 0x810]
    rows["mapq"] = [60, 0, 7]
    rows["qlen"] = [3, 7, 7]
    rows["qpos"] = [0, 6, 2]
    rows["bq"] = [93, 1, 40]
    rows["bq_sum"] = [200, 100, 100]
    rows["n_sub"] = [1, 2, 2]
    rows["n_indel"] = [0, 3, 3]
    rows["window_mismatches"] = [0, 4, 1]
    counts = np.array([[5, 2], [4, 0], [4, 1]], np.int32)
    got = support.format_rows("c1", sites, rows, counts, lambda i, qid: "r{}/{}".format(i, qid))
    assert got == ["c1\t5\tG\tT\tPASS\t2\t5\tr1/1\t+\t60\t3\t0\t93\t66.67\t1\t0\t0",
                   "c1\t5\tG\tT\tPASS\t2\t5\tr4/2\t-\t0\t7\t6\t1\t14.29\t2\t3\t4",
                   "c1\t9\tA\tC\tLowBQ\t0\t4" + "\t." * 10,
                   "c1\t9\tA\tG\tLowBQ\t1\t4\tr4/2\t-\t7\t7\t2\t40\t14.29\t2\t3\t1"]
    assert len(support.COLUMNS) == 17 and all(len(line.split("\t")) == 17 for line in got)
    assert support.format_rows("c1", [], np.zeros(0, SUPPORT_ROW_DTYPE), np.zeros((0, 2), np.int32), None) == []


def test_model_window_follows_the_three_branches():
    # (qpos, qlen, w) -> window around position 1000
    assert M.mismatch_range(1000, 50, 100, 20) == (980, 1020)
    assert M.mismatch_range(1000, 5, 100, 20) == (995, 1035)             # qpos < w
    assert M.mismatch_range(1000, 95, 100, 20) == (965, 1005)            # qpos + w > qlen
    assert M.mismatch_range(1000, 5, 30, 20) == (995, 1035)              # qlen < 2 w: the first branch wins
    assert M.mismatch_range(1000, 80, 100, 20) == (980, 1020)            # qpos + w == qlen: symmetric
    assert M.mismatch_range(1000, 7, 9, 0) == (1000, 1000)


def test_driver_refuses_a_distributed_launch(monkeypatch, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError) as e:
        support.dump_support("in.bam", "s.vcf", None, None, 0, 20, False, 1, str(tmp_path / "t.tsv"))
    assert "single process" in str(e.value)
