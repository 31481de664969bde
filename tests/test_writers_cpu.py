"""The bytes the VCF header builders, the record writers and the counter logs write, pinned against
tests/golden/writers_parent.json: the text the functions of the commit before the writers were folded (one header
builder, dump_vcf, dump_counter_log) wrote for the fixed arguments below.  ``python -m tests.test_writers_cpu`` records
the file again from whatever the tree writes now; it was run once, on that commit.  The ``##fileDate=`` line is dropped
from every header.  No GPU here."""
import itertools
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "writers_parent.json")
CONTIGS = {"chr7": 1000, "chr10": 50, "chrX": 7}
REGIONS = {"region": ("chr7", None), "region_list": ("chr7", "loci.bed"), "whole": (None, None)}      # (region, region_list)


def _undated(text):
    return "\n".join(l for l in text.split("\n") if not l.startswith("##fileDate="))


def _variants(with_no_ref=True):
    for (rname, (region, region_list)), ref_file, cs in itertools.product(REGIONS.items(), ("ref.fa", None), (True, False)):
        if ref_file is None and not with_no_ref:
            continue
        yield "{}/{}/{}".format(rname, "ref" if ref_file else "noref", "cs" if cs else "nocs"), region, region_list, ref_file, cs


# (phase, non_human_sample, reference_sample, create_panel_of_normals): the five branches of the reference's builder that
# make a command line (the two non-human ones with and without --reference_sample), and one that makes none
CALL_FLAGS = [(True, True, False, False), (True, True, True, False), (True, False, False, False), (False, True, False, False),
              (False, True, True, False), (False, False, False, True), (False, False, False, False)]
CALL_FLAGS_NO_COMMAND = (False, False, True, False)


def _call_header(flags):
    from himut_amd import vcflib
    phase, non_human, ref_sample, make_pon = flags
    return vcflib.get_himut_vcf_header("in.bam", "germ.vcf", "phased.vcf", None, "loci.bed", CONTIGS, "com.vcf", "pon.vcf", 30, 60, 4000,
                                       20000, 0.99, 20, 93, 0.01, 0, 20, 52.5, 3, 1, 3, 4, 1 / (10 ** 6), 1 / (10 ** 3), 1 / (10 ** 4),
                                       phase, non_human, ref_sample, make_pon, "1.2.3", "o.vcf", "SMP")


def headers():
    from himut_amd import vcflib
    out = {}
    for name, region, region_list, ref_file, cs in _variants():
        out["germline/" + name] = vcflib.get_germline_vcf_header("in.bam", region, region_list, CONTIGS, 0, 20, 20, 2, 2, 80.25, 1e-3, 4,
                                                                 "1.2.3", "g.vcf", "SMP", ref_file=ref_file, cs_from_ref=cs)
        out["dbs/" + name] = vcflib.get_dbs_vcf_header("in.bam", region, region_list, CONTIGS, "com.vcf", None, 30, 60, 4000, 20000, 0.99,
                                                       20, 93, 0.01, 0, 20, 52.5, 3, 1, 1e-3, 4, "1.2.3", "d.vcf", "SMP",
                                                       ref_file=ref_file, cs_from_ref=cs)
    for name, region, region_list, ref_file, cs in _variants(with_no_ref=False):
        out["indels/" + name] = vcflib.get_indels_vcf_header("in.bam", region, region_list, CONTIGS, 0, 20, 2, 2, 80.25, 1e-4, 0.01, 50, 4,
                                                             "1.2.3", "i.vcf", "SMP", ref_file=ref_file, cs_from_ref=cs)
    for flags in CALL_FLAGS:
        out["call/" + "".join("ny"[f] for f in flags)] = _call_header(flags)
    return {k: _undated(v) for k, v in out.items()}


def _germline_recs():
    from tests import germline_model as M
    from tests.test_germline_cpu import LINES
    return np.array([r for r, _ in LINES], M.RECORD_DTYPE)


def _dbs_recs():
    from tests import dbs_model as M
    from tests.test_dbs_cpu import CASES
    return np.concatenate([M.run(b, regions, **kw)[0] for _name, b, regions, kw, _e in CASES])


def _indel_recs():
    """(records, the contig's string) of the hand cases that share the first one's reference."""
    from tests import indels_cases as C
    from tests import indels_model as M
    ref = C.CASES[0][3]
    return np.concatenate([M.run(c[1], c[2], c[3], **c[4])[0] for c in C.CASES if c[3] == ref]), ref


def data_files(tmp):
    """The three record files for two contigs, the second without records, under one-line headers."""
    from himut_amd import vcflib
    chroms = ["chr7", "chr10"]
    g, d, (i, ref) = _germline_recs(), _dbs_recs(), _indel_recs()
    assert len(g) and len(d) and len(i)
    path = os.path.join(str(tmp), "out.vcf")
    out = {}
    recs, seq = {"chr7": g, "chr10": g[:0]}, {"chr7": ref, "chr10": "ACGT"}
    vcflib.dump_vcf(path, "#germline header", chroms, lambda chrom: vcflib.germline_lines(chrom, recs[chrom]))
    out["germline"] = open(path).read()
    recs = {"chr7": d, "chr10": d[:0]}
    vcflib.dump_vcf(path, "#dbs header", chroms, lambda chrom: vcflib.dbs_lines(chrom, recs[chrom]))
    out["dbs"] = open(path).read()
    recs = {"chr7": i, "chr10": i[:0]}
    vcflib.dump_vcf(path, "#indels header", chroms, lambda chrom: vcflib.indel_lines(chrom, recs[chrom], seq[chrom]))
    out["indels"] = open(path).read()
    return out


def _counters(n, k):
    return [(7 * j + 3 * k) * 10 ** (j % 5) for j in range(n)]


def logs(tmp):
    """The four tab-separated logs and himut_sites.log, for two contigs and for one."""
    from himut_amd import sites, vcflib
    path = os.path.join(str(tmp), "out.log")

    def counter_log(rows):
        return lambda chroms, chrom2log, path: vcflib.dump_counter_log(rows, chroms, chrom2log, path), len(rows)
    writers = {"call": (vcflib.dump_call_log, len(vcflib.LOG_ROWS)),
               "germline": counter_log(vcflib.GERMLINE_LOG_ROWS),
               "dbs": counter_log(vcflib.DBS_LOG_ROWS),
               "indels": counter_log(vcflib.INDEL_LOG_ROWS),
               "sites": (sites.dump_sites_log, len(sites.LOG_ROWS))}
    out = {}
    for name, (dump, n) in writers.items():
        for chroms in (["chr7", "chr10"], ["chrX"]):
            dump(chroms, {c: _counters(n, k) for k, c in enumerate(chroms)}, path=path)
            out["{}/{}".format(name, len(chroms))] = open(path).read()
    return out


def everything(tmp):
    return {"headers": headers(), "data": data_files(tmp), "logs": logs(tmp)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_headers(golden):
    got = headers()
    assert sorted(got) == sorted(golden["headers"]) and len(got) == 12 + 12 + 6 + len(CALL_FLAGS)
    for name in sorted(got):
        assert got[name] == golden["headers"][name], name


def test_call_header_without_a_command_line_raises():
    with pytest.raises(UnboundLocalError):
        _call_header(CALL_FLAGS_NO_COMMAND)


def test_data_files(golden, tmp_path):
    assert data_files(tmp_path) == golden["data"]


def test_suffix_check(tmp_path):
    from himut_amd import vcflib
    g = _germline_recs()
    with pytest.raises(ValueError, match="VCF file must have .vcf suffix"):
        vcflib.dump_vcf(str(tmp_path / "out.txt"), "#h", ["chr7"], lambda chrom: vcflib.germline_lines(chrom, g))
    assert not os.path.exists(str(tmp_path / "out.txt"))


def test_logs(golden, tmp_path):
    got = logs(tmp_path)
    assert sorted(got) == sorted(golden["logs"]) and len(got) == 10
    for name in sorted(got):
        assert got[name] == golden["logs"][name], name


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp_dir:
        recorded = everything(tmp_dir)
    with open(GOLDEN, "w") as fh:
        json.dump(recorded, fh, indent=1, sort_keys=True)
        fh.write("\n")
