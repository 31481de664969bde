"""The germline run's contract on the CPU: the plain-Python model (tests/germline_model.py) against the reference-made
genotype fixtures, the VCF lines against literals, the lines through the package's own loaders, the command line."""
import numpy as np
import pytest

from tests import germline_model as M
from tests import gt_piles as G
from tests import util


def _check_vector(v, col, recs, report_homref):
    """The record of the column of vector v (or none): the fixture's gt, gq, state and the column's counts."""
    at = recs[recs["tpos"] == col + 1]
    nonref = set(v["alleles"]) != {v["ref"]}
    want = nonref and (report_homref or v["state"] != "homref")
    assert len(at) == (1 if want else 0), (v, len(at))
    if not want:
        return 0
    r = at[0]
    assert chr(r["gt0"]) + chr(r["gt1"]) == v["gt"] and int(r["gq"]) == v["gq"]
    assert M.STATES[int(r["gt_state"])] == v["state"]
    assert [int(x) for x in r["counts"][:4]] == [v["alleles"].count(b) for b in M.BASES]
    assert [int(x) for x in r["bqsum"]] == [sum(q for a, q in zip(v["alleles"], v["bqs"]) if a == b) for b in M.BASES]
    return 1


def _reversed(v):
    """Vector v with its reads in the opposite fetch order and the genotype the reference's sums give then, or None
    where gt, gq and state come out the same (the vector does not tell the two orders apart)."""
    a, q = v["alleles"][::-1], v["bqs"][::-1]
    g = G.genotype(v["ref"], a, q, v["prior"])
    if (g["gt"], g["gq"], g["state"]) == (v["gt"], v["gq"], v["state"]):
        return None
    return dict(v, alleles=a, bqs=q, gt=g["gt"], gq=g["gq"], state=g["state"])


def test_model_reproduces_leaf_fixture():
    """All 400 leaf_gtlib columns in one pile at prior 1e-3: every column with a non-reference allele is a record that
    carries the fixture's genotype; a column of reference alleles only is no candidate."""
    vs = G.leaf_vectors(util.load_json("leaf_gtlib")["vectors"])
    assert len(vs) == 400
    P = G.build(vs)
    for homref in (True, False):
        recs, log = M.run(P.batch, P.call_chunks, 1 / (10 ** 3), report_homref=homref)
        n = sum(_check_vector(v, c[0], recs, homref) for v, c in zip(vs, P.cols))
        assert n == len(recs) and log[0] == sum(set(v["alleles"]) != {v["ref"]} for v in vs)
        assert log[2:6] == [sum(v["state"] == s and set(v["alleles"]) != {v["ref"]} for v in vs) for s in M.STATES]


def test_model_reproduces_gt_edges_fixture():
    """All 193 boundary columns, each in its own pile at its own prior with min_gq = k: 136 hold a non-reference allele;
    those whose record depends on the fetch order give the other record with their reads turned round; the order pairs
    differ as the fixture says; the LowGQ decision sits where the fixture's gq and k put it."""
    edges = util.load_json("gt_edges")["vectors"]
    assert len(edges) == 193
    seen, turned = 0, 0
    for i, v in enumerate(edges):
        P = G.build([v], orders=[G.ORDERS[i % 3]])
        for homref in (True, False):
            recs, log = M.run(P.batch, P.call_chunks, v["prior"], report_homref=homref, min_gq=v["k"], min_bq=1,
                              min_ref_count=0, min_alt_count=0)
            n = _check_vector(v, P.cols[0][0], recs, homref)
            assert len(recs) == n
            if n and v["state"] != "homref":
                assert (int(recs[0]["status"]) == M.ST_LOWGQ) == (v["gq"] < v["k"])
        seen += set(v["alleles"]) != {v["ref"]}
        w = _reversed(v) if set(v["alleles"]) != {v["ref"]} else None
        if w is not None:
            P = G.build([w], orders=[G.ORDERS[i % 3]])
            recs, _ = M.run(P.batch, P.call_chunks, v["prior"], report_homref=True, min_gq=v["k"], min_bq=1,
                            min_ref_count=0, min_alt_count=0)
            assert _check_vector(w, P.cols[0][0], recs, True) == len(recs) == 1
            turned += 1
    assert seen == 136 and turned > 50
    # the fixture's own order pairs are columns of reference alleles only: they differ in the fixture, and are no
    # candidates here (checked above: no record with or without report_homref)
    by = {}
    for v in edges:
        if v["kind"] == "order":
            by.setdefault(v["pair"], []).append(v)
    assert len(by) >= 5 and all(set(v["alleles"]) == {v["ref"]} for p in by.values() for v in p)
    assert all((a["gt"], a["gq"], a["state"]) != (b["gt"], b["gq"], b["state"]) for a, b in by.values())


def _rec(tpos, ref, gt, state, gq, status, counts):
    alt = {0: ref, 1: gt[1], 2: gt[0], 3: gt[0]}[state]
    return (tpos, -1, -1, gq, ord(ref), ord(alt), ord(gt[0]), ord(gt[1]), status, state, 0, 0, counts, [0, 0, 0, 0])


LINES = [
    # het
    (_rec(101, "A", "AG", 1, 57, M.ST_PASS, [9, 0, 11, 0, 0, 0]), "chr7\t101\t.\tA\tG\t57\tPASS\t.\tGT:GQ:DP:AD:VAF\t0/1:57:20:9,11:0.55\n"),
    # homalt without and with reference reads (a deletion counts in DP)
    (_rec(202, "C", "TT", 3, 99, M.ST_PASS, [0, 18, 0, 0, 2, 1]), "chr7\t202\t.\tC\tT\t99\tPASS\t.\tGT:GQ:DP:AD:VAF\t1/1:99:19:0,18:0.95\n"),
    (_rec(203, "C", "TT", 3, 31, M.ST_HIGHDEPTH, [0, 27, 0, 3, 0, 0]), "chr7\t203\t.\tC\tT\t31\tHighDepth\t.\tGT:GQ:DP:AD:VAF\t1/1:31:30:3,27:0.90\n"),
    # hetalt in genotype order
    (_rec(300, "A", "CG", 2, 40, M.ST_PASS, [1, 0, 6, 5, 0, 0]), "chr7\t300\t.\tA\tC,G\t40\tPASS\t.\tGT:GQ:DP:AD:VAF\t1/2:40:12:1,5,6:0.42,0.50\n"),
    (_rec(301, "A", "TA", 0, 60, M.ST_PASS, [10, 1, 0, 0, 0, 0]), None),                       # homref: never printed
    (_rec(400, "G", "GA", 1, 3, M.ST_LOWGQ, [2, 0, 5, 0, 0, 0]), "chr7\t400\t.\tG\tA\t3\tLowGQ\t.\tGT:GQ:DP:AD:VAF\t0/1:3:7:5,2:0.29\n"),
    (_rec(401, "G", "GT", 1, 30, M.ST_LOWBQ, [0, 3, 5, 0, 0, 0]), "chr7\t401\t.\tG\tT\t30\tLowBQ\t.\tGT:GQ:DP:AD:VAF\t0/1:30:8:5,3:0.38\n"),
    (_rec(402, "T", "TC", 1, 25, M.ST_LOWDEPTH, [0, 9, 0, 1, 0, 0]), "chr7\t402\t.\tT\tC\t25\tLowDepth\t.\tGT:GQ:DP:AD:VAF\t0/1:25:10:9,1:0.10\n"),
]


def test_vcf_lines_against_literals():
    from himut_amd import vcflib
    recs = np.array([r for r, _ in LINES], M.RECORD_DTYPE)
    want = [line for _, line in LINES if line is not None]
    assert vcflib.germline_lines("chr7", recs) == want
    assert M.vcf_lines("chr7", recs) == want


def test_lines_through_the_package_loaders(tmp_path):
    """load_hetsnps returns exactly the PASS 0/1 records, load_germline_counts the het and hom counts; a hetalt line is
    skipped by both; the header names the five filters, the format fields, the contigs and the sample."""
    from himut_amd import vcflib
    recs = np.array([r for r, _ in LINES], M.RECORD_DTYPE)
    head = vcflib.get_germline_vcf_header("in.bam", None, None, {"chr7": 1000, "chr10": 50}, 0, 20, 20, 2, 2, 80, 1e-3, 1,
                                          "1.0", "g.vcf", "SMP")
    path = str(tmp_path / "g.vcf")
    vcflib.dump_vcf(path, head, ["chr7"], lambda chrom: vcflib.germline_lines(chrom, recs))
    text = open(path).read()
    assert text.startswith("##fileformat=VCFv4.2\n")
    for fid in ("PASS", "LowGQ", "LowBQ", "LowDepth", "HighDepth"):
        assert "##FILTER=<ID={},".format(fid) in text
    for fid in ("GT", "GQ", "DP", "AD", "VAF"):
        assert "##FORMAT=<ID={},".format(fid) in text
    assert text.index("##contig=<ID=chr7,length=1000>") < text.index("##contig=<ID=chr10,length=50>")
    assert "##himut_command=himut germline -i in.bam  --min_mapq 0 --min_gq 20 --min_bq 20 --min_ref_count 2 " \
           "--min_alt_count 2 --germline_snv_prior 0.001 --threads 1 -o g.vcf\n" in text
    assert "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSMP\n" in text
    hetsnps, _, _ = vcflib.load_hetsnps(path, "chr7", 1000)
    assert hetsnps == [(101, "A", "G")]
    assert vcflib.load_germline_counts(path, ["chr7"]) == (1, 1, 0, 0)
    assert vcflib.load_germline_counts(path, ["chr10"]) == (0, 0, 0, 0)
    vcflib.dump_counter_log(vcflib.GERMLINE_LOG_ROWS, ["chr7", "chr10"], {"chr7": list(range(12)), "chr10": [1] * 12},
                            str(tmp_path / "g.log"))
    rows = [l.split() for l in open(tmp_path / "g.log")]
    assert rows[0] == ["chr7", "chr10", "total"] and rows[1] == ["num_pos", "0", "1", "1"] and rows[7] == ["num_pass", "6", "1", "7"]
    assert len(rows) == 13


def test_parser_defaults_and_torchrun_refusal(monkeypatch, tmp_path):
    from himut_amd import germline
    from himut_amd.parse_args import parse_args
    _, o = parse_args("x", ["germline", "-i", "a.bam", "-o", "g.vcf"])
    assert (o.sub, o.bam, o.output, o.region, o.region_list, o.ref, o.cs_from_ref) == ("germline", "a.bam", "g.vcf", None, None, None, False)
    assert (o.min_mapq, o.min_gq, o.min_bq, o.min_ref_count, o.min_alt_count, o.germline_snv_prior) == (0, 20, 20, 2, 2, 1e-3)
    _, c = parse_args("x", ["call", "-i", "a.bam", "-o", "c.vcf"])
    assert (o.threads, o.devices) == (c.threads, c.devices)
    with pytest.raises(SystemExit):
        parse_args("x", ["germline", "-i", "a.bam", "-o", "g.vcf", "--cs_from_ref"])
    with pytest.raises(SystemExit):
        parse_args("x", ["germline", "-o", "g.vcf"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single process"):
        germline.call_germline_snvs(str(tmp_path / "none.bam"), None, None, 0, 20, 20, 2, 2, 1e-3, 1, "x",
                                    str(tmp_path / "g.vcf"))


def test_model_rules_on_hand_built_reads():
    """The contract's rules, stated on a dozen reads: regions select, they never shape a pile; secondary out,
    supplementary in; min_mapq takes marks and cells away; n as the reference base is counted, not genotyped."""
    import random
    from himut_amd.readbatch import batch_from_records
    rs = random.Random(5)
    ref = "".join(rs.choice("ATGC") for _ in range(400))
    alt = {p: "ATGC"[("ATGC".index(ref[p]) + 1) % 4] for p in range(400)}
    recs = [M.make_read(ref, 10, 90, {50: alt[50]}), M.make_read(ref, 20, 80, {50: alt[50]}),         # both end at 100
            M.make_read(ref, 30, 150, {50: alt[50], 100: alt[100], 120: alt[120]}, mapq=5),
            M.make_read(ref, 40, 150, {100: alt[100]}, flag=0x800), M.make_read(ref, 45, 150, {50: alt[50]}, flag=0x100),
            M.make_read(ref, 60, 150, {100: alt[100], 130: alt[130]}, nref=(130,))]
    b = batch_from_records("chrH", 400, recs)
    kw = dict(min_gq=0, min_bq=1, min_ref_count=0, min_alt_count=0, report_homref=True)
    one, log = M.run(b, [(1, 400)], **kw)
    assert list(one["tpos"]) == [51, 101, 121] and log[:2] == [3, 1]
    assert int(one[0]["counts"].sum()) == 4 and int(one[1]["counts"].sum()) == 3       # the secondary read is out
    two, log2 = M.run(b, [(1, 101), (101, 200), (90, 110), (51, 51)], **kw)           # shared, overlapping, out of order
    assert log2 == log and all(np.array_equal(one[k], two[k]) for k in M.FIELDS)
    part, _ = M.run(b, [(101, 101)], **kw)
    assert all(np.array_equal(part[k], one[1:2][k]) for k in M.FIELDS)                # the pile does not depend on the regions
    hi, logh = M.run(b, [(1, 400)], min_mapq=20, **kw)
    assert list(hi["tpos"]) == [51, 101] and int(hi[0]["counts"].sum()) == 3 and logh[:2] == [2, 1]
