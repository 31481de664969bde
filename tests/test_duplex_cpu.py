"""The duplex contract without a GPU: the plain-Python model (tests/duplex_model.py) on the hand-built reads of
tests/duplex_cases.py against what each rule says, the identities between its counters, the rules of mate[]; the host's
pairing of by-strand names (himut_amd.duplex.mate_index); the VCF lines, the header and the --ss table; the parser."""
import numpy as np
import pytest

from tests import duplex_cases as C
from tests import duplex_model as M

CASES = C.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_on_hand_built(case):
    _name, b, mate, chunks, kw, expect = case
    recs, ss, log = M.run(b, mate, chunks, **kw)
    d = M.check_identities(recs, ss, log)
    assert expect is not None
    expect(recs, ss, d)
    assert list(recs["site"]) == list(range(len(recs)))
    keys = [(int(r["tpos"]), "ATGC".index(chr(r["ref"])), "ATGC".index(chr(r["alt"]))) for r in recs]
    assert keys == sorted(set(keys))                                 # position, then allele: each candidate once


def test_every_state_and_rule_is_reached():
    total = dict.fromkeys(M.LOG, 0)
    for _name, b, mate, chunks, kw, _e in CASES:
        for k, v in M.logd(M.run(b, mate, chunks, **kw)[2]).items():
            total[k] += v
    for k in M.STATES + M.CAUSES + ("num_trim", "num_window", "num_lowbq", "num_mate_window", "ds_events", "pairs_in_play"):
        assert total[k] > 0, k
    assert total["ds_events"] > total["ds_events_in_chunk"] > 0


@pytest.mark.parametrize("seed", range(3))
def test_identities_on_the_sweep(seed):
    b, mate, chunks, kw = C.random_case(seed)
    recs, ss, log = M.run(b, mate, chunks, **kw)
    d = M.check_identities(recs, ss, log)
    assert d["pairs"] == int((mate >= 0).sum()) // 2 and d["reads"] == b.n


def test_mate_rules():
    M.check_mate([1, 0, -1], 3)
    for bad in ([3, -1, -1], [-2, -1, -1], [0, -1, -1], [1, -1, -1], [1, 2, 1], [1, 0]):
        with pytest.raises(ValueError):
            M.check_mate(bad, 3)


def test_mate_index_on_names():
    from himut_amd import duplex
    names = ["m/1/ccs/fwd", "m/1/ccs/rev",              # a pair
             "m/2/ccs",                                  # no suffix
             "m/3/ccs/fwd",                              # a lone strand
             "m/4/ccs/fwd", "m/4/ccs/rev", "m/4/ccs/rev",    # two primaries of a strand: none of the three pairs
             "m/5/ccs/rev", "m/5/ccs/fwd", "m/5/ccs/fwd",    # the second /fwd is supplementary: ignored, the pair stands
             "m/6/ccs/fwd", "m/6/ccs/rev",               # the /rev is secondary: the /fwd is a lone strand
             "fwd", "/fwd"]                              # a bare word has no suffix; a bare suffix has the empty stem
    flag = np.array([0, 16, 0, 0, 0, 16, 16, 16, 0, 0x800, 0, 0x110, 0, 0], np.uint16)
    mapq = np.full(len(names), 60, np.uint8)
    mate = duplex.mate_index(names, flag, mapq)
    assert mate.dtype == np.int32 and list(mate) == [1, 0, -1, -1, -1, -1, -1, 8, 7, -1, -1, -1, -1, -1]
    assert list(mate) == list(C.pair_by_name(names, flag))
    M.check_mate(mate, len(names))
    _mate, counts = duplex.pair_reads(names, flag)
    assert dict(zip(duplex.HOST_LOG_ROWS, counts)) == dict(num_reads_paired=4, num_reads_unsuffixed=2, num_reads_not_primary=2,
                                                           num_reads_single=3, num_reads_ambiguous=3)
    assert sum(counts) == len(names)
    mapq[0] = 0                                          # a mapping quality unpairs nothing on the host
    assert list(duplex.mate_index(names, flag, mapq)) == list(mate)
    assert list(duplex.mate_index([], np.zeros(0, np.uint16))) == []


def test_vcf_and_ss_text():
    from himut_amd import duplex, vcflib
    case = {c[0]: c for c in CASES}
    _n, b, mate, chunks, kw, _e = case["alt_on_unpaired_reads"]
    recs, ss, log = M.run(b, mate, chunks, **kw)
    r = recs[0]
    ref, alt = C.REF[500], C.A1[500]
    c = [int(x) for x in r["counts"]]
    n_ref, n_alt, dp = c["ATGC".index(ref)], c["ATGC".index(alt)], c[0] + c[1] + c[2] + c[3] + c[5]
    assert (n_alt, dp) == (5, 27)
    assert vcflib.duplex_lines("chr1", recs) == [
        "chr1\t501\t.\t{}\t{}\t.\t{}\tDS=1;SS=1;UNP=2\tGT:GQ:BQ:DP:AD:VAF:DS:SS:UNP\t./.:{}:40.0:27:{},5:0.19:1:1:2\n".format(
            ref, alt, M.S.STATUS[int(r["status"])], int(r["gq"]), n_ref)]
    _n, b, mate, chunks, kw, _e = case["single_strand_classes"]
    recs, ss, log = M.run(b, mate, chunks, **kw)
    lines = duplex.ss_lines(ss, log)
    assert lines[0] == "class\tcount\n" and [l.split("\t")[0] for l in lines[1:13]] == list(M.SS_CLASSES)
    assert [int(l.split("\t")[1]) for l in lines[1:13]] == ss and sum(ss) == 2
    d = M.logd(log)
    assert lines[13:] == ["ds_bases\t{}\n".format(d["ds_bases"]), "ds_pairs_overlap\t1\n"]
    header = vcflib.get_duplex_vcf_header("in.bam", None, None, {"chr1": 4000}, None, None, 30, 60, 100, 200, 0.99, 20, 93, 0.01, 0,
                                          20, 50, 3, 1, 1e-3, 1, "v", "o.vcf", "sample", ss_file="ss.tsv")
    for word in ("##INFO=<ID=DS,", "##INFO=<ID=SS,", "##INFO=<ID=UNP,", "##FORMAT=<ID=DS,", "##FILTER=<ID=Germline,", "##molecules=",
                 "##pile=", "the two reads of a molecule are two reads", "himut duplex -i in.bam ", "--ss ss.tsv",
                 "##content=himut double-strand single base substitutions"):
        assert word in header, word
    assert header.splitlines()[-1].endswith("\tFORMAT\tsample")


def test_parser():
    from himut_amd.parse_args import parse_args
    _p, o = parse_args("x", ["duplex", "-i", "bystrand.bam", "-o", "duplex.vcf"])
    assert o.sub == "duplex" and o.bam == "bystrand.bam" and o.output == "duplex.vcf" and o.ss is None
    _p, call = parse_args("x", ["call", "-i", "in.bam", "-o", "out.vcf"])
    for k in ("min_qv", "min_mapq", "min_sequence_identity", "min_gq", "min_bq", "min_ref_count", "min_alt_count", "min_trim",
              "max_mismatch_count", "mismatch_window_size", "germline_snv_prior"):
        assert getattr(o, k) == getattr(call, k), k
    assert o.cs_from_ref is False and o.ref is None and o.common_snps is None and o.panel_of_normals is None and o.devices == "0"
    _p, o = parse_args("x", ["duplex", "-i", "b.bam", "-o", "d.vcf", "--ss", "ss.tsv", "--ref", "r.fa", "--cs_from_ref", "--common_snps",
                             "c.vcf", "--panel_of_normals", "p.vcf"])
    assert (o.ss, o.ref, o.cs_from_ref, o.common_snps, o.panel_of_normals) == ("ss.tsv", "r.fa", True, "c.vcf", "p.vcf")
    with pytest.raises(SystemExit):
        parse_args("x", ["duplex", "-i", "b.bam", "-o", "d.vcf", "--cs_from_ref"])          # needs --ref
    with pytest.raises(SystemExit):
        parse_args("x", ["duplex", "-o", "d.vcf"])


def test_refuses_a_process_group(monkeypatch):
    """Under torch.distributed.run the driver raises before it opens anything, as `support` does."""
    from himut_amd import duplex
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(RuntimeError) as e:
        duplex.call_duplex_substitutions("none.bam", None, None, None, None, 30, 60, 0.99, 20, 93, 0.01, 0, 20, 3, 1, 1e-3, 1, "v",
                                         "o.vcf")
    assert "duplex" in str(e.value)
