"""`tricount`, `sbs96`, `sbs1536` and `burden` without a GPU: the parser, the label lists, the FASTA record index and
the host mirrors of the device paths against the reference's files (tests/golden/mutpatterns.json)."""
import json
import os

import pytest

from himut_amd import mutlib, normcounts, reflib
from himut_amd.parse_args import parse_args

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    """mutpatterns.json with its shared texts put back ("@<hash>" -> blobs[...]; burden's FASTA is norm_host.json's)."""
    g = json.load(open(os.path.join(GOLDEN, "mutpatterns.json")))
    blobs = g.pop("blobs")

    def put(x):
        if isinstance(x, dict):
            return {k: put(v) for k, v in x.items()}
        if isinstance(x, list):
            return [put(v) for v in x]
        return blobs[x] if isinstance(x, str) and x.startswith("@") else x
    g = put(g)
    fasta = json.load(open(os.path.join(GOLDEN, "norm_host.json")))["fasta_text"]
    for c in g["burden"]:
        if c["fasta"] == "norm_host":
            c["fasta"] = fasta
    return g


G = load_golden()


def _write(path, text):
    with open(path, "w", newline="") as o:
        o.write(text)
    return str(path)


def _raises(name):
    return {"KeyError": KeyError, "IndexError": IndexError, "ZeroDivisionError": ZeroDivisionError,
            "SystemExit(0)": SystemExit}[name]


def test_parser_reference_defaults():
    _, o = parse_args("t", ["tricount", "-i", "g.fa", "-o", "o.tsv"])
    assert (o.ref, o.region, o.region_list, o.threads, o.output, o.devices) == ("g.fa", None, None, 1, "o.tsv", "0")
    _, o = parse_args("t", ["burden", "-i", "n.tsv", "--tri", "t.tsv", "--region_list", "l", "-o", "b"])
    assert (o.input, o.ref, o.tri, o.region_list, o.threads, o.output) == ("n.tsv", None, "t.tsv", "l", 1, "b")
    for sub in ("sbs96", "sbs1536"):
        _, o = parse_args("t", [sub, "-i", "x.vcf", "--ref", "g.fa", "-o", "o.tsv", "--region", "chr1"])
        assert (o.sub, o.input, o.ref, o.region, o.region_list, o.output) == (sub, "x.vcf", "g.fa", "chr1", None, "o.tsv")
        with pytest.raises(SystemExit):
            parse_args("t", [sub, "-i", "x.vcf", "-o", "o.tsv"])          # --ref is required


def test_label_lists_match_reference():
    assert normcounts.TRI_LST == G["tri_lst"]
    assert normcounts.SBS96_LST == G["sbs96_lst"]
    assert mutlib.SBS1536_LST == G["sbs1536_lst"]


@pytest.mark.parametrize("case", G["tricount"], ids=[c["name"] for c in G["tricount"]])
def test_tricount_host_mirror_golden(case, tmp_path):
    fa = _write(tmp_path / "g.fa", case["fasta"])
    rl = _write(tmp_path / "r.list", case["region_list"]) if "region_list" in case else None
    out = str(tmp_path / "o.tsv")
    args = (fa, case.get("region"), rl, 1, out)
    if case["raises"]:
        with pytest.raises(_raises(case["raises"])):
            reflib.get_ref_tricount(*args, tricounts=reflib.get_genome_tricounts_host)
    else:
        reflib.get_ref_tricount(*args, tricounts=reflib.get_genome_tricounts_host)
    got = open(out).read() if os.path.exists(out) else None
    assert got == case["tsv"]


def test_index_fasta_matches_read_fasta_rules(tmp_path):
    text = "junk\n>\n>a d\r\nAC\n\nGT\n>b\nTT>x\n>a\nCC\r\n>c"
    fa = _write(tmp_path / "g.fa", text)
    idx = reflib.index_fasta(text.encode())
    assert list(idx) == ["a", "b", "c"]
    body = {k: text.encode()[s:e] for k, (s, e) in idx.items()}
    assert body == {"a": b"CC\r", "b": b"TT>x", "c": b""}
    assert normcounts.read_fasta(fa) == {"a": "CC", "b": "TT>x", "c": ""}
    assert normcounts.read_fasta(_write(tmp_path / "e.fa", "")) == {}


@pytest.mark.parametrize("case", G["sbs"], ids=[c["name"] for c in G["sbs"]])
def test_sbs_host_mirror_golden(case, tmp_path):
    from himut_amd.util import load_loci
    fa = _write(tmp_path / "g.fa", case["fasta"])
    vcf = _write(tmp_path / "s.vcf", case["vcf"])
    rl = _write(tmp_path / "r.list", case["region_list"]) if case["region_list"] is not None else None
    _, tname2tsize = mutlib.get_sample(vcf)
    chrom_lst, _ = load_loci(case["region"], rl, tname2tsize)
    refseq = normcounts.read_fasta(fa)
    for kind, load, write in (("sbs96", normcounts.load_sbs96_counts, mutlib.write_sbs96_counts),
                              ("sbs1536", mutlib.load_sbs1536_counts, mutlib.write_sbs1536_counts)):
        out = str(tmp_path / (kind + ".tsv"))

        def run():
            write(load(vcf, refseq, chrom_lst), out)
        if case[kind + "_raises"]:
            with pytest.raises(_raises(case[kind + "_raises"])):
                run()
        else:
            run()
        assert (open(out).read() if os.path.exists(out) else None) == case[kind + "_tsv"], kind


@pytest.mark.parametrize("case", G["burden"], ids=[c["name"] for c in G["burden"]])
def test_burden_golden(case, tmp_path):
    inf = _write(tmp_path / "n.tsv", case["table"])
    tri = _write(tmp_path / "t.tsv", case["tri"]) if case["tri"] is not None else None
    fa = _write(tmp_path / "g.fa", case["fasta"]) if case["fasta"] is not None else None
    rl = _write(tmp_path / "r.list", case["region_list"])
    out = str(tmp_path / "b.txt")
    args = (inf, fa, tri, rl, 1, out)
    if case["raises"]:
        with pytest.raises(_raises(case["raises"])):
            mutlib.get_burden_per_cell(*args, tricounts=reflib.get_genome_tricounts_host)
    else:
        mutlib.get_burden_per_cell(*args, tricounts=reflib.get_genome_tricounts_host)
    assert (open(out).read() if os.path.exists(out) else None) == case["out"]


def test_burden_without_region_list_is_type_error(tmp_path):
    inf = _write(tmp_path / "n.tsv", G["burden"][0]["table"])
    tri = _write(tmp_path / "t.tsv", G["burden"][0]["tri"])
    with pytest.raises(TypeError):
        mutlib.get_burden_per_cell(inf, None, tri, None, 1, str(tmp_path / "b.txt"))


def test_sbs_region_and_region_list_rejected(tmp_path, capsys):
    from himut_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["sbs96", "-i", "x.vcf", "--ref", "g.fa", "--region", "chr1", "--region_list", "l", "-o",
              str(tmp_path / "o.tsv")])
    assert e.value.code == 0
    assert "not for both parameters" in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "o.tsv")
