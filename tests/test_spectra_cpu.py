"""`himut id83` and `himut dbs78`, the parts that need no GPU: the plain model on the hand-built
cases, the doublet table, the host parser on the hand-written VCF, the two subparsers and the writers."""
import os
import re

import numpy as np
import pytest

from himut_amd import spectra
from himut_amd.parse_args import parse_args
from tests import spectra_cases as C, spectra_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_model_gives_the_hand_written_label(case):
    _name, seq, a, kind, L, ins, label = case
    assert M.id83_label(seq, a, kind, L, ins) == label


def test_cases_cover_every_class_and_both_counters():
    labels = {c[6] for c in C.CASES}
    assert set(M.ID83_LABELS) <= labels and M.NBASE in labels and M.RANGE in labels


def test_model_refuses_an_inserted_n():
    assert M.id83_label("GCAA", 1, "ins", 2, "AN") == M.NBASE


def test_product_label_lists_are_the_models():
    assert spectra.ID83_LST == M.ID83_LABELS
    assert spectra.DBS78_LST == M.DBS78_LABELS


def test_device_table_is_the_label_list():
    """The string the kernel searches (csrc/himut_spectra.h) spells the 78 labels in bin order."""
    text = open(os.path.join(ROOT, "himut_amd", "csrc", "himut_spectra.h")).read()
    body = text[text.index("DBS78_TABLE["):]
    body = body[:body.index(";")]
    letters = "".join(re.findall(r'"([ACGT]+)"', body))
    assert [letters[i:i + 2] + ">" + letters[i + 2:i + 4] for i in range(0, len(letters), 4)] == M.DBS78_LABELS


def test_doublet_pairs_land_on_78_classes():
    pairs = [a + b for a in "ACGT" for b in "ACGT"]
    hits = {}
    for ref in pairs:
        for alt in pairs:
            k = M.dbs78_label(ref, alt)
            if ref[0] != alt[0] and ref[1] != alt[1]:
                hits[k] = hits.get(k, 0) + 1
            else:
                assert k == M.UNCHANGED
    assert sorted(hits) == sorted(M.DBS78_LABELS) and sum(hits.values()) == 144 and set(hits.values()) == {1, 2}
    # a class is hit twice unless the doublet is its own reverse complement
    for k, n in hits.items():
        ref, alt = k.split(">")
        assert n == (1 if M.revcomp(ref) == ref and M.revcomp(alt) == alt else 2), k
    assert M.dbs78_label("ac", "gt") == "AC>GT" and M.dbs78_label("GT", "AC") == "AC>GT"
    assert M.dbs78_label("AT", "TG") == "AT>CA" and M.dbs78_label("TA", "AC") == "TA>GT"
    assert M.dbs78_label("NC", "GT") == M.NLETTER and M.dbs78_label("AC", "GR") == M.NLETTER
    assert M.dbs78_label("NC", "NT") == M.NLETTER                   # the letter rule comes first
    assert M.dbs78_label("AC", "AT") == M.UNCHANGED and M.dbs78_label("AC", "GC") == M.UNCHANGED


def _write(path, text):
    with open(path, "w") as o:
        o.write(text)
    return str(path)


def _seq_of(chrom):
    return {"c1": C.C1.encode(), "c2": C.C2.encode()}.get(chrom)


@pytest.mark.parametrize("all_filters", [False, True])
def test_host_parser_on_the_hand_written_vcf(tmp_path, all_filters):
    vcf = _write(tmp_path / "in.vcf", C.VCF_TEXT)
    assert spectra.vcf_contigs(vcf) == {"c1": 21, "c2": 13, "c3": 100}
    per_chrom, absent = spectra.load_indel_alleles(vcf, ["c1", "c2", "c3"], _seq_of, all_filters)
    assert absent == C.ID83_ABSENT and sorted(per_chrom) == ["c1", "c2"]
    _counts, lines, log = C.ID83_EXPECT[all_filters]
    got = []
    for chrom in ("c1", "c2"):
        al = per_chrom[chrom]
        # the host's counters: everything but num_range and num_classified, and the deleted N the device finds
        assert al.log[:6] == log[chrom][:6], chrom
        anchor, typ, length, bases = al.arrays()
        assert anchor.dtype == np.int32 and typ.dtype == np.uint8 and length.dtype == np.int32 and bases.shape == (len(anchor), 16)
        for (pos, ref, alt), a, t, L, b in zip(al.text, anchor, typ, length, bases):
            assert a == pos - 1 and L == abs(len(ref) - len(alt)) and t == (1 if len(alt) > len(ref) else 0)
            ins = "".join("ATGC"[(int(b[j >> 2]) >> (2 * (j & 3))) & 3] for j in range(L)) if t else ""
            assert ins == (alt[1:] if t else "")
            label = M.id83_label(_seq_of(chrom).decode(), int(a), "ins" if t else "del", int(L), ins)
            got.append((chrom, pos, ref, alt, label))
    # the alleles handed to the device, labelled by the model: the --classes lines and the range allele
    assert ["\t".join(str(x) for x in g) for g in got if g[4] != M.RANGE] == lines
    assert [g[:2] for g in got if g[4] == M.RANGE] == [("c2", 14)]
    # a contig list narrows the parse
    only, _ = spectra.load_indel_alleles(vcf, ["c2"], _seq_of, all_filters)
    assert sorted(only) == ["c2"] and only["c2"].log == per_chrom["c2"].log


def test_host_parser_reads_bgz_and_headerless_contigs(tmp_path):
    import gzip
    bgz = str(tmp_path / "in.vcf.bgz")
    with gzip.open(bgz, "wt") as o:
        o.write("".join(l for l in C.VCF_TEXT.splitlines(True) if not l.startswith("##contig")))
    assert spectra.vcf_contigs(bgz) == {"c1": 0, "c2": 0, "c3": 0}
    per_chrom, absent = spectra.load_indel_alleles(bgz, ["c1", "c2", "c3"], _seq_of)
    assert absent == C.ID83_ABSENT and per_chrom["c1"].log[:6] == C.ID83_EXPECT[False][2]["c1"][:6]
    with pytest.raises(ValueError):
        spectra.vcf_contigs(str(tmp_path / "in.txt"))


@pytest.mark.parametrize("all_filters", [False, True])
def test_doublet_parser_on_the_hand_written_vcf(tmp_path, all_filters):
    vcf = _write(tmp_path / "in.vcf", C.VCF_TEXT)
    per_chrom = spectra.load_doublets(vcf, ["c1", "c2", "c3"], all_filters)
    counts, log = C.DBS78_EXPECT[all_filters]
    assert sorted(per_chrom) == ["c1"]
    labels = [M.dbs78_label(r, a) for r, a in zip(*per_chrom["c1"])]
    assert len(labels) == log["c1"][0] and labels.count(M.NLETTER) == log["c1"][1] and labels.count(M.UNCHANGED) == log["c1"][2]
    assert {k: labels.count(k) for k in labels if k in M.DBS78_LABELS} == counts


def test_pack_bases_is_the_indel_records_packing():
    row = spectra.pack_bases("ACGTTGCA" * 8)
    assert row.dtype == np.uint8 and row.shape == (16,)
    assert "".join("ATGC"[(int(row[j >> 2]) >> (2 * (j & 3))) & 3] for j in range(64)) == "ACGTTGCA" * 8
    assert list(spectra.pack_bases("T")) == [1] + [0] * 15


def test_subparsers_flags():
    _p, o = parse_args("x", ["id83", "-i", "a.vcf", "--ref", "r.fa", "-o", "o.tsv"])
    assert (o.sub, o.input, o.ref, o.output, o.region, o.region_list, o.all_filters, o.classes, o.devices) == \
        ("id83", "a.vcf", "r.fa", "o.tsv", None, None, False, None, "0")
    _p, o = parse_args("x", ["id83", "-i", "a.vcf.bgz", "--ref", "r.fa", "-o", "o.tsv", "--region", "chr1", "--all_filters",
                             "--classes", "c.tsv", "--devices", "1"])
    assert (o.region, o.all_filters, o.classes, o.devices) == ("chr1", True, "c.tsv", "1")
    _p, o = parse_args("x", ["dbs78", "-i", "d.vcf", "-o", "o.tsv", "--region_list", "l.txt"])
    assert (o.sub, o.input, o.output, o.region, o.region_list, o.all_filters, o.devices) == \
        ("dbs78", "d.vcf", "o.tsv", None, "l.txt", False, "0")
    assert not hasattr(o, "ref") and not hasattr(o, "classes")
    for bad in (["id83", "-i", "a.vcf", "-o", "o.tsv"],                                   # --ref is required
                ["id83", "-i", "a.vcf", "--ref", "r.fa"],
                ["dbs78", "-o", "o.tsv"],
                ["dbs78", "-i", "d.vcf", "-o", "o.tsv", "--ref", "r.fa"],                # no FASTA is taken
                ["id83", "-i", "a.vcf", "--ref", "r.fa", "-o", "o.tsv", "--region", "c", "--region_list", "l"],
                ["dbs78", "-i", "d.vcf", "-o", "o.tsv", "--region", "c", "--region_list", "l"]):
        with pytest.raises(SystemExit):
            parse_args("x", bad)


@pytest.mark.parametrize("sub", ["id83", "dbs78"])
def test_help_says_whose_definition_it_is(sub, capsys):
    with pytest.raises(SystemExit):
        parse_args("x", [sub, "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "this package's definition of the COSMIC scheme" in text


def test_writers(tmp_path):
    counts = list(range(83))
    out = str(tmp_path / "id83.tsv")
    spectra.write_counts("id83", spectra.ID83_LST, counts, out)
    lines = open(out).read().split("\n")
    assert lines[0] == "id83\tcounts" and lines[1] == "1:Del:C:0\t0" and lines[83] == "5:Del:M:5\t82" and lines[84] == "" and len(lines) == 85
    out = str(tmp_path / "dbs78.tsv")
    spectra.write_counts("dbs78", spectra.DBS78_LST, np.arange(78), out)
    lines = open(out).read().split("\n")
    assert lines[0] == "dbs78\tcounts" and lines[1] == "AC>CA\t0" and lines[78] == "TT>GG\t77" and len(lines) == 80
    al = spectra.IndelAlleles()
    al.text = [(2, "TA", "T"), (5, "T", "TA"), (9, "G", "GAC")]
    path = str(tmp_path / "classes.tsv")
    with open(path, "w") as fh:
        spectra.write_classes(fh, "c9", al, np.array([10, 255, 82], np.uint8))
    assert open(path).read() == "c9\t2\tTA\tT\t1:Del:T:4\nc9\t9\tG\tGAC\t5:Del:M:5\n"
