"""The transcription-strand spectrum without a GPU: the plain model (tests/strands_model.py) on the hand-built cases, the
gene parsers, the segment list's invariants, the label lists and the subparsers."""
import numpy as np
import pytest

from tests import strands_cases as K
from tests import strands_model as SM


def _as_arrays(subs):
    return [p - 1 for p, *_ in subs], [r for _p, r, *_ in subs], [a for _p, _r, a, *_ in subs]


@pytest.mark.parametrize("seq,start,mask,subs", [(K.CHR1, K.CHR1_SEG_START, K.CHR1_SEG_MASK, K.CHR1_SUBS),
                                                 (K.CHR2, K.CHR2_SEG_START, K.CHR2_SEG_MASK, K.CHR2_SUBS)])
def test_model_gives_the_hand_written_labels(seq, start, mask, subs):
    labels = SM.bin_labels()
    cls, out = SM.sbs384(seq, start, mask, *_as_arrays(subs))
    flags = {"n": 0, "outside": 0, "range": 0}
    for k, (_pos, _ref, _alt, cat, label) in zip(cls.tolist(), subs):
        if cat is None:
            assert k == SM.NO_CLASS
            flags[label] += 1
        else:
            assert labels[k] == label and label[0] == cat and SM.CATS[k // 96] == cat
    assert [int(x) for x in out[384:]] == [flags["n"], flags["outside"], flags["range"]]
    assert int(out.sum()) == len(subs)


def test_every_mask_against_both_kinds_of_letter():
    want = {(0, "C"): "N", (0, "G"): "N", (1, "C"): "U", (1, "T"): "U", (1, "A"): "T", (1, "G"): "T", (2, "C"): "T",
            (2, "T"): "T", (2, "A"): "U", (2, "G"): "U", (3, "T"): "B", (3, "A"): "B"}
    for (mask, letter), cat in want.items():
        assert SM.CATS[SM.category(mask, letter)] == cat
    from himut_amd import strands
    for (mask, letter), cat in want.items():
        assert strands.CATEGORIES[strands.category_of(mask, letter in "AG")] == cat
    # a - gene with a + strand C gives T (chr1, position 14)
    assert ("T", "T:A[C>A]G") == K.CHR1_SUBS[9][3:]


def test_model_opportunity_counts():
    names = SM.tri_names()
    for seq, start, mask, want in ((K.CHR1, K.CHR1_SEG_START, K.CHR1_SEG_MASK, K.CHR1_OPP),
                                   (K.CHR2, K.CHR2_SEG_START, K.CHR2_SEG_MASK, K.CHR2_OPP)):
        got = SM.strand_tricounts(seq, start, mask)
        found = {(SM.CATS[c], names[t]): int(got[c, t]) for c in range(4) for t in range(32) if got[c, t]}
        assert found == want
    assert SM.tri_class(K.CHR1, 0) is None and SM.tri_class(K.CHR1, len(K.CHR1) - 1) is None


def test_segments_of_the_cases():
    from himut_amd import strands
    for genes, length, start, mask in ((K.CHR1_GENES, len(K.CHR1), K.CHR1_SEG_START, K.CHR1_SEG_MASK),
                                       (K.CHR2_GENES, len(K.CHR2), K.CHR2_SEG_START, K.CHR2_SEG_MASK)):
        s, m = strands.segments(genes, length)
        assert s.dtype == np.int32 and m.dtype == np.uint8
        assert s.tolist() == start and m.tolist() == mask
    assert strands.bases_per_mask(K.CHR1_SEG_START, K.CHR1_SEG_MASK, len(K.CHR1)) == K.CHR1_BASES_PER_MASK


def _covered(genes, length):
    plus, minus = np.zeros(length, bool), np.zeros(length, bool)
    for s, e, strand in genes:
        (plus if strand == "+" else minus)[max(s, 0):max(min(e, length), 0)] = True
    return plus.astype(np.uint8) | (minus.astype(np.uint8) << 1)


@pytest.mark.parametrize("seed", range(6))
def test_segments_invariants(seed):
    from himut_amd import strands
    import random
    rs = random.Random(seed)
    length = rs.choice((1, 2, 50, 333))
    genes = []
    for _ in range(rs.randrange(0, 12)):
        s = rs.randrange(-20, length + 20)
        genes.append((s, s + rs.randrange(-3, 80), rs.choice("+-")))
    start, mask = strands.segments(genes, length)
    assert start[0] == 0 and np.all(np.diff(start) > 0) and start[-1] < length and mask.max() <= 3
    per_base = mask[np.searchsorted(start, np.arange(length), side="right") - 1]
    assert np.array_equal(per_base, _covered(genes, length))
    assert sum(strands.bases_per_mask(start, mask, length)) == length


def test_a_contig_without_genes_is_one_segment():
    from himut_amd import strands
    start, mask = strands.segments([], 100)
    assert start.tolist() == [0] and mask.tolist() == [0]
    start, mask = strands.segments([(100, 200, "+"), (50, 50, "-"), (-9, 0, "+")], 100)     # all clipped away or empty
    assert start.tolist() == [0] and mask.tolist() == [0]
    start, mask = strands.segments([(90, 500, "-")], 100)                                   # reaches past the end
    assert start.tolist() == [0, 90] and mask.tolist() == [0, 2]


def test_read_genes_bed(tmp_path):
    from himut_amd import strands
    path = tmp_path / "genes.bed"
    path.write_text(K.bed_text())
    genes, unstranded = strands.read_genes(str(path))
    assert genes["chr1"] == K.CHR1_GENES and genes["chr2"] == K.CHR2_GENES and genes["chr9"] == [(5, 50, "+")]
    assert unstranded == {"chr1": 1}
    five = tmp_path / "five.bed"
    five.write_text("chr1\t0\t10\tg\t0\n")
    with pytest.raises(ValueError, match="six"):
        strands.read_genes(str(five))


def test_read_genes_gff(tmp_path):
    from himut_amd import strands
    for name in ("genes.gff3", "genes.gtf", "GENES.GFF"):
        path = tmp_path / name
        path.write_text(K.gff_text())
        genes, unstranded = strands.read_genes(str(path))
        assert genes["chr1"] == K.CHR1_GENES and genes["chr2"] == K.CHR2_GENES     # 1-based inclusive -> 0-based half-open
        assert genes["chr9"] == [(5, 50, "+")] and unstranded == {"chr1": 1}
    exons, _ = strands.read_genes(str(tmp_path / "genes.gff3"), feature="exon")
    assert exons["chr1"] == [(0, 3, "-"), (0, 3, "+"), (0, 3, "+"), (0, 3, "+"), (0, 3, "-")]
    short = tmp_path / "short.gff"
    short.write_text("chr1\tsrc\tgene\t1\t40\t.\t+\t.\n")
    with pytest.raises(ValueError, match="nine"):
        strands.read_genes(str(short))


def test_label_lists():
    from himut_amd import strands
    from himut_amd.normcounts import SBS96_LST
    assert len(strands.SBS384_LST) == 384 == len(set(strands.SBS384_LST))
    for c, cat in enumerate("TUBN"):
        assert strands.SBS384_LST[96 * c:96 * (c + 1)] == [cat + ":" + k for k in SBS96_LST]
    assert strands.SBS384_LST == SM.file_labels() and strands.SBS384_BIN_LST == SM.bin_labels()
    assert sorted(strands.SBS384_BIN_LST) == sorted(strands.SBS384_LST)
    assert strands.SBS192_LST == SM.file_labels()[:192] and all(k[0] in "TU" for k in strands.SBS192_LST)
    assert list(strands.TRI_NAMES) == SM.tri_names()
    assert strands.SBS384_BIN_LST[1 * 96 + 2 * 16 + 0 * 4 + 2] == "U:A[C>T]G"


def test_host_categories_match_the_model():
    from himut_amd import strands
    pos0, ref, _alt = _as_arrays(K.CHR1_SUBS)
    got = strands.sbs_categories(K.CHR1_SEG_START, K.CHR1_SEG_MASK, pos0, ref)
    assert [SM.CATS[c] for c in got.tolist()][:14] == [s[3] for s in K.CHR1_SUBS[:14]]


def test_subparsers():
    from himut_amd import parse_args
    parser = parse_args.build_parser("test")
    o = parser.parse_args(["sbs384", "-i", "a.vcf", "--ref", "r.fa", "--genes", "g.bed", "-o", "o.tsv"])
    assert (o.sub, o.feature, o.sbs192, o.opp, o.classes, o.devices) == ("sbs384", "gene", None, None, None, "0")
    o = parser.parse_args(["sbs384", "-i", "a.vcf", "--ref", "r.fa", "--genes", "g.gff3", "--feature", "mRNA", "-o", "o.tsv",
                           "--sbs192", "s.tsv", "--opp", "p.tsv", "--classes", "c.tsv", "--region", "chr1"])
    assert (o.feature, o.sbs192, o.opp, o.classes, o.region) == ("mRNA", "s.tsv", "p.tsv", "c.tsv", "chr1")
    with pytest.raises(SystemExit):
        parser.parse_args(["sbs384", "-i", "a.vcf", "--ref", "r.fa", "-o", "o.tsv"])          # --genes is required
    base = ["intervals", "-i", "a.bam", "--ref", "r.fa", "--bin_size", "100", "-o", "o.tsv"]
    _p, o = parse_args.parse_args("test", base)
    assert o.genes is None and o.strands is None and o.feature == "gene"
    _p, o = parse_args.parse_args("test", base + ["--genes", "g.bed", "--strands", "s.tsv"])
    assert (o.genes, o.strands) == ("g.bed", "s.tsv")
    for half in (["--genes", "g.bed"], ["--strands", "s.tsv"]):
        with pytest.raises(SystemExit):
            parse_args.parse_args("test", base + half)
    with pytest.raises(SystemExit):
        parse_args.parse_args("test", ["sbs384", "-i", "a.vcf", "--ref", "r.fa", "--genes", "g.bed", "-o", "o.tsv",
                                       "--region", "chr1", "--region_list", "l.txt"])


def test_abi_rows():
    from himut_amd import _ffi
    for name, n in (("himut_set_strands", 4), ("himut_sbs384_counts", 7), ("himut_strand_tricounts", 2),
                    ("himut_strand_callable", 3)):
        assert len(_ffi._ABI[name][1]) == n
    assert hasattr(_ffi.lib(), "himut_strand_callable") and _ffi.lib().himut_abi_version() == 2
