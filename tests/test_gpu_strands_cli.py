"""`himut sbs384` and `himut intervals --genes --strands` end to end.  The hand-written FASTA, VCF and genes of
tests/strands_cases.py through `sbs384` with a BED and with a GFF3, against the counts written down there; a contig the
FASTA lacks; a synthetic BAM through `intervals` with the strand tally, against the plain models; and `intervals`
without the new flags, against dump_intervals called the way it was called before they existed."""
import os

import numpy as np
import pytest

from tests import callmap_model as M
from tests import strands_cases as K
from tests import strands_model as SM
from tests import util

pytestmark = pytest.mark.gpu


def _write_inputs(tmp_path, extra_contig=False):
    paths = {k: str(tmp_path / n) for k, n in (("fa", "g.fa"), ("vcf", "calls.vcf"), ("bed", "genes.bed"), ("gff", "genes.gff3"))}
    for key, text in (("fa", K.fasta_text()), ("vcf", K.vcf_text(extra_contig)), ("bed", K.bed_text()), ("gff", K.gff_text())):
        with open(paths[key], "w") as o:
            o.write(text)
    return paths


def _expected_files():
    counts, _flags = K.expected_counts()
    opp = K.expected_opp()
    labels = SM.file_labels()
    main = ["sbs384\tcounts\n"] + ["{}\t{}\n".format(k, counts.get(k, 0)) for k in labels]
    half = ["sbs192\tcounts\n"] + ["{}\t{}\n".format(k, counts.get(k, 0)) for k in labels[:192]]
    opps = ["category\ttri\tref_count\n"] + ["{}\t{}\t{}\n".format(c, t, opp.get((c, t), 0)) for c in SM.CATS for t in SM.tri_names()]
    classes = ["chrom\tpos\tref\talt\tsbs384\n"]
    for chrom, subs in (("chr1", K.CHR1_SUBS), ("chr2", K.CHR2_SUBS)):
        classes += ["{}\t{}\t{}\t{}\t{}\n".format(chrom, p, r, a, label) for p, r, a, cat, label in subs if cat is not None]
    return main, half, opps, classes


def _log(path):
    rows = {}
    lines = open(path).read().splitlines()
    head = lines[0].split()
    for line in lines[1:]:
        cells = line.split()
        rows[cells[0]] = dict(zip(head, (int(x) for x in cells[1:])))
    return head, rows


@pytest.mark.parametrize("genes", ["bed", "gff"])
def test_sbs384_files(tmp_path, genes):
    from himut_amd import __main__ as cli
    p = _write_inputs(tmp_path)
    out, half, opp, classes = (str(tmp_path / n) for n in ("sbs384.tsv", "sbs192.tsv", "opp.tsv", "classes.tsv"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli.main(["sbs384", "-i", p["vcf"], "--ref", p["fa"], "--genes", p[genes], "-o", out, "--sbs192", half, "--opp", opp,
                  "--classes", classes])
        want = _expected_files()
        assert open(out).readlines() == want[0] and len(want[0]) == 385
        assert open(half).readlines() == want[1] and len(want[1]) == 193
        assert open(opp).readlines() == want[2] and len(want[2]) == 129
        assert open(classes).readlines() == want[3]
        head, rows = _log(str(tmp_path / "himut_sbs384.log"))
        assert head == ["chr1", "chr2", "total"]
        assert rows["num_genes"] == {"chr1": 5, "chr2": 1, "total": 6}
        assert rows["num_unstranded_genes"]["total"] == 1 and rows["num_genes_absent_contig"]["total"] == 0
        assert rows["num_segments"] == {"chr1": 8, "chr2": 3, "total": 11}
        assert [rows[k]["chr1"] for k in ("num_bases_no_gene", "num_bases_plus_gene", "num_bases_minus_gene",
                                          "num_bases_both")] == K.CHR1_BASES_PER_MASK
        assert rows["num_sbs"] == {"chr1": 16, "chr2": 6, "total": 22}
        counts, flags = K.expected_counts()
        for cat in "TUBN":
            assert rows["num_sbs_" + cat]["total"] == sum(v for k, v in counts.items() if k[0] == cat)
        for flag, row in K.FLAG_ROW.items():
            assert rows[row]["total"] == flags[flag]
        # the selection is `sbs96`'s: --region takes one contig
        cli.main(["sbs384", "-i", p["vcf"], "--ref", p["fa"], "--genes", p[genes], "-o", out, "--region", "chr2"])
        lines = open(out).readlines()
        assert sum(int(x.split("\t")[1]) for x in lines[1:]) == 3 and "T:T[C>T]A\t1\n" in lines
    finally:
        os.chdir(cwd)


def test_sbs384_contig_the_fasta_lacks(tmp_path, capsys):
    from himut_amd import __main__ as cli
    p = _write_inputs(tmp_path, extra_contig=True)
    out = str(tmp_path / "sbs384.tsv")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli.main(["sbs384", "-i", p["vcf"], "--ref", p["fa"], "--genes", p["bed"], "-o", out])
        assert open(out).readlines() == _expected_files()[0]
        assert "chr3" in capsys.readouterr().out
        head, rows = _log(str(tmp_path / "himut_sbs384.log"))
        assert head == ["chr1", "chr2", "chr3", "total"] and rows["num_sbs"]["chr3"] == 0 and rows["num_segments"]["chr3"] == 0
    finally:
        os.chdir(cwd)


def _sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=384, contig_len=24_000, depth=24, read_len_mean=5000, read_len_sd=1000,
                                            read_len_min=2000, read_len_max=9000, som_rate=4e-4, snp_rate=3e-3,
                                            name="chr7"), want_ref=True)


# every 400 bases a gene on + and a gene on - that overlap: stretches of mask 1, 3, 2 and 0 all over the contig, so that the
# callable positions, wherever the reads leave them, fall into every category; a one-base gene; one past the contig's end
GENES = [(a + k, a + k + w, strand) for a in range(0, 24_000, 400) for k, w, strand in ((0, 150, "+"), (100, 200, "-"))] + \
        [(350, 351, "-"), (23_990, 30_000, "+")]


def _per_base_segments(genes, length):
    per_base = np.zeros(length, np.uint8)
    for s, e, strand in genes:
        per_base[s:min(e, length)] |= 1 if strand == "+" else 2
    start = np.concatenate([[0], np.flatnonzero(np.diff(per_base)) + 1])
    return start.tolist(), per_base[start].tolist(), per_base


def test_intervals_strands_and_unchanged_files(tmp_path):
    from himut_amd import __main__ as cli
    from himut_amd import bamio, intervals, normcounts, parse_args
    from himut_amd import util as hutil
    s = _sample()
    text = bytes(s.ref).decode()
    n = len(text)
    bam, vcf, fa, regions, bed, genes = (str(tmp_path / x) for x in ("in.bam", "calls.vcf", "g.fa", "regions.txt", "t.bed", "genes.bed"))
    with open(regions, "w") as o:           # a chunk that starts inside a segment, a gap, a second chunk to the end
        o.write("chr7\t750\t10000\nchr7\t11000\t{}\n".format(n))
    with open(bed, "w") as o:
        o.write("chr7\t0\t{}\tall\nchr7\t9000\t12000\tseam\n".format(n))
    with open(genes, "w") as o:
        o.writelines("chr7\t{}\t{}\tg{}\t0\t{}\n".format(a, b, k, strand) for k, (a, b, strand) in enumerate(GENES))
        o.write("chrQ\t0\t10\telsewhere\t0\t+\n")
    with open(fa, "w") as o:
        o.write(">chr7\n" + "\n".join(text[i:i + 60] for i in range(0, n, 60)) + "\n")
    names = ("iv.tsv", "iv.tri.tsv", "iv.states.tsv")
    new, plain, old = ([str(tmp_path / (tag + x)) for x in names] for tag in ("new.", "plain.", "old."))
    strands_out, strands_nosbs = str(tmp_path / "strands.tsv"), str(tmp_path / "strands.nosbs.tsv")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [s.batch], sample="SMP")
        cli.main(["call", "-i", bam, "-o", vcf])
        lo, hi, md = normcounts.get_thresholds(vcf)
        p = dict(util.CALL_DEFAULTS, qlen_lower_limit=lo, qlen_upper_limit=hi, md_threshold=md)
        _chroms, chrom2chunks = hutil.load_loci(None, regions, {"chr7": n})
        chunks = [(int(a), int(b)) for (_c, a, b) in chrom2chunks["chr7"]]
        res = M.run(s.batch, text, chunks, p)
        start, mask, per_base = _per_base_segments(GENES, n)
        want_pos, want_bases = SM.strand_callable(res.state, res.bases, chunks, text, start, mask)
        assert int(want_pos.sum()) > 1000 and all(int(want_pos[c].sum()) > 0 for c in range(4))
        sbs = np.zeros((4, 32), np.int64)
        n_snvs = 0
        for line in open(vcf):
            f = line.rstrip("\n").split("\t")
            if not line.startswith("#") and f[6] == "PASS" and len(f[3]) == 1 and len(f[4]) == 1 and f[4] in "ACGT":
                pos = int(f[1]) - 1
                n_snvs += 1
                if SM.tri_class(text, pos) is not None:
                    sbs[SM.category(int(per_base[pos]), f[3]), SM.tri_class(text, pos)] += 1
        assert n_snvs >= 1
        base = ["intervals", "-i", bam, "--ref", fa, "--sbs", vcf, "--region_list", regions, "--bed", bed]
        # ---- with the strand tally
        cli.main(base + ["-o", new[0], "--tri", new[1], "--states", new[2], "--genes", genes, "--strands", strands_out])
        want = ["chrom\tcategory\ttri\tcallable_pos\tcallable_bases\tsbs\n"]
        for c, cat in enumerate(SM.CATS):
            for t, tri in enumerate(SM.tri_names()):
                want.append("chr7\t{}\t{}\t{}\t{}\t{}\n".format(cat, tri, want_pos[c, t], want_bases[c, t], sbs[c, t]))
        assert open(strands_out).readlines() == want
        # summed over the categories: the --tri file's line of the interval over the whole contig
        tri_lines = [x.rstrip("\n").split("\t") for x in open(new[1]) if x.startswith("chr7\t0\t{}\tall\t".format(n))]
        assert [int(x[6]) for x in tri_lines[:32]] == want_pos.sum(axis=0).tolist()
        assert [int(x[7]) for x in tri_lines[:32]] == want_bases.sum(axis=0).tolist()
        # ---- without the new flags, and through dump_intervals called as before them: the same bytes in all three files
        cli.main(base + ["-o", plain[0], "--tri", plain[1], "--states", plain[2]])
        po = parse_args.build_parser("test").parse_args(base + ["-o", old[0]])
        intervals.dump_intervals(
            po.bam, po.ref, po.bed, po.bin_size, po.sbs, po.vcf, po.phased_vcf, po.common_snps, po.panel_of_normals, po.region,
            po.region_list, po.min_qv, po.min_mapq, po.min_sequence_identity, po.min_gq, po.min_bq, po.min_trim,
            po.mismatch_window, po.max_mismatch_count, po.min_ref_count, po.min_alt_count, po.min_hap_count,
            po.somatic_snv_prior, po.germline_snv_prior, po.germline_indel_prior, po.threads, po.phase, po.non_human_sample,
            po.reference_sample, old[0], tri_file=old[1], states_file=old[2], devices=[0], cs_from_ref=po.cs_from_ref)
        for a, b, c in zip(new, plain, old):
            assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read() and os.path.getsize(a) > 0
        # ---- without --sbs: no sbs column; no thresholds from a header, the same map
        cli.main(["intervals", "-i", bam, "--ref", fa, "--region_list", regions, "--bin_size", "5000", "-o", plain[0],
                  "--genes", genes, "--strands", strands_nosbs])
        assert open(strands_nosbs).readlines() == [x.rsplit("\t", 1)[0] + "\n" for x in want]
        with pytest.raises(ValueError):
            intervals.dump_intervals(
                po.bam, po.ref, po.bed, po.bin_size, po.sbs, po.vcf, po.phased_vcf, po.common_snps, po.panel_of_normals,
                po.region, po.region_list, po.min_qv, po.min_mapq, po.min_sequence_identity, po.min_gq, po.min_bq,
                po.min_trim, po.mismatch_window, po.max_mismatch_count, po.min_ref_count, po.min_alt_count,
                po.min_hap_count, po.somatic_snv_prior, po.germline_snv_prior, po.germline_indel_prior, po.threads,
                po.phase, po.non_human_sample, po.reference_sample, old[0], genes_file=genes)
    finally:
        os.chdir(cwd)
