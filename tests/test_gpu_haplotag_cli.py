"""`himut haplotag` end to end: a synthetic BAM and its phased VCF through the subcommand, with and without
--cs_from_ref; the TSV per read, the --snps file and himut_haplotag.log against the lines the contract's model
(tests/haplotag_model.py) gives for the same reads and hetSNPs."""
import os

import numpy as np
import pytest

from tests import cs_from_cigar as CC
from tests import haplotag_model as M

pytestmark = pytest.mark.gpu


def _sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=72, contig_len=50_000, depth=30, read_len_mean=6000, read_len_sd=1200,
                                            read_len_min=2000, read_len_max=12000, snp_rate=3e-3, frac_softclip=0.3,
                                            softclip_max=100, name="chr7"), want_ref=True)


def _expected(batch, vcf, **kw):
    """(the read TSV, the hetSNP TSV, the log's counters) the model gives for the VCF's hetSNPs of the batch's contig."""
    from himut_amd import haplotag
    s = haplotag.load_phased(vcf, [batch.name], {batch.name: batch.length})[0][batch.name]
    rows, snp_rows, log = M.haplotag(batch, s.tuples(), **kw)
    reads = "\t".join(M.READ_COLUMNS) + "\n" + "".join(x + "\n" for x in M.read_lines(batch.name, batch, rows, s.names))
    snps = "\t".join(M.SNP_COLUMNS) + "\n" + "".join(x + "\n" for x in M.snp_lines(batch.name, s.tuples(), snp_rows, s.names))
    derived = [len(snp_rows), int(np.sum(M.depth(snp_rows) > 0)), int(np.sum(snp_rows["disagree"] > snp_rows["agree"]))]
    return reads, snps, log + derived


def _log_text(names, chrom, values):
    return "{:30}{}\n".format("", "\t".join([chrom, "total"])) + "".join(
        "{:30}{}\n".format(n, "\t".join([str(v), str(v)])) for n, v in zip(names, values))


def test_haplotag_end_to_end(tmp_path, capsys):
    from himut_amd import __main__ as cli
    from himut_amd import bamio, haplotag, synth
    s = _sample()
    bam, vcf, tsv, snp_tsv = (str(tmp_path / n) for n in ("in.bam", "phased.vcf", "reads.tsv", "snps.tsv"))
    fa = str(tmp_path / "g.fa")
    with open(fa, "w") as o:
        text = bytes(s.ref).decode()
        o.write(">chr7\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [s.batch], sample="SMP")
        synth.write_phased_vcf(vcf, s, block=30)
        cli.main(["haplotag", "-i", bam, "--phased_vcf", vcf, "-o", tsv, "--snps", snp_tsv])
        reads, snps, log = _expected(s.batch, vcf)
        got = open(tsv).read()
        assert got == reads and open(snp_tsv).read() == snps
        assert open("himut_haplotag.log").read() == _log_text(haplotag.LOG_ROWS, "chr7", log)
        body = [line.split("\t") for line in got.splitlines()[1:]]
        assert len(body) == s.batch.n and {f[7] for f in body} >= {"1", "2"} and {f[4] for f in body} <= {"+", "-"}
        assert all(f[1].startswith("ccs/") for f in body) and log[2] > 0 and log[3] > 0

        # other thresholds, no --snps file
        os.remove(snp_tsv)
        cli.main(["haplotag", "-i", bam, "--phased_vcf", vcf, "-o", tsv, "--min_mapq", "60", "--min_bq", "93", "--min_snps", "3",
                  "--min_agree", "0.95"])
        reads_hi, _snps, log_hi = _expected(s.batch, vcf, min_mapq=60, min_bq=93, min_snps=3, min_agree_permille=950)
        assert open(tsv).read() == reads_hi != reads and not os.path.exists(snp_tsv)
        assert open("himut_haplotag.log").read() == _log_text(haplotag.LOG_ROWS, "chr7", log_hi)

        # a BAM without cs tags: the text derived from CIGAR, SEQ and the reference gives the same lines
        bare = str(tmp_path / "bare.bam")
        CC.batch_bam(bare, s.batch, "EQX", sample="SMP")
        cli.main(["haplotag", "-i", bare, "--phased_vcf", vcf, "-o", tsv, "--snps", snp_tsv, "--ref", fa, "--cs_from_ref"])
        assert open(tsv).read() == reads and open(snp_tsv).read() == snps

        # a VCF that names a contig the BAM lacks: reported and skipped
        other = str(tmp_path / "other.vcf")
        with open(other, "w") as o:
            o.write(open(vcf).read() + "chrZ\t5\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0|1:5\n")
        capsys.readouterr()
        cli.main(["haplotag", "-i", bam, "--phased_vcf", other, "-o", tsv, "--snps", snp_tsv])
        assert "contig chrZ" in capsys.readouterr().out and open(tsv).read() == reads and open(snp_tsv).read() == snps

        # two contigs, the larger one second: each contig's lines are written as it finishes, in the order of the target list
        small = synth.generate(synth.SynthConfig(seed=73, contig_len=20_000, depth=20, read_len_mean=6000, read_len_sd=1200,
                                                 read_len_min=2000, read_len_max=12000, snp_rate=3e-3, name="chr3"))
        bam2, vcf3, vcf2 = str(tmp_path / "two.bam"), str(tmp_path / "chr3.vcf"), str(tmp_path / "two.vcf")
        bamio.write_bam(bam2, [small.batch, s.batch], sample="SMP")
        synth.write_phased_vcf(vcf3, small, block=30)
        with open(vcf2, "w") as o:
            o.write(open(vcf3).read() + "".join(x for x in open(vcf) if not x.startswith("#")))
        order = haplotag.dump_haplotags(bam2, vcf2, None, None, 0, 20, 1, 800, 1, tsv, snps_file=snp_tsv)
        assert sorted(order) == ["chr3", "chr7"]
        parts = {"chr3": _expected(small.batch, vcf2), "chr7": (reads, snps, log)}
        for path, k in ((tsv, 0), (snp_tsv, 1)):
            want = parts[order[0]][k] + "".join(parts[order[1]][k].splitlines(True)[1:])
            assert open(path).read() == want
        totals = [a + b for a, b in zip(parts[order[0]][2], parts[order[1]][2])]
        assert open("himut_haplotag.log").read().splitlines()[1].split() == ["num_reads"] + [str(parts[c][2][0]) for c in order] + [str(totals[0])]
    finally:
        os.chdir(cwd)
