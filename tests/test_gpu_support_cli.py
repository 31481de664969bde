"""`himut support` end to end: a synthetic BAM through `call`, then `support` on that VCF; the TSV against the text the
contract's model (tests/support_model.py) and the formatter give for the same reads and sites."""
import os

import pytest

from tests import cs_from_cigar as C
from tests import support_model as M

pytestmark = pytest.mark.gpu


def _sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=71, contig_len=50_000, depth=30, read_len_mean=6000, read_len_sd=1200,
                                            read_len_min=2000, read_len_max=12000, som_rate=2e-4, hetalt_frac=0.3,
                                            snp_rate=3e-3, frac_softclip=0.3, softclip_max=100, name="chr7"), want_ref=True)


def _expected(batch, vcf, all_filters=False, **kw):
    from himut_amd import support
    sites, _skipped = support.load_sites(vcf, all_filters)
    sites = sites[batch.name]
    rows, counts = M.support(batch, [s[:3] for s in sites], **kw)
    lines = support.format_rows(batch.name, sites, rows, counts, lambda _i, qid: "ccs/{}".format(qid))
    return "\t".join(support.COLUMNS) + "\n" + "".join(line + "\n" for line in lines), sites


def test_call_then_support(tmp_path, capsys):
    from himut_amd import __main__ as cli
    from himut_amd import bamio
    s = _sample()
    bam, vcf, tsv = str(tmp_path / "in.bam"), str(tmp_path / "calls.vcf"), str(tmp_path / "support.tsv")
    fa = str(tmp_path / "g.fa")
    with open(fa, "w") as o:
        text = bytes(s.ref).decode()
        o.write(">chr7\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [s.batch], sample="SMP")
        cli.main(["call", "-i", bam, "-o", vcf])
        cli.main(["support", "-i", bam, "--sbs", vcf, "-o", tsv])
        want, sites = _expected(s.batch, vcf)
        got = open(tsv).read()
        assert got == want
        body = [line.split("\t") for line in got.splitlines()[1:]]
        assert len(sites) > 5 and all(f[4] == "PASS" and f[7].startswith("ccs/") and int(f[5]) >= 1 for f in body)
        assert {f[8] for f in body} <= {"+", "-"}

        # every FILTER: a superset, with the HetAltSite line as one site per allele
        cli.main(["support", "-i", bam, "--sbs", vcf, "-o", tsv, "--all_filters", "--min_mapq", "20",
                  "--mismatch_window_size", "7"])
        want_all, sites_all = _expected(s.batch, vcf, True, min_mapq=20, mismatch_window_size=7)
        got_all = open(tsv).read()
        assert got_all == want_all
        assert set(sites) < set(sites_all)
        hetalt = [line.split("\t") for line in open(vcf) if not line.startswith("#") and "," in line.split("\t")[4]]
        assert hetalt
        for f in hetalt:
            for alt in f[4].split(","):
                assert (int(f[1]), f[3], alt, f[6]) in sites_all
                assert "chr7\t{}\t{}\t{}\tHetAltSite\t".format(f[1], f[3], alt) in got_all

        # a BAM without cs tags: the text derived from CIGAR, SEQ and the reference gives the same rows
        bare = str(tmp_path / "bare.bam")
        C.batch_bam(bare, s.batch, "EQX", sample="SMP")
        with pytest.raises(KeyError):
            cli.main(["support", "-i", bare, "--sbs", vcf, "-o", tsv])
        cli.main(["support", "-i", bare, "--sbs", vcf, "-o", tsv, "--ref", fa, "--cs_from_ref"])
        assert open(tsv).read() == want

        # a VCF that names a contig the BAM lacks: skipped with a message
        other = str(tmp_path / "other.vcf")
        with open(other, "w") as o:
            o.write(open(vcf).read() + "chrZ\t5\t.\tA\tC\t.\tPASS\t.\tGT\t./.\n")
        capsys.readouterr()
        cli.main(["support", "-i", bam, "--sbs", other, "-o", tsv])
        assert "contig chrZ" in capsys.readouterr().out and open(tsv).read() == want
    finally:
        os.chdir(cwd)


def test_read_names_by_ordinal(tmp_path):
    from himut_amd import _ffi, bamio
    s = _sample()
    bam = str(tmp_path / "in.bam")
    bamio.write_bam(bam, [s.batch], sample="SMP")
    stream = bamio.BamStream(bam)
    with _ffi.Context(0) as ctx:
        res = stream.ingest_contig(ctx, "chr7", keep_names=True)
        assert res["n_reads"] == s.batch.n
        assert [stream.read_name(i) for i in range(s.batch.n)] == [s.batch.query_name(i) for i in range(s.batch.n)]
        with pytest.raises(LookupError):
            stream.read_name(s.batch.n)
        stream.ingest_contig(ctx, "chr7")
        with pytest.raises(LookupError):
            stream.read_name(0)
    stream.close()
