"""`himut callable` end to end: a synthetic BAM through `call` (for the thresholds in its VCF header), then `callable` with
and without --sbs; the BED against the merged runs of the contract's model (tests/callmap_model.py), --callable_only
against its CALLABLE lines, the --summary totals and the log against the counters."""
import os

import numpy as np
import pytest

from tests import callmap_model as M
from tests import util

pytestmark = pytest.mark.gpu


def _sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=72, contig_len=60_000, depth=30, read_len_mean=6000, read_len_sd=1200,
                                            read_len_min=2000, read_len_max=12000, som_rate=2e-4, snp_rate=3e-3,
                                            name="chr7"), want_ref=True)


def test_bam_to_bed(tmp_path):
    from himut_amd import __main__ as cli
    from himut_amd import bamio, normcounts
    from himut_amd import util as hutil
    s = _sample()
    bam, vcf, fa = str(tmp_path / "in.bam"), str(tmp_path / "calls.vcf"), str(tmp_path / "g.fa")
    bed, bed2, only, summary = (str(tmp_path / n) for n in ("callable.bed", "nosbs.bed", "only.bed", "summary.tsv"))
    regions = str(tmp_path / "regions.txt")
    with open(regions, "w") as o:           # two chunks that abut (one BED line across the seam), a gap, a third chunk
        o.write("chr7\t100\t20000\nchr7\t20000\t45000\nchr7\t50000\t59000\n")
    text = bytes(s.ref).decode()
    with open(fa, "w") as o:
        o.write(">chr7\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [s.batch], sample="SMP")
        cli.main(["call", "-i", bam, "-o", vcf])
        cli.main(["callable", "-i", bam, "--ref", fa, "--sbs", vcf, "--region_list", regions, "-o", bed, "--summary", summary])
        # the model under the thresholds of the VCF header and the chunks the drivers cut a contig into
        lo, hi, md = normcounts.get_thresholds(vcf)
        p = dict(util.CALL_DEFAULTS, qlen_lower_limit=lo, qlen_upper_limit=hi, md_threshold=md)
        _chroms, chrom2chunks = hutil.load_loci(None, regions, {"chr7": s.batch.length})
        chunks = [(int(a), int(b)) for (_c, a, b) in chrom2chunks["chr7"]]
        res = M.run(s.batch, text, chunks, p)
        lines = M.merged_lines(res.runs)
        want = ["chr7\t{}\t{}\t{}\t{}\n".format(a, b, M.STATE_NAMES[st], n) for a, b, st, n in lines]
        got = open(bed).readlines()
        assert got == want
        assert len(chunks) == 3 and len(want) < res.runs.shape[0]          # the seam at 20,000 lies inside one line
        assert not any(45000 <= int(f.split("\t")[1]) < 50000 for f in want)
        assert len(want) >= 3 and {f.split("\t")[3] for f in want} >= {"CALLABLE", "NO_BASE"}
        # the thresholds computed as `himut call` computes them: the same lines
        cli.main(["callable", "-i", bam, "--ref", fa, "--region_list", regions, "-o", bed2])
        assert open(bed2).readlines() == want
        cli.main(["callable", "-i", bam, "--ref", fa, "--sbs", vcf, "--region_list", regions, "-o", only, "--callable_only"])
        assert open(only).readlines() == [line for line in want if line.split("\t")[3] == "CALLABLE"]
        # the summary: positions and bases per state; the log file: the counters
        rows = [line.rstrip("\n").split("\t") for line in open(summary).readlines()[1:]]
        assert all(r[0] == "chr7" for r in rows)
        by_state = {r[1]: (int(r[2]), int(r[3])) for r in rows}
        code = {name: c for c, name in M.STATE_NAMES.items()}
        assert sum(n for n, _b in by_state.values()) == sum(b - a for a, b in chunks)
        for name, (npos, nbases) in by_state.items():
            assert npos == int(np.count_nonzero(res.state == code[name]))
            if code[name] >= 2:
                assert nbases == res.log[code[name]]
        assert sum(b for _n, b in by_state.values()) == res.log[1]
        log_rows = {line[:30].strip(): line[30:].split("\t") for line in open(tmp_path / "callable.log").readlines()[1:]}
        assert [int(log_rows[name][0]) for name in normcounts.NORM_LOG_ROWS] == res.log
    finally:
        os.chdir(cwd)
