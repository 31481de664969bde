"""`himut duplex` end to end: a small by-strand BAM written by the package's own writer (the reads named
<movie>/<zmw>/ccs/fwd and .../rev) goes through the subcommand to the VCF, the --ss table and himut_duplex.log; the data
lines are the model's records (tests/duplex_model.py) rendered by the same writer, the table and the log's counters the
model's, the pairing counters what the names say."""
import os

import pytest

from tests import duplex_cases as C
from tests import duplex_model as M

pytestmark = pytest.mark.gpu


def test_duplex_end_to_end(tmp_path):
    from himut_amd import __main__ as cli
    from himut_amd import bamio, bamlib, duplex, util as U, vcflib
    b, mate, _chunks, _kw = C.random_case(41, n_mol=60, n_lone=25)
    bam, vcf, ss_tsv = (str(tmp_path / n) for n in ("bystrand.bam", "duplex.vcf", "ss.tsv"))
    sizes = {b.name: b.length}
    lo, hi, md = bamlib.get_thresholds({b.name: b}, [b.name], sizes)
    _chroms, chunks = U.load_loci(None, None, sizes)
    regions = [(x, y) for _c, x, y in chunks[b.name]]
    kw = dict(min_qv=25, min_mapq=20, qlen_lower_limit=lo, qlen_upper_limit=hi, min_sequence_identity=0.9, min_gq=5, min_bq=25,
              min_trim=0.05, max_mismatch_count=1, mismatch_window_size=10, md_threshold=md, min_ref_count=1, min_alt_count=1,
              min_hap_count=3)
    recs, ss, log = M.run(b, mate, regions, **kw)
    d = M.logd(log)
    assert len(recs) >= 5 and d["single"] > 0 and 0 < d["pairs_in_play"] < d["pairs"] and d["ds_bases"] > 0, d
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [b], sample="SMP", names=True)
        cli.main(["duplex", "-i", bam, "-o", vcf, "--ss", ss_tsv, "--min_qv", "25", "--min_mapq", "20", "--min_sequence_identity", "0.9",
                  "--min_gq", "5", "--min_bq", "25", "--min_trim", "0.05", "--max_mismatch_count", "1", "--mismatch_window_size", "10",
                  "--min_ref_count", "1"])
        text = open(vcf).read()
        body = vcflib.duplex_lines(b.name, recs)
        assert [l for l in text.splitlines(True) if not l.startswith("#")] == body
        assert "##himut_command=himut duplex -i {} ".format(bam) in text and "##INFO=<ID=DS," in text and "##pile=" in text
        assert text.splitlines()[-len(body) - 1].endswith("\tSMP")
        assert open(ss_tsv).read() == "class\tcount\n" + "".join("{}\t{}\n".format(c, x) for c, x in zip(M.SS_CLASSES, ss)) + \
            "ds_bases\t{}\nds_pairs_overlap\t{}\n".format(d["ds_bases"], d["ds_pairs_overlap"])
        rows = [l.split() for l in open("himut_duplex.log")]
        assert rows[0] == [b.name, "total"] and [r[0] for r in rows[1:]] == duplex.LOG_ROWS
        n_pair = int((mate >= 0).sum())
        assert [int(r[1]) for r in rows[1:]] == [n_pair, b.n - n_pair, 0, 0, 0] + log
    finally:
        os.chdir(cwd)
