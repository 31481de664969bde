"""`himut sindels` end to end, in a fresh child process: a small BAM written by the package's own writer goes to VCF, and
the lines are the model's records rendered by the same writer (vcflib.sindel_lines), the log's counters the model's --
once with the text derived from CIGAR and the FASTA (--cs_from_ref), once under an error table (--error_table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import indelcal_model as IC
from tests import sindels_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sample():
    """(batch, contig string): 240 reads of 1,200 to 1,800 bases over a 20 kb contig; thirty pooled indels, some inside
    planted repeats, each in one read in eight that span it, and scattered one-read indels; a few reads of low quality."""
    from tests import indels_cases as C
    from tests import sindels_cases as SC
    rs = np.random.RandomState(98)
    n = 20_000
    at = [400 + 600 * k for k in range(30)]
    ref = C.contig(41, n, plant=[(p - 4, ("A" * 9, "CA" * 5, "GTT" * 3, "ACGTTGCA")[k % 4]) for k, p in enumerate(at)])
    pool = {p: (("D", 1 + k % 4) if k % 2 else ("I", ref[p:p + 1 + k % 3])) for k, p in enumerate(at)}
    recs = []
    for _ in range(240):
        length = int(rs.randint(1200, 1801))
        start = int(rs.randint(0, n - length))
        ins, dels = {}, {}
        for p, (kind, v) in pool.items():
            if start + 30 <= p <= start + length - 30 and rs.rand() < 0.125:
                (ins if kind == "I" else dels)[p] = v
        if rs.rand() < 0.6:
            p = start + 40 + int(rs.randint(0, length - 80))
            if all(abs(p - q) > 25 for q in pool):
                dels[p] = 1 + int(rs.randint(0, 3))
        recs.append(SC.read(ref, start, length, ins=ins, dels=dels, bq=int(rs.choice([40, 40, 40, 40, 25])),
                            qname="ccs/{}".format(len(recs))))
    return SC.batch(recs, n, name="chr9"), ref


def test_cli_sindels(tmp_path):
    from himut_amd import bamio, bamlib, util as U, vcflib
    from tests import cs_from_cigar
    b, seq = _sample()
    tagged, bare, fa, tsv = str(tmp_path / "t.bam"), str(tmp_path / "b.bam"), str(tmp_path / "g.fa"), str(tmp_path / "e.tsv")
    with open(fa, "w") as o:
        o.write(">chr9\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
    bamio.write_bam(tagged, [b], sample="SMP")
    cs_from_cigar.batch_bam(bare, b, "M", sample="SMP")
    sizes = {b.name: b.length}
    lo, hi, md = bamlib.get_thresholds({b.name: b}, [b.name], sizes)
    _chroms, chunks = U.load_loci(None, None, sizes)
    regions = [(x, y) for _c, x, y in chunks[b.name]]
    table, _log = IC.run(b, regions, seq)
    with open(tsv, "w") as o:
        o.writelines(IC.table_lines(table))
    l_hit, l_err = IC.error_logs(table, 0.01, min_spans=20)
    flags = ["--min_bq", "30", "--min_qv", "30", "--min_sequence_identity", "0.97", "--min_gq", "10", "--max_run", "3"]
    kw = dict(min_mapq=60, min_qv=30, qlen_lower_limit=lo, qlen_upper_limit=hi, min_sequence_identity=0.97, min_gq=10, min_bq=30,
              min_trim=0.01, max_mismatch_count=0, mismatch_window_size=20, md_threshold=md, min_ref_count=3, min_alt_count=1,
              max_len=50, max_run=3)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    bodies = []
    for name, bam, extra, tab in (("derived", bare, ["--cs_from_ref"], (None, None)),
                                  ("table", tagged, ["--error_table", tsv, "--min_spans", "20"], (l_hit, l_err))):
        recs, log = S.run(b, regions, seq, *tab, **kw)
        body = vcflib.sindel_lines("chr9", recs, seq)
        d = S.logd(log)
        assert len(body) >= 20 and d["proposing_reads"] < d["pile_reads"] and d["Repeat"] > 0 and d["PASS"] > 0, d
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([sys.executable, "-m", "himut_amd", "sindels", "-i", bam, "--ref", fa, "-o", str(d / "sindels.vcf")] + flags + extra,
                           cwd=str(d), env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        text = open(d / "sindels.vcf").read()
        assert [l for l in text.splitlines(True) if not l.startswith("#")] == body, name
        assert "##himut_command=himut sindels -i {} --ref {} ".format(bam, fa) in text
        assert text.splitlines()[-len(body) - 1].endswith("\tSMP") and "##candidates=not calls" in text
        assert ("##indel_error_table=" in text) == (name == "table")
        rows = [l.split() for l in open(d / "himut_sindels.log")]
        assert rows[0] == ["chr9", "total"] and [r[0] for r in rows[1:]] == vcflib.SINDEL_LOG_ROWS
        assert [int(r[1]) for r in rows[1:]] == log
        bodies.append(body)
    assert bodies[0] != bodies[1]                                # the table moves a gq or a verdict
