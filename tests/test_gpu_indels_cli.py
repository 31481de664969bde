"""`himut indels` end to end: a small BAM written by the package's own writer goes to VCF, and the text is the text the
model's records give -- once with the cs tags of the file, once with the text derived from CIGAR and the FASTA
(--cs_from_ref)."""
import os

import numpy as np
import pytest

from tests import indels_model as M

pytestmark = pytest.mark.gpu


def _sample():
    """(batch, contig string): 240 reads of 1,500 bases over a 20 kb contig; thirty indels, some inside planted repeats,
    each in about half of the reads that span it, and scattered one-read indels."""
    from tests import indels_cases as C
    rs = np.random.RandomState(97)
    n = 20_000
    at = [400 + 600 * k for k in range(30)]
    ref = C.contig(31, n, plant=[(p - 4, ("A" * 9, "CA" * 5, "GTT" * 3, "ACGTTGCA")[k % 4]) for k, p in enumerate(at)])
    pool = {p: (("D", 1 + k % 4) if k % 2 else ("I", ref[p:p + 1 + k % 3])) for k, p in enumerate(at)}
    recs = []
    for _ in range(240):
        start = int(rs.randint(0, n - 1500))
        ins, dels = {}, {}
        for p, (kind, v) in pool.items():
            if start + 10 <= p <= start + 1480 and rs.rand() < 0.5:
                (ins if kind == "I" else dels)[p] = v
        if rs.rand() < 0.5:
            p = start + 30 + 600 * int(rs.randint(0, 2)) + int(rs.randint(0, 200))
            if all(abs(p - q) > 20 for q in pool):
                dels[p] = 1
        recs.append(C.read(ref, start, 1500, ins=ins, dels=dels, qname="ccs/{}".format(len(recs))))
    return C.batch(recs, n, name="chr9"), ref


def test_cli_indels(tmp_path):
    from himut_amd import __main__ as cli
    from himut_amd import bamio, bamlib, util as U
    from tests import cs_from_cigar
    b, seq = _sample()
    tagged, bare, fa = str(tmp_path / "t.bam"), str(tmp_path / "b.bam"), str(tmp_path / "g.fa")
    with open(fa, "w") as o:
        o.write(">chr9\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
    bamio.write_bam(tagged, [b], sample="SMP")
    cs_from_cigar.batch_bam(bare, b, "M", sample="SMP")
    sizes = {b.name: b.length}
    _lo, _hi, md = bamlib.get_thresholds({b.name: b}, [b.name], sizes)
    _chroms, chunks = U.load_loci(None, None, sizes)
    flags = ["--min_alt_count", "1", "--min_gq", "5"]
    recs, log = M.run(b, [(x, y) for _c, x, y in chunks[b.name]], seq, md_threshold=md, min_alt_count=1, min_gq=5)
    body = M.vcf_lines("chr9", recs, seq)
    assert len(body) >= 25 and log[0] > 300 and log[6] > 50
    cwd = os.getcwd()
    for name, bam, extra in (("tags", tagged, []), ("derived", bare, ["--cs_from_ref"])):
        d = tmp_path / name
        d.mkdir()
        os.chdir(d)
        try:
            cli.main(["indels", "-i", bam, "--ref", fa, "-o", str(d / "indels.vcf")] + flags + extra)
        finally:
            os.chdir(cwd)
        text = open(d / "indels.vcf").read()
        assert [l for l in text.splitlines(True) if not l.startswith("#")] == body, name
        assert "##himut_command=himut indels -i {} --ref {} ".format(bam, fa) in text
        assert text.splitlines()[-len(body) - 1].endswith("\tSMP") and "one line per allele" in text
        rows = [l.split() for l in open(d / "himut_indels.log")]
        assert rows[0] == ["chr9", "total"] and [int(r[1]) for r in rows[1:]] == log
