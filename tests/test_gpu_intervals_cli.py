"""`himut intervals` end to end: a synthetic BAM through `call` (for the VCF: thresholds and substitutions), then
`intervals` with --bed and --sbs, and with --bin_size; the three files against the rows of the contract's model
(tests/intervals_model.py over tests/callmap_model.py) and the derived columns written out here; and `callable` on the
same inputs still writes the BED it wrote before."""
import os

import pytest

from tests import callmap_model as M
from tests import intervals_model as IM
from tests import util

pytestmark = pytest.mark.gpu


def _sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=72, contig_len=60_000, depth=30, read_len_mean=6000, read_len_sd=1200,
                                            read_len_min=2000, read_len_max=12000, som_rate=2e-4, snp_rate=3e-3,
                                            name="chr7"), want_ref=True)


def _pass_snvs(vcf):
    """0-based positions of the PASS, bi-allelic, single-base substitutions of a VCF, read here line by line."""
    out = []
    for line in open(vcf):
        if line.startswith("#"):
            continue
        f = line.rstrip("\n").split("\t")
        if f[6] == "PASS" and len(f[3]) == 1 and len(f[4]) == 1 and f[4] in "ACGT":
            out.append((f[0], int(f[1]) - 1, f[3]))
    return out


def _na(x):
    return "NA" if x is None else repr(x)


def _expected(intervals, mp, text, snvs):
    """(main, tri, states) lines for [(chrom, start, end, name)] on chr7."""
    main = ["chrom\tstart\tend\tname\tlength\tentries\tcallable_pos\tcallable_bases\tsbs\tsbs_uncallable\trate\tburden\n"]
    tri = ["chrom\tstart\tend\tname\ttri\tall_tri\tref_tri\tccs_tri\tsbs\n"]
    states = ["chrom\tstart\tend\tname\tstate\tpositions\tbases\n"]
    for chrom, s, e, name in intervals:
        r = mp.row(s, e)
        head = "{}\t{}\t{}\t{}".format(chrom, s, e, name)
        sbs = [0] * 33
        if snvs is not None:
            for c, p, ref in snvs:
                assert text[p].upper() == ref
                if c == chrom and s <= p < e:
                    sbs[IM.tri_class(text, p)] += 1
        ccs, al = [int(x) for x in r["ccs_tri"]], [int(x) for x in r["all_tri"]]
        n = sum(sbs)
        unc = sbs[32] + sum(sbs[c] for c in range(32) if ccs[c] == 0)
        denom = sum(ccs[:32])
        rate = burden = None
        if denom:
            rate = (n - unc) / denom
            burden = 0.0
            for c in range(32):
                if ccs[c] > 0:
                    burden += sbs[c] / ccs[c] * al[c]
            burden = 2 * burden
        tail = "NA\tNA\tNA\tNA" if snvs is None else "{}\t{}\t{}\t{}".format(n, unc, _na(rate), _na(burden))
        main.append("{}\t{}\t{}\t{}\t{}\t{}\n".format(head, max(e - s, 0), int(r["entries"]), int(r["positions"][13]),
                                                      int(r["bases"][13]), tail))
        for c in range(33):
            tri.append("{}\t{}\t{}\t{}\t{}\t{}\n".format(head, IM.TRI_NAMES[c], al[c], int(r["ref_tri"][c]), ccs[c],
                                                         "NA" if snvs is None else sbs[c]))
        for code, state in M.STATE_NAMES.items():
            if r["positions"][code]:
                states.append("{}\t{}\t{}\t{}\n".format(head, state, int(r["positions"][code]), int(r["bases"][code])))
    return main, tri, states


def test_bam_to_tsv(tmp_path):
    from himut_amd import __main__ as cli
    from himut_amd import bamio, normcounts
    from himut_amd import util as hutil
    s = _sample()
    bam, vcf, fa = str(tmp_path / "in.bam"), str(tmp_path / "calls.vcf"), str(tmp_path / "g.fa")
    out, tri, states, out2, tri2, states2, bed_out = (str(tmp_path / n) for n in (
        "iv.tsv", "iv.tri.tsv", "iv.states.tsv", "bins.tsv", "bins.tri.tsv", "bins.states.tsv", "callable.bed"))
    regions, bed = str(tmp_path / "regions.txt"), str(tmp_path / "targets.bed")
    with open(regions, "w") as o:           # two chunks that abut, a gap, a third chunk
        o.write("chr7\t100\t20000\nchr7\t20000\t45000\nchr7\t50000\t59000\n")
    with open(bed, "w") as o:               # out of order; one across the seam and the gap; one on a contig that is not swept
        o.write("# targets\ntrack name=targets\nchr7\t19000\t52000\tacross\nchr7\t0\t1500\nchrQ\t5\t500\tabsent\n"
                "chr7\t30000\t30001\tone\n")
    text = bytes(s.ref).decode()
    with open(fa, "w") as o:
        o.write(">chr7\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [s.batch], sample="SMP")
        cli.main(["call", "-i", bam, "-o", vcf])
        lo, hi, md = normcounts.get_thresholds(vcf)
        p = dict(util.CALL_DEFAULTS, qlen_lower_limit=lo, qlen_upper_limit=hi, md_threshold=md)
        _chroms, chrom2chunks = hutil.load_loci(None, regions, {"chr7": s.batch.length})
        chunks = [(int(a), int(b)) for (_c, a, b) in chrom2chunks["chr7"]]
        res = M.run(s.batch, text, chunks, p)
        mp = IM.Map.of(res, text)
        snvs = _pass_snvs(vcf)
        assert len(snvs) >= 1
        # ---- --bed with --sbs
        cli.main(["intervals", "-i", bam, "--ref", fa, "--sbs", vcf, "--region_list", regions, "--bed", bed, "-o", out,
                  "--tri", tri, "--states", states])
        want = _expected([("chr7", 19000, 52000, "across"), ("chr7", 0, 1500, "."), ("chr7", 30000, 30001, "one")], mp, text, snvs)
        assert open(out).readlines() == want[0]
        assert open(tri).readlines() == want[1]
        assert open(states).readlines() == want[2]
        across = want[0][1].split("\t")
        assert int(across[5]) == 1000 + 25000 + 2000 and int(across[6]) > 0 and across[10] != "NA"
        # ---- --bin_size, no --sbs: the thresholds computed as `himut call` computes them give the same map
        cli.main(["intervals", "-i", bam, "--ref", fa, "--region_list", regions, "--bin_size", "700", "-o", out2,
                  "--tri", tri2, "--states", states2])
        bins = [("chr7", a, min(a + 700, 60_000), "chr7:{}-{}".format(a, min(a + 700, 60_000))) for a in range(0, 60_000, 700)]
        assert bins[-1][2] == 60_000 and bins[-1][2] - bins[-1][1] == 60_000 % 700
        want = _expected(bins, mp, text, None)
        assert open(out2).readlines() == want[0]
        assert open(tri2).readlines() == want[1]
        assert open(states2).readlines() == want[2]
        assert sum(int(line.split("\t")[5]) for line in want[0][1:]) == res.state.shape[0]
        # ---- `callable` writes what it wrote before
        cli.main(["callable", "-i", bam, "--ref", fa, "--sbs", vcf, "--region_list", regions, "-o", bed_out])
        lines = ["chr7\t{}\t{}\t{}\t{}\n".format(a, b, M.STATE_NAMES[st], n) for a, b, st, n in M.merged_lines(res.runs)]
        assert open(bed_out).readlines() == lines
    finally:
        os.chdir(cwd)
