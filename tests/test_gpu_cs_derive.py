"""The ingest that derives the cs text itself (himut_ingest_derive_cs; k_cs_measure / k_cs_emit of csrc/himut_ingest.h;
DESIGN 11): BAM files without cs:Z tags, in M-form and in =/X-form CIGAR, must leave the context exactly as the same
reads with tags do.  The expected texts come from tests/cs_from_cigar.py (the rule in plain Python, itself held to
hand-written texts and to the synthetic generator's tags by tests/test_cs_derive_cpu.py)."""
import os

import numpy as np
import pytest

from tests import bam_spec
from tests import cs_from_cigar as C
from tests import util

pytestmark = pytest.mark.gpu

FIELDS = ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "qid", "qoff", "cs_off", "seq", "bq", "cs", "tp")


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _same(a, b, fields=FIELDS):
    assert a.n == b.n
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and np.array_equal(x, y), k


def _ingest(worker, path, chrom, ref=None, window=None):
    """The read batch the device holds after ingesting ``chrom`` of ``path``; with ``ref`` the cs text is derived."""
    from himut_amd import bamio
    st = bamio.BamStream(path, threads=3)
    try:
        if ref is not None:
            bamio.set_contig_reference(worker.ctx, ref)
        res = st.ingest_contig(worker.ctx, chrom, window_bytes=window, derive_cs=ref is not None)
        d = worker.ctx.ingest_derive_result()
        if ref is not None:
            assert res["n_missing_cs"] == 0
            assert (d["n_derived"], d["n_underivable"], d["cs_bytes"]) == (res["n_reads"], 0, res["cs_bytes"])
        else:
            assert (d["n_derived"], d["n_underivable"], d["cs_bytes"]) == (0, 0, 0)
        return worker.ctx.download_reads(res, chrom, st.tname2tsize[chrom])
    finally:
        st.close()


# ---- 1. records written by hand

def test_hand_records(worker, tmp_path):
    tagged, bare = str(tmp_path / "tagged.bam"), str(tmp_path / "bare.bam")
    want = C.hand_bam(tagged, True)
    assert C.hand_bam(bare, False) == want
    cases = C.hand_cases()
    n_literal = 0
    for contig, (name, ref) in enumerate((("hand", C.hand_reference()), ("long", C.long_reference()))):
        got = _ingest(worker, bare, name, ref)
        mine = [c for c in cases if c[0] == contig]
        assert got.n == len(mine) == len(want[contig])
        texts = [bytes(got.cs[int(got.cs_off[i]):int(got.cs_off[i + 1])]).decode() for i in range(got.n)]
        for i, (case, text) in enumerate(zip(mine, texts)):
            assert text == want[contig][i], (case[1], case[2])
            if case[4] is not None:
                assert text == case[4], (case[1], case[2])
                n_literal += 1
            if case[5] == "":
                assert len(text) == 3 * len(case[3])
        assert int(got.cs_off[-1]) == sum(len(t) for t in want[contig]) == got.cs.shape[0]
        # every array equals what the ingest gives on the same records with tags, without the derivation
        _same(got, _ingest(worker, tagged, name))
    assert n_literal >= 6
    # the file without tags is refused without the derivation, as before (the record with a tag of its own is not counted)
    with pytest.raises(KeyError) as e:
        _ingest(worker, bare, "long")
    assert "tag 'cs' not present in 3 records" in str(e.value)


# ---- 2. synthetic parity, 3. window geometry

def _synth_files(tmp_path, s):
    from himut_amd import bamio
    a, b, c = (str(tmp_path / n) for n in ("a.bam", "b.bam", "c.bam"))
    bamio.write_bam(a, [s.batch])
    C.batch_bam(b, s.batch, "M")
    C.batch_bam(c, s.batch, "EQX")
    return a, b, c


def _downstream(worker, s):
    """What the three pipelines make of the resident reads: call records and counters, normcounts histograms and log,
    phase edge counts on the sample's hetSNPs."""
    from himut_amd import normcounts, phaselib, util as hutil
    b = s.batch
    chunks = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=1800, qlen_upper_limit=4500, md_threshold=30)
    worker.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"],
                     p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"],
                     p["md_threshold"], p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"],
                     False)
    het = (s.snp_gt == 1) | (s.snp_gt == 2)
    hpos, href = (s.snp_pos[het] + 1).astype(np.int32), s.snp_ref[het]
    edges = worker.ctx.run_edges(hpos, href, 40, 20, phaselib.edge_band(b, hpos))
    recs, log = worker.call_resident(chunks)
    ccs, rf, nlog = normcounts.norm_contig(worker, None, chunks, bytes(s.ref))
    return recs, log, ccs, rf, nlog, edges


@pytest.mark.parametrize("rates", C.SYNTH_RATES)
@pytest.mark.parametrize("seed", C.SYNTH_SEEDS)
def test_synthetic_parity(worker, tmp_path, seed, rates):
    s = C.synth_sample(seed, rates)
    ref = bytes(s.ref)
    a, b, c = _synth_files(tmp_path, s)
    base = _ingest(worker, a, "chrD")
    _same(base, s.batch)                                  # no read is left out
    down = _downstream(worker, s) if rates == C.SYNTH_RATES[0] else None
    if down is not None:
        assert len(down[0]) > 0 and down[4][13] > 0 and int(down[5].sum()) > 0
    for path in (a, b, c):
        _same(_ingest(worker, path, "chrD", ref), base)
        if down is not None:
            got = _downstream(worker, s)
            assert got[1] == down[1] and np.array_equal(got[0], down[0]), path
            assert got[2] == down[2] and got[3] == down[3] and got[4] == down[4], path
            assert np.array_equal(got[5], down[5]), path


def test_small_windows(worker, tmp_path, monkeypatch):
    """Records and the CIGAR side array straddle windows: the same files through 96 KB windows (the environment's
    setting, what the command line uses)."""
    s = C.synth_sample(C.SYNTH_SEEDS[1], C.SYNTH_RATES[1])
    a, b, c = _synth_files(tmp_path, s)
    base = _ingest(worker, a, "chrD")
    monkeypatch.setenv("HIMUT_INGEST_WINDOW_KB", "96")
    for path in (a, b, c):
        _same(_ingest(worker, path, "chrD", bytes(s.ref)), base)


def test_cigar_bytes_beyond_sequence_and_tag_bytes(worker, tmp_path):
    """3000 reads of 40 bases, `20=` and twenty times `1=`, no auxiliary field: a window's CIGAR bytes exceed its
    auxiliary bytes (none) and its SEQ bytes, so the side array must be sized by what the host counted, not guessed."""
    rs = np.random.RandomState(5)
    ref = bytes(rs.choice(np.frombuffer(b"ACGT", np.uint8), 40_000))
    cigar = [(20, C.EQ)] + [(1, C.EQ)] * 20
    recs, want = [], []
    for k in range(3000):
        pos = k * 13
        seq = bytearray(ref[pos:pos + 40])
        if k % 7 == 3:
            seq[k % 40] = ord(C._COMP[chr(seq[k % 40])])
        codes = [bam_spec.NIBBLES.index(chr(ch)) for ch in seq]
        want.append(C.derive_cs(cigar, pos, codes, ref))
        recs.append(bam_spec.record(0, pos, "s{}".format(k), 60, 0, cigar, codes, bytes([50] * 40), b""))
    path = str(tmp_path / "short.bam")
    bam_spec.write_bgzf(path, bam_spec.header([("chrS", 40_000)], "syn") + b"".join(recs))
    for window in (96 << 10, None):
        got = _ingest(worker, path, "chrS", ref, window)
        assert got.n == 3000 and bytes(got.cs).decode() == "".join(want)
        assert np.array_equal(got.cs_off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert want[0] == ":40" and sum(w != ":40" for w in want) > 400


# ---- 4. refusals

def _refusal_records():
    good = lambda pos: ("10M", pos, "ACGTACGTAC", {})                               # noqa: E731
    return {
        "no_cigar": ([good(10), ("", 20, "ACGTA", {}), good(30), ("", 40, "AC", {})], 2),
        "n_or_p_op": ([("5M10N5M", 10, "ACGTACGTAC", {}), good(20), ("5M1P5M", 30, "ACGTACGTAC", {}),
                       ("1S2M70000N2M", 40, "ACGTA", {})], 3),
        "lengths_disagree": ([good(10), ("5M", 20, "ACGTAC", {}), ("3S5M", 30, "ACGTACG", {}), ("4M2I", 40, "ACGTA", {})], 3),
        "leaves_the_reference": ([good(10), ("5M10D5M", 4985, "ACGTACGTAC", {}), good(4990), ("10M", 4991, "ACGTACGTAC", {})], 2),
    }


@pytest.mark.parametrize("kind", sorted(_refusal_records()))
def test_underivable_records_are_counted_and_refused(worker, tmp_path, kind):
    from himut_amd import bamio
    from himut_amd.caller import Worker
    rows, n_bad = _refusal_records()[kind]
    ref = C.hand_reference()
    recs = [bam_spec.record(0, pos, "u{}".format(k), 60, 0, cigar, seq, bytes([40] * len(seq)), b"")
            for k, (cigar, pos, seq, _kw) in enumerate(rows)]
    path = str(tmp_path / (kind + ".bam"))
    bam_spec.write_bgzf(path, bam_spec.header([("hand", 5000)], "syn") + b"".join(recs))
    for k, (cigar, pos, seq, _kw) in enumerate(rows):
        codes = [bam_spec.NIBBLES.index(ch) for ch in seq]
        assert (C.derive_cs(cigar, pos, codes, ref) is None) == (k in _bad_rows(kind)), (kind, k)
    st = bamio.BamStream(path)
    bamio.set_contig_reference(worker.ctx, ref)
    with pytest.raises(ValueError) as e:
        st.ingest_contig(worker.ctx, "hand", derive_cs=True)
    assert "{}: cs cannot be derived for {} records of hand (".format(path, n_bad) in str(e.value)
    d = worker.ctx.ingest_derive_result()
    assert (d["n_derived"], d["n_underivable"]) == (len(rows) - n_bad, n_bad)
    st.close()
    # the pinned windows are free again: another context opens an ingest, and this one ingests a good file
    other = Worker(0)
    try:
        other.ctx.ingest_begin(0, 1 << 16)
        other.ctx.ingest_end(True)
    finally:
        other.close()
    s = C.synth_sample(C.SYNTH_SEEDS[0], C.SYNTH_RATES[0])
    good = str(tmp_path / "b.bam")
    C.batch_bam(good, s.batch, "M")
    _same(_ingest(worker, good, "chrD", bytes(s.ref)), s.batch)


def _bad_rows(kind):
    return {"no_cigar": (1, 3), "n_or_p_op": (0, 2, 3), "lengths_disagree": (1, 2, 3), "leaves_the_reference": (1, 3)}[kind]


def test_derivation_needs_a_reference():
    from himut_amd._ffi import HimutError
    from himut_amd.caller import Worker
    w = Worker(0)
    try:
        with pytest.raises(HimutError) as e:
            w.ctx.ingest_derive_cs(1)
        assert e.value.code == 1                                                  # HIMUT_ERR_ARG
        w.ctx.ingest_derive_cs(0)
    finally:
        w.close()


# ---- 5. command line

def test_call_with_cs_from_ref_writes_the_vcf_of_the_tagged_file(tmp_path):
    from himut_amd import __main__ as cli
    from himut_amd import bamio
    s = C.synth_sample(C.SYNTH_SEEDS[0], C.SYNTH_RATES[0])
    bam, fa, out = str(tmp_path / "in.bam"), str(tmp_path / "g.fa"), str(tmp_path / "out.vcf")
    with open(fa, "w") as o:
        text = bytes(s.ref).decode()
        o.write(">chrD\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        bamio.write_bam(bam, [s.batch])
        cli.main(["call", "-i", bam, "-o", out])
        want = open(out, "rb").read()
        sm = out.replace(".vcf", ".single_molecule_mutations.vcf")
        want_sm = open(sm, "rb").read()
        os.remove(out), os.remove(sm), os.remove(bam)
        if os.path.exists(bam + ".bai"):
            os.remove(bam + ".bai")
        C.batch_bam(bam, s.batch, "EQX")                  # the same path: the header's command line names it
        with pytest.raises(KeyError) as e:
            cli.main(["call", "-i", bam, "-o", out])
        assert "tag 'cs' not present in {} records".format(s.batch.n) in str(e.value)
        cli.main(["call", "-i", bam, "-o", out, "--ref", fa, "--cs_from_ref"])
        assert open(out, "rb").read() == want and open(sm, "rb").read() == want_sm
        assert want.count(b"\n") > want.count(b"\n##") + 1                       # there are calls
        # a FASTA that does not go with the BAM is refused before any ingest
        short = str(tmp_path / "short.fa")
        with open(short, "w") as o:
            o.write(">chrD\nACGT\n")
        with pytest.raises(ValueError) as e:
            cli.main(["call", "-i", bam, "-o", out, "--ref", short, "--cs_from_ref"])
        assert "@SQ LN" in str(e.value)
        with open(short, "w") as o:
            o.write(">other\nACGT\n")
        with pytest.raises(ValueError) as e:
            cli.main(["call", "-i", bam, "-o", out, "--ref", short, "--cs_from_ref"])
        assert "not in the FASTA" in str(e.value)
    finally:
        os.chdir(cwd)
