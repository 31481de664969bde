"""The dbs run (himut_run_dbs / himut_get_dbs) through the C ABI against the plain-Python model of its contract
(tests/dbs_model.py): equal record bytes and equal counters.  The hand-built alignments of tests/dbs_cases.py pin the
rules and the shapes at which the kernels can go wrong; a synthetic sample pins the run at size and against the call run
of the same context; sequences on one context pin the state the runs leave each other; then errors, the ingest and
the command line."""
import os

import numpy as np
import pytest

from tests import dbs_cases as C
from tests import dbs_model as M
from tests.test_dbs_cpu import CASES, SAMPLE_KW, assert_twins, sample, sample_model

pytestmark = pytest.mark.gpu

PARAM_NAMES = ("min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq", "min_bq", "max_mismatch_count",
               "mismatch_window_size", "md_threshold", "min_ref_count", "min_alt_count", "min_hap_count", "min_sequence_identity",
               "min_trim")


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _configure(c, kw, prior=1 / (10 ** 3)):
    from himut_amd import gtlib
    p = dict(M.DEFAULTS, **kw)
    c.set_params(**{k: p[k] for k in PARAM_NAMES})
    c.set_gt_lut(*gtlib.build_tables(prior))
    c.set_site_set(0, np.array(sorted(kw.get("pon_keys", ())), np.uint64))
    c.set_site_set(1, np.array(sorted(kw.get("com_keys", ())), np.uint64))


def _dbs(c, batch, regions, kw, push=True, prior=1 / (10 ** 3)):
    _configure(c, kw, prior)
    c.set_chunks(regions)
    if push:
        c.push_reads(batch)
    c.run_dbs()
    return c.dbs()


def _both(c, batch, regions, kw, prior=1 / (10 ** 3)):
    got, glog = _dbs(c, batch, regions, kw, prior=prior)
    want, wlog = M.run(batch, regions, prior=prior, **kw)
    M.assert_same(got, glog, want, wlog)
    return got, glog


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(ctx, case):
    """Every rule of the contract and every shape: the run's bytes are the model's, and say what the rule says."""
    _name, b, regions, kw, expect = case
    recs, log = _both(ctx, b, regions, kw)
    expect(recs, log)


def test_synthetic_sample(ctx):
    """The 260 kb sample (407 proposals, two workgroups of the evaluation) equals the model, twice with the same bytes;
    with the mismatch window open, himut_run on one chunk (0, length) on the same context gives the twins of every
    record; random regions give the one-region records they hold."""
    b, kw, want, wlog, dropped = sample_model()
    got, glog = _dbs(ctx, b, [(1, b.length)], kw)
    M.assert_same(got, glog, want, wlog)
    again, alog = _dbs(ctx, b, [(1, b.length)], kw, push=False)
    assert again.tobytes() == got.tobytes() and alog == glog
    st = ctx.stats()
    assert st["n_records"] == len(want) and st["n_candidates"] >= wlog[5] and st["ms_total"] > 0
    _configure(ctx, dict(kw, max_mismatch_count=1 << 20))
    ctx.set_chunks([(0, b.length)])
    ctx.run()
    assert_twins(got, dropped, ctx.records())
    served, slog = ctx.dbs()                               # the call run left the dbs records alone
    assert served.tobytes() == got.tobytes() and slog == glog
    rs = np.random.RandomState(5)
    cuts = rs.randint(1, b.length, 10)
    regions = [(int(min(x, y)), int(max(x, y))) for x, y in zip(cuts[0::2], cuts[1::2])]
    part, _ = _both(ctx, b, regions, kw)
    assert 0 < len(part) < len(got)


def test_context_reuse():
    """dbs -> call -> dbs; a small contig, then a big one that overflows the capacities the small one left (reran), then
    the small one again; after dbs -> germline the call records and the germline records are still served."""
    from himut_amd import _ffi
    from tests import germline_model as G
    from tests.test_gpu_germline import _sample
    big, kw, bwant, blog, _d = sample_model()
    small = _sample(73, 30_000, depth=8.0, sub_rate=5e-3).batch
    swant, slog = M.run(small, [(1, small.length)], **kw)
    assert 0 < len(swant) < len(bwant)
    with _ffi.Context(0) as c:
        got, glog = _dbs(c, small, [(1, small.length)], kw)
        M.assert_same(got, glog, swant, slog)
        assert c.stats()["reran"] == 0
        _configure(c, dict(kw, max_mismatch_count=1 << 20))
        c.set_chunks([(0, small.length)])
        c.run()
        crecs = c.records()
        got, glog = _dbs(c, small, [(1, small.length)], kw, push=False)
        M.assert_same(got, glog, swant, slog)
        assert c.stats()["reran"] == 0
        got, glog = _dbs(c, big, [(1, big.length)], kw)
        M.assert_same(got, glog, bwant, blog)
        assert c.stats()["reran"] == 1
        got, glog = _dbs(c, big, [(1, big.length)], kw, push=False)
        M.assert_same(got, glog, bwant, blog)
        assert c.stats()["reran"] == 0
        got, glog = _dbs(c, small, [(1, small.length)], kw)
        M.assert_same(got, glog, swant, slog)
        assert c.stats()["reran"] == 0
        # the call run on the small contig again, then dbs, then germline: each getter serves its own last run
        _configure(c, dict(kw, max_mismatch_count=1 << 20))
        c.set_chunks([(0, small.length)])
        c.run()
        assert c.records().tobytes() == crecs.tobytes() and len(crecs) > 0
        got, glog = _dbs(c, small, [(1, small.length)], kw, push=False)
        c.run_germline()
        grecs, gl = c.germline()
        G.assert_same(grecs, gl, *G.run(small, [(1, small.length)]))
        assert c.records().tobytes() == crecs.tobytes()
        served, slog2 = c.dbs()
        assert served.tobytes() == got.tobytes() == swant.tobytes() and slog2 == slog


def test_errors_then_a_good_contig(ctx):
    """Quality 0 in a column of a candidate: HIMUT_ERR_BQ0; quality 0 elsewhere is no error; a query N in an aligned
    position of a pile read: HIMUT_ERR_BASE; the same context runs a good contig right afterwards.  (Inputs the library
    rejects cleanly.)"""
    from himut_amd._ffi import HimutError
    good = C.pile(500)
    gb = C.batch(good)
    want, wlog = M.run(gb, [(1, C.N)], **C.OPEN)
    assert len(want) == 1
    for what, code in (("bq0_first", M.ERR_BQ0), ("bq0_second", M.ERR_BQ0), ("n", M.ERR_BASE), ("bq0_elsewhere", 0)):
        reads = [dict(r) for r in good]
        if what.startswith("bq0"):
            pos = {"bq0_first": 500, "bq0_second": 501, "bq0_elsewhere": 502}[what]
            reads[5]["bq"] = list(reads[5]["bq"]); reads[5]["bq"][pos - reads[5]["tstart"]] = 0
        else:
            s = reads[3]["seq"]; k = 450 - reads[3]["tstart"]
            reads[3]["seq"] = s[:k] + "N" + s[k + 1:]
        b = C.batch(reads)
        if code:
            with pytest.raises(HimutError) as e:
                _dbs(ctx, b, [(1, C.N)], C.OPEN)
            assert e.value.code == code
            with pytest.raises(M.ModelError) as me:
                M.run(b, [(1, C.N)], **C.OPEN)
            assert me.value.code == code
        else:
            _both(ctx, b, [(1, C.N)], C.OPEN)
        got, glog = _dbs(ctx, gb, [(1, C.N)], C.OPEN)
        M.assert_same(got, glog, want, wlog)


def test_argument_errors():
    from himut_amd import _ffi, gtlib
    b = C.batch(C.pile(500))
    p = dict(M.DEFAULTS, **C.OPEN)
    with _ffi.Context(0) as c:
        for step in (lambda: c.set_params(**{k: p[k] for k in PARAM_NAMES}), lambda: c.set_gt_lut(*gtlib.build_tables(1e-3)),
                     lambda: c.push_reads(b), lambda: c.set_chunks([(1, C.N)])):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_dbs()
            assert e.value.code == 1
            step()
        c.run_dbs()                            # the site sets were never set: allowed; phase = 1 without phase sets: ignored
        assert len(c.dbs()[0]) == 1
        c.set_params(**dict({k: p[k] for k in PARAM_NAMES}, phase=1))
        c.run_dbs()
        assert len(c.dbs()[0]) == 1
        c.set_chunks([(5, 4)])
        with pytest.raises(_ffi.HimutError) as e:
            c.run_dbs()
        assert e.value.code == 6               # HIMUT_ERR_CHUNK


def test_ingest_path_equals_pushed_reads(ctx, tmp_path):
    """The device-side ingest (ingest_contig), with the cs tags of the file and with the text derived from CIGAR and the
    reference, gives the records of the pushed reads."""
    from himut_amd import bamio, synth
    from tests import cs_from_cigar
    s = synth.generate(synth.SynthConfig(seed=75, contig_len=60_000, depth=20.0, read_len_mean=6000, read_len_sd=1200,
                                         read_len_min=2000, read_len_max=12000, hetalt_frac=0.1, sub_rate=5e-3, name="chrI"),
                       want_ref=True)
    want, wlog = M.run(s.batch, [(1, s.batch.length)], **SAMPLE_KW)
    assert len(want) > 20
    tagged, bare = str(tmp_path / "t.bam"), str(tmp_path / "b.bam")
    bamio.write_bam(tagged, [s.batch], sample="S")
    cs_from_cigar.batch_bam(bare, s.batch, "M", sample="S")
    for path, derive in ((tagged, False), (bare, True)):
        st = bamio.BamStream(path, threads=2)
        if derive:
            bamio.set_contig_reference(ctx, bytes(s.ref))
        st.ingest_contig(ctx, "chrI", derive_cs=derive)
        st.close()
        _configure(ctx, SAMPLE_KW)
        ctx.set_chunks([(1, s.batch.length)])
        ctx.run_dbs()
        got, glog = ctx.dbs()
        M.assert_same(got, glog, want, wlog)
    ctx.ingest_derive_cs(0)


def test_cli_dbs(tmp_path):
    """`dbs` on a two-contig BAM writes the model's VCF body and log byte for byte; --devices 0,0 gives the same bytes."""
    from himut_amd import __main__ as cli
    from himut_amd import bamio, bamlib, util as hutil
    s1 = sample(81, sub_rate=5e-3, name="chr2", contig_len=110_000)
    s2 = sample(82, sub_rate=5e-3, name="chr10", contig_len=70_000)
    bam = str(tmp_path / "in.bam")
    bamio.write_bam(bam, [s2, s1], sample="SMP")
    batches = {"chr2": s1, "chr10": s2}
    sizes = {"chr10": 70_000, "chr2": 110_000}
    chrom_lst, c2c = hutil.load_loci(None, None, sizes)
    ql, qu, md = bamlib.get_thresholds(batches, chrom_lst, sizes)
    flags = ["--min_qv", "0", "--min_mapq", "0", "--min_sequence_identity", "0", "--min_bq", "30", "--max_mismatch_count", "3"]
    kw = dict(M.DEFAULTS, min_qv=0, min_mapq=0, min_sequence_identity=0.0, min_bq=30, max_mismatch_count=3, qlen_lower_limit=ql,
              qlen_upper_limit=qu, md_threshold=md)
    body, logs = [], {}
    for c in chrom_lst:
        recs, logs[c] = M.run(batches[c], [(x[1], x[2]) for x in c2c[c]], **kw)
        body += M.vcf_lines(c, recs)
    assert len(body) > 50
    out, cwd = {}, os.getcwd()
    for name, dev in (("one", "0"), ("two", "0,0")):
        d = tmp_path / name
        d.mkdir()
        os.chdir(d)
        try:
            cli.main(["dbs", "-i", bam, "-o", str(d / "dbs.vcf"), "--devices", dev] + flags)
        finally:
            os.chdir(cwd)
        out[name] = open(d / "dbs.vcf").read()
        assert [l for l in out[name].splitlines(True) if not l.startswith("#")] == body
        rows = [l.split() for l in open(d / "himut_dbs.log")]
        assert rows[0] == chrom_lst + ["total"] and [r[0] for r in rows[1:]] == M.LOG_ROWS
        assert [[int(x) for x in r[1:3]] for r in rows[1:]] == [[logs[c][k] for c in chrom_lst] for k in range(20)]
    assert out["one"].replace("/one/", "/two/") == out["two"]
    assert "##himut_command=himut dbs -i {} ".format(bam) in out["one"] and out["one"].splitlines()[-len(body) - 1].endswith("\tSMP")
