"""The indels run (himut_run_indels / himut_get_indels) through the C ABI against the plain-Python model of its contract
(tests/indels_model.py): equal record bytes and equal counters.  The hand-built alignments of tests/indels_cases.py pin
the rules and the shapes at which the kernels can go wrong; a contig with one locus per (DP, n_alt) pins the fp64
genotype and every GQ cut-off; sequences on one context pin the kept capacities and the state the runs leave each other;
seeded random rounds; then the errors."""
import numpy as np
import pytest

from tests import indels_cases as C
from tests import indels_model as M
from tests.test_indels_cpu import BOUNDARY_N, boundary_sample, random_round

pytestmark = pytest.mark.gpu

ERR_ARG = 1


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _indels(c, batch, regions, ref, kw, push=True):
    from himut_amd import bamio
    if push:
        bamio.set_contig_reference(c, ref)
        c.push_reads(batch)
    c.set_chunks(regions)
    c.run_indels(**kw)
    return c.indels()


def _both(c, batch, regions, ref, kw):
    got, glog = _indels(c, batch, regions, ref, kw)
    want, wlog = M.run(batch, regions, ref, **kw)
    M.assert_same(got, glog, want, wlog)
    return got, glog


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_hand_built(ctx, case):
    """Every rule of the contract and every shape: the run's bytes are the model's, and say what the rule says."""
    _name, b, regions, ref, kw, expect = case
    recs, log = _both(ctx, b, regions, ref, kw)
    expect(recs, log)


def test_fp64_boundaries(ctx):
    """One locus for every (DP, n_alt) with DP <= 24: state and gq of all 300 alleles; then min_gq at every distinct gq the
    model produces and one above it, the status of all 300 each time."""
    b, ref, items, log, loci = boundary_sample()
    regions = [(0, BOUNDARY_N)]
    kw = dict(report_homref=True, min_gq=0)
    got, glog = _indels(ctx, b, regions, ref, kw)
    want, wlog = M.evaluate(items, log, **kw)
    assert len(got) == 300
    print("states", [int(x) for x in glog[6:9]], "gq", sorted(set(int(x) for x in want["gq"])))
    assert np.array_equal(got["gt_state"], want["gt_state"]) and np.array_equal(got["gq"], want["gq"])
    assert [(int(r["dp"]), int(r["n_alt"])) for r in got] == loci
    M.assert_same(got, glog, want, wlog)
    for g in sorted(set(int(x) for x in want["gq"])):
        for cut in (g, g + 1):
            kw = dict(report_homref=True, min_gq=cut)
            got, glog = _indels(ctx, b, regions, ref, kw, push=False)
            want, wlog = M.evaluate(items, log, **kw)
            assert np.array_equal(got["status"], want["status"]), cut
            M.assert_same(got, glog, want, wlog)


def _case(name):
    return [c for c in C.CASES if c[0] == name][0]


def test_capacities_grow_and_shrink():
    """Indels runs of growing and then shrinking event counts on one context: the capacity the first run leaves holds the
    second, the third overflows it and is made again with exact sizes (reran), the rest fit what that left."""
    from himut_amd import _ffi
    small, medium = _case("het_del"), _case("shape_many_segments")
    b, ref, items, log, _loci = boundary_sample()
    big = ("boundary", b, [(0, BOUNDARY_N)], ref, dict(report_homref=True), None)
    with _ffi.Context(0) as c:
        for case, reran in ((small, 0), (medium, 0), (big, 1), (big, 0), (medium, 0), (small, 0), (big, 0)):
            _name, bb, regions, rr, kw, _e = case
            got, glog = _both(c, bb, regions, rr, kw)
            st = c.stats()
            assert st["reran"] == reran, (case[0], st)
            assert st["n_records"] == len(got) and st["n_candidates"] == glog[0] and st["ms_total"] > 0
            again, alog = _indels(c, bb, regions, rr, kw, push=False)
            assert again.tobytes() == got.tobytes() and alog == glog


def test_interleaved_with_call_germline_dbs():
    """call, germline, dbs and indels runs on the same reads of one context: each run's results are what it gives alone,
    whatever ran before it, and every getter keeps serving its own last run."""
    from himut_amd import _ffi, bamio, gtlib, synth
    from tests import dbs_model as D
    from tests.test_gpu_dbs import PARAM_NAMES
    s = synth.generate(synth.SynthConfig(seed=73, contig_len=30_000, depth=8.0, read_len_mean=6000, read_len_sd=1200,
                                         read_len_min=2000, read_len_max=12000, snp_rate=1e-3, sub_rate=5e-3, ins_rate=2e-3,
                                         del_rate=2e-3, name="chrS"), want_ref=True)
    b = s.batch
    ref = bytes(np.asarray(s.ref, np.uint8)).decode("ascii")
    regions = [(1, b.length)]
    ikw = dict(min_alt_count=1, report_homref=True)
    want, wlog = M.run(b, regions, ref, **ikw)
    assert wlog[0] > 100 and len(want) > 50
    with _ffi.Context(0) as c:
        p = dict(D.DEFAULTS, max_mismatch_count=1 << 20)
        c.set_params(**{k: p[k] for k in PARAM_NAMES})
        c.set_gt_lut(*gtlib.build_tables(1 / (10 ** 3)))
        c.set_site_set(0, np.zeros(0, np.uint64))
        c.set_site_set(1, np.zeros(0, np.uint64))
        bamio.set_contig_reference(c, ref)
        c.push_reads(b)
        c.set_chunks(regions)

        def call():
            c.run()
            return c.records().tobytes(), c.log()

        def germ():
            c.run_germline()
            r, l = c.germline()
            return r.tobytes(), l

        def dbs():
            c.run_dbs()
            r, l = c.dbs()
            return r.tobytes(), l

        def ind():
            c.run_indels(**ikw)
            r, l = c.indels()
            M.assert_same(r, l, want, wlog)
            return r.tobytes(), l
        alone = {f: f() for f in (call, germ, dbs, ind)}
        assert len(alone[call][0]) > 0 and len(alone[germ][0]) > 0
        for f in (ind, call, ind, germ, ind, dbs, ind, ind, call, germ, dbs, call):
            assert f() == alone[f], f.__name__
        c.run()
        c.run_indels(**ikw)
        assert c.records().tobytes() == alone[call][0]           # himut_get_records still serves the call run
        assert c.germline()[0].tobytes() == alone[germ][0] and c.dbs()[0].tobytes() == alone[dbs][0]
        assert c.indels()[0].tobytes() == alone[ind][0]


@pytest.mark.parametrize("part", range(4))
def test_random_rounds(ctx, part):
    """Two hundred seeded small batches, fifty a part: 20-200 reads of 100-2,000 bases over repeat-rich contigs with random
    indels, flags and mapping qualities."""
    for seed in range(1000 + 50 * part, 1050 + 50 * part):
        b, regions, ref, kw = random_round(seed)
        got, glog = _indels(ctx, b, regions, ref, kw)
        want, wlog = M.run(b, regions, ref, **kw)
        try:
            M.assert_same(got, glog, want, wlog)
        except AssertionError as e:
            raise AssertionError("seed {}: {}".format(seed, e))


def test_errors():
    """HIMUT_ERR_ARG without a reference, without regions, and for max_len 0 or 65; the context stays usable."""
    from himut_amd import _ffi, bamio
    _name, b, regions, ref, kw, _e = _case("het_del")
    with _ffi.Context(0) as c:
        c.push_reads(b)
        c.set_chunks(regions)
        with pytest.raises(_ffi.HimutError) as e:
            c.run_indels()
        assert e.value.code == ERR_ARG and "reference" in e.value.message
        bamio.set_contig_reference(c, ref)
        c.set_chunks([])
        with pytest.raises(_ffi.HimutError) as e:
            c.run_indels()
        assert e.value.code == ERR_ARG and "regions" in e.value.message
        c.set_chunks(regions)
        for ml in (0, 65):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_indels(max_len=ml)
            assert e.value.code == ERR_ARG and "max_len" in e.value.message
        got, glog = c.indels()                                   # nothing ran: no records
        assert len(got) == 0 and glog == [0] * 13
        c.run_indels(**kw)
        got, glog = c.indels()
        M.assert_same(got, glog, *M.run(b, regions, ref, **kw))
    with _ffi.Context(0) as c:                                   # no reads at all
        bamio.set_contig_reference(c, ref)
        c.set_chunks(regions)
        with pytest.raises(_ffi.HimutError) as e:
            c.run_indels()
        assert e.value.code == ERR_ARG
