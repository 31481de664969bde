"""The sindels run (himut_run_sindels / himut_get_sindels) through the C ABI against the plain-Python model of its
contract (tests/sindels_model.py): equal record bytes and equal counters.  The hand-built alignments of
tests/sindels_cases.py pin the rules and the shapes at which the kernels can go wrong; a contig with one locus per
(DP, n_alt) pins the fp64 genotype and every GQ cut-off; sequences on one context pin the kept capacities and the state
the runs leave each other; seeded random rounds; then the errors."""
import numpy as np
import pytest

from tests import indels_model as M
from tests import sindels_cases as C
from tests import sindels_model as S
from tests.test_indels_cpu import BOUNDARY_N, boundary_sample
from tests.test_sindels_cpu import ROUND_FLOORS, ROUND_NONZERO, ROUND_SEEDS, synth_round

pytestmark = pytest.mark.gpu

ERR_ARG = 1


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _sindels(c, batch, regions, ref, kw, push=True, l_hit=None, l_err=None):
    from himut_amd import bamio
    if push:
        bamio.set_contig_reference(c, ref)
        c.push_reads(batch)
    c.set_chunks(regions)
    c.set_indel_error_table(*(() if l_hit is None else (l_hit, l_err)))
    c.run_sindels(**kw)
    return c.sindels()


def _both(c, batch, regions, ref, kw, l_hit=None, l_err=None):
    got, glog = _sindels(c, batch, regions, ref, kw, l_hit=l_hit, l_err=l_err)
    want, wlog = S.run(batch, regions, ref, l_hit, l_err, **kw)
    S.assert_same(got, glog, want, wlog)
    return got, glog


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_hand_built(ctx, case):
    """Every rule of the contract and every shape: the run's bytes are the model's, and say what the rule says."""
    _name, b, regions, ref, kw, expect = case
    kw, l_hit, l_err = C.table_of(kw)
    recs, log = _both(ctx, b, regions, ref, kw, l_hit, l_err)
    expect(recs, log)


BOUNDARY_KW = dict(min_mapq=0, min_qv=30, min_bq=30, min_ref_count=0, min_alt_count=1, max_run=2, min_sequence_identity=0.9,
                   min_trim=0.01, mismatch_window_size=20, max_mismatch_count=0)


def test_fp64_boundaries(ctx):
    """One locus for every (DP, n_alt) with DP <= 24, every carrier proposing: which alleles are dropped as germline and
    the gq of the others; then min_gq at every distinct gq the model produces and one above it, the status of all records
    each time."""
    b, ref, items, _log, loci = boundary_sample()
    regions = [(0, BOUNDARY_N)]
    lg = M.logs(0.01, 1e-4)
    states = [M.genotype(dp - na, na, lg)[0] for dp, na in loci]
    got, glog = _both(ctx, b, regions, ref, dict(BOUNDARY_KW, min_gq=0))
    d = S.logd(glog)
    assert d["candidates"] == 300 and d["num_germ_het"] == states.count(1) and d["num_germ_homalt"] == states.count(2)
    assert [(int(r["dp"]), int(r["n_alt"])) for r in got] == [x for x, s in zip(loci, states) if s == 0]
    assert [int(r["gq"]) for r in got] == [M.genotype(dp - na, na, lg)[1] for (dp, na), s in zip(loci, states) if s == 0]
    assert all(int(r["n_prop"]) == int(r["n_alt"]) for r in got)
    collected = S.collect(b, regions, ref, **BOUNDARY_KW)
    cuts = sorted(set(int(x) for x in got["gq"]))
    print("homref", len(got), "gq", cuts)
    assert len(cuts) >= 10
    for g in cuts:
        for cut in (g, g + 1):
            kw = dict(BOUNDARY_KW, min_gq=cut)
            again, alog = _sindels(ctx, b, regions, ref, kw, push=False)
            want, wlog = S.evaluate(collected, ref, **kw)
            assert np.array_equal(again["status"], want["status"]), cut
            S.assert_same(again, alog, want, wlog)
            assert [int(s) == S.ST_LOWGQ for s in again["status"]] == [int(q) < cut for q in again["gq"]]


def _case(name):
    return [c for c in C.CASES if c[0] == name][0]


def test_capacities_grow_and_shrink():
    """Runs of growing and then shrinking event counts on one context: the capacity the first run leaves holds the second,
    the third overflows it and is made again with exact sizes (reran), the rest fit what that left."""
    from himut_amd import _ffi
    small, medium = _case("lone_del"), _case("shape_stage_overflow")
    b, ref, _items, _log, _loci = boundary_sample()
    big = ("boundary", b, [(0, BOUNDARY_N)], ref, dict(BOUNDARY_KW, min_gq=0), None)
    with _ffi.Context(0) as c:
        for case, reran in ((small, 0), (medium, 0), (big, 1), (big, 0), (medium, 0), (small, 0), (big, 0)):
            _name, bb, regions, rr, kw, _e = case
            got, glog = _both(c, bb, regions, rr, kw)
            st = c.stats()
            assert st["reran"] == reran, (case[0], st)
            assert st["n_records"] == len(got) and st["n_candidates"] == glog[0] and st["ms_total"] > 0
            again, alog = _sindels(c, bb, regions, rr, kw, push=False)
            assert again.tobytes() == got.tobytes() and alog == glog


def test_interleaved_with_the_other_runs():
    """call, germline, dbs, indels, indelcal and sindels runs on the same reads of one context: each run's results are what
    it gives alone, whatever ran before it; the error table set and cleared between runs moves the two runs that read it
    and nothing else."""
    from himut_amd import _ffi, bamio, gtlib
    from tests import dbs_model as D
    from tests import indelcal_model as IC
    from tests.test_gpu_dbs import PARAM_NAMES
    b, regions, ref, kw, want, wlog = synth_round(ROUND_SEEDS[0])
    ikw = dict(min_alt_count=1, report_homref=True)
    iwant, iwlog = M.run(b, regions, ref, **ikw)
    ctab, clog = IC.run(b, regions, ref)
    l_hit, l_err = IC.error_logs(ctab, 0.01, min_spans=50)
    twant, twlog = S.run(b, regions, ref, l_hit, l_err, **kw)
    assert twant.tobytes() != want.tobytes()                     # the table moves a gq or a verdict
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
            c.set_indel_error_table()
            c.run_indels(**ikw)
            r, l = c.indels()
            M.assert_same(r, l, iwant, iwlog)
            return r.tobytes(), l

        def cal():
            c.run_indelcal()
            t, l = c.indelcal()
            IC.assert_same(t, l, ctab, clog)
            return t.tobytes(), l

        def sin():
            c.set_indel_error_table()
            c.run_sindels(**kw)
            r, l = c.sindels()
            S.assert_same(r, l, want, wlog)
            return r.tobytes(), l

        def sin_table():
            c.set_indel_error_table(l_hit, l_err)
            c.run_sindels(**kw)
            r, l = c.sindels()
            S.assert_same(r, l, twant, twlog)
            return r.tobytes(), l
        alone = {f: f() for f in (call, germ, dbs, ind, cal, sin, sin_table)}
        assert len(alone[call][0]) > 0 and len(alone[germ][0]) > 0
        for f in (sin, call, sin, germ, sin_table, dbs, sin, ind, sin, cal, sin_table, sin, call, ind, cal, germ, dbs):
            assert f() == alone[f], f.__name__
        c.run()
        sin()
        assert c.records().tobytes() == alone[call][0]           # every getter still serves its own last run
        assert c.germline()[0].tobytes() == alone[germ][0] and c.dbs()[0].tobytes() == alone[dbs][0]
        assert c.indels()[0].tobytes() == alone[ind][0] and c.indelcal()[0].tobytes() == alone[cal][0]
        assert c.sindels()[0].tobytes() == alone[sin][0]


def test_random_rounds(ctx):
    """The seeded synth rounds of tests/test_sindels_cpu.py (30 kb, depth 8): the model's floors, met by the run."""
    total = dict.fromkeys(S.LOG, 0)
    for seed in ROUND_SEEDS:
        b, regions, ref, kw, want, wlog = synth_round(seed)
        got, glog = _sindels(ctx, b, regions, ref, kw)
        try:
            S.assert_same(got, glog, want, wlog)
        except AssertionError as e:
            raise AssertionError("seed {}: {}".format(seed, e))
        d = S.logd(glog)
        assert d["candidates"] >= ROUND_FLOORS["candidates"] and len(got) >= ROUND_FLOORS["records"]
        for k in S.LOG:
            total[k] += d[k]
    assert all(total[k] > 0 for k in ROUND_NONZERO), total


def test_errors():
    """Each HIMUT_ERR_ARG rule by name in himut_last_error(); nothing runs; then a good run on the same context."""
    from himut_amd import _ffi, bamio
    _name, b, regions, ref, kw, _e = _case("lone_del")
    with _ffi.Context(0) as c:
        c.push_reads(b)
        c.set_chunks(regions)
        with pytest.raises(_ffi.HimutError) as e:
            c.run_sindels(**kw)
        assert e.value.code == ERR_ARG and "reference" in e.value.message
        bamio.set_contig_reference(c, ref)
        c.set_chunks([])
        with pytest.raises(_ffi.HimutError) as e:
            c.run_sindels(**kw)
        assert e.value.code == ERR_ARG and "regions" in e.value.message
        c.set_chunks(regions)
        for bad, word in ((dict(max_len=0), "max_len"), (dict(max_len=65), "max_len"), (dict(min_trim=-0.01), "min_trim"),
                          (dict(min_trim=0.51), "min_trim"), (dict(min_trim=float("nan")), "min_trim"), (dict(max_run=-1), "max_run"),
                          (dict(mismatch_window_size=-1), "mismatch_window_size"), (dict(max_mismatch_count=-1), "max_mismatch_count")):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_sindels(**dict(kw, **bad))
            assert e.value.code == ERR_ARG and word in e.value.message and "himut_run_sindels" in e.value.message, (bad, e.value.message)
        got, glog = c.sindels()                                  # nothing ran: no records
        assert len(got) == 0 and glog == [0] * 20
        for edge in (dict(min_trim=0.0), dict(min_trim=0.5), dict(max_run=0), dict(mismatch_window_size=0)):
            k = dict(kw, **edge)
            c.run_sindels(**k)
            S.assert_same(*c.sindels(), *S.run(b, regions, ref, **k))
        c.run_sindels(**kw)
        S.assert_same(*c.sindels(), *S.run(b, regions, ref, **kw))
    with _ffi.Context(0) as c:                                   # no reads at all
        bamio.set_contig_reference(c, ref)
        c.set_chunks(regions)
        with pytest.raises(_ffi.HimutError) as e:
            c.run_sindels(**kw)
        assert e.value.code == ERR_ARG
