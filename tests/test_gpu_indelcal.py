"""The indelcal run (himut_run_indelcal / himut_get_indelcal) and the indels run under an error table
(himut_set_indel_error_table) through the C ABI against the plain-Python model of their contract
(tests/indelcal_model.py): equal tables, equal counters, equal record bytes.  The hand-built alignments of
tests/indelcal_cases.py pin the rules and the shapes at which the kernels can go wrong; seeded random rounds over contigs
of runs; a sequence on one context pins the kept capacities and what the runs leave each other; then the errors."""
import numpy as np
import pytest

from tests import indelcal_cases as C
from tests import indelcal_model as K
from tests import indels_model as M
from tests.test_indelcal_cpu import SEEDS, random_round
from tests.test_indels_cpu import BOUNDARY_N, boundary_sample

pytestmark = pytest.mark.gpu

ERR_ARG = 1


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _indelcal(c, batch, regions, ref, kw, push=True):
    from himut_amd import bamio
    if push:
        bamio.set_contig_reference(c, ref)
        c.push_reads(batch)
    c.set_chunks(regions)
    c.run_indelcal(**kw)
    return c.indelcal()


def _both(c, batch, regions, ref, kw, push=True):
    table, log = _indelcal(c, batch, regions, ref, kw, push)
    K.assert_same(table, log, *K.run(batch, regions, ref, **kw))
    return table, log


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_hand_built(ctx, case):
    """Every rule of the contract and every shape: the run's table and counters are the model's, and say what the rule says."""
    _name, b, regions, ref, kw, expect = case
    table, log = _both(ctx, b, regions, ref, kw)
    expect(table, log)
    K.check_invariants(table, log)


def test_random_rounds(ctx):
    """The seeded rounds of the CPU test: 15-120 reads of 60-1,200 bases over contigs of runs up to 70 long, events placed
    in runs, variant anchors, flags and mapping qualities."""
    for seed in SEEDS:
        b, regions, ref, kw = random_round(seed)
        table, log = _indelcal(ctx, b, regions, ref, kw)
        try:
            K.assert_same(table, log, *K.run(b, regions, ref, **kw))
        except AssertionError as e:
            raise AssertionError("seed {}: {}".format(seed, e))


@pytest.mark.parametrize("workgroups,budget", [(1, 0), (3, 0), (2, 1), (0, 1)])
def test_sweep_geometry(workgroups, budget):
    """The span sweep is a resident grid that strides over the 256-position blocks and keeps its histogram in LDS: with one,
    two and three workgroups for every hand-built case (12 blocks each) a workgroup sweeps several blocks, dead ones among
    them; with a budget of 1 it adds its cells to the table in front of every block.  Same tables, same counters."""
    from himut_amd import _ffi
    with _ffi.Context(0) as c:
        c.debug_indelcal(workgroups, budget)
        for _name, b, regions, ref, kw, expect in C.CASES:
            table, log = _both(c, b, regions, ref, kw)
            expect(table, log)
        for seed in SEEDS[:8]:
            b, regions, ref, kw = random_round(seed)
            _both(c, b, regions, ref, kw)
        c.debug_indelcal()


def _case(name):
    return [c for c in C.CASES if c[0] == name][0]


def test_sequence_on_one_context():
    """indelcal, indels, indelcal and call on one context: every getter keeps serving its own last run; the event capacity
    an indelcal run leaves holds a smaller one and is outgrown by a larger one (reran 1, then 0)."""
    from himut_amd import _ffi, gtlib
    from tests import dbs_model as D
    from tests.test_gpu_dbs import PARAM_NAMES
    small = _case("event_columns")
    b, ref, _items, _log, _loci = boundary_sample()
    regions = [(1, BOUNDARY_N)]
    big_want = K.run(b, regions, ref)                             # (the model once per parameter set: it looks at every read per run)
    alt_kw = dict(min_alt_count=1, vaf_permille=100)
    alt_want = K.run(b, regions, ref, **alt_kw)
    assert alt_want[1] != big_want[1]
    ind_want = M.run(b, regions, ref, report_homref=True)
    assert big_want[1][0] > 2000                                  # events: far above what the small case leaves room for
    with _ffi.Context(0) as c:
        table, log = _both(c, small[1], small[2], small[3], small[4])
        assert c.stats()["reran"] == 0 and c.stats()["n_candidates"] == log[0] == 7
        table, log = _indelcal(c, b, regions, ref, {})
        K.assert_same(table, log, *big_want)
        assert c.stats()["reran"] == 1
        table, log = _indelcal(c, b, regions, ref, {}, push=False)
        K.assert_same(table, log, *big_want)
        st = c.stats()
        assert st["reran"] == 0 and st["n_candidates"] == log[0] and st["ms_total"] > 0 and st["n_records"] == 0
        c.run_indels(report_homref=True)                          # an event list of its own: nothing kept yet, no repeat
        assert c.stats()["reran"] == 0
        recs, ilog = c.indels()
        M.assert_same(recs, ilog, *ind_want)
        again = c.indelcal()
        K.assert_same(again[0], again[1], table, log)             # the indels run left the table alone
        K.assert_same(*_indelcal(c, b, regions, ref, alt_kw, push=False), *alt_want)
        assert c.stats()["reran"] == 0
        M.assert_same(*c.indels(), *ind_want)                     # ... and the indelcal run the records
        p = dict(D.DEFAULTS, max_mismatch_count=1 << 20)
        c.set_params(**{k: p[k] for k in PARAM_NAMES})
        c.set_gt_lut(*gtlib.build_tables(1 / (10 ** 3)))
        c.set_site_set(0, np.zeros(0, np.uint64))
        c.set_site_set(1, np.zeros(0, np.uint64))
        c.run()
        call = c.records().tobytes(), c.log()
        K.assert_same(*c.indelcal(), *alt_want)
        M.assert_same(*c.indels(), *ind_want)
        K.assert_same(*_indelcal(c, b, regions, ref, {}, push=False), *big_want)
        assert c.stats()["reran"] == 0
        assert (c.records().tobytes(), c.log()) == call           # himut_get_records still serves the call run
        c.run()
        assert (c.records().tobytes(), c.log()) == call
        _both(c, small[1], small[2], small[3], small[4])          # shrinks: fits what the large run left
        assert c.stats()["reran"] == 0


def test_indels_under_a_table(ctx):
    """The boundary sample (one locus for every (DP, n_alt), DP <= 24) under two tables that give the loci's class another
    error: the records are the bytes of the model with the allele's own logs; cleared, the bytes of the run without a table."""
    b, ref, items, log, loci = boundary_sample()
    regions = [(0, BOUNDARY_N)]
    kw = dict(report_homref=True, min_gq=0)
    from himut_amd import bamio, indelcal
    bamio.set_contig_reference(ctx, ref)
    ctx.push_reads(b)
    ctx.set_chunks(regions)
    ctx.set_indel_error_table()
    ctx.run_indels(**kw)
    plain, plog = ctx.indels()
    M.assert_same(plain, plog, *M.evaluate(items, log, **kw))
    cls, column, _n = K.event_cell(ref, K.runs_of(ref), *items[0][0][:3], "")
    seen = {plain.tobytes()}
    for count in (0, 400):                                        # e = 1 / 5002 and 401 / 5002 for the loci; 0.01 elsewhere
        table = np.zeros((128, 10), np.int64)
        table[cls] = [300, 0, 5000] + [count if k == column else 7 for k in range(7)]
        l_hit, l_err = indelcal.error_logs(table, 0.01, min_spans=1000)
        ctx.set_indel_error_table(l_hit, l_err)
        ctx.run_indels(**kw)
        got, glog = ctx.indels()
        want, wlog = K.evaluate_with_table(items, log, ref, *K.error_logs(table, 0.01, 1000), **kw)
        assert len(got) == 300
        M.assert_same(got, glog, want, wlog)
        assert got.tobytes() not in seen
        seen.add(got.tobytes())
        assert not np.array_equal(got["gq"], plain["gq"])
    ctx.set_indel_error_table()
    ctx.run_indels(**kw)
    got, glog = ctx.indels()
    assert got.tobytes() == plain.tobytes() and glog == plog
    # a table in which every class keeps the constant is no table: the same bytes
    ctx.set_indel_error_table(*indelcal.error_logs(np.zeros((128, 10), np.int64), 0.01))
    ctx.run_indels(**kw)
    assert ctx.indels()[0].tobytes() == plain.tobytes()
    ctx.set_indel_error_table()


def test_errors():
    """HIMUT_ERR_ARG without a reference, for max_len 65, a vaf above 1000 and a table of another length; the context stays
    usable and the getter serves zeros until a run completes."""
    from himut_amd import _ffi, bamio
    _name, b, regions, ref, kw, _e = _case("event_columns")
    with _ffi.Context(0) as c:
        c.push_reads(b)
        c.set_chunks(regions)
        with pytest.raises(_ffi.HimutError) as e:
            c.run_indelcal()
        assert e.value.code == ERR_ARG and "reference" in e.value.message
        bamio.set_contig_reference(c, ref)
        for bad in (dict(max_len=65), dict(max_len=0), dict(vaf_permille=1001), dict(min_alt_count=-1)):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_indelcal(**bad)
            assert e.value.code == ERR_ARG and list(bad)[0] in e.value.message
        table, log = c.indelcal()
        assert not table.any() and log == [0] * 14
        for n in (1, 895, 897):
            with pytest.raises(_ffi.HimutError) as e:
                c.set_indel_error_table(np.zeros(n), np.zeros(n))
            assert e.value.code == ERR_ARG and "896" in e.value.message
        with pytest.raises(ValueError):
            c.set_indel_error_table(np.zeros(896), np.zeros(895))
        table, log = _both(c, b, regions, ref, kw, push=False)
        assert log[0] == 7
        c.run_indels()                                            # the refused tables left none behind
        M.assert_same(*c.indels(), *M.run(b, regions, ref))
