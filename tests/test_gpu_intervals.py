"""The intervals run (himut_run_intervals) through the C ABI against the plain model (tests/intervals_model.py): rows
compared by equality, on intervals placed where a span, a slice or a vector load of the tally can go wrong, on the
string's ends, on chunks that are neither ascending nor disjoint, against what himut_run_normcounts sums for the same
batch, and the run's independence of the other getters and of a later himut_set_chunks."""
import random

import numpy as np
import pytest

from tests import callmap_model as M
from tests import intervals_cases as K
from tests import intervals_model as IM
from tests.test_gpu_callmap import ORDER, Device, _configure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def callable_run(worker, case):
    sc = case.scene
    _configure(worker, sc.params)
    dev = Device(worker, sc.batch, sc.chunks, sc.ref.encode(), order=ORDER)
    assert np.array_equal(dev.state, case.res.state) and np.array_equal(dev.bases, case.res.bases)
    return dev


def device_rows(worker, intervals):
    worker.ctx.run_intervals([s for s, _e in intervals], [e for _s, e in intervals])
    rows = worker.ctx.intervals()
    assert rows.shape[0] == len(intervals) and rows.dtype.itemsize == 1024
    return rows


def assert_rows(got, want):
    for f in IM.FIELDS:                                      # (the field and the first rows that differ, then the bytes)
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero((got[f] != want[f]).reshape(len(want), -1).any(axis=1))[:8])
    assert got.tobytes() == want.tobytes()


def test_boundary_scene(worker):
    """656 short intervals at every alignment, lengths around 64, 256, 2048 and 4096 from entry 0 and from an odd entry,
    an interval across three small chunks, one over more than 100,000 NO_BASE positions (several spans, many slices, one
    row), the non-ACGT stretch, all chunks, none, start > end, beyond both ends of the contig, repeats and nests; shuffled:
    the rows follow the input order."""
    case = K.boundary()
    callable_run(worker, case)
    intervals = K.boundary_intervals()
    assert len(intervals) >= 656 + 24 + 13
    random.Random(14).shuffle(intervals)
    want = case.map.rows(intervals)
    got = device_rows(worker, intervals)
    assert_rows(got, want)
    st = worker.ctx.stats()
    assert st["n_records"] == len(intervals) and st["positions"] == case.res.state.shape[0] and st["ms_total"] > 0
    lo, hi = K.span_of(case.scene.chunks)
    whole = got[intervals.index((lo, hi))]
    assert int(whole["entries"]) == case.res.state.shape[0]
    assert int(whole["ref_tri"][IM.OTHER]) == 4 and int(whole["ccs_tri"][IM.OTHER]) == 40
    assert int(got[intervals.index((5000, 4000))]["entries"]) == 0
    _c, a, _b = case.scene.notes["no_base"]
    far = got[intervals.index((a - 3, case.scene.chunks[5][1] + 11))]
    assert int(far["entries"]) > 100_000 and int(far["positions"][M.CALLABLE]) > 0


def test_string_ends(worker):
    case = K.string_ends()
    callable_run(worker, case)
    n = len(case.scene.ref)
    intervals = [(0, 1), (0, 2), (n - 1, n), (0, n)]
    got = device_rows(worker, intervals)
    assert_rows(got, case.map.rows(intervals))
    assert int(got[0]["all_tri"][IM.OTHER]) == 1 and int(got[2]["all_tri"][IM.OTHER]) == 1
    assert int(got[1]["all_tri"][IM.OTHER]) == 1 and int(got[1]["entries"]) == 2
    assert int(got[3]["all_tri"][IM.OTHER]) == 2


def test_unordered_and_overlapping_chunks(worker):
    case = K.hetalt_unordered()
    callable_run(worker, case)
    intervals = [(0, 3000), (1500, 1700), (1400, 1800), (1699, 1701), (40, 60), (1700, 1500), (950, 951), (0, 50),
                 (1999, 2001)] + K.steps(0, 2100, 97)
    got = device_rows(worker, intervals)
    assert_rows(got, case.map.rows(intervals))
    assert int(got[1]["entries"]) == 400 and int(got[0]["entries"]) == 500 + 800 + 50


def test_against_the_normcounts_run(worker):
    """One context: the normcounts run, the callable run, then a partition into 1,000-position intervals whose rows sum to
    the normcounts run's two histograms (the 32 keys, and the rest in slot 32) and to its log."""
    from himut_amd import normcounts
    case = K.boundary()
    sc = case.scene
    _configure(worker, sc.params)
    ccs, rf, log = normcounts.norm_contig(worker, sc.batch, sc.chunks, sc.ref.encode(), None, None, False, ORDER)
    callable_run(worker, case)
    lo, hi = K.span_of(sc.chunks)
    got = device_rows(worker, K.steps(lo, hi, 1000))
    total = IM.total(got)
    assert np.array_equal(total["ref_tri"], IM.fold_tri(rf)) and np.array_equal(total["ccs_tri"], IM.fold_tri(ccs))
    for code in (2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13):
        assert int(total["bases"][code]) == log[code], code
    assert int(total["bases"][2:].sum()) == log[1]
    assert int(total["entries"]) == case.res.state.shape[0]


def test_independence(worker):
    case = K.boundary()
    dev = callable_run(worker, case)
    ctx = worker.ctx
    intervals = K.steps(0, len(case.scene.ref), 777) + [K.span_of(case.scene.chunks)]
    want = case.map.rows(intervals)
    first = device_rows(worker, intervals)
    assert_rows(first, want)
    runs, log = ctx.callable()                               # the callable run's getters keep serving that run
    state, bases = ctx.callable_map(dev.n)
    assert runs.tobytes() == dev.runs.tobytes() and log == dev.log
    assert np.array_equal(state, dev.state) and np.array_equal(bases, dev.bases)
    ctx.set_chunks([(5, 10), (2000, 2500)])                  # the run reads the callable run's chunks, not the context's
    second = device_rows(worker, intervals)
    assert second.tobytes() == first.tobytes()
    ctx.run_intervals([], [])                                # n == 0: a run with zero rows
    assert ctx.intervals().shape[0] == 0 and ctx.stats()["n_records"] == 0
    assert device_rows(worker, intervals).tobytes() == first.tobytes()


def test_error_paths_run_nothing():
    """HIMUT_ERR_ARG (1) on a fresh context, behind a callable run that failed, and under a reference string of another
    length; nothing is queued (the stats of the run before stay as they are)."""
    from himut_amd import _ffi, normcounts
    from himut_amd.caller import Worker
    case = K.hetalt()
    sc = case.scene
    w = Worker(0)
    try:
        for call in (lambda: w.ctx.run_intervals([0], [10]), lambda: w.ctx.run_intervals([], []), lambda: w.ctx.intervals()):
            with pytest.raises(_ffi.HimutError) as e:
                call()
            assert e.value.code == 1
        assert w.ctx.stats()["ms_total"] == 0
        callable_run(w, case)
        assert_rows(device_rows(w, [(0, 3000)]), case.map.rows([(0, 3000)]))
        w.ctx.set_chunks([])
        with pytest.raises(_ffi.HimutError) as e:             # a callable run that fails: no chunks
            w.ctx.run_callable(normcounts.alt_order_table(ORDER))
        assert e.value.code == 1
        after_failure = w.ctx.stats()
        with pytest.raises(_ffi.HimutError) as e:
            w.ctx.run_intervals([0], [3000])
        assert e.value.code == 1 and "himut_run_callable" in e.value.message
        assert w.ctx.stats() == after_failure
        assert_rows(w.ctx.intervals(), case.map.rows([(0, 3000)]))      # the rows of the last run that completed
        dev = callable_run(w, case)
        before = w.ctx.stats()
        chars, cls = normcounts.tri_classes(sc.ref)
        w.ctx.set_reference(sc.ref[:-1], cls, len(chars))
        with pytest.raises(_ffi.HimutError) as e:             # a string of another length
            w.ctx.run_intervals([0], [3000])
        assert e.value.code == 1 and "reference" in e.value.message
        assert w.ctx.stats() == before
        L = _ffi.lib()
        assert L.himut_run_intervals(w.ctx.handle, None, None, 1) == 1 and L.himut_run_intervals(w.ctx.handle, None, None, -1) == 1
        w.ctx.set_reference(sc.ref, cls, len(chars))
        assert_rows(device_rows(w, [(0, 3000), (1200, 1201)]), case.map.rows([(0, 3000), (1200, 1201)]))
        assert dev.n == 1100
    finally:
        w.close()
