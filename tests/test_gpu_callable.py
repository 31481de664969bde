"""k_callable bit by bit: the bits himut_debug_norm_callable reads back after a normcounts pass against the plain model
(tests/callable_model.py) on the hand-built reads of tests/callable_cases.py -- every word of every read, at every
parameter set of a case.  tests/test_callable_cpu.py pins the model to what the reference's update_tri2count gave for
the same reads."""
import numpy as np
import pytest

from tests import callable_cases as C
from tests import callable_model as M

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_BASE = 1, 4                                                       # HIMUT_ERR_*
ORDER = {"A": ["T", "G", "C"], "T": ["C", "A", "G"], "G": ["A", "C", "T"], "C": ["G", "T", "A"]}


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def built():
    """name -> (case, batch, {parameter set number: the model's (live, words)}), filled as the tests ask."""
    return {}


def _case(built, name):
    if name not in built:
        case = C.build(name)
        batch = C.batch_of(case)
        if name == "padding":
            batch = C.poison_padding(batch)
        built[name] = (case, batch, {})
    return built[name]


def _want(built, name, k):
    case, batch, cache = _case(built, name)
    if k not in cache:
        cache[k] = M.callable_bits(batch, case.chunks, C.params_of(case.params[k]))
    return cache[k]


def _configure(worker, p):
    worker.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"],
                     p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"],
                     p["md_threshold"], p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"],
                     False)


def _run(worker, case, batch, p):
    """One normcounts pass; (live, words) of the hook, sized by the batch."""
    from himut_amd import normcounts
    _configure(worker, p)
    res = normcounts.norm_contig(worker, batch, case.chunks, case.ref.encode(), alt_order=ORDER)
    words, live = worker.ctx.norm_callable(int(batch.bq.shape[0]) >> 5, batch.n)
    return live, words, res


def _check(worker, built, name, k):
    case, batch, _ = _case(built, name)
    want_live, want_words = _want(built, name, k)
    live, words, _res = _run(worker, case, batch, C.params_of(case.params[k]))
    diff = M.first_difference(batch, live, words, want_live, want_words)
    assert diff is None, "{} {}: {}".format(name, case.params[k], diff)
    assert np.array_equal(live, want_live) and np.array_equal(words, want_words)


@pytest.mark.parametrize("name", [c for c in C.CASES if c != "long"])
def test_every_word_equals_the_model(worker, built, name):
    """live and every word of the bit array, at every parameter set of the case (padding: the bytes of bq behind each
    read set to 255 first)."""
    case, _batch, _ = _case(built, name)
    for k in range(len(case.params)):
        _check(worker, built, name, k)


@pytest.mark.parametrize("k", [0, 1])
def test_long_reads_equal_the_model(worker, built, k):
    """2047, 2048 and 2049 words and 70,001 bases: the last read the bitmap of marked words holds, the first it does not."""
    _check(worker, built, "long", k)
    case, batch, _ = _case(built, "long")
    assert sorted(int(x) for x in batch.qlen) == sorted(C.LONG_QLEN) and _want(built, "long", k)[0].all()


@pytest.mark.parametrize("sweep", [0, 1])
@pytest.mark.parametrize("name", C.CASES)
def test_sweeps_read_the_bits_they_were_given(worker, built, name, sweep):
    """Every read ten times at the same start under distinct names, so that positions are deep enough to classify, through
    k_norm_quad (sweep 0) and k_norm_tile (sweep 1): the oracle's two dicts and 14 counters.  Reads of more than 65,535
    bases go through both like any other read."""
    from oracle import oracle as O
    from himut_amd import normcounts
    case, _batch, cache = _case(built, name)
    b10 = C.batch_of(case, copies=10)
    if name == "padding":
        b10 = C.poison_padding(b10)
    refseq = case.ref.encode()
    for k in sorted({0, len(case.params) - 1}):
        p = C.params_of(case.params[k])
        if ("oracle", k) not in cache:
            cache[("oracle", k)] = O.normcounts(b10, case.chunks, p, refseq, p["germline_snv_prior"], alt_order=ORDER)
        o_ccs, o_ref, o_log = cache[("oracle", k)]
        _configure(worker, p)
        worker.ctx.debug_normcounts(sweep=sweep)
        try:
            ccs, rf, log = normcounts.norm_contig(worker, b10, case.chunks, refseq, alt_order=ORDER)
        finally:
            worker.ctx.debug_normcounts()
        assert log == o_log, (name, case.params[k])
        assert ccs == o_ccs and rf == o_ref
        assert log[13] > 0


def test_every_word_is_rewritten_between_passes(worker, built):
    """The bit array is not cleared between passes: long, then word_edges (whose 27 reads lie over the first words of the
    long reads), then long again, on one context."""
    for name, k in (("long", 0), ("word_edges", 3), ("long", 1), ("filters", 0), ("long", 0)):
        _check(worker, built, name, k)


def test_bits_after_a_call_run_on_the_same_context(worker, built):
    case, batch, _ = _case(built, "read_start")
    p = C.params_of(case.params[1])
    _configure(worker, p)
    recs, _log = worker.call_contig(batch, case.chunks)
    assert len(recs) > 0
    _check(worker, built, "counts", 2)
    _check(worker, built, "read_start", 1)


def test_hook_is_refused_without_a_completed_pass(built):
    """Before any pass; with more words or reads than the pass wrote; after a pass that ended in HIMUT_ERR_BASE (an
    aligned base outside ATGC in a fetched read)."""
    from himut_amd import normcounts
    from himut_amd._ffi import HimutError
    from himut_amd.caller import Worker
    w = Worker(0)
    try:
        with pytest.raises(HimutError) as e:
            w.ctx.norm_callable(1, 1)
        assert e.value.code == ERR_ARG and "has not completed" in str(e.value)
        case, batch, _ = _case(built, "trim")
        n_words = int(batch.bq.shape[0]) >> 5
        live, words, _res = _run(w, case, batch, C.params_of(case.params[1]))
        assert live.all() and words.any()
        for nw, nr in ((n_words + 1, batch.n), (n_words, batch.n + 1)):
            with pytest.raises(HimutError) as e:
                w.ctx.norm_callable(nw, nr)
            assert e.value.code == ERR_ARG
        part_words, part_live = w.ctx.norm_callable(3, 2)
        assert np.array_equal(part_words, words[:3]) and np.array_equal(part_live, live[:2])
        # the hook changes nothing: the pass's results are still served, and a rerun gives the same bits
        assert w.ctx.normcounts()[2] == _res[2]
        again = _run(w, case, batch, C.params_of(case.params[1]))
        assert np.array_equal(again[0], live) and np.array_equal(again[1], words) and again[2] == _res
        bad = [dict(r) for r in case.records]
        bad[0]["seq"] = bad[0]["seq"][:50] + "N" + bad[0]["seq"][51:]
        from himut_amd.readbatch import batch_from_records
        nb = batch_from_records(C.CONTIG, case.length, bad)
        _configure(w, C.params_of(case.params[1]))
        with pytest.raises(HimutError) as e:
            normcounts.norm_contig(w, nb, case.chunks, case.ref.encode(), alt_order=ORDER)
        assert e.value.code == ERR_BASE
        with pytest.raises(HimutError) as e:
            w.ctx.norm_callable(n_words, batch.n)
        assert e.value.code == ERR_ARG
    finally:
        w.close()
