"""The callable run (himut_run_callable) through the C ABI against the plain model (tests/callmap_model.py): the
per-position map, the run records and the fourteen counters, bit for bit; its sums against what himut_run_normcounts
returns for the same batch in the same context; and hand-built contigs whose states change at the kernels' seams."""
import numpy as np
import pytest

from tests import callmap_cases as C
from tests import callmap_model as M
from tests import util
from tests.test_oracle_golden import NORM_CASES, load_norm_case

pytestmark = pytest.mark.gpu

ORDER = {"A": ["T", "G", "C"], "T": ["C", "A", "G"], "G": ["A", "C", "T"], "C": ["G", "T", "A"]}
RUN_FIELDS = ("chunk", "start", "end", "state", "bases")


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _configure(worker, p, phase=False):
    worker.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"],
                     p["min_sequence_identity"], p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"],
                     p["mismatch_window_size"], p["md_threshold"], p["min_ref_count"], p["min_alt_count"],
                     p["min_hap_count"], p["germline_snv_prior"], phase)


class Device:
    """What a callable run left in the context: the map, the runs, the counters."""

    def __init__(self, worker, batch, chunks, refseq, pon=None, com=None, non_human=False, order=ORDER, phase_sets=None):
        from himut_amd import callable as callable_
        self.chunks = [(int(s), int(e)) for s, e in chunks]
        self.runs, self.log = callable_.callable_contig(worker, batch, self.chunks, refseq, pon, com, non_human, order,
                                                        phase_sets)
        self.n = sum(e - s for s, e in self.chunks)
        self.state, self.bases = worker.ctx.callable_map(self.n)
        self.mapoff = np.concatenate([[0], np.cumsum([e - s for s, e in self.chunks])]).astype(np.int64)
        self.stats = worker.ctx.stats()


def assert_same(dev, res):
    assert np.array_equal(dev.state, res.state), np.flatnonzero(dev.state != res.state)[:8]
    assert np.array_equal(dev.bases, res.bases), np.flatnonzero(dev.bases != res.bases)[:8]
    assert dev.runs.shape[0] == res.runs.shape[0]
    for f in RUN_FIELDS:
        assert np.array_equal(dev.runs[f], res.runs[f]), f
    assert dev.log == res.log
    assert dev.stats["n_records"] == res.runs.shape[0] and dev.stats["positions"] == res.state.shape[0]


@pytest.mark.parametrize("case", NORM_CASES)
def test_golden_cases_against_the_model_and_the_normcounts_run(worker, case):
    from himut_amd import normcounts
    batch, exp, p, refseq, pon, com = load_norm_case(case)
    phase = util.phase_of(exp)
    chunks = util.chunks_of(exp)
    _configure(worker, p, phase is not None)
    res = M.run(batch, refseq, chunks, p, pon, com, exp["alt_order"], exp["non_human_sample"], phase)
    # the normcounts run first: its sums are what the map must fold to, and what it serves must survive the callable run
    ccs, rf, log = normcounts.norm_contig(worker, batch, chunks, refseq, pon, com, exp["non_human_sample"], exp["alt_order"],
                                          phase_sets=phase)
    before = worker.ctx.normcounts()
    dev = Device(worker, batch, chunks, refseq, pon, com, exp["non_human_sample"], exp["alt_order"], phase)
    assert_same(dev, res)
    after = worker.ctx.normcounts()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    rows, ref_tri, ccs_tri = M.fold(dev, refseq)
    assert dev.log == log == exp["log"]
    assert rows[1:] == log[1:]
    assert {k: c for k, c in ref_tri.items() if c} == {k: c for k, c in rf.items() if c}
    assert {k: c for k, c in ccs_tri.items() if c} == {k: c for k, c in ccs.items() if c}


def test_alt_order_variants(worker):
    batch, exp, p, refseq, pon, com = load_norm_case("norm_order")
    _configure(worker, p, False)
    for v in exp["variants"]:
        res = M.run(batch, refseq, util.chunks_of(exp), p, pon, com, v["alt_order"], exp["non_human_sample"])
        dev = Device(worker, batch, util.chunks_of(exp), refseq, pon, com, exp["non_human_sample"], v["alt_order"])
        assert_same(dev, res)
        assert dev.log == v["log"], v["hashseed"]


@pytest.mark.parametrize("seed,length,chunks", [
    (31, 300_000, None),                                     # reference chunking, two chunks
    (32, 120_000, [(500, 40_000), (40_000, 41_000), (90_000, 119_000)]),   # gaps and a 1 kb chunk
])
def test_synth_cases(worker, seed, length, chunks):
    """The two cases of test_normcounts_oracle_parity."""
    from oracle import oracle as O
    from himut_amd import synth, util as hutil
    s = synth.generate(synth.SynthConfig(seed=seed, contig_len=length, name="chrN"), want_ref=True)
    refseq = bytes(s.ref)
    if chunks is None:
        chunks = [(c[1], c[2]) for c in hutil.chunkloci((s.batch.name, 0, s.batch.length))]
    p = dict(util.CALL_DEFAULTS)
    p.update(qlen_lower_limit=9000, qlen_upper_limit=22500, md_threshold=52)
    rs = np.random.RandomState(seed)
    sites = [(int(x) + 1, chr(r), chr(a)) for x, r, a in zip(s.snp_pos, s.snp_ref, s.snp_alt)]
    extra = [(int(rs.randint(1, length)), "ACGT"[i], "ACGT"[j]) for i, j in rs.randint(0, 4, (2000, 2)) if i != j]
    pon = O.site_keys(extra[::2] + sites[::3])
    com = O.site_keys(extra[1::2] + sites[1::3])
    res = M.run(s.batch, refseq, chunks, p, pon, com, ORDER)
    _configure(worker, p)
    dev = Device(worker, s.batch, chunks, refseq, pon, com, False, ORDER)
    assert_same(dev, res)
    assert dev.runs.shape[0] >= 3
    states = set(dev.runs["state"].tolist())
    assert M.CALLABLE in states and M.NO_BASE in states and states & {M.HET, M.HETALT, M.HOMALT}


# ---------------------------------------------------------------------------------------------- the kernels' seams
@pytest.fixture(scope="module")
def scene():
    from himut_amd import _ffi
    sc = C.boundary_scene(_ffi.CALLMAP_TILE, _ffi.CALLMAP_BLOCK)
    return sc, M.run(sc.batch, sc.ref, sc.chunks, sc.params)


def test_boundary_scene(worker, scene):
    """Chunk starts and lengths that are no multiple of 256, chunks shorter than a tile and of one position, a state
    change at a tile boundary and at a compaction-block boundary, a run over more than three blocks (the int64 carry), a
    NO_BASE run of more than 100,000 positions, a whole block of runs of one position (nothing truncated: as many records
    as the model has), a pile deeper than one LDS batch beside a shallow one.  tests/test_callmap_cpu.py checks that the
    scene holds all of that."""
    from himut_amd import _ffi
    sc, res = scene
    _configure(worker, sc.params)
    dev = Device(worker, sc.batch, sc.chunks, sc.ref.encode(), order=ORDER)
    assert_same(dev, res)
    c, a, b = sc.notes["alternating"]
    ones = dev.runs[(dev.runs["chunk"] == c) & (dev.runs["start"] >= a) & (dev.runs["end"] <= b)]
    assert ones.shape[0] == b - a >= 2 * _ffi.CALLMAP_BLOCK and np.all(ones["end"] - ones["start"] == 1)
    assert dev.runs.shape[0] == res.runs.shape[0] > _ffi.CALLMAP_BLOCK
    c, a, b = sc.notes["long_run"]
    one = dev.runs[(dev.runs["chunk"] == c) & (dev.runs["start"] == a)]
    assert one.shape[0] == 1 and int(one["end"][0]) == b and int(one["bases"][0]) == 4 * (b - a)
    seam = dev.runs[(dev.runs["chunk"] >= 2) & (dev.runs["chunk"] <= 4)]
    assert seam.shape[0] == 3 and len(set(seam["state"].tolist())) == 1       # abutting chunks, equal state: a run each


def test_two_runs_back_to_back_are_independent(worker, scene):
    """Other chunks in the same context: fewer positions, fewer runs, another order; then the first again."""
    sc, res = scene
    _configure(worker, sc.params)
    first = Device(worker, sc.batch, sc.chunks, sc.ref.encode(), order=ORDER)
    assert_same(first, res)
    other = [sc.chunks[5][:1] + (sc.chunks[5][0] + 1500,), (sc.chunks[1][0] + 3, sc.chunks[1][0] + 700), sc.chunks[3]]
    res2 = M.run(sc.batch, sc.ref, other, sc.params)
    second = Device(worker, sc.batch, other, sc.ref.encode(), order=ORDER)
    assert_same(second, res2)
    assert second.runs.shape[0] < first.runs.shape[0]
    with pytest.raises(Exception) as e:                       # more than the last run swept
        worker.ctx.callable_map(first.n)
    assert getattr(e.value, "code", None) == 1
    again = Device(worker, sc.batch, sc.chunks, sc.ref.encode(), order=ORDER)
    assert_same(again, res)


def test_hetalt_scene(worker):
    sc = C.hetalt_scene()
    _configure(worker, sc.params)
    dev = Device(worker, sc.batch, sc.chunks, sc.ref.encode(), order=ORDER)
    assert_same(dev, M.run(sc.batch, sc.ref, sc.chunks, sc.params))
    assert M.HETALT in set(dev.runs["state"].tolist())


def test_a_contig_without_reads(worker):
    from himut_amd.readbatch import batch_from_records
    sc = C.hetalt_scene()
    ref = sc.ref[:50] + "N" + sc.ref[51:60] + "acgt" + sc.ref[64:]
    empty = batch_from_records(C.CONTIG, len(ref), [])
    _configure(worker, sc.params)
    dev = Device(worker, empty, [(10, 300), (300, 301)], ref.encode(), order=ORDER)
    assert_same(dev, M.run(empty, ref, [(10, 300), (300, 301)], sc.params))
    assert set(dev.runs["state"].tolist()) == {M.NON_ACGT, M.NO_BASE} and dev.log == [0] * 14


def test_error_paths_run_nothing():
    """HIMUT_ERR_ARG (1): the map before any run, no reference, no chunks."""
    from himut_amd import _ffi, normcounts
    from himut_amd.caller import Worker
    sc = C.hetalt_scene()
    w = Worker(0)
    try:
        for call in (lambda: w.ctx.callable_map(1), lambda: w.ctx.callable()):
            with pytest.raises(_ffi.HimutError) as e:
                call()
            assert e.value.code == 1
        _configure(w, sc.params)
        w.load(sc.chunks, None, None, None, sc.batch)
        with pytest.raises(_ffi.HimutError) as e:             # no reference string
            w.ctx.run_callable(normcounts.alt_order_table(ORDER))
        assert e.value.code == 1 and "himut_set_reference" in e.value.message
        chars, cls = normcounts.tri_classes(sc.ref)
        w.ctx.set_reference(sc.ref, cls, len(chars))
        w.ctx.set_chunks([])
        with pytest.raises(_ffi.HimutError) as e:             # no chunks
            w.ctx.run_callable(normcounts.alt_order_table(ORDER))
        assert e.value.code == 1 and "chunks" in e.value.message
        with pytest.raises(_ffi.HimutError) as e:             # still no run has completed
            w.ctx.callable_map(1)
        assert e.value.code == 1
        assert w.ctx.stats()["ms_total"] == 0
        w.ctx.set_chunks(sc.chunks)
        w.ctx.run_callable(normcounts.alt_order_table(ORDER))
        runs, _log = w.ctx.callable()
        assert runs.shape[0] >= 3
    finally:
        w.close()
