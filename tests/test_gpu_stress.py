"""Context reuse: the golden cases run repeatedly in random order through ONE context.
Catches state that leaks between contigs (stale device buffers, out-of-range probes)."""
import random

import pytest

from tests import util

pytestmark = pytest.mark.gpu


def test_random_order_reuse():
    from himut_amd import caller
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _run_hip
    w = Worker(0)
    try:
        data = {}
        for c in util.WORKER_CASES + util.PHASE_CASES:
            batch, exp = util.load_case(c)
            p = util.params_of(exp)
            pon = caller.site_keys([tuple(t) for t in exp["pon_set"]]) if "pon_set" in exp else None
            com = caller.site_keys([tuple(t) for t in exp["common_set"]]) if "common_set" in exp else None
            data[c] = (batch, exp, p, pon, com)
        rnd = random.Random(1)
        prev = None
        for _ in range(4):
            order = list(data)
            rnd.shuffle(order)
            for c in order:
                batch, exp, p, pon, com = data[c]
                recs, log = _run_hip(w, batch, util.chunks_of(exp), p, pon, com, util.phase_of(exp))
                got = caller.records_to_tuples(exp["contig"], recs)
                assert got == util.expected_tuples(exp), "{} after {}".format(c, prev)
                assert log == exp["log"], "{} after {}".format(c, prev)
                prev = c
    finally:
        w.close()


def test_kept_capacities_small_large_small():
    """A context keeps the candidate / column capacities of its last sized run and launches the next
    one without waiting for the counts (design 6).  A larger contig after a smaller one
    overflows them and is repeated with exact sizes; a smaller one afterwards runs inside capacities
    far larger than it needs.  Every run must equal the oracle, whichever way it was sized."""
    import numpy as np
    from oracle import oracle as O
    from himut_amd import synth, util as hutil
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _run_hip
    sizes = [60_000, 900_000, 60_000, 250_000, 900_000]
    w = Worker(0)
    try:
        for k, L in enumerate(sizes):
            s = synth.generate(synth.SynthConfig(seed=70 + (k % 2), contig_len=L, read_len_mean=6000, read_len_sd=1200,
                                                 read_len_min=2000, read_len_max=12000, som_rate=1e-4, name="chr7"))
            b = s.batch
            chunks = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
            p = dict(util.CALL_DEFAULTS, qlen_lower_limit=3000, qlen_upper_limit=11000, md_threshold=52)
            orecs, olog = O.call(b, chunks, p, p["germline_snv_prior"], None, None, None)
            for _ in range(2):        # the second pass of a size always runs on kept capacities
                hrecs, hlog = _run_hip(w, b, chunks, p)
                assert hlog == olog, (k, L)
                assert len(hrecs) == len(orecs)
                for name in ("tpos", "chunk", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum"):
                    assert np.array_equal(hrecs[name], orecs[name]), (k, L, name)
                st = w.ctx.stats()
                assert st["n_records"] == len(orecs) and st["n_candidates"] >= len(orecs)
    finally:
        w.close()


def test_stage_timing_levels():
    """himut_set_stage_timing: which stage times a run reports (0 total, 1 + capture, 2 all)."""
    from himut_amd import synth, util as hutil
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _run_hip
    s = synth.generate(synth.SynthConfig(seed=77, contig_len=300_000, read_len_mean=6000, read_len_sd=1200,
                                         read_len_min=2000, read_len_max=12000, name="chr7"))
    b = s.batch
    chunks = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=3000, qlen_upper_limit=11000, md_threshold=52)
    w = Worker(0)
    try:
        ref = None
        for level in (1, 0, 2, 1):
            w.ctx.set_stage_timing(level)
            recs, log = _run_hip(w, b, chunks, p)
            ref = ref or (recs.tobytes(), log)
            assert (recs.tobytes(), log) == ref
            st = w.ctx.stats()
            assert st["ms_total"] > 0
            assert (st["ms_capture"] > 0) == (level >= 1)
            assert (st["ms_parse"] > 0) == (level >= 2) and (st["ms_eval"] > 0) == (level >= 2)
        with pytest.raises(Exception):
            w.ctx.set_stage_timing(3)
    finally:
        w.close()


# ---- the repeat on kept capacities: himut_run and its two-half form

def _tiled(length, step=10_000):
    return [(s, min(s + step, length)) for s in range(0, length, step)]


def _same(got, want):
    return got[1] == want[1] and got[0].tobytes() == want[0].tobytes()


@pytest.fixture(scope="module")
def sized():
    """30 kb and 260 kb: both span many 256-position blocks and several chunks, and the step from the small one to
    the large one overflows the capacities a context keeps.  With each, what a fresh context gives."""
    from himut_amd import synth
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _run_hip
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=3000, qlen_upper_limit=11000, md_threshold=52)
    out = {"p": p}
    for name, L in (("small", 30_000), ("large", 260_000)):
        b = synth.generate(synth.SynthConfig(seed=90, contig_len=L, read_len_mean=6000, read_len_sd=1200, read_len_min=2000,
                                             read_len_max=12000, som_rate=1e-4, name="chr9")).batch
        w = Worker(0)
        try:
            out[name] = (b, _tiled(L), _run_hip(w, b, _tiled(L), p))
            assert w.ctx.stats()["reran"] == 0
        finally:
            w.close()
    assert len(out["small"][2][0]) > 0 and len(out["large"][2][0]) > len(out["small"][2][0])
    return out


SEQUENCE = ("small", "large", "large", "small")


@pytest.fixture(scope="module")
def run_path(sized):
    """SEQUENCE through himut_run on one context: per run (records, log), and `reran`."""
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _run_hip
    w = Worker(0)
    try:
        got, reran = [], []
        for name in SEQUENCE:
            b, chunks, _ = sized[name]
            got.append(_run_hip(w, b, chunks, sized["p"]))
            reran.append(w.ctx.stats()["reran"])
        return got, reran
    finally:
        w.close()


def test_repeat_on_kept_capacities_is_reported(sized, run_path):
    """small, large, large, small on one context: the first large run overflows what the small one kept and is made
    again with exact sizes (reran), no other run is; each gives the records and counters of a fresh context."""
    got, reran = run_path
    assert reran == [0, 1, 0, 0]
    for name, g in zip(SEQUENCE, got):
        assert _same(g, sized[name][2]), name


def test_two_half_run_repeats_like_the_whole_one(sized, run_path):
    """The same sequence through himut_run_begin / himut_run_end (the overflow shows in the second half, which makes
    the run again): records, counters and reran equal himut_run's."""
    import numpy as np
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _configure
    w = Worker(0)
    try:
        got, reran = [], []
        for name in SEQUENCE:
            b, chunks, _ = sized[name]
            _configure(w, sized["p"], False)
            w.ctx.set_chunks(chunks)
            w.ctx.set_site_set(0, np.zeros(0, np.uint64)); w.ctx.set_site_set(1, np.zeros(0, np.uint64))
            w.ctx.push_reads(b)
            w.ctx.run_begin()
            w.ctx.run_end()
            got.append((w.ctx.records(), w.ctx.log()))
            reran.append(w.ctx.stats()["reran"])
        assert reran == run_path[1] == [0, 1, 0, 0]
        for name, g, r in zip(SEQUENCE, got, run_path[0]):
            assert _same(g, r), name
    finally:
        w.close()


# ---- the candidate-count step: no candidates at all, and a chunk list that is not in order

RECORD_FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum")


def _equals_oracle(got, want):
    import numpy as np
    (recs, log), (orecs, olog) = got, want
    return (log == olog and len(recs) == len(orecs) and not recs["flags"].any()
            and all(np.array_equal(recs[k], orecs[k]) for k in RECORD_FIELDS))


def test_reads_that_propose_nothing_between_runs_that_do():
    """Five clean reads propose nothing: no candidate, no mask sweep, and num_ccs comes from k_count_flags.  A sixth
    with one low-quality substitution gives one candidate and the counters of k_finalize_flags.  Empty-handed, one
    candidate, empty-handed twice on ONE context: the mask and bitmap left for the next run go through both branches
    of the finalisation, and every run equals the oracle."""
    from oracle import oracle as O
    from himut_amd.caller import Worker
    from himut_amd.readbatch import batch_from_records
    from tests.test_gpu_parity import _run_hip
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=10, qlen_upper_limit=10000, md_threshold=52)
    seq = "ACGT" * 50
    clean = [dict(tstart=10 + k, tend=210 + k, seq=seq, bq=[93] * 200, cs=":200") for k in range(5)]
    sub = dict(tstart=12, tend=212, seq=seq[:100] + "T" + seq[101:], bq=[93] * 100 + [5] + [93] * 99, cs=":100*at:99")
    chunks = [(0, 1000)]
    batch = {"none": batch_from_records("c", 1000, clean),
             "one": batch_from_records("c", 1000, sorted(clean + [sub], key=lambda r: r["tstart"]))}
    want = {k: O.call(b, chunks, p, p["germline_snv_prior"]) for k, b in batch.items()}
    assert len(want["none"][0]) == 0 and want["none"][1] == [5] + [0] * 14
    assert len(want["one"][0]) == 1 and want["one"][1] == [6, 1, 0, 0, 0, 1] + [0] * 9
    w = Worker(0)
    try:
        for step, name in enumerate(("none", "one", "none", "none")):
            got = _run_hip(w, batch[name], chunks, p)
            assert _equals_oracle(got, want[name]), (step, name, got[1])
            assert w.ctx.stats()["reran"] == 0, (step, name)
    finally:
        w.close()


def test_unordered_chunks_around_a_kept_capacity_run():
    """A chunk list out of coordinate order takes the sort and never runs on kept capacities; an ordered one does from
    its second run.  unordered, unordered, ordered, ordered, unordered on one context, through himut_run and through
    himut_run_begin / himut_run_end: the last run needs the sort's temporary storage behind a run that sized nothing.
    Every run equals the oracle, the two forms equal each other, nothing is run again."""
    import numpy as np
    from oracle import oracle as O
    from himut_amd import synth
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _configure, _run_hip
    b = synth.generate(synth.SynthConfig(seed=5, contig_len=120_000, read_len_mean=5000, read_len_sd=900, read_len_min=2000,
                                         read_len_max=9000, som_rate=2e-4, name="chr5")).batch
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=3000, qlen_upper_limit=7500, md_threshold=52)
    chunks = {"unordered": [(50_000, 90_000), (1000, 60_000), (59_990, 60_010), (100_000, 120_000)],
              "ordered": [(1000, 60_000), (60_000, 120_000)]}
    want = {k: O.call(b, ch, p, p["germline_snv_prior"]) for k, ch in chunks.items()}
    assert len(want["unordered"][0]) == 1071 and len(want["ordered"][0]) == 1182
    order = ("unordered", "unordered", "ordered", "ordered", "unordered")

    def whole(w, ch):
        return _run_hip(w, b, ch, p)

    def halves(w, ch):
        _configure(w, p, False)
        w.ctx.set_chunks(ch)
        w.ctx.set_site_set(0, np.zeros(0, np.uint64)); w.ctx.set_site_set(1, np.zeros(0, np.uint64))
        w.ctx.push_reads(b)
        w.ctx.run_begin()
        w.ctx.run_end()
        return w.ctx.records(), w.ctx.log()
    got = {}
    for form in (whole, halves):
        w = Worker(0)
        try:
            got[form] = []
            for step, name in enumerate(order):
                g = form(w, chunks[name])
                assert _equals_oracle(g, want[name]), (form.__name__, step, name, g[1])
                assert w.ctx.stats()["reran"] == 0, (form.__name__, step, name)
                got[form].append(g)
        finally:
            w.close()
    for step, (a, h) in enumerate(zip(got[whole], got[halves])):
        assert _same(a, h), step
