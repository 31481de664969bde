"""phaselib.get_edges through the C ABI: the reference's golden vectors and the oracle
on a larger contig.  Bit-exact: the same edges, in the same order, with the same four counts."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["edges_basic", "edges_lowq"])
def test_edges_golden(case):
    from himut_amd import phaselib
    batch, exp = util.load_case(case)
    hets = [tuple(h) for h in exp["hetsnps"]]
    hidx = {h: i for i, h in enumerate(hets)}
    edge_lst, e2c = phaselib.get_edges(exp["contig"], None, exp["min_bq"], exp["min_mapq"], [h[0] for h in hets], hets, hidx,
                                       read_batch=batch)
    assert [list(e) for e in edge_lst] == exp["edge_lst"]
    assert {"{},{}".format(*k): [float(x) for x in v] for k, v in e2c.items()} == exp["edge2counts"]


def test_edges_oracle_parity_dense_snps():
    """2 Mb, hetSNPs dense enough that reads span more than 64 of them (several blocks of lanes per read)."""
    from oracle import oracle as O
    from himut_amd import phaselib, synth
    s = synth.generate(synth.SynthConfig(seed=71, contig_len=2_000_000, snp_rate=8e-3, name="chrH"))
    hets = sorted(set((int(p) + 1, chr(r), chr(a)) for p, r, a, g in zip(s.snp_pos, s.snp_ref, s.snp_alt, s.snp_gt)
                      if g in (1, 2)))
    hidx = {h: i for i, h in enumerate(hets)}
    o_lst, o_e2c = O.edges(s.batch, hets, 40, 20)
    edge_lst, e2c = phaselib.get_edges("chrH", None, 40, 20, [h[0] for h in hets], hets, hidx, read_batch=s.batch)
    assert O.edge_band(s.batch, [h[0] for h in hets]) > 64
    assert edge_lst == o_lst
    assert {k: [float(x) for x in v] for k, v in e2c.items()} == o_e2c
    assert len(edge_lst) > 100_000


# ---- hand-built cases (tests/edges_cases.py) against the reference-made fixtures edges_blocks / edges_rules and the
# ---- plain model (tests/edges_model.py); tests/test_edges_cpu.py pins model, oracle and fixtures to each other

ERR_ARG = 1                                                                    # HIMUT_ERR_ARG


def _unflat(flat):
    rows = [flat[k:k + 6] for k in range(0, len(flat), 6)]
    return [(r[0], r[1]) for r in rows], {(r[0], r[1]): r[2:] for r in rows}


def _ints(res):
    edge_lst, e2c = res
    return [tuple(e) for e in edge_lst], {tuple(k): [int(x) for x in v] for k, v in e2c.items()}


def _get_edges(batch, hets, min_bq, min_mapq, **kw):
    """phaselib.get_edges on the device, counts as integers."""
    from himut_amd import phaselib
    hets = [tuple(h) for h in hets]
    hidx = {h: i for i, h in enumerate(hets)}
    kw.setdefault("read_batch", batch)
    res = phaselib.get_edges(batch.name if batch is not None else "chrR", None, min_bq, min_mapq, [h[0] for h in hets], hets,
                             hidx, **kw)
    assert all(float(x) == int(x) for v in res[1].values() for x in v)
    return _ints(res)


def _model(batch, hets, min_bq, min_mapq):
    from tests import edges_model as M
    return _ints(M.edges(batch, hets, min_bq, min_mapq))


@pytest.fixture(scope="module")
def fixtures():
    """case -> (batch, hetSNPs, runs) of the two hand-built fixtures."""
    out = {}
    for case in ("edges_blocks", "edges_rules"):
        batch, exp = util.load_case(case)
        out[case] = (batch, [tuple(h) for h in exp["hetsnps"]], exp["runs"])
    return out


@pytest.fixture(scope="module")
def ctx():
    """A context of the tests' own with the parameter block the cs decode asks for (as phaselib.get_edges sets it)."""
    from himut_amd.caller import Worker
    w = Worker(0)
    w.configure(0, 0, 0, 1 << 30, 0.0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0, 1 / (10 ** 3), False)
    yield w.ctx
    w.close()


def _arrays(hets):
    return np.array([h[0] for h in hets], np.int32), np.array([ord(h[1]) for h in hets], np.uint8)


def _table(ctx, batch, hets, min_bq, min_mapq, band, push=True):
    if push:
        ctx.push_reads(batch)
    hpos, href = _arrays(hets)
    t = ctx.run_edges(hpos, href, min_bq, min_mapq, band)
    assert t.shape == (max(1, len(hets)) * band * 4,)
    return t


def _model_table(batch, hets, min_bq, min_mapq, band):
    from tests import edges_model as M
    return M.band_table(M.edges(batch, hets, min_bq, min_mapq)[1], len(hets), band)


@pytest.mark.parametrize("case", ["edges_blocks", "edges_rules"])
def test_hand_built_fixtures(fixtures, case):
    """Spans of exactly 0 ... 130 hetSNPs (edges_blocks); span ends, indels, soft clips, filters and deep edges at every
    pair of min_bq 0 ... 94 and min_mapq 0 ... 255 (edges_rules): what the reference's get_edges gave."""
    batch, hets, runs = fixtures[case]
    assert len(runs) == (1 if case == "edges_blocks" else 24)
    for run in runs:
        got = _get_edges(batch, hets, run["min_bq"], run["min_mapq"])
        assert got == _unflat(run["edges"]), (run["min_bq"], run["min_mapq"])


def test_spans_of_193_and_257_hetsnps():
    """Pairs three and four blocks of 64 lanes apart, last blocks of 1 lane: against the model and the oracle."""
    from oracle import oracle as O
    from tests import edges_cases as C
    case = C.blocks(C.BLOCKS_LARGE_K)
    batch = C.batch_of(case)
    for min_bq in (20, 21):
        want = _model(batch, case.hets, min_bq, 20)
        assert want == _ints(O.edges(batch, case.hets, min_bq, 20))
        assert max(j - i for i, j in want[0]) == (256 if min_bq == 20 else 255)      # hetSNP 256 has quality 20
        assert _get_edges(batch, case.hets, min_bq, 20) == want


@pytest.mark.parametrize("name", ["spans", "cs_geometry", "filters", "deep"])
def test_rule_cases_one_by_one(name):
    """Each rule case alone (12, 7, 22 and 303 reads: whole and partial workgroups of four) against the model."""
    from tests import edges_cases as C
    case = getattr(C, name)()
    batch = C.batch_of(case)
    for params in ((0, 0), (20, 20), (21, 21)):
        assert _get_edges(batch, case.hets, *params) == _model(batch, case.hets, *params), params


@pytest.mark.parametrize("case", ["edges_blocks", "edges_rules"])
def test_raw_band_table(ctx, fixtures, case):
    """The table himut_run_edges fills, not only its non-zero edges: the model's counts at [(i * band + (j - i - 1)) * 4 +
    k], zero in every slot that names no edge, the same for any band that is wide enough, HIMUT_ERR_ARG for one that is
    not."""
    from himut_amd import phaselib
    from himut_amd._ffi import HimutError
    batch, hets, runs = fixtures[case]
    n = len(hets)
    need = phaselib.edge_band(batch, [h[0] for h in hets])
    assert need >= 2
    for min_bq, min_mapq in ((20, 20), (0, 0)):
        want = _model_table(batch, hets, min_bq, min_mapq, need)
        assert int(want.sum()) > 0
        for k, band in enumerate((need, need + 1, 2 * need)):
            t = _table(ctx, batch, hets, min_bq, min_mapq, band, push=k == 0).reshape(n, band, 4)
            assert np.array_equal(t[:, :need, :].reshape(-1), want), band
            assert not t[:, need:, :].any(), band
            i, d = np.meshgrid(np.arange(n), np.arange(band), indexing="ij")
            assert not t[i + 1 + d >= n].any(), band
    with pytest.raises(HimutError) as e:
        _table(ctx, batch, hets, 0, 0, need - 1, push=False)
    assert e.value.code == ERR_ARG
    # the context is as good as before
    assert np.array_equal(_table(ctx, batch, hets, 0, 0, need, push=False), _model_table(batch, hets, 0, 0, need))


def test_degenerate_inputs(ctx, fixtures):
    """No hetSNP, one hetSNP, hetSNPs that no read spans, reads that are all filtered out: zeros and no error."""
    batch, hets, _ = fixtures["edges_rules"]
    ctx.push_reads(batch)
    for band in (1, 5):
        assert not _table(ctx, batch, [], 0, 0, band, push=False).any()
        assert not _table(ctx, batch, hets[:1], 0, 0, band, push=False).any()
        assert not _table(ctx, batch, [(2900, "A", "C"), (2950, "C", "G"), (2999, "G", "T")], 0, 0, band, push=False).any()
    assert int(batch.tend.max()) < 2899
    blocks, bhets, _ = fixtures["edges_blocks"]
    assert int(blocks.mapq.max()) == 60
    assert not _table(ctx, blocks, bhets, 0, 61, 129).any()
    assert _table(ctx, blocks, bhets, 0, 60, 129, push=False).any()


def test_runs_repeat_and_carry_nothing_over(ctx, fixtures):
    from tests import edges_cases as C
    blocks, bhets, _ = fixtures["edges_blocks"]
    a = _table(ctx, blocks, bhets, 20, 20, 129)
    b = _table(ctx, blocks, bhets, 20, 20, 129, push=False)
    assert a.any() and np.array_equal(a, b)
    deep = C.deep()
    batch = C.batch_of(deep)
    t = _table(ctx, batch, deep.hets, 20, 20, 4)
    assert np.array_equal(t, _model_table(batch, deep.hets, 20, 20, 4))
    assert sorted(t[t > 0].tolist()) == [3] * 10 + [300] * 10
    # the same hetSNP arrays as the run before, other reads; then a wider table than the one before
    assert np.array_equal(_table(ctx, batch, deep.hets, 20, 20, 129), _model_table(batch, deep.hets, 20, 20, 129))


def test_context_state_around_an_edge_run():
    """himut_run_edges between call runs: the records of the run before stay served and a rerun gives them again; the
    phase sets' arrays are reused, so a phased run is refused until himut_set_phase is called again, and then gives
    what it gave before."""
    from oracle import oracle as O
    from himut_amd import caller
    from himut_amd._ffi import HimutError
    from tests import edges_model as M
    batch, exp = util.load_case("worker_phase")
    p, chunks, phase_sets = util.params_of(exp), util.chunks_of(exp), util.phase_of(exp)
    hets = sorted(set(t for v in phase_sets[2].values() for t in v))
    hpos, href = _arrays(hets)
    band = O.edge_band(batch, hpos)
    want_edges = M.band_table(O.edges(batch, hets, 20, 20)[1], len(hets), band)
    assert want_edges.any()
    w = caller.Worker(0)
    try:
        def configure(phase):
            w.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"],
                        p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"],
                        p["md_threshold"], p["min_ref_count"], p["min_alt_count"], p["min_hap_count"],
                        p["germline_snv_prior"], phase)
        configure(False)
        recs, log = w.call_contig(batch, chunks)
        assert len(recs) > 0
        assert np.array_equal(w.ctx.run_edges(hpos, href, 20, 20, band), want_edges)
        assert np.array_equal(w.ctx.records(), recs) and w.ctx.log() == log
        w.ctx.run()
        assert np.array_equal(w.ctx.records(), recs) and w.ctx.log() == log
        configure(True)
        precs, plog = w.call_contig(batch, chunks, phase_sets=phase_sets)
        assert caller.records_to_tuples(exp["contig"], precs) == util.expected_tuples(exp) and plog == exp["log"]
        assert np.array_equal(w.ctx.run_edges(hpos, href, 20, 20, band), want_edges)
        with pytest.raises(HimutError) as e:
            w.ctx.run()
        assert e.value.code == ERR_ARG and "himut_set_phase has not been called" in str(e.value)
        w.ctx.set_phase(*caller.pack_phase_sets(chunks, *phase_sets))
        w.ctx.run()
        assert np.array_equal(w.ctx.records(), precs) and w.ctx.log() == plog
    finally:
        w.close()


def test_edges_through_a_bam(fixtures, tmp_path):
    """The edges_rules batch written as a BAM: the host reader's batch (soft clips, trailing insertions, long-form
    text) gives the fixture's results; the ingest that derives the cs text from CIGAR and the reference leaves reads
    in HBM that give the same.  The derivation cannot describe an N in SEQ as a match, so that file is written without
    the two reads that hold one, and the model says what the rest gives."""
    from himut_amd import bamio
    from himut_amd.caller import _worker_for
    from himut_amd.feed import ContigFeed
    from tests import edges_cases as C
    batch, hets, runs = fixtures["edges_rules"]
    bam = str(tmp_path / "rules.bam")
    bamio.write_bam(bam, [batch])
    loaded = bamio.BamFile(bam).batches["chrR"]
    assert loaded.n == batch.n and int(loaded.qstart.max()) == 7
    for run in runs:
        assert _get_edges(loaded, hets, run["min_bq"], run["min_mapq"]) == _unflat(run["edges"]), (run["min_bq"], run["min_mapq"])
    case = C.rules(derivable_only=True)
    assert case.hets == hets and len(case.records) == batch.n - 2
    derivable = C.batch_of(case)
    bam2, fa = str(tmp_path / "derivable.bam"), str(tmp_path / "rules.fa")
    bamio.write_bam(bam2, [derivable])
    with open(fa, "w") as o:
        o.write(">chrR\n" + "\n".join(case.ref[i:i + 60] for i in range(0, len(case.ref), 60)) + "\n")
    with ContigFeed(bam2, None, None, 1, (0,)) as feed:
        feed.derive_cs_from(fa)
        _w, resident = feed.ingest("chrR", worker=_worker_for(0))
        assert resident["n_reads"] == derivable.n
        n_edges = 0
        for run in runs:
            want = _model(derivable, hets, run["min_bq"], run["min_mapq"])
            got = _get_edges(None, hets, run["min_bq"], run["min_mapq"], read_batch=None, resident=resident)
            assert got == want, (run["min_bq"], run["min_mapq"])
            n_edges += len(want[0])
        assert n_edges > 500
