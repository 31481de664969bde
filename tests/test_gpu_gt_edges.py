"""Genotype calls and GQ cut-offs at fp64 rounding boundaries on the GPU: the piles of tests/gt_piles.py through the
call run (k_eval_columns), normcounts (k_norm_quad's pure-reference path, k_norm_dirty, k_norm_tile), the callable run
(k_callmap_sweep: its own column walk, two rows at a time over a zero table row, under its own register budget) and,
laid out as halves of doublet candidates (gt_piles.build_dbs), the dbs run (k_dbs_eval: dbs_half's separate sums of the
reference and the alt allele).  Expected values come from the fixtures (tests/golden/gt_edges.json and leaf_gtlib.json,
the reference's gtlib outputs); the CPU oracle and the plain models (tests/callmap_model.py, tests/dbs_model.py) must
agree as well.  A kernel that keeps the maths but changes the rounding -- partial sums, another association, the
prior added first, contracted multiply-adds -- moves some of these decisions: every state of the callable map and
every half of a doublet record is held against the fixture, not only against the model."""
import numpy as np
import pytest

from tests import callmap_model
from tests import dbs_model
from tests import gt_piles as G
from tests import util
from tests.test_callmap_cpu import EDGE_KINDS, EDGE_MODES, check_columns, edge_model, edges_of, leaf_model
from tests.test_dbs_cpu import DBS_KINDS, LEAF_K, check_halves, doublets_of, edge_doublet_model, leaf_doublet_model
from tests.test_gpu_callmap import Device, assert_same as assert_same_map
from tests.test_gpu_dbs import _dbs, ctx  # noqa: F401  (ctx: the module-scoped context fixture)
from tests.test_gt_edges_cpu import ORDER, check_records

pytestmark = pytest.mark.gpu

CALL_FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum")
FORCED = {"tile": dict(sweep=1), "pool": dict(pool_slots=1), "dirty": dict(dirty_cap=1)}


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _configure(w, p, phase=False):
    w.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"],
                p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"],
                p["md_threshold"], p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"],
                phase)


def _call(w, vs, P, p):
    """The call run on the pile: log and records equal the oracle's, and each column's records carry the fixture's gq,
    genotype and state."""
    from oracle import oracle as O
    _configure(w, p)
    recs, log = w.call_contig(P.batch, P.call_chunks)
    orecs, olog = O.call(P.batch, P.call_chunks, p, p["germline_snv_prior"])
    assert log == olog
    assert len(recs) == len(orecs)
    for name in CALL_FIELDS:
        assert np.array_equal(recs[name], orecs[name]), name
    check_records(vs, P, recs, p["min_gq"])


def _norm(w, vs, P, p, copies=1, **dbg):
    """normcounts on the pile (under a forced path if dbg says so): the log the fixture implies, the oracle's log and
    tri dicts.  Returns the run's stats."""
    from himut_amd import normcounts
    from oracle import oracle as O
    _configure(w, p)
    if dbg:
        w.ctx.debug_normcounts(**dbg)
    try:
        ccs, ref, log = normcounts.norm_contig(w, P.batch, P.norm_chunks, P.refseq, alt_order=ORDER)
        st = w.ctx.stats()
    finally:
        w.ctx.debug_normcounts()
    assert log == G.norm_log(vs, p["min_gq"], ORDER, p["min_ref_count"], p["min_alt_count"], copies=copies), dbg
    o_ccs, o_ref, o_log = O.normcounts(P.batch, P.norm_chunks, p, P.refseq, p["germline_snv_prior"], alt_order=ORDER)
    assert log == o_log and ccs == o_ccs and ref == o_ref, dbg
    return st


@pytest.fixture(scope="module")
def leaf():
    vs = G.leaf_vectors(util.load_json("leaf_gtlib")["vectors"])
    return vs, G.params(20, 1 / (10 ** 3), max(len(v["alleles"]) for v in vs))


def test_leaf_vectors_call(worker, leaf):
    """leaf_gtlib's 400 columns, one pile at prior 1e-3: k_eval_columns."""
    vs, p = leaf
    _call(worker, vs, G.build(vs), p)


def test_leaf_vectors_normcounts(worker, leaf):
    """The same columns through normcounts: the quad sweep, then the whole contig by k_norm_tile; then each column
    twice in one chunk, so that a wave needs two pool slots and a workgroup two entries of its left-over list: one pool
    slot sends the tiles to k_norm_tile, a list part of one entry makes the sweep run again."""
    vs, p = leaf
    P = G.build(vs)
    st = _norm(worker, vs, P, p)
    assert st["reran"] == 0 and st["column_slots"] == 0
    _norm(worker, vs, P, p, **FORCED["tile"])
    T = G.build(vs, twin=True)
    st = _norm(worker, vs, T, p, copies=2)
    assert st["reran"] == 0 and st["column_slots"] == 0
    st = _norm(worker, vs, T, p, copies=2, **FORCED["pool"])
    assert st["reran"] == 0 and st["column_slots"] > 0
    st = _norm(worker, vs, T, p, copies=2, **FORCED["dirty"])
    assert st["reran"] == 1


@pytest.fixture(scope="module")
def edges():
    return util.load_json("gt_edges")["vectors"]


def test_gt_edges_call(worker, edges):
    """Each boundary vector in its own pile at its own prior with min_gq = k: the records of k_eval_columns (columns
    deeper than a wave included)."""
    for i, v in enumerate(edges):
        P = G.build([v], orders=[G.ORDERS[i % 3]])
        _call(worker, [v], P, G.params(v["k"], v["prior"], len(v["alleles"])))


def test_gt_edges_normcounts(worker, edges):
    """Each boundary vector in its own pile at its own prior with min_gq = k through normcounts: the quad sweep (a
    column deeper than the plan's 128 items goes to k_norm_tile), the whole contig by k_norm_tile, and the column twice
    in one chunk by the quad sweep, with one pool slot and with a left-over list part of one entry."""
    seen = {"deep": 0, "pool": 0, "dirty": 0}
    for i, v in enumerate(edges):
        depth = len(v["alleles"])
        p = G.params(v["k"], v["prior"], depth)
        P = G.build([v], orders=[G.ORDERS[i % 3]])
        st = _norm(worker, [v], P, p)
        assert st["reran"] == 0
        assert (st["column_slots"] > 0) == (depth > 128), v
        seen["deep"] += st["column_slots"] > 0
        _norm(worker, [v], P, p, **FORCED["tile"])
        T = G.build([v], orders=[G.ORDERS[i % 3]], twin=True)
        _norm(worker, [v], T, p, copies=2)
        st = _norm(worker, [v], T, p, copies=2, **FORCED["pool"])
        seen["pool"] += st["column_slots"] > 0
        st = _norm(worker, [v], T, p, copies=2, **FORCED["dirty"])
        seen["dirty"] += st["reran"]
    # the forced paths ran where the columns can take them (not the pure-reference columns k_norm_quad settles)
    print("gt_edges normcounts paths:", seen, "of", len(edges))
    assert seen["deep"] == sum(len(v["alleles"]) > 128 for v in edges)
    assert seen["pool"] > 0 and seen["dirty"] > 0, seen


def _callable(w, model, mode):
    """The callable run on a pile: every column's state and bases equal the fixture's; map, runs and log equal the
    model's; over the columns' own chunks the map folds to the norm.log the fixture implies."""
    vs, P, chunks, p, res = model
    _configure(w, p)
    dev = Device(w, P.batch, chunks, P.refseq, order=ORDER)
    check_columns(dev, vs, P, chunks, p, mode)
    assert_same_map(dev, res)
    if mode != "wide":
        want = G.norm_log(vs, p["min_gq"], ORDER, p["min_ref_count"], p["min_alt_count"], copies=len(P.cols[0]))
        assert dev.log == want and callmap_model.fold(dev, P.refseq)[0][1:] == want[1:], vs[0]["id"]


@pytest.mark.parametrize("mode", EDGE_MODES)
def test_leaf_vectors_callable(worker, mode):
    """leaf_gtlib's 400 columns, one pile at prior 1e-3: k_callmap_sweep over the columns' own chunks, with every
    column twice in one tile, and over the wide chunks (the column in the middle of a tile)."""
    _callable(worker, leaf_model(mode), mode)


@pytest.mark.parametrize("mode", EDGE_MODES)
@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_gt_edges_callable(worker, kind, mode):
    """Each boundary vector in its own pile at its own prior with min_gq = k through k_callmap_sweep, in the three
    layouts; columns up to depth 1000 cross many of the sweep's 48-row batches."""
    for i in edges_of(kind):
        _callable(worker, edge_model(i, mode), mode)


def test_leaf_vectors_dbs(ctx):  # noqa: F811
    """The leaf columns that hold another allele as halves of doublets in one contig and one region: more than 256 keys
    (two workgroups of k_dbs_eval), record bytes and counters equal the model's, every record's half the fixture's."""
    vs, P, kw, prior, want, wlog = leaf_doublet_model()
    recs, log = _dbs(ctx, P.batch, P.regions, kw, prior=prior)
    assert log[5] > 256 and ctx.stats()["n_candidates"] > 256
    assert len(check_halves(recs, vs, P, LEAF_K)["leaf"]) == len(recs) > 0
    dbs_model.assert_same(recs, log, want, wlog)
    assert any((int(t) - 1) // 256 != int(t) // 256 for t in recs["tpos"])


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("kind", DBS_KINDS)
def test_gt_edges_dbs(ctx, kind, half):  # noqa: F811
    """Every (vector, alt, half) pile at its own prior with min_gq = k through k_dbs_eval: records and counters equal
    the model's, the vector's half carries the fixture's gt, gq and state, LowGQ where a homref half's gq is below k."""
    n = 0
    for d in doublets_of(kind, half):
        v, P, kw, prior, want, wlog = edge_doublet_model(*d)
        recs, log = _dbs(ctx, P.batch, P.regions, kw, prior=prior)
        n += len(check_halves(recs, [v], P, None)[kind])
        dbs_model.assert_same(recs, log, want, wlog)
    assert n > 0
