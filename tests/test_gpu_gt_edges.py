"""Genotype calls and GQ cut-offs at fp64 rounding boundaries on the GPU: the piles of tests/gt_piles.py through the
call run (k_eval_columns) and normcounts (k_norm_quad's pure-reference path, k_norm_dirty, k_norm_tile).  Expected
values come from the fixtures (tests/golden/gt_edges.json and leaf_gtlib.json, the reference's gtlib outputs); the CPU oracle
must agree as well.  A kernel that keeps the maths but changes the rounding -- partial sums, another association, the
prior added first, contracted multiply-adds -- moves some of these decisions."""
import numpy as np
import pytest

from tests import gt_piles as G
from tests import util
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
