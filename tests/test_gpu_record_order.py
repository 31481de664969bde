"""The order of the records of the germline, dbs and call runs where the record back end (himut_amd/csrc/himut_emit.h)
can get it wrong: a thread's place among its workgroup's emitting threads (wg_rank), the move of a workgroup's records
behind those of the workgroups in front of it (k_compact_runs; the call run's k_run_totals / k_compact), and the
de-duplication of a HetAltSite pair across a workgroup edge.  Every comparison is against the plain models
(tests/germline_model.py, tests/dbs_model.py) or the oracle, never against the code under test; the tests without a GPU
mark assert, from the models alone, that the inputs put the boundaries where they are meant to be.

Germline.  k_germline_eval takes 8192 positions per workgroup and 256 marked positions per round.  The issue that asked
for these tests wants, on one contig of 3 x 8192 positions, workgroup 1 without a marked position AND positions 8191
and 8192 (0-based) both marked: 8192 is workgroup 1's first position, so one contig cannot have both.  There are two
contigs that differ in position 8192 only ("gap": workgroup 1 holds nothing; "edge": it holds 8192 alone), and a third,
"dense", whose marked positions exceed the capacity a run on "gap" keeps."""
import functools

import numpy as np
import pytest

from tests import dbs_cases as DC
from tests import dbs_model as DM
from tests import germline_model as GM

WG = 8192                        # positions per workgroup of k_germline_eval
LENGTH = 3 * WG
PRIOR = 1 / (10 ** 3)
KINDS = ("gap", "edge", "dense")


# ---- germline

def _marks(kind):
    """{0-based position: whether its column is reported without report_homref}"""
    step, n0 = (4, 1700) if kind == "dense" else (20, 300)
    # workgroup 0: in the first round of 256 every third marked position reports nothing, behind it every second one
    marks = {7 + step * i: (i % 3 != 0) if i < 256 else (i % 2 == 0) for i in range(n0)}
    marks[WG - 1] = True                                   # the last position of workgroup 0
    if kind == "edge":
        marks[WG] = True                                   # the first position of workgroup 1
    marks.update({2 * WG: True, 2 * WG + 116: False, 2 * WG + 3616: True, LENGTH - 300: True})
    return marks


@functools.lru_cache(maxsize=None)
def germ_batch(kind):
    """Six layers of reads of 1024 bases, each layer 128 further left than the one before: six reads over every position.
    A reported position: every read holds the other base (homalt).  A silent one: one read holds it at quality 2 among
    five reference reads of quality 93 (homref)."""
    from himut_amd.readbatch import batch_from_records
    ref, a1, _a2, _a3 = DC.contig(LENGTH, seed=11)
    marks = _marks(kind)
    at = sorted(marks)
    reads = []
    for layer in range(6):
        for s in range(-128 * layer, LENGTH, 1024):
            lo, hi = max(s, 0), min(s + 1024, LENGTH)
            mine = [p for p in at[np.searchsorted(at, lo):np.searchsorted(at, hi)] if marks[p] or layer == 0]
            reads.append(GM.make_read(ref, lo, hi - lo, {p: a1[p] for p in mine}, bq=93, bq_at={p: 2 for p in mine if not marks[p]}))
    reads.sort(key=lambda r: r["tstart"])
    return batch_from_records("chrO", LENGTH, reads)


@functools.lru_cache(maxsize=None)
def germ_want(kind, homref):
    return GM.run(germ_batch(kind), [(1, LENGTH)], PRIOR, report_homref=homref)


@pytest.mark.parametrize("kind", KINDS)
def test_germline_fixture_reaches_every_boundary(kind):
    """From the model alone: the marked positions per window of 8192, silent ones among the first 256 of workgroup 0 with
    reported ones behind them, both kinds from rank 256 on, the empty window, the two positions at the workgroup edge."""
    every, _ = germ_want(kind, True)                       # a record per marked position
    said, _ = germ_want(kind, False)
    marked = [int(t) - 1 for t in every["tpos"]]
    assert marked == sorted(_marks(kind))
    speaks = set(int(t) - 1 for t in said["tpos"])
    assert speaks == {p for p, e in _marks(kind).items() if e}
    per_wg = [sum(1 for p in marked if p // WG == w) for w in range(3)]
    w0 = [p in speaks for p in marked if p < WG]
    assert per_wg[0] > 256 and per_wg[1] == (1 if kind == "edge" else 0) and 1 <= per_wg[2] <= 8, per_wg
    first, rest = w0[:256], w0[256:]
    assert not all(first) and any(first[first.index(False):])      # a record whose place is in front of its thread
    assert any(rest) and not all(rest)
    assert WG - 1 in speaks and (WG in speaks) == (kind == "edge") and 2 * WG in speaks
    if kind == "dense":                                            # more than a run on "gap" keeps room for
        gap = len(germ_want("gap", True)[0])
        assert len(marked) > gap + gap // 4 + 1024


def _germ_run(c, batch, homref, push):
    from himut_amd import gtlib
    c.set_gt_lut(*gtlib.build_tables(PRIOR))
    c.set_chunks([(1, LENGTH)])
    if push:
        c.push_reads(batch)
    c.run_germline(report_homref=homref)
    return c.germline()


def _germ_check(got, glog, kind, homref):
    GM.assert_same(got, glog, *germ_want(kind, homref))
    assert np.all(np.diff(got["tpos"].astype(np.int64)) > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("homref", [False, True])
@pytest.mark.parametrize("kind", ["gap", "edge"])
def test_germline_order_across_rounds_and_workgroups(kind, homref):
    """A fresh context: the run with exact sizes, the run on the capacities it kept, then a contig whose marked positions
    overflow them (the run is made again with exact sizes)."""
    from himut_amd import _ffi
    with _ffi.Context(0) as c:
        _germ_check(*_germ_run(c, germ_batch(kind), homref, True), kind, homref)
        assert c.stats()["reran"] == 0
        _germ_check(*_germ_run(c, germ_batch(kind), homref, False), kind, homref)
        assert c.stats()["reran"] == 0
        _germ_check(*_germ_run(c, germ_batch("dense"), homref, True), "dense", homref)
        assert c.stats()["reran"] == 1


# ---- dbs

@functools.lru_cache(maxsize=None)
def dbs_case():
    (case,) = DC.order_cases()
    _name, batch, regions, kw, _expect = case
    return case, DM.run(batch, regions, prior=PRIOR, **kw)


def test_dbs_fixture_fills_a_workgroup_with_one_key():
    """From the model alone: nothing is dropped, so the sorted keys are the records' candidates, each as often as it was
    proposed; keys 256 .. 511 (workgroup 1 of k_dbs_eval) are all the one deep candidate, which starts in workgroup 0
    and ends in workgroup 2 with a candidate on either side."""
    (_name, _batch, _regions, _kw, expect), (want, wlog) = dbs_case()
    expect(want, wlog)
    assert wlog[5] == 3 and wlog[6] == 0
    keys = [k for k, r in enumerate(want) for _ in range(int(r["n_proposers"]))]
    assert set(keys[256:512]) == {1} and keys[0] == 0 and keys[255] == 1 and keys[512] == 1 and keys[-1] == 2 and len(keys) > 512


@pytest.mark.gpu
def test_dbs_order_with_a_silent_workgroup():
    from himut_amd import _ffi
    from tests.test_gpu_dbs import _dbs
    (_name, batch, regions, kw, expect), (want, wlog) = dbs_case()
    with _ffi.Context(0) as c:
        got, glog = _dbs(c, batch, regions, kw, prior=PRIOR)
    DM.assert_same(got, glog, want, wlog)
    expect(got, glog)


# ---- call

CALL_LENGTH = 6000
N_HEAD, N_HET0, N_HET1, N_TAIL = 5, 250, 264, 5          # emitted, germline, the HetAltSite pair, germline, emitted
CALL_FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum")


@functools.lru_cache(maxsize=None)
def call_case():
    """(batch, candidates in record-key order, the HetAltSite position, parameters).  One candidate column every eight
    positions, six reads deep (seven at the HetAltSite column): a lone alt read (reported), three alt reads of six (het:
    dropped as germline), and three reads each of two alt alleles beside one reference read (HetAltSite, two candidates)."""
    from himut_amd.readbatch import batch_from_records
    ref, a1, a2, _a3 = DC.contig(CALL_LENGTH, seed=12)
    kinds = ["one"] * N_HEAD + ["het"] * N_HET0 + ["hetalt"] + ["het"] * N_HET1 + ["one"] * N_TAIL
    col = {100 + 8 * k: kind for k, kind in enumerate(kinds)}
    at = sorted(col)
    hetalt = next(p for p in at if col[p] == "hetalt")

    def subs(layer, lo, hi):
        out = {}
        for p in at[np.searchsorted(at, lo):np.searchsorted(at, hi)]:
            if col[p] == "hetalt":
                if layer < 6:
                    out[p] = (a1 if layer < 3 else a2)[p]
            elif layer < (1 if col[p] == "one" else 3):
                out[p] = a1[p]
        return out
    reads = []
    for layer in range(7):                                  # the seventh layer: the reference read of the HetAltSite column
        for s in range(-100 * layer, CALL_LENGTH, 1000):
            lo, hi = max(s, 0), min(s + 1000, CALL_LENGTH)
            if layer < 6 or lo <= hetalt < hi:
                reads.append(GM.make_read(ref, lo, hi - lo, subs(layer, lo, hi), bq=93))
    reads.sort(key=lambda r: r["tstart"])
    cands = sorted((p + 1, "ATGC".index(ref[p]), "ATGC".index(a[p])) for p in at for a in ((a1, a2) if col[p] == "hetalt" else (a1,)))
    return batch_from_records("chrO", CALL_LENGTH, reads), cands, hetalt + 1, dict(DC.OPEN)


@functools.lru_cache(maxsize=None)
def call_want():
    from oracle import oracle as O
    batch, _cands, _tpos, p = call_case()
    return O.call(batch, [(0, CALL_LENGTH)], p, PRIOR)


def test_call_fixture_has_a_silent_workgroup_and_a_pair_across_its_edge():
    """From the oracle alone: every substitution is a candidate; candidates 255 and 256 are the HetAltSite pair, reported
    once; no candidate from 256 to 511 (workgroup 1 of k_compact) is reported, candidates on either side are."""
    from oracle import oracle as O
    _batch, cands, hetalt, _p = call_case()
    recs, log = call_want()
    assert log[1] == len(cands) > 512
    told = {(int(r["tpos"]), "ATGC".index(chr(r["ref"])), "ATGC".index(chr(r["alt"]))) for r in recs}
    assert len(told) == len(recs) and told <= set(cands)
    index = sorted(cands.index(t) for t in told)
    assert cands[255][0] == cands[256][0] == hetalt
    assert [O.STATUS[int(r["status"])] for r in recs if int(r["tpos"]) == hetalt] == ["HetAltSite"]
    assert index == list(range(N_HEAD)) + [255] + list(range(len(cands) - N_TAIL, len(cands))), index
    assert log[2] == N_HET0 + N_HET1 and index[-N_TAIL] >= 512


@pytest.mark.gpu
def test_call_order_with_a_silent_workgroup():
    from himut_amd import _ffi, gtlib
    from tests.test_gpu_column_shared import PARAM_NAMES
    batch, _cands, _tpos, p = call_case()
    want, wlog = call_want()
    with _ffi.Context(0) as c:
        c.set_params(**{k: p[k] for k in PARAM_NAMES})
        c.set_gt_lut(*gtlib.build_tables(PRIOR))
        c.set_site_set(0, np.zeros(0, np.uint64))
        c.set_site_set(1, np.zeros(0, np.uint64))
        c.push_reads(batch)
        c.set_chunks([(0, CALL_LENGTH)])
        c.run()
        got, glog = c.records(), c.log()
    assert [int(x) for x in glog] == wlog
    assert len(got) == len(want)
    for name in CALL_FIELDS:
        assert np.array_equal(got[name], want[name]), name
