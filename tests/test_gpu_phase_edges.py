"""The hand-built phased cases of tests/phase_cases.py on the GPU: k_read_hap and the haplotype vote of k_eval_columns<true>
(by column row and by query name) through `Worker.call_contig` and `normcounts.norm_contig`, against the CPU oracle, against
what the reference gave (tests/golden/phase_edges.json) and against each case's own statement.  Bit-exact.

HIMUT_ERR_COVER has no case: k_read_hap reports it for a hetSNP under the read that no segment covers (the reference's
KeyError in tpos2qbase), and the segments of a valid cs tag -- matches, substitutions and deletions -- cover every
position of [tstart, tend) while the hetSNPs under a read are those at the 1-based positions tstart + 1 .. tend.  Only a
tag that does not add up to tend - tstart can leave one uncovered, and the kernel is not fed malformed segments here."""
import numpy as np
import pytest

from tests import phase_cases as C
from tests import util

pytestmark = pytest.mark.gpu

FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum")
GOLDEN = util.load_json("phase_edges")
UNPHASED = 11                   # index of "Unphased" among the record statuses
UNIQUE = [c for c in C.CASES if not c.name.startswith("name_")]


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _configure(worker, p, phase=True):
    worker.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"],
                     p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"],
                     p["md_threshold"], p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"], phase)


def _same_records(got, want):
    assert len(got) == len(want)
    for name in FIELDS:
        assert np.array_equal(got[name], want[name]), name


def _golden_tuples(name):
    return [tuple([C.CONTIG] + r) for r in GOLDEN["cases"][name]["records"]]


def _nonzero(d):
    return {k: int(v) for k, v in d.items() if v}


_ORACLE = {}


def _oracle(case):
    """(records, log, ccs table, ref table, normcounts log) of the oracle, computed once per case."""
    if case.name not in _ORACLE:
        from oracle import oracle as O
        p = C.params_of(case)
        recs, log = O.call(case.batch, case.chunks, p, p["germline_snv_prior"], None, None, case.phase_sets)
        ccs, rf, nlog = O.normcounts(case.batch, case.chunks, p, case.refseq, p["germline_snv_prior"],
                                     alt_order=GOLDEN["cases"][case.name]["alt_order"], phase=case.phase_sets)
        _ORACLE[case.name] = (recs, log, ccs, rf, nlog)
    return _ORACLE[case.name]


def _call(worker, case, batch=None):
    _configure(worker, C.params_of(case))
    return worker.call_contig(case.batch if batch is None else batch, case.chunks, None, None, case.phase_sets)


def _norm(worker, case):
    from himut_amd import normcounts
    _configure(worker, C.params_of(case))
    return normcounts.norm_contig(worker, case.batch, case.chunks, case.refseq.encode("ascii"),
                                  alt_order=GOLDEN["cases"][case.name]["alt_order"], phase_sets=case.phase_sets)


def _check_call(case, recs, log):
    from himut_amd import caller
    orecs, olog = _oracle(case)[:2]
    assert log == olog
    _same_records(recs, orecs)
    tuples = caller.records_to_tuples(C.CONTIG, recs)
    assert log == GOLDEN["cases"][case.name]["log"]
    assert tuples == _golden_tuples(case.name)
    return tuples


def _check_norm(case, ccs, rf, log):
    _, _, o_ccs, o_ref, o_log = _oracle(case)
    g = GOLDEN["cases"][case.name]
    assert log == o_log and log == g["norm_log"]
    assert ccs == o_ccs and rf == o_ref
    assert _nonzero(ccs) == g["ccs_tri2count"] and _nonzero(rf) == g["ref_tri2count"]


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_call_phase_case(worker, case):
    recs, log = _call(worker, case)
    tuples = _check_call(case, recs, log)
    case.expect(tuples, log)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_normcounts_phase_case(worker, case):
    _check_norm(case, *_norm(worker, case))


@pytest.mark.parametrize("case", UNIQUE, ids=lambda c: c.name)
def test_vote_by_name_equals_vote_by_row(worker, case):
    """Two reads more that share a name, outside every chunk: unique_qnames is off and every candidate of the case is
    voted on by name, with the same result."""
    from oracle import oracle as O
    b = C.with_shared_pair(case)
    assert len(set(b.qid.tolist())) == b.n - 1
    recs, log = _call(worker, case)
    nrecs, nlog = _call(worker, case, b)
    _same_records(nrecs, recs)
    assert nlog[1:] == log[1:]
    p = C.params_of(case)
    assert nlog[0] == O.call(b, case.chunks, p, p["germline_snv_prior"], None, None, case.phase_sets)[1][0]


def test_one_context_through_all_cases(worker):
    """All cases through one context, in order and in reverse, call and normcounts in turn, then one run without
    phasing: every result is what the case gives alone, so nothing of the haplotypes or the pair offsets of the
    previous phase sets is left behind."""
    from oracle import oracle as O
    assert len(C.CASES) % 2 == 0            # the way back gives every case the run it did not get on the way out
    for k, case in enumerate(list(C.CASES) + list(reversed(C.CASES))):
        if k & 1:
            _check_norm(case, *_norm(worker, case))
        else:
            _check_call(case, *_call(worker, case))
    case = next(c for c in C.CASES if c.name == "chunks_ten_sets")
    p = C.params_of(case)
    orecs, olog = O.call(case.batch, case.chunks, p, p["germline_snv_prior"], None, None, None)
    _configure(worker, p, False)
    recs, log = worker.call_contig(case.batch, case.chunks)
    assert log == olog
    _same_records(recs, orecs)
    assert len(recs) and not (recs["status"] == UNPHASED).any() and (recs["phase_set"] < 0).all()
