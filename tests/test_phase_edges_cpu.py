"""The hand-built phased cases of tests/phase_cases.py on the CPU: the oracle's `call --phase` and `normcounts --phase`
against what the reference gave for each (tests/golden/phase_edges.json), and each case's own statement against the
reference's output, so that a case that does not reach its edge fails here.  Bit-exact; CPU only."""
import pytest

from oracle import oracle as O
from tests import phase_cases as C
from tests import util

GOLDEN = util.load_json("phase_edges")


def golden_tuples(name):
    return [tuple([C.CONTIG] + r) for r in GOLDEN["cases"][name]["records"]]


def nonzero(d):
    return {k: int(v) for k, v in d.items() if v}


def test_every_case_has_a_golden():
    assert GOLDEN["order"] == [c.name for c in C.CASES]
    assert set(GOLDEN["cases"]) == set(GOLDEN["order"]) and len(GOLDEN["order"]) == len(C.CASES)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_oracle_call_matches_reference(case):
    p = C.params_of(case)
    g = GOLDEN["cases"][case.name]
    recs, log = O.call(case.batch, case.chunks, p, p["germline_snv_prior"], None, None, case.phase_sets)
    assert log == g["log"]
    assert O.records_to_tuples(C.CONTIG, recs) == golden_tuples(case.name)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_oracle_normcounts_matches_reference(case):
    p = C.params_of(case)
    g = GOLDEN["cases"][case.name]
    ccs, rf, log = O.normcounts(case.batch, case.chunks, p, case.refseq, p["germline_snv_prior"], alt_order=g["alt_order"],
                                phase=case.phase_sets)
    assert log == g["norm_log"]
    assert nonzero(ccs) == g["ccs_tri2count"] and nonzero(rf) == g["ref_tri2count"]


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_case_reaches_its_edge_in_the_reference(case):
    g = GOLDEN["cases"][case.name]
    case.expect(golden_tuples(case.name), g["log"])


def test_vote_cases_decide_between_pass_and_unphased():
    """Every vote case has one record at its candidate that the vote decided, and each of the two vote implementations
    (by column row where the names are unique, by name where they are not) meets both outcomes."""
    for group, unique in ((C.VOTE_BY_ROW, True), (C.VOTE_BY_NAME, False)):
        seen = set()
        assert group
        for c in group:
            names = [c.batch.query_name(i) for i in range(c.batch.n)]
            assert (len(set(names)) == len(names)) == unique, c.name
            at = C.at(golden_tuples(c.name), c.tpos)
            assert len(at) == 1 and at[0][4] in ("PASS", "Unphased"), (c.name, at)
            seen.add(at[0][4])
        assert seen == {"PASS", "Unphased"}


def test_shared_pair_leaves_the_reads_alone():
    """The pair of reads the GPU tests add to make the names non-unique lies outside every chunk and every read."""
    for c in C.CASES[::17]:
        b = C.with_shared_pair(c)
        assert b.n == c.batch.n + 2
        names = [b.query_name(i) for i in range(b.n)]
        assert names.count("pair") == 2 and [n for n in names if n != "pair"] == [c.batch.query_name(i) for i in range(c.batch.n)]
        assert all(e <= C.FREE[0] or s >= C.FREE[1] for s, e in c.chunks)
        p = C.params_of(c)
        recs, log = O.call(b, c.chunks, p, p["germline_snv_prior"], None, None, c.phase_sets)
        assert log == GOLDEN["cases"][c.name]["log"]
        assert O.records_to_tuples(C.CONTIG, recs) == golden_tuples(c.name)
