"""Genotype calls and GQ cut-offs at fp64 rounding boundaries (tests/golden/gt_edges.json, made by
tests/golden/make_golden.py from the reference's gtlib): the CPU oracle against the reference's outputs bit for bit,
the fixture's own guarantee that every vector discriminates, and the piles of tests/gt_piles.py through the oracle's
call run and normcounts.  CPU only; tests/test_gpu_gt_edges.py runs the same piles through the kernels."""
import collections
import os

import pytest

from oracle import oracle as O
from tests import gt_piles as G
from tests import util

NEED = {"gq_int": 60, "cap99": 10, "germ_gq_int": 20, "assoc": 30, "order": 10, "qual": 20, "state": 20}
ORDER = {"A": ["T", "G", "C"], "T": ["C", "A", "G"], "G": ["A", "C", "T"], "C": ["G", "T", "A"]}


@pytest.fixture(scope="module")
def edges():
    return util.load_json("gt_edges")["vectors"]


def _idx(v):
    return [O.BASE2IDX[a] for a in v["alleles"]]


def test_fixture_shape(edges):
    """The kinds, depths and references the fixture promises, under its size limit."""
    assert os.path.getsize(os.path.join(util.GOLDEN, "gt_edges.json")) < 150 * 1024
    kinds = collections.Counter(v["kind"] for v in edges)
    for kind, n in NEED.items():
        assert kinds[kind] >= n, kind
    depths = {len(v["alleles"]) for v in edges}
    for d in (2, 3, 4, 5, 8, 12, 20, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000):
        assert d in depths, d
    assert all(1e-4 <= v["prior"] <= 1e-2 for v in edges)
    assert {v["ref"] for v in edges if v["kind"] == "assoc"} == set("ATGC")
    # assoc: exact bit ties (the lower index wins) and pairs apart by a few ulps (the last bit wins)
    ties = [v for v in edges if v["kind"] == "assoc" and sorted(v["pls"])[0] == sorted(v["pls"])[1]]
    assert 0 < len(ties) < kinds["assoc"]
    cap = [v["gq"] for v in edges if v["kind"] == "cap99"]
    assert 98 in cap and 99 in cap
    # pure-reference columns (the normcounts fast path) and columns with other alleles
    pure = [v for v in edges if v["kind"] == "gq_int" and set(v["alleles"]) == {v["ref"]}]
    assert 0 < len(pure) < kinds["gq_int"]
    assert any(min(v["bqs"]) <= 3 for v in edges if v["kind"] == "qual")
    assert any(min(v["bqs"]) >= 163 for v in edges if v["kind"] == "qual")     # hom terms of exactly 0.0
    assert any(94 <= min(v["bqs"]) < 163 for v in edges if v["kind"] == "qual")
    # state: the genotype's state changes at the crossing, and adding the prior first moves it
    st = [v for v in edges if v["kind"] == "state"]
    assert {v["state"] for v in st} > {"homref"} and all("prior_first" in G.flips(v) for v in st)
    # order: pairs of one quality multiset in two fetch orders with different outcomes
    by = collections.defaultdict(list)
    for v in edges:
        if v["kind"] == "order":
            by[v["pair"]].append(v)
    assert len(by) >= 5
    for a, b in by.values():
        assert sorted(zip(a["alleles"], a["bqs"])) == sorted(zip(b["alleles"], b["bqs"])) and a["prior"] == b["prior"]
        assert a["alleles"] != b["alleles"] or a["bqs"] != b["bqs"]
        assert (a["gt"], a["gq"], a["state"]) != (b["gt"], b["gq"], b["state"])


def test_oracle_germ_gt_gt_edges(edges):
    """orc_germ_gt: the ten PLs bit for bit, gt, gq and state, at each vector's own prior."""
    for v in edges:
        gt, gq, state, pls = O.germ_gt(v["ref"], _idx(v), v["bqs"], v["prior"])
        assert pls == v["pls"], v
        assert (gt, gq, state) == (v["gt"], v["gq"], v["state"]), v


def test_oracle_germ_gq_gt_edges(edges):
    """orc_germ_gq: get_germ_gq with each single-base alt left out (the normcounts form)."""
    for v in edges:
        for alt, want in v["germ_gq"].items():
            assert O.germ_gq(v["ref"], _idx(v), v["bqs"], alt, v["prior"])[0] == want, (v, alt)


def test_oracle_germ_gq_leaf_vectors():
    """The alt-omitted form on the 400 leaf_gtlib columns: with no base left out it is the plain gq."""
    for v in util.load_json("leaf_gtlib")["vectors"]:
        m = G.genotype(v["ref"], v["alleles"], v["bqs"], 1 / (10 ** 3))
        assert m["pls"] == v["pls"]
        for alt, want in m["germ_gq"].items():
            assert O.germ_gq(v["ref"], _idx(v), v["bqs"], alt)[0] == want


def test_every_vector_discriminates(edges):
    """The restatement in reference order equals the fixture; summing in reverse, with math.fsum, with the prior first
    or in another base order changes each vector's outcome (gt, state, gq, gq >= k or an alt-omitted quality)."""
    for v in edges:
        g = G.genotype(v["ref"], v["alleles"], v["bqs"], v["prior"])
        assert (g["pls"], g["gt"], g["gq"], g["state"], g["germ_gq"]) == \
            (v["pls"], v["gt"], v["gq"], v["state"], v["germ_gq"]), v
        assert G.flips(v), v
    # the crossings: second - best within a few ulps of the pair's integer k
    for v in edges:
        if v["kind"] in ("gq_int", "cap99", "qual"):
            g = G.genotype(v["ref"], v["alleles"], v["bqs"], v["prior"])
            assert abs(g["gqf"] - v["k"]) <= 16 * max(abs(x) for x in v["pls"]) * 2.0 ** -52, v


def _oracle_norm(P, p, prior):
    return O.normcounts(P.batch, P.norm_chunks, p, P.refseq, prior, alt_order=ORDER)


@pytest.mark.parametrize("twin", [False, True])
def test_piles_leaf_vectors_oracle(twin):
    """The 400 leaf_gtlib columns as one pile: the oracle's normcounts log is the one the fixture implies, and every
    column with a candidate has its records with the fixture's gq, genotype and state."""
    vs = G.leaf_vectors(util.load_json("leaf_gtlib")["vectors"])
    P = G.build(vs, twin=twin)
    p = G.params(20, 1 / (10 ** 3), max(len(v["alleles"]) for v in vs))
    _, _, log = _oracle_norm(P, p, p["germline_snv_prior"])
    assert log == G.norm_log(vs, 20, ORDER, p["min_ref_count"], p["min_alt_count"], copies=2 if twin else 1)
    if not twin:
        recs, _ = O.call(P.batch, P.call_chunks, p, p["germline_snv_prior"])
        check_records(vs, P, recs, 20)


def check_records(vs, P, recs, min_gq):
    """Records at each vector's column: one per candidate the germline rule keeps, with the vector's gq, gt and state
    (LowGQ exactly when a hom-ref column's gq is below min_gq)."""
    at = collections.defaultdict(list)
    for r in recs:
        at[int(r["tpos"])].append(r)
    states = ["homref", "het", "hetalt", "homalt"]
    for v, cols in zip(vs, P.cols):
        rs = at.pop(cols[0] + 1, [])
        kept = sum(G.candidates(v).values())
        # (a hetalt column's records all read (ref, "a1,a2"): the same record, written once)
        assert len(rs) == (min(kept, 1) if v["state"] == "hetalt" else kept), v
        for r in rs:
            assert int(r["gq"]) == v["gq"], v
            assert chr(r["gt0"]) + chr(r["gt1"]) == v["gt"] and states[int(r["gt_state"])] == v["state"], v
            if v["state"] == "homref":
                assert (O.STATUS[int(r["status"])] == "LowGQ") == (v["gq"] < min_gq), v
    assert not at


def test_piles_gt_edges_oracle(edges):
    """Each boundary vector in its own pile at its own prior with min_gq = k: the oracle's call records and
    normcounts log are the ones the fixture implies."""
    for i, v in enumerate(edges):
        P = G.build([v], orders=[G.ORDERS[i % 3]])
        p = G.params(v["k"], v["prior"], len(v["alleles"]))
        _, _, log = _oracle_norm(P, p, v["prior"])
        assert log == G.norm_log([v], v["k"], ORDER, p["min_ref_count"], p["min_alt_count"]), v
        recs, _ = O.call(P.batch, P.call_chunks, p, v["prior"])
        check_records([v], P, recs, v["k"])
