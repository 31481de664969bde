"""The hetSNP edge counts of `himut phase` without a GPU: the plain model (tests/edges_model.py) and the C oracle
(orc_edges) against what the reference's phaselib.get_edges gave for the captured contigs (edges_basic, edges_lowq) and
for the hand-built cases of tests/edges_cases.py (edges_blocks, edges_rules: tests/golden/make_golden.py), and proof
that those cases tell every rule from its wrong variant.  tests/test_gpu_edges.py holds k_edges to the same fixtures."""
import numpy as np
import pytest

from tests import edges_cases as C
from tests import edges_model as M
from tests import util

BATCH_ARRAYS = ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "qid", "qoff", "cs_off", "seq", "bq", "cs", "tp")


def unflat(flat):
    """(edge_lst, {(i, j): [4 counts]}) of a fixture run's flat list i, j, c0..c3."""
    rows = [flat[k:k + 6] for k in range(0, len(flat), 6)]
    return [(r[0], r[1]) for r in rows], {(r[0], r[1]): r[2:] for r in rows}


def ints(res):
    edge_lst, e2c = res
    return [tuple(e) for e in edge_lst], {tuple(k): [int(x) for x in v] for k, v in e2c.items()}


def model(batch, hets, min_bq, min_mapq, rules=()):
    """The model's result, or ("error", code) where it raises."""
    try:
        return ints(M.edges(batch, hets, min_bq, min_mapq, rules))
    except M.ModelError as e:
        return "error", e.code


def oracle(batch, hets, min_bq, min_mapq):
    from oracle import oracle as O
    return ints(O.edges(batch, hets, min_bq, min_mapq))


@pytest.fixture(scope="module")
def hand():
    """name -> (batch, hetSNPs) of the hand-built cases, built once."""
    cases = {"blocks": C.blocks(C.BLOCKS_FIXTURE_K), "blocks_large": C.blocks(C.BLOCKS_LARGE_K), "spans": C.spans(),
             "cs_geometry": C.cs_geometry(), "filters": C.filters(), "deep": C.deep(), "rules": C.rules()}
    return {k: (C.batch_of(c), c.hets) for k, c in cases.items()}


@pytest.mark.parametrize("case", ["edges_basic", "edges_lowq"])
def test_model_reproduces_captured_contigs(case):
    batch, exp = util.load_case(case)
    hets = [tuple(h) for h in exp["hetsnps"]]
    edge_lst, e2c = model(batch, hets, exp["min_bq"], exp["min_mapq"])
    assert [list(e) for e in edge_lst] == exp["edge_lst"]
    assert {"{},{}".format(*k): [float(x) for x in v] for k, v in e2c.items()} == exp["edge2counts"]


@pytest.mark.parametrize("case,built", [("edges_blocks", "blocks"), ("edges_rules", "rules")])
def test_model_and_oracle_reproduce_hand_built_fixtures(hand, case, built):
    batch, exp = util.load_case(case)
    hets = [tuple(h) for h in exp["hetsnps"]]
    # the fixture's input is what the builders give today
    mine, my_hets = hand[built]
    assert my_hets == hets
    for k in BATCH_ARRAYS:
        assert np.array_equal(getattr(mine, k), getattr(batch, k)), k
    want_params = [C.BLOCKS_PARAMS] if case == "edges_blocks" else [(q, m) for q in C.RULES_MIN_BQ for m in C.RULES_MIN_MAPQ]
    assert [(r["min_bq"], r["min_mapq"]) for r in exp["runs"]] == want_params
    for run in exp["runs"]:
        want = unflat(run["edges"])
        assert model(batch, hets, run["min_bq"], run["min_mapq"]) == want, (run["min_bq"], run["min_mapq"])
        assert oracle(batch, hets, run["min_bq"], run["min_mapq"]) == want, (run["min_bq"], run["min_mapq"])
    if case == "edges_rules":
        # deep: 300 in one column and 3 in another on each of the ten edges
        first = hets.index(hand["deep"][1][0])
        e2c = unflat(exp["runs"][C.RULES_MIN_MAPQ.index(20) + 4 * C.RULES_MIN_BQ.index(20)]["edges"])[1]
        assert [e2c[(first + a, first + b)] for a in range(5) for b in range(a + 1, 5)] == [[300, 3, 0, 0]] * 10


def test_model_and_oracle_agree_beyond_the_fixtures(hand):
    """Spans of 193 and 257 hetSNPs (pairs three and four blocks of 64 apart) and a synthetic contig with indels."""
    from himut_amd import synth
    batch, hets = hand["blocks_large"]
    got = model(batch, hets, *C.BLOCKS_PARAMS)
    assert got == oracle(batch, hets, *C.BLOCKS_PARAMS)
    assert max(j - i for i, j in got[0]) == 256
    s = synth.generate(synth.SynthConfig(seed=77, contig_len=20000, read_len_mean=2500, read_len_sd=500, read_len_min=800,
                                         read_len_max=5000, snp_rate=5e-3, ins_rate=2e-3, del_rate=2e-3, name="chrS"))
    hets = sorted(set((int(p) + 1, chr(r), chr(a)) for p, r, a, g in zip(s.snp_pos, s.snp_ref, s.snp_alt, s.snp_gt)
                      if g in (1, 2)))
    for min_bq in (0, 40):
        got = model(s.batch, hets, min_bq, 20)
        assert got == oracle(s.batch, hets, min_bq, 20)
        assert len(got[0]) > 500


# rule -> the case written for it, (min_bq, min_mapq)
SENSITIVITY = [("next_lane", "blocks", (20, 20)), ("left_start", "spans", (20, 20)), ("left_end", "spans", (20, 20)),
               ("no_clip", "spans", (20, 20)), ("del_ref", "cs_geometry", (0, 20)), ("bq_gt", "filters", (20, 20)),
               ("drop_supp", "filters", (20, 20)), ("trans_swap", "cs_geometry", (20, 20))]


@pytest.mark.parametrize("rule,case,params", SENSITIVITY)
def test_cases_tell_the_rule_from_its_wrong_variant(hand, rule, case, params):
    batch, hets = hand[case]
    right = model(batch, hets, *params)
    assert right[0] != "error" and right[0]
    assert model(batch, hets, *params, rules=(rule,)) != right
    # and so does the combined fixture input
    batch, hets = hand["blocks" if case == "blocks" else "rules"]
    assert model(batch, hets, *params, rules=(rule,)) != model(batch, hets, *params)


def test_every_switch_has_a_case():
    assert {r for r, _c, _p in SENSITIVITY} == set(M.RULES)


def test_clip_sensitivity_comes_from_the_clipped_reads(hand):
    """Only the four soft-clipped reads of spans can tell the query offset's rule: without them nothing changes."""
    c = C.spans()
    plain = C.Case(c.name, c.length, c.ref, [r for r in c.records if r["qstart"] == 0], c.hets)
    b = C.batch_of(plain)
    assert b.n == 8 and model(b, c.hets, 20, 20, rules=("no_clip",)) == model(b, c.hets, 20, 20)


def test_span_rule_on_the_twelve_reads():
    """x on tstart and on tend + 1 is out (the read adds its pair's edge alone), x on tstart + 1 and on tend is in."""
    c = C.spans()
    for rec in c.records:
        b = C.batch_of(C.Case(c.name, c.length, c.ref, [rec], c.hets))
        edge_lst, _ = model(b, c.hets, 20, 20)
        where = rec["qname"].rsplit("_", 1)[1]
        assert len(edge_lst) == (3 if where in ("tstart+1", "tend") else 1), rec["qname"]


def test_deleted_positions_count_only_at_min_bq_0(hand):
    """A deleted position has quality 0: usable (state "other") at min_bq 0, never above."""
    c = C.cs_geometry()
    g = {o: i for i, o in enumerate(sorted(C.GEOMETRY_SITES))}
    batch = C.batch_of(C.Case(c.name, c.length, c.ref, [r for r in c.records if r["qname"] == "g_indel"], c.hets))
    at0, at1 = model(batch, c.hets, 0, 0)[1], model(batch, c.hets, 1, 0)[1]
    inside = [g[10], g[11], g[12], g[45], g[46]]
    assert all(any(h in e for e in at0) for h in inside) and not any(h in e for e in at1 for h in inside)
    assert at0[(g[10], g[11])] == [0, 1, 0, 0] and at0[(g[5], g[10])] == [0, 0, 1, 0]


def test_no_edge_at_min_bq_94(hand):
    for name, (batch, hets) in hand.items():
        assert model(batch, hets, 94, 0) == ([], {}), name
        assert oracle(batch, hets, 94, 0) == ([], {}), name


def test_missing_position_is_a_cover_error():
    """A hetSNP inside the read's span that its cs text never reaches: KeyError in the reference."""
    from oracle import oracle as O
    c = C.filters()
    rec = dict(next(r for r in c.records if r["qname"] == "f_mapq60"))
    rec["tend"] += 40                                       # the text still ends where it did
    hets = c.hets + [(rec["tend"] - 1, "A", "C")]
    b = C.batch_of(C.Case(c.name, c.length, c.ref, [rec], hets))
    assert model(b, hets, 0, 0) == ("error", M.ERR_COVER)
    with pytest.raises(O.OracleError):
        O.edges(b, hets, 0, 0)
