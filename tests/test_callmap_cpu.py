"""The plain model of the callable run (tests/callmap_model.py) pinned to the reference: folded the way the reference folds
its verdicts, the model's map must give the recorded outputs of the reference's worker (tests/golden/norm_*.json)
exactly.  Then the run builder on maps made by hand, the writer's merge, and the command line.  Last, the model's own
genotype at fp64 rounding boundaries: the piles of tests/gt_piles.py (tests/golden/gt_edges.json and leaf_gtlib.json)
give the state the fixture implies at every column, and the perturbed sums of gt_piles.genotype would not.  CPU only;
tests/test_gpu_gt_edges.py runs the same piles through k_callmap_sweep."""
import collections
import functools

import numpy as np
import pytest

from tests import callable_model as CM
from tests import callmap_cases as C
from tests import callmap_model as M
from tests import gt_piles as G
from tests import util
from tests.test_gt_edges_cpu import ORDER
from tests.test_oracle_golden import NORM_CASES, load_norm_case

ALL_STATES = {0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13}


def golden_variants():
    """(case, index of the variant or None) for every NORM_CASES entry and every ``variants`` entry of norm_order."""
    out = [(case, None) for case in NORM_CASES]
    n = len(util.load_json("norm_order")["variants"])
    return out + [("norm_order", k) for k in range(n)]


_RESULTS = {}


def golden_result(case, variant):
    """The model's result for a golden case, computed once and left unchanged."""
    key = (case, variant)
    if key not in _RESULTS:
        batch, exp, p, refseq, pon, com = load_norm_case(case)
        v = exp if variant is None else exp["variants"][variant]
        res = M.run(batch, refseq, util.chunks_of(exp), p, pon, com, v["alt_order"], exp["non_human_sample"],
                    util.phase_of(exp))
        _RESULTS[key] = (res, v, refseq)
    return _RESULTS[key]


@pytest.mark.parametrize("case,variant", golden_variants())
def test_model_folds_to_the_reference(case, variant):
    """Per-state sums of bases = log; count and bases of the CALLABLE positions binned by get_tri_context =
    ref_tri2count and ccs_tri2count."""
    res, v, refseq = golden_result(case, variant)
    rows, ref_tri, ccs_tri = M.fold(res, refseq)
    assert res.log == v["log"]
    assert rows[1:] == v["log"][1:]
    assert {k: c for k, c in ref_tri.items() if c} == {k: int(c) for k, c in v["ref_tri2count"].items() if c}
    assert {k: c for k, c in ccs_tri.items() if c} == {k: int(c) for k, c in v["ccs_tri2count"].items() if c}
    assert int(res.bases[res.state <= M.NO_BASE].sum()) == 0
    assert 6 not in set(np.unique(res.state).tolist())


def test_every_state_is_reached():
    """The golden cases reach every state but HETALT (4); tests/callmap_cases.hetalt_scene adds a pile with two alternative
    alleles and none of the reference's, and the genotype there is checked against the oracle's leaf (gtlib.get_germ_gt
    as the leaf_gtlib fixture pins it)."""
    from oracle import oracle as O
    seen = set()
    for case, variant in golden_variants():
        seen |= set(np.unique(golden_result(case, variant)[0].state).tolist())
    assert seen == ALL_STATES - {M.HETALT}
    sc = C.hetalt_scene()
    res = M.run(sc.batch, sc.ref, sc.chunks, sc.params)
    s0 = sc.chunks[0][0]
    assert int(res.state[sc.notes["hetalt"] - s0]) == M.HETALT
    assert int(res.state[sc.notes["homalt"] - s0]) == M.HOMALT and int(res.state[sc.notes["het"] - s0]) == M.HET
    pos = sc.notes["hetalt"]
    alleles = ["ATGC".index(C.other(sc.ref[pos], 1 + (k % 2))) for k in range(12)]
    _gt, _gq, state, _pl = O.germ_gt(sc.ref[pos], alleles, [40] * 12, sc.params["germline_snv_prior"])
    assert state == "hetalt"
    assert seen | set(np.unique(res.state).tolist()) == ALL_STATES


@pytest.mark.parametrize("case", ["norm_basic", "norm_nsub", "norm_insins", "norm_softmask"])
def test_counted_mask_is_callable_models_rule(case):
    """counted_mask (numpy) against callable_model.counted (dictionaries and bisect), read by read."""
    batch, _exp, p, _refseq, _pon, _com = load_norm_case(case)
    for i in range(0, batch.n, max(1, batch.n // 25)):
        want = CM.read_counted(batch, i, p)
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        got = M.counted_mask(ts, te, int(batch.qstart[i]), int(batch.qlen[i]), batch.query_qualities(i), batch.cs_tag(i), p)
        assert sorted(want) == (np.flatnonzero(got) + ts).tolist(), i


def test_counted_mask_on_the_hand_built_reads():
    from tests import callable_cases as K
    for name in ("word_edges", "read_start", "read_end", "counts", "indel_geometry", "nsub", "trim"):
        case = K.build(name)
        batch = K.batch_of(case)
        for overrides in case.params[:3]:
            p = K.params_of(overrides)
            for i in range(batch.n):
                ts, te = int(batch.tstart[i]), int(batch.tend[i])
                got = M.counted_mask(ts, te, int(batch.qstart[i]), int(batch.qlen[i]), batch.query_qualities(i),
                                     batch.cs_tag(i), p)
                assert sorted(CM.read_counted(batch, i, p)) == (np.flatnonzero(got) + ts).tolist(), (name, i)


# ---------------------------------------------------------------------------------------------- the run builder
def _runs(chunks, state, bases):
    r = M.runs_of(chunks, np.array(state, np.uint8), np.array(bases, np.uint16))
    return [tuple(int(x) for x in row) for row in r.tolist()]


def test_runs_chunk_of_length_one():
    assert _runs([(7, 8)], [13], [5]) == [(0, 7, 8, 13, 5)]


def test_runs_abutting_chunks_with_equal_state_at_the_seam():
    chunks = [(10, 13), (13, 15)]
    runs = M.runs_of(chunks, np.array([1, 13, 13, 13, 13], np.uint8), np.array([0, 2, 3, 4, 5], np.uint16))
    assert [tuple(int(x) for x in r) for r in runs.tolist()] == [(0, 10, 11, 1, 0), (0, 11, 13, 13, 5), (1, 13, 15, 13, 9)]
    assert M.merged_lines(runs) == [(10, 11, 1, 0), (11, 15, 13, 14)]          # the device: two runs; the writer: one line


def test_runs_gap_between_chunks():
    chunks = [(10, 12), (20, 22)]
    runs = M.runs_of(chunks, np.array([13, 13, 13, 13], np.uint8), np.array([1, 1, 1, 1], np.uint16))
    assert [tuple(int(x) for x in r) for r in runs.tolist()] == [(0, 10, 12, 13, 2), (1, 20, 22, 13, 2)]
    assert M.merged_lines(runs) == [(10, 12, 13, 2), (20, 22, 13, 2)]


def test_runs_alternating_states_at_every_position():
    n = 5000
    state = [13 if k % 2 == 0 else 1 for k in range(n)]
    bases = [3 if k % 2 == 0 else 0 for k in range(n)]
    runs = _runs([(100, 100 + n)], state, bases)
    assert len(runs) == n
    assert runs[0] == (0, 100, 101, 13, 3) and runs[-1] == (0, 100 + n - 1, 100 + n, 1, 0)
    assert all(r[2] - r[1] == 1 for r in runs)


def test_runs_one_state_throughout():
    n = 70_000
    assert _runs([(0, n)], [13] * n, [65535] * n) == [(0, 0, n, 13, 65535 * n)]        # (more than 2^32: an int64 sum)


def test_runs_overlapping_chunks_are_written_as_they_come():
    chunks = [(10, 14), (12, 16)]
    runs = M.runs_of(chunks, np.array([13] * 8, np.uint8), np.array([1] * 8, np.uint16))
    assert M.merged_lines(runs) == [(10, 14, 13, 4), (12, 16, 13, 4)]


def test_boundary_scene_is_what_its_notes_say():
    """The hand-built scene of the GPU tests puts the state changes where it claims to."""
    from himut_amd import _ffi
    tile, block = _ffi.CALLMAP_TILE, _ffi.CALLMAP_BLOCK
    sc = C.boundary_scene(tile, block)
    res = M.run(sc.batch, sc.ref, sc.chunks, sc.params)

    def entry(chunk, pos):
        return int(res.mapoff[chunk]) + pos - sc.chunks[chunk][0]
    c, a, _b = sc.notes["tile_edge"]
    assert sc.chunks[c][0] % tile != 0 and (sc.chunks[c][1] - sc.chunks[c][0]) % tile != 0
    assert (a + 1 - sc.chunks[c][0]) % tile == 0 and res.state[entry(c, a)] != res.state[entry(c, a + 1)]
    c, a, _b = sc.notes["block_edge"]
    assert entry(c, a + 1) % block == 0 and res.state[entry(c, a)] != res.state[entry(c, a + 1)]
    c, a, b = sc.notes["long_run"]
    long_run = [r for r in res.runs if r["chunk"] == c and r["start"] == a and r["end"] == b]
    assert len(long_run) == 1 and long_run[0]["bases"] == 4 * (b - a) and entry(c, b) // block - entry(c, a) // block >= 3
    c, a, b = sc.notes["alternating"]
    st = res.state[entry(c, a):entry(c, b)]
    assert np.all(st[1:] != st[:-1]) and (entry(c, a) + block - 1) // block * block + block <= entry(c, b)
    c, a, b = sc.notes["no_base"]
    assert any(r["state"] == M.NO_BASE and r["end"] - r["start"] >= 100_000 for r in res.runs)
    assert np.all(res.state[entry(c, a):entry(c, b)] == M.NO_BASE)
    c, a, b = sc.notes["deep"]
    assert int(res.bases[entry(c, a)]) > 48 and {M.HET, M.HETALT, M.HOMALT, M.INDEL} <= set(res.state[entry(c, a):entry(c, b)].tolist())
    c, a, b = sc.notes["non_acgt"]
    assert res.state[entry(c, a)] == M.NON_ACGT and res.state[entry(c, b - 1)] == M.NON_ACGT
    seam = [r for r in res.runs if r["chunk"] in (2, 3, 4)]
    assert len(seam) == 3 and len(M.merged_lines(np.array(seam))) == 1
    assert min(e - s for s, e in sc.chunks) == 1 and any(e - s < tile for s, e in sc.chunks)


# ---------------------------------------------------------------------------------------------- the command line
def test_callable_takes_the_normcounts_flags():
    from himut_amd.parse_args import build_parser
    parser = build_parser("t")
    sub = parser._subparsers._group_actions[0].choices
    norm = {a.dest: a for a in sub["normcounts"]._actions}
    call = {a.dest: a for a in sub["callable"]._actions}
    assert set(norm) <= set(call) and set(call) - set(norm) == {"callable_only", "summary"}
    for dest, a in norm.items():
        b = call[dest]
        assert (a.option_strings, a.type, a.default, a.nargs, a.const) == (b.option_strings, b.type, b.default, b.nargs, b.const), dest
        assert a.required == b.required or dest == "sbs"
    assert norm["sbs"].required and not call["sbs"].required
    o = parser.parse_args(["callable", "-i", "in.bam", "--ref", "ref.fa", "-o", "callable.bed"])
    assert o.sub == "callable" and o.sbs is None and o.callable_only is False and o.summary is None
    o = parser.parse_args(["callable", "-i", "in.bam", "--ref", "ref.fa", "--sbs", "calls.vcf", "-o", "c.bed", "--phase",
                           "--phased_vcf", "p.vcf", "--min_bq", "50", "--callable_only", "--summary", "s.tsv"])
    assert (o.sbs, o.phase, o.min_bq, o.callable_only, o.summary) == ("calls.vcf", True, 50, True, "s.tsv")


# ---------------------------------------------------------------------------------------------- fp64 rounding boundaries
EDGE_KINDS = ("gq_int", "cap99", "germ_gq_int", "assoc", "order", "qual", "state")
EDGE_MODES = ("norm", "twin", "wide")           # the column alone; twice in one tile; in the middle of the wide chunk
LEAF_PRIOR, LEAF_K = 1 / (10 ** 3), 20
# the boundary vectors whose norm.log row moves under at least one of gt_piles.PERTURBATIONS, by kind (assoc: both
# outcomes are HET)
CALLABLE_FLIPS = {"gq_int": 33, "state": 24, "order": 12, "cap99": 9, "germ_gq_int": 8, "qual": 5}


@functools.lru_cache(maxsize=None)
def edge_vectors():
    """The boundary vectors, each with an id for the assertions' messages."""
    return [dict(v, id="gt_edges[{}] {} depth {}".format(i, v["kind"], len(v["alleles"])))
            for i, v in enumerate(util.load_json("gt_edges")["vectors"])]


@functools.lru_cache(maxsize=None)
def leaf_vectors():
    return [dict(v, id="leaf_gtlib[{}] depth {}".format(i, len(v["alleles"])))
            for i, v in enumerate(G.leaf_vectors(util.load_json("leaf_gtlib")["vectors"], LEAF_PRIOR, LEAF_K))]


def edges_of(kind):
    return [i for i, v in enumerate(edge_vectors()) if v["kind"] == kind]


def _pile(vs, mode, orders=G.ORDERS):
    P = G.build(vs, orders=orders, twin=mode == "twin")
    return P, (P.call_chunks if mode == "wide" else P.norm_chunks)


@functools.lru_cache(maxsize=None)
def edge_model(i, mode):
    """(vectors, pile, chunks, parameters, the model's result) of boundary vector i in its own pile at its own prior
    with min_gq = k; computed once and left unchanged."""
    v = edge_vectors()[i]
    P, chunks = _pile([v], mode, [G.ORDERS[i % 3]])
    p = G.params(v["k"], v["prior"], len(v["alleles"]))
    return [v], P, chunks, p, M.run(P.batch, P.refseq, chunks, p, alt_order=ORDER)


@functools.lru_cache(maxsize=None)
def leaf_model(mode):
    """The same of the 400 leaf vectors in one pile."""
    vs = leaf_vectors()
    P, chunks = _pile(vs, mode)
    p = G.params(LEAF_K, LEAF_PRIOR, max(len(v["alleles"]) for v in vs))
    return vs, P, chunks, p, M.run(P.batch, P.refseq, chunks, p, alt_order=ORDER)


def check_columns(res, vs, P, chunks, p, mode):
    """A map (the model's or the device's) against the fixture: every vector's column has the state of its norm.log
    row and the column's depth as bases.  Over the columns' own chunks nothing else is covered: NO_BASE, no bases."""
    mine = np.zeros(res.state.shape[0], bool)
    for j, (v, cols) in enumerate(zip(vs, P.cols)):
        row = G.norm_row(v, p["min_gq"], ORDER, p["min_ref_count"], p["min_alt_count"])
        for c in cols:
            assert chunks[j][0] <= c < chunks[j][1]
            e = int(res.mapoff[j]) + c - chunks[j][0]
            got = (int(res.state[e]), int(res.bases[e]))
            assert got == (row, len(v["alleles"])), "{} ({}, position {}): (state, bases) {} for {}".format(
                v["id"], mode, c, got, (row, len(v["alleles"])))
            mine[e] = True
    if mode != "wide":
        assert np.all(res.state[~mine] == M.NO_BASE) and not res.bases[~mine].any(), mode


@pytest.mark.parametrize("mode", EDGE_MODES)
@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_gt_edges_columns(kind, mode):
    """Each boundary vector in its own pile: the model's state and bases at the column are the fixture's."""
    idx = edges_of(kind)
    assert idx
    for i in idx:
        vs, P, chunks, p, res = edge_model(i, mode)
        check_columns(res, vs, P, chunks, p, mode)
        if mode == "norm":
            want = G.norm_log(vs, p["min_gq"], ORDER, p["min_ref_count"], p["min_alt_count"])
            assert res.log == want and M.fold(res, P.refseq)[0][1:] == want[1:], vs[0]["id"]


@pytest.mark.parametrize("mode", EDGE_MODES)
def test_leaf_vectors_columns(mode):
    """leaf_gtlib's 400 columns in one pile at prior 1e-3, min_gq 20."""
    vs, P, chunks, p, res = leaf_model(mode)
    assert len(vs) == 400
    check_columns(res, vs, P, chunks, p, mode)
    if mode != "wide":
        want = G.norm_log(vs, LEAF_K, ORDER, p["min_ref_count"], p["min_alt_count"], copies=2 if mode == "twin" else 1)
        assert res.log == want and M.fold(res, P.refseq)[0][1:] == want[1:]


def test_gt_tables_are_gtlibs():
    """The model's own tables and log priors equal gtlib.build_tables bit for bit at qualities 1 to 255 (quality 0 is
    log10(0) in the reference and an error in every run)."""
    from himut_amd.gtlib import build_tables
    T = M.gt_tables()
    priors = sorted({1 / (10 ** 3), 1 / (10 ** 4), 1 / (10 ** 2)} | {v["prior"] for v in edge_vectors()})
    assert len(priors) > 3
    for prior in priors:
        hom, het, err, logp = build_tables(prior)
        for k, lut in enumerate((hom, het, err)):
            want = np.asarray(lut, np.float64)
            assert want.shape[0] >= 256 and T[k, 1:256].tobytes() == want[1:256].tobytes(), (prior, k)
        assert np.array(M.gt_priors(prior), np.float64).tobytes() == np.asarray(logp, np.float64)[:4].tobytes(), prior


def perturbed(v, how):
    """The vector with the outcome a kernel would give that sums as gt_piles.genotype(..., how) does."""
    g = G.genotype(v["ref"], v["alleles"], v["bqs"], v["prior"], how)
    return dict(v, gt=g["gt"], gq=g["gq"], state=g["state"], germ_gq=g["germ_gq"])


def test_perturbed_sums_move_the_callable_row():
    """The GPU test bites: a kernel that sums in reverse, in partial sums, with the prior first or in another base order
    puts 91 of the 193 columns in another row of norm.log, some of each kind that crosses a GQ boundary or a state."""
    moved = collections.Counter()
    for v in edge_vectors():
        row = G.norm_row(v, v["k"], ORDER, 3, 1)
        if any(G.norm_row(perturbed(v, how), v["k"], ORDER, 3, 1) != row for how in G.PERTURBATIONS):
            moved[v["kind"]] += 1
    assert dict(moved) == CALLABLE_FLIPS and sum(moved.values()) == 91
    for kind in ("gq_int", "cap99", "state", "qual"):
        assert moved[kind] > 0


def test_swapped_neighbours_move_the_callable_row():
    """A column walk that takes each pair of rows in the opposite order (the rows of k_callmap_sweep's loop come two at
    a time) sums every base's reads in another order: whichever way the pairs fall on the column's reads, at least 20
    columns land in another row."""
    for first in (0, 1):
        moved = 0
        for v in edge_vectors():
            order = list(range(len(v["alleles"])))
            for k in range(first, len(order) - 1, 2):
                order[k], order[k + 1] = order[k + 1], order[k]
            g = G.genotype(v["ref"], [v["alleles"][k] for k in order], [v["bqs"][k] for k in order], v["prior"])
            w = dict(v, gt=g["gt"], gq=g["gq"], state=g["state"], germ_gq=g["germ_gq"])
            moved += G.norm_row(w, v["k"], ORDER, 3, 1) != G.norm_row(v, v["k"], ORDER, 3, 1)
        print("pairs from read", first, ":", moved, "rows moved")
        assert moved >= 20, (first, moved)
