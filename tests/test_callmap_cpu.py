"""The plain model of the callable run (tests/callmap_model.py) pinned to the reference: folded the way the reference folds
its verdicts, the model's map must give the recorded outputs of the reference's worker (tests/golden/norm_*.json)
exactly.  Then the run builder on maps made by hand, the writer's merge, and the command line.  CPU only."""
import numpy as np
import pytest

from tests import callable_model as CM
from tests import callmap_cases as C
from tests import callmap_model as M
from tests import util
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
