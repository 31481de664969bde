"""The bqcal run (himut_run_bqcal / himut_get_bqcal) through the C ABI against the plain-Python model of its contract
(tests/bqcal_model.py): np.array_equal on match[256] and mismatch[256], equality of the twelve counters.  The goldens
(tests/golden/bqcal_*.json) pin the run to the reference's own worker; the genotype fixtures pin k_bqcal's fp64 sums and
the GQ boundary; hand-built alignments pin the rules of the contract one at a time; geometry and histogram cases pin
the paths of the kernel (tile borders, the segment-list fall-back, more rows than one LDS batch, more reads than one
window round, runs of equal and of changing qualities); sequences on one context pin the state the runs leave each other."""
import os
import random

import numpy as np
import pytest

from tests import bqcal_model as M
from tests import germline_model as GM
from tests import gt_piles as G
from tests import util
from tests.test_bqcal_cpu import GOLDENS, golden_model, load_golden
from tests.test_germline_cpu import _reversed

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CHUNK = 1, 6


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _load(c, batch, refseq, regions, prior=1 / (10 ** 3), push=True):
    from himut_amd import bamio, gtlib
    c.set_gt_lut(*gtlib.build_tables(prior))
    bamio.set_contig_reference(c, refseq)
    c.set_chunks(regions)
    if push:
        c.push_reads(batch)


def _bqcal(c, batch, refseq, regions, prior=1 / (10 ** 3), push=True, **kw):
    _load(c, batch, refseq, regions, prior, push)
    c.run_bqcal(**kw)
    return c.bqcal()


def _same(got, want):
    assert got[2] == [int(x) for x in want[2]], (got[2], want[2])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0][0] == 0 and got[1][0] == 0


def _both(c, batch, refseq, regions, prior=1 / (10 ** 3), want=None, **kw):
    """The run and the model on the same input: equal (an error of the model's is the run's error); returns what the
    run gave, or None behind an error."""
    from himut_amd._ffi import HimutError
    try:
        want = want or M.run(batch, refseq, regions, prior, **kw)
    except GM.ModelError as me:
        with pytest.raises(HimutError) as e:
            _bqcal(c, batch, refseq, regions, prior, **kw)
        assert e.value.code == me.code
        return None
    got = _bqcal(c, batch, refseq, regions, prior, **kw)
    _same(got, want)
    return got


def _bins(quals):
    return np.bincount(np.asarray(quals, np.int64), minlength=256).astype(np.int64)


# ---- 1. the reference's own numbers

@pytest.mark.parametrize("case", GOLDENS)
def test_goldens(ctx, case):
    g, b, seq = load_golden(case)
    match, mismatch, log = _both(ctx, b, seq, g["regions"], g["germline_snv_prior"], want=golden_model(case), min_gq=g["min_gq"],
                                 md_threshold=g["md_threshold"])
    assert [int(x) for x in match[1:94]] == g["match"] and [int(x) for x in mismatch[1:94]] == g["mismatch"]
    assert mismatch.sum() > 0
    if case == "bqcal_dense_md":
        assert log[2] > 0


# ---- 2. fp64 order and the GQ boundary

def _vector_counts(v, k):
    """What the fixture's genotype makes of the column of vector v at min_gq = k."""
    if v["gq"] < k:
        return _bins([]), _bins([])
    outside = [q for a, q in zip(v["alleles"], v["bqs"]) if a not in v["gt"]]
    return (_bins([]), _bins(outside)) if outside else (_bins(v["bqs"]), _bins([]))


def test_leaf_vectors(ctx):
    """leaf_gtlib's 400 columns in one pile, one region per column: every column that passes puts its bases where the
    fixture's genotype says."""
    vs = G.leaf_vectors(util.load_json("leaf_gtlib")["vectors"])
    P = G.build(vs)
    match, mismatch, log = _both(ctx, P.batch, P.refseq, P.norm_chunks, min_gq=20)
    want = [_vector_counts(v, 20) for v in vs]
    assert np.array_equal(match, sum(w[0] for w in want)) and np.array_equal(mismatch, sum(w[1] for w in want))
    assert log[0] == 400 and log[4] == sum(v["gq"] < 20 for v in vs) > 0
    assert log[5:9] == [sum(v["gq"] >= 20 and v["state"] == s for v in vs) for s in M.STATES] and min(log[5:9]) > 0


def test_gt_edges_vectors(ctx):
    """Each boundary vector in its own pile at its own prior with min_gq = k, and with its reads turned round where the
    fetch order decides: the bins are the ones the fixture's genotype (or the turned column's) gives."""
    edges = util.load_json("gt_edges")["vectors"]
    skipped = turned = 0
    for i, v in enumerate(edges):
        w = _reversed(v)
        for u in (v, w):
            if u is None:
                continue
            P = G.build([u], orders=[G.ORDERS[i % 3]])
            match, mismatch, log = _both(ctx, P.batch, P.refseq, P.norm_chunks, u["prior"], min_gq=u["k"])
            m, mm = _vector_counts(u, u["k"])
            assert np.array_equal(match, m) and np.array_equal(mismatch, mm), (i, u)
            assert log[0] == 1 and log[4] == (u["gq"] < u["k"])
            skipped += log[4]
        turned += w is not None
    assert skipped > 10 and turned > 50


# ---- 3. the rules, one at a time, on hand-built alignments

def _contig(n=4000, seed=3):
    rs = random.Random(seed)
    ref = "".join(rs.choice("ATGC") for _ in range(n))
    return ref, {p: "ATGC"[("ATGC".index(ref[p]) + 1) % 4] for p in range(n)}, {p: "ATGC"[("ATGC".index(ref[p]) + 2) % 4] for p in range(n)}


def _batch(ref, recs):
    from himut_amd.readbatch import batch_from_records
    return batch_from_records("chrH", len(ref), sorted(recs, key=lambda r: r["tstart"]))


def _column(ref, pos, cells, length=120, **kw):
    """Reads over pos in file order, one per cell (base, quality at pos[, extra record fields]); 93 elsewhere."""
    out = []
    for k, cell in enumerate(cells):
        base, q, extra = cell[0], cell[1], (cell[2] if len(cell) > 2 else {})
        out.append(GM.make_read(ref, pos - 60 + k % 50, length, {pos: base} if base != ref[pos] else {}, bq=93, bq_at={pos: q},
                                **dict(kw, **extra)))
    return out


def test_het_columns(ctx):
    """Every read carries an allele of the het genotype: all matches.  With a third allele the position adds only that
    allele's quality as a mismatch and the genotype's own cells add nothing.  A homref column with one alt read."""
    ref, a1, a2 = _contig()
    p = 400
    het = [(ref[p], 50)] * 5 + [(a1[p], 60)] * 5
    match, mismatch, log = _both(ctx, _batch(ref, _column(ref, p, het)), ref, [(p, p + 1)])
    assert np.array_equal(match, _bins([50] * 5 + [60] * 5)) and mismatch.sum() == 0 and (log[6], log[9], log[10]) == (1, 1, 0)
    match, mismatch, log = _both(ctx, _batch(ref, _column(ref, p, het + [(a2[p], 33)])), ref, [(p, p + 1)])
    assert match.sum() == 0 and np.array_equal(mismatch, _bins([33])) and (log[6], log[9], log[10]) == (1, 0, 1)
    match, mismatch, log = _both(ctx, _batch(ref, _column(ref, p, [(ref[p], 93)] * 9 + [(a1[p], 20)])), ref, [(p, p + 1)])
    assert match.sum() == 0 and np.array_equal(mismatch, _bins([20])) and (log[5], log[10]) == (1, 1)


def test_depth_threshold_is_inclusive(ctx):
    """depth == md_threshold - 1 is counted, depth == md_threshold is skipped at step 2."""
    ref, _a1, _a2 = _contig()
    b = _batch(ref, _column(ref, 400, [(ref[400], 41)] * 10))
    match, _mm, log = _both(ctx, b, ref, [(400, 401)], md_threshold=11)
    assert match[41] == 10 and log[2] == 0 and log[5] == 1
    match, _mm, log = _both(ctx, b, ref, [(400, 401)], md_threshold=10)
    assert match.sum() == 0 and log[2] == 1


def test_indels_skip_their_positions(ctx):
    """An insertion skips the position that FOLLOWS it; a deletion skips each deleted position; the neighbours count."""
    ref, _a1, _a2 = _contig()
    reads = [GM.make_read(ref, 340 + k, 130, bq=30 + k) for k in range(8)]
    reads[3] = GM.make_read(ref, 343, 130, ins={401: "AC"}, dels={410: 3}, bq=33)
    b = _batch(ref, reads)
    match, _mm, log = _both(ctx, b, ref, [(398, 416)])
    assert log[0] == 18 and log[3] == 4 and log[5] == 14 and match.sum() == 14 * 8
    for p, skipped in ((400, False), (401, True), (402, False), (409, False), (410, True), (411, True), (412, True), (413, False)):
        _m, _mm, log = _both(ctx, b, ref, [(p, p + 1)])
        assert log[3] == skipped, p
    # an insertion at the very end of a read's text sits at its tend
    tail = _batch(ref, reads + [GM.make_read(ref, 300, 105, ins={405: "G"}, bq=35)])
    _m, _mm, log = _both(ctx, tail, ref, [(404, 407)])
    assert log[3] == 1 and log[5] == 2


def test_reference_letters(ctx):
    """A lower-case letter or an N in the reference string: the position is skipped at step 1, whatever the pile holds."""
    ref, _a1, _a2 = _contig()
    b = _batch(ref, [GM.make_read(ref, 340 + k, 130, bq=93) for k in range(8)])
    masked = ref[:410] + ref[410].lower() + "N" + ref[412:]
    match, _mm, log = _both(ctx, b, masked, [(405, 415)])
    assert log[1] == 2 and log[5] == 8 and match[93] == 64


def test_pile_membership(ctx):
    """A secondary read is left out; min_mapq removes reads and flips the verdict from het to homref."""
    ref, a1, _a2 = _contig()
    p = 400
    cells = [(ref[p], 93)] * 9 + [(a1[p], 25, dict(flag=0x100))]
    match, mismatch, log = _both(ctx, _batch(ref, _column(ref, p, cells)), ref, [(p, p + 1)])
    assert match[93] == 9 and mismatch.sum() == 0 and log[5] == 1
    cells = [(ref[p], 93)] * 6 + [(a1[p], 70, dict(mapq=10))] * 5
    b = _batch(ref, _column(ref, p, cells))
    match, mismatch, log = _both(ctx, b, ref, [(p, p + 1)], min_mapq=0)
    assert log[6] == 1 and match[93] == 6 and match[70] == 5
    match, mismatch, log = _both(ctx, b, ref, [(p, p + 1)], min_mapq=20)
    assert log[5] == 1 and match[93] == 6 and match[70] == 0 and mismatch.sum() == 0


def test_empty_columns_and_overlapping_regions(ctx):
    """An empty column passes as homref by the prior and adds nothing; a region without any read; a position two regions
    hold is swept once per region."""
    ref, a1, _a2 = _contig()
    b = _batch(ref, _column(ref, 400, [(ref[400], 93)] * 9 + [(a1[400], 20)]))
    match, mismatch, log = _both(ctx, b, ref, [(2000, 2700)])
    assert log[0] == log[5] == 700 and log[9] == log[10] == 0 and match.sum() == mismatch.sum() == 0
    one = _both(ctx, b, ref, [(380, 420)])
    two = _both(ctx, b, ref, [(380, 405), (395, 420), (3000, 3100)])
    again = _both(ctx, b, ref, [(395, 405)])
    assert np.array_equal(two[0], one[0] + again[0]) and np.array_equal(two[1], one[1] + again[1]) and two[1][20] == 2
    assert two[2][0] == 40 + 10 + 100


# ---- 4. geometry

def _sample(seed, length, **kw):
    from himut_amd import synth
    cfg = dict(seed=seed, contig_len=length, depth=20.0, read_len_mean=3000, read_len_sd=800, read_len_min=500,
               read_len_max=8000, snp_rate=2e-3, hetalt_frac=0.1, sub_rate=1e-3, ins_rate=5e-4, del_rate=5e-4, name="chrS")
    cfg.update(kw)
    s = synth.generate(synth.SynthConfig(**cfg), want_ref=True)
    return s.batch, bytes(s.ref).decode("ascii")


@pytest.fixture(scope="module")
def sample():
    return _sample(91, 12_000)


def test_regions_off_the_tile_grid(ctx, sample):
    """A region that starts and ends off the tile grid and spans three tiles (its reads cross the tile borders); the
    same positions as three regions cut at other places; a region with no read at all behind the contig's reads."""
    b, seq = sample
    whole = _both(ctx, b, seq, [(777, 777 + 2 * 512 + 300)])
    assert whole[2][0] == 1324 and whole[0].sum() > 10_000
    parts = _both(ctx, b, seq, [(777, 1000), (1000, 1811), (1811, 2101)])
    assert np.array_equal(parts[0], whole[0]) and np.array_equal(parts[1], whole[1]) and parts[2] == whole[2]


def test_row_batches_give_the_same_numbers(ctx, sample):
    """More pile rows than one LDS batch: the batches are staged a second time behind the verdict.  The path is forced
    with himut_debug_bqcal (rows per batch; 0 is the default, all the kernel has room for) on a 20-deep pile, and taken
    without the hook by a pile deeper than the kernel's batch of 64 rows."""
    b, seq = sample
    want = M.run(b, seq, [(0, b.length)])
    try:
        for rows in (0, 1, 5, 64, 1000):
            ctx.debug_bqcal(rows)
            _both(ctx, b, seq, [(0, b.length)], want=want)
    finally:
        ctx.debug_bqcal(0)
    ref, a1, _a2 = _contig()
    deep = _column(ref, 400, [(ref[400], 1 + k % 93) for k in range(75)] + [(a1[400], 17)] * 5)
    match, mismatch, log = _both(ctx, _batch(ref, deep), ref, [(350, 470)])
    assert mismatch[17] == 5 and log[10] == 1 and match.sum() > 5000


def test_many_pieces_and_many_reads_in_one_tile(ctx):
    """A read with more than four pieces in one tile goes position by position from its segment list; more reads than
    one round of the window takes (the tile's threads) overlap one tile."""
    ref, a1, _a2 = _contig()
    reads = [GM.make_read(ref, 250 + 3 * k, 300, bq=40 + k) for k in range(8)]
    reads.append(GM.make_read(ref, 260, 300, dels={300: 2, 320: 1, 340: 2, 360: 1}, ins={380: "A", 400: "TT"}, subs={330: a1[330]}, bq=77))
    match, mismatch, log = _both(ctx, _batch(ref, reads), ref, [(0, 1000)])
    assert log[3] == 8 and mismatch[77] == 1 and match[77] > 200
    rs = random.Random(5)
    many = [GM.make_read(ref, 1030 + rs.randrange(440), 40, bq=rs.choice((93, 93, 93, 40, 12))) for _ in range(700)]
    match, _mm, log = _both(ctx, _batch(ref, many), ref, [(1024, 1536)])
    assert match.sum() == 700 * 40 and log[0] == 512


# ---- 5. the histogram

def test_histogram_runs(ctx):
    """Every base of one quality (one run per column); the 93 qualities 1 .. 93 in one column stack (a run per row,
    deeper than one row batch); one read of quality 200 (a bin above 93)."""
    ref, _a1, _a2 = _contig()
    b = _batch(ref, [GM.make_read(ref, 100 + k, 700, bq=93) for k in range(12)])
    match, _mm, _log = _both(ctx, b, ref, [(0, 1000)])
    assert match[93] == 12 * 700 == match.sum()
    b = _batch(ref, [GM.make_read(ref, 100, 700, bq=q) for q in range(1, 94)])
    match, mismatch, _log = _both(ctx, b, ref, [(0, 1000)])
    assert np.all(match[1:94] == 700) and match.sum() == 93 * 700 and mismatch.sum() == 0
    b = _batch(ref, [GM.make_read(ref, 100 + k, 700, bq=200 if k == 4 else 93) for k in range(12)])
    match, _mm, _log = _both(ctx, b, ref, [(0, 1000)])
    assert match[200] == 700 and match[93] == 11 * 700


# ---- 6. errors

def test_errors_then_a_good_contig(ctx):
    """Quality 0 in a column that reaches the genotyper: HIMUT_ERR_BQ0; quality 0 in a column skipped at step 2 or 3: no
    error; a query N in an aligned position: HIMUT_ERR_BASE; a region behind the reference string or with start > end:
    HIMUT_ERR_CHUNK.  The same context runs a good contig right after each."""
    from himut_amd._ffi import HimutError
    ref, _a1, _a2 = _contig()
    good = [GM.make_read(ref, 340 + k, 130, bq=93) for k in range(8)]
    want = M.run(_batch(ref, good), ref, [(300, 500)])

    def with_bq0(reads, k, pos):
        reads = [dict(r) for r in reads]
        reads[k]["bq"] = list(reads[k]["bq"])
        reads[k]["bq"][pos - reads[k]["tstart"]] = 0
        return reads
    ins = list(good)
    ins[3] = GM.make_read(ref, 343, 130, ins={401: "AC"}, bq=93)
    cases = [("bq0", with_bq0(good, 2, 400), {}, GM.ERR_BQ0),
             ("bq0 under the depth bar", with_bq0(good, 2, 400), dict(md_threshold=8), 0),
             ("bq0 behind an insertion", with_bq0(ins, 2, 401), {}, 0)]
    n = [dict(r) for r in good]
    n[5]["seq"] = n[5]["seq"][:20] + "N" + n[5]["seq"][21:]
    cases.append(("n", n, {}, GM.ERR_BASE))
    for what, reads, kw, code in cases:
        b = _batch(ref, reads)
        got = _both(ctx, b, ref, [(300, 500)], **kw)
        assert (got is None) == (code != 0), what
        if code:
            with pytest.raises(GM.ModelError) as me:
                M.run(b, ref, [(300, 500)], **kw)
            assert me.value.code == code
        _same(_bqcal(ctx, _batch(ref, good), ref, [(300, 500)]), want)
    for regions in ([(300, len(ref) + 1)], [(500, 300)], [(-1, 300)]):
        with pytest.raises(HimutError) as e:
            _bqcal(ctx, _batch(ref, good), ref, regions)
        assert e.value.code == ERR_CHUNK
        _same(_bqcal(ctx, _batch(ref, good), ref, [(300, 500)]), want)
    _same(_bqcal(ctx, _batch(ref, good), ref, [(300, len(ref))]), M.run(_batch(ref, good), ref, [(300, len(ref))]))


def test_argument_errors():
    """No tables, no reads, no regions, no reference string: HIMUT_ERR_ARG each; himut_set_params is never needed."""
    from himut_amd import _ffi, bamio, gtlib
    ref, _a1, _a2 = _contig()
    b = _batch(ref, [GM.make_read(ref, 100, 600)])
    with _ffi.Context(0) as c:
        for step in (lambda: c.set_gt_lut(*gtlib.build_tables(1e-3)), lambda: c.push_reads(b), lambda: c.set_chunks([(0, 4000)]),
                     lambda: bamio.set_contig_reference(c, ref)):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_bqcal()
            assert e.value.code == ERR_ARG
            step()
        c.run_bqcal()
        match, _mm, log = c.bqcal()
        assert log[0] == 4000 and match.sum() == 600
        st = c.stats()
        assert st["ms_total"] > 0 and (st["n_reads"], st["read_bases"], st["positions"]) == (1, 600, 4000)


# ---- 7. state

def test_call_bqcal_germline_call_on_one_context(sample):
    """call -> bqcal -> germline -> call -> bqcal on one context: every run gives what it gives alone, a run's results
    stay in reach while the others run, and the second bqcal run equals the first."""
    from himut_amd.caller import Worker
    b, seq = sample
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=500, qlen_upper_limit=8000, md_threshold=60)
    germ_kw = dict(min_gq=20, min_bq=20, min_ref_count=2, min_alt_count=2)

    def call(w):
        w.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"], p["min_gq"],
                    p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"], p["md_threshold"],
                    p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"], False)
        return w.call_contig(b, [(0, b.length)])

    def same_records(x, y):
        return len(x) == len(y) and all(np.array_equal(x[k], y[k]) for k in x.dtype.names)
    with Worker(0).ctx as f:
        _load(f, b, seq, [(1, b.length)])
        f.run_germline(**germ_kw)
        germ_alone = f.germline()
    want = M.run(b, seq, [(0, b.length)], md_threshold=60)
    w = Worker(0)
    try:
        recs, log = call(w)
        w._lut_prior = None
        first = _bqcal(w.ctx, b, seq, [(0, b.length)], md_threshold=60)
        _same(first, want)
        assert same_records(w.ctx.records(), recs) and w.ctx.log() == log
        w.ctx.set_chunks([(1, b.length)])
        w.ctx.run_germline(**germ_kw)
        germ = w.ctx.germline()
        assert same_records(germ[0], germ_alone[0]) and germ[1] == germ_alone[1] and len(germ[0]) > 0
        _same(w.ctx.bqcal(), want)
        assert same_records(w.ctx.records(), recs)
        w._lut_prior = None
        recs2, log2 = call(w)
        assert same_records(recs2, recs) and log2 == log
        again = w.ctx.germline()
        assert same_records(again[0], germ_alone[0])
        w._lut_prior = None
        _same(_bqcal(w.ctx, b, seq, [(0, b.length)], md_threshold=60), first)
        assert same_records(w.ctx.records(), recs)
    finally:
        w.close()


# ---- 8. a seeded random round

def test_random_round(ctx):
    """Two dozen small synthetic batches with indels, substitutions and low-quality reads, random regions and parameters,
    random row batches: the run equals the model on each."""
    rs = random.Random(2024)
    passed = 0
    try:
        for k in range(24):
            length = rs.randrange(1000, 2500)
            b, seq = _sample(500 + k, length, depth=rs.choice((4.0, 15.0, 35.0, 80.0)), read_len_mean=rs.choice((300, 900)),
                             read_len_sd=200, read_len_min=60, read_len_max=2500, snp_rate=5e-3, sub_rate=4e-3, ins_rate=2e-3,
                             del_rate=2e-3, frac_lowbq=0.3, frac_lowmapq=0.2, bq93_prob=rs.choice((0.85, 0.3)))
            cuts = sorted(rs.sample(range(length + 1), 4))
            regions = [(cuts[0], cuts[1]), (cuts[2], cuts[3])] if k % 3 else [(0, length)]
            ctx.debug_bqcal(rs.choice((0, 0, 3, 17)))
            got = _both(ctx, b, seq, regions, rs.choice((1e-3, 1e-2)), min_mapq=rs.choice((0, 0, 30)), min_gq=rs.choice((0, 20, 40)),
                        md_threshold=rs.choice((1 << 30, 30, 12)))
            passed += got is not None and got[1].sum() > 0
    finally:
        ctx.debug_bqcal(0)
    assert passed >= 12


# ---- 9. the command

def test_cli_end_to_end(tmp_path):
    """`himut bqcal` on a synthetic BAM written by the package's own writer: the TSV is the text the model's counts
    format to, under the depth threshold the driver takes from the samples."""
    from himut_amd import __main__ as cli
    from himut_amd import bamio, bamlib, util as U
    b, seq = _sample(93, 60_000, depth=10.0, name="chr9")
    bam, fa, tsv = str(tmp_path / "in.bam"), str(tmp_path / "g.fa"), str(tmp_path / "bq.tsv")
    with open(fa, "w") as o:
        o.write(">chr9\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
    bamio.write_bam(bam, [b], sample="SMP")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli.main(["bqcal", "-i", bam, "--ref", fa, "-o", tsv])
    finally:
        os.chdir(cwd)
    sizes = {b.name: b.length}
    _lo, _hi, md = bamlib.get_thresholds({b.name: b}, [b.name], sizes)
    _chroms, chunks = U.load_loci(None, None, sizes)
    match, mismatch, log = M.run(b, seq, [(s, e) for _c, s, e in chunks[b.name]], md_threshold=md)
    assert open(tsv).read() == M.table_text(match, mismatch)
    assert log[2] > 0 and match.sum() > 100_000 and mismatch.sum() > 0
