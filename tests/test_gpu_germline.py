"""The germline run (himut_run_germline / himut_get_germline) through the C ABI against the plain-Python model of its
contract (tests/germline_model.py): np.array_equal on every field of the record arrays and equality of the twelve
counters.  The genotype fixtures (tests/golden/leaf_gtlib.json, gt_edges.json) pin k_germline_eval's fp64 sums to
the reference's gtlib.get_germ_gt; hand-built alignments pin the rules of the contract; a synthetic sample pins the
run at the sizes where the capture and the column index change steps; sequences on one context pin the state a germline
run and a call run leave each other."""
import os
import random

import numpy as np
import pytest

from tests import germline_model as M
from tests import gt_piles as G
from tests import util
from tests.test_germline_cpu import _check_vector, _reversed

pytestmark = pytest.mark.gpu

OPEN = dict(min_gq=0, min_bq=1, min_ref_count=0, min_alt_count=0)       # every non-homref record is PASS


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _lut(c, prior):
    from himut_amd import gtlib
    c.set_gt_lut(*gtlib.build_tables(prior))


def _germ(c, batch, regions, prior=1 / (10 ** 3), push=True, **kw):
    _lut(c, prior)
    c.set_chunks(regions)
    if push:
        c.push_reads(batch)
    c.run_germline(**kw)
    return c.germline()


def _both(c, batch, regions, prior=1 / (10 ** 3), **kw):
    """The run and the model on the same input: equal; returns (records, log)."""
    got, glog = _germ(c, batch, regions, prior, **kw)
    want, wlog = M.run(batch, regions, prior, **kw)
    M.assert_same(got, glog, want, wlog)
    return got, glog


# ---- 1. fp64 boundaries

def _key(r):
    return chr(r["gt0"]) + chr(r["gt1"]), int(r["gq"]), int(r["gt_state"])


def test_leaf_vectors(ctx):
    """leaf_gtlib's 400 columns in one pile at prior 1e-3: every column with a non-reference allele gives one record
    equal to the fixture in gt, gq, state and counts; without report_homref the homref columns give none."""
    vs = G.leaf_vectors(util.load_json("leaf_gtlib")["vectors"])
    P = G.build(vs)
    for homref in (True, False):
        recs, _ = _both(ctx, P.batch, P.call_chunks, report_homref=homref, min_gq=20, min_bq=1, min_ref_count=3, min_alt_count=1)
        assert sum(_check_vector(v, c[0], recs, homref) for v, c in zip(vs, P.cols)) == len(recs) > 100


def test_gt_edges_vectors(ctx):
    """Each boundary vector in its own pile at its own prior with min_gq = k (columns deeper than a wave and than the
    eval's batch included): the 136 columns with a non-reference allele give the fixture's record; the state pairs
    appear and disappear with report_homref.  Fetch order: every such column whose gt, gq or state depends on the order
    of its reads is run a second time with the reads turned round and gives the other record.  The fixture's own
    order pairs hold reference alleles only, so by the contract they are no candidates: they differ in the fixture
    and give no record here, with or without report_homref."""
    edges = util.load_json("gt_edges")["vectors"]
    seen, lowgq, turned, out = 0, 0, 0, {}
    for i, v in enumerate(edges):
        P = G.build([v], orders=[G.ORDERS[i % 3]])
        kw = dict(min_gq=v["k"], min_bq=1, min_ref_count=0, min_alt_count=0)
        nonref = set(v["alleles"]) != {v["ref"]}
        for homref in (True, False):
            recs, _ = _both(ctx, P.batch, P.call_chunks, v["prior"], report_homref=homref, **kw)
            n = _check_vector(v, P.cols[0][0], recs, homref)
            assert len(recs) == n
            if n and v["state"] != "homref":
                assert (int(recs[0]["status"]) == M.ST_LOWGQ) == (v["gq"] < v["k"])
                lowgq += v["gq"] < v["k"]
            if homref:
                assert n == nonref
                out[i] = _key(recs[0]) if n else None
        seen += nonref
        w = _reversed(v) if nonref else None
        if w is not None:
            P = G.build([w], orders=[G.ORDERS[i % 3]])
            recs, _ = _both(ctx, P.batch, P.call_chunks, v["prior"], report_homref=True, **kw)
            assert _check_vector(w, P.cols[0][0], recs, True) == len(recs) == 1 and _key(recs[0]) != out[i]
            turned += 1
    assert seen == 136 and lowgq > 0 and turned > 50
    pairs = {}
    for i, v in enumerate(edges):
        if v["kind"] == "order":
            pairs.setdefault(v["pair"], []).append(i)
    assert len(pairs) >= 5
    for a, b in pairs.values():
        va, vb = edges[a], edges[b]
        assert (va["gt"], va["gq"], va["state"]) != (vb["gt"], vb["gq"], vb["state"])
        assert set(va["alleles"]) == set(vb["alleles"]) == {va["ref"]} and out[a] is None and out[b] is None
    st = [i for i, v in enumerate(edges) if v["kind"] == "state"]
    assert {out[i][2] for i in st if out[i]} > {0}


# ---- 2. rules on hand-built alignments

def _contig(n=4000, seed=3):
    rs = random.Random(seed)
    ref = "".join(rs.choice("ATGC") for _ in range(n))
    return ref, {p: "ATGC"[("ATGC".index(ref[p]) + 1) % 4] for p in range(n)}, {p: "ATGC"[("ATGC".index(ref[p]) + 2) % 4] for p in range(n)}


def _batch(ref, recs):
    from himut_amd.readbatch import batch_from_records
    recs = sorted(recs, key=lambda r: r["tstart"])
    return batch_from_records("chrH", len(ref), recs)


def test_regions_select_and_never_shape(ctx):
    """A position held by two adjacent regions is reported once; a position outside every region is not reported;
    overlapping and out-of-order regions give the same record for every position they share; a read that ends exactly at
    a region's start IS in the column at tpos == start, and the call run's column there is shallower."""
    ref, a1, _ = _contig()
    reads = [M.make_read(ref, 300 + 7 * k, 300 - 7 * k, {599: a1[599]} if k < 3 else {}, bq=93) for k in range(4)]     # end at 600
    reads += [M.make_read(ref, 400 + 11 * k, 700, {599: a1[599]} if k == 0 else ({900: a1[900]} if k < 3 else {}), bq=93,
                          bq_at={599: 2} if k == 0 else None) for k in range(5)]
    b = _batch(ref, reads)
    one, log = _both(ctx, b, [(1, 4000)], report_homref=True, **OPEN)
    assert list(one["tpos"]) == [600, 901] and int(one[0]["counts"][:4].sum()) == 9
    adj, alog = _both(ctx, b, [(1, 600), (600, 1200)], report_homref=True, **OPEN)
    assert alog == log and all(np.array_equal(adj[k], one[k]) for k in M.FIELDS)
    mixed, _ = _both(ctx, b, [(850, 1000), (590, 900), (600, 600), (2000, 3000)], report_homref=True, **OPEN)
    assert all(np.array_equal(mixed[k], one[k]) for k in M.FIELDS)
    at_start, _ = _both(ctx, b, [(600, 800)], report_homref=True, **OPEN)
    assert all(np.array_equal(at_start[k], one[:1][k]) for k in M.FIELDS)
    none, nlog = _both(ctx, b, [(1, 599), (601, 700)], report_homref=True, **OPEN)
    assert len(none) == 0 and nlog == [0] * 12
    # the same reads through himut_run with the chunk (600, 800): the reads that end at 600 are not fetched by it
    p = G.params(0, 1 / (10 ** 3), 20)
    ctx.set_params(**{k: v for k, v in p.items() if k != "germline_snv_prior"})
    ctx.set_site_set(0, np.zeros(0, np.uint64)); ctx.set_site_set(1, np.zeros(0, np.uint64))
    ctx.set_chunks([(600, 800)])
    ctx.run()
    crecs = ctx.records()
    assert list(crecs["tpos"]) == [600] and int(crecs[0]["counts"][:4].sum()) == 5
    # ... and the germline records are still served, the call's by himut_get_records
    again, _ = ctx.germline()
    assert all(np.array_equal(again[k], none[k]) for k in M.FIELDS)


def test_pile_membership(ctx):
    """A secondary read is out, a supplementary read is in; a read that fails every filter of `call` (mapq 0, identity,
    length, a substitution in its first base and inside a mismatch window) marks and counts with min_mapq = 0, and leaves
    both the marks and the columns with min_mapq = 20."""
    ref, a1, _ = _contig()
    reads = [M.make_read(ref, 100 + 13 * k, 600, {400: a1[400]} if k % 2 else {}, bq=93) for k in range(8)]
    reads.append(M.make_read(ref, 350, 300, {400: a1[400]}, bq=93, flag=0x100))
    reads.append(M.make_read(ref, 360, 300, {400: a1[400]}, bq=93, flag=0x800))
    bad = {p: a1[p] for p in (380, 381, 383, 400, 410, 411, 415, 419)}
    reads.append(M.make_read(ref, 380, 40, bad, bq=5, mapq=0))
    b = _batch(ref, reads)
    lo, llog = _both(ctx, b, [(1, 4000)], report_homref=True, **OPEN)
    assert list(lo["tpos"]) == [381, 382, 384, 401, 411, 412, 416, 420] and llog[0] == 8
    at = lo[lo["tpos"] == 401][0]
    assert int(at["counts"][:4].sum()) == 10                    # 8 + supplementary + the mapq-0 read, not the secondary
    hi, hlog = _both(ctx, b, [(1, 4000)], report_homref=True, min_mapq=20, **OPEN)
    assert list(hi["tpos"]) == [401] and int(hi[0]["counts"][:4].sum()) == 9 and hlog[0] == 1


def test_cs_forms_indels_and_n_reference(ctx):
    """Long-form cs; an insertion in front of a column and a deletion over it show in counts[4] and counts[5]; a *n?
    substitution is counted in num_nref with no record."""
    ref, a1, a2 = _contig()
    reads = []
    for k in range(10):
        subs = {700: a1[700]} if k % 2 else {}
        if k == 3:
            subs[800] = a1[800]
        reads.append(M.make_read(ref, 500 + 9 * k, 500, subs, ins={700: "AC"} if k in (0, 1) else ({1000 + 9 * k: "G"} if k == 7 else None),
                                 dels={699: 3} if k == 2 else ({640: 5} if k == 4 else None), bq=60, long_cs=k % 3 == 0,
                                 nref=(800,)))
    b = _batch(ref, reads)
    recs, log = _both(ctx, b, [(1, 4000)], report_homref=True, **OPEN)
    assert list(recs["tpos"]) == [701] and log[:2] == [1, 1]
    assert int(recs[0]["counts"][4]) == 2 and int(recs[0]["counts"][5]) == 1 and int(recs[0]["counts"][:4].sum()) == 9
    # two reads that name different reference bases at one position: malformed input
    from himut_amd._ffi import HimutError
    two = [M.make_read(ref, 500, 400, {700: a1[700]}, bq=60), M.make_read(ref, 510, 400, {700: a1[700]}, bq=60)]
    two[1]["cs"] = two[1]["cs"].replace("*" + ref[700].lower(), "*" + a2[700].lower())
    with pytest.raises(HimutError) as e:
        _germ(ctx, _batch(ref, two), [(1, 4000)])
    assert e.value.code == M.ERR_CS
    with pytest.raises(M.ModelError):
        M.run(_batch(ref, two), [(1, 4000)])


def test_filter_cascade(ctx):
    """Each FILTER value once, first rule first; het-alt in genotype order.  A het-alt genotype with an allele that no
    read carries cannot come out of the reference's arithmetic (with reads of one of its alleles only, the hom-alt
    genotype has the larger likelihood term for each of them and the larger prior): the LowBQ het-alt here is the one
    where every read of one genotype allele is below min_bq."""
    ref, a1, a2 = _contig()
    cols = {
        500: dict(n=12, alt=6),                        # het, PASS
        700: dict(n=3, alt=2, q=60),                   # het with gq 0
        900: dict(n=16, alt=16, qalt=19),              # hom-alt, every alt read below min_bq (and deeper than md_threshold)
        1100: dict(n=3, alt=2),                        # het with one reference read
        1300: dict(n=12, alt=12),                      # hom-alt, PASS
        1500: dict(n=12, alt=6, alt2=6),               # het-alt, PASS
        1700: dict(n=20, alt=4, alt2=16, q2=19),       # het-alt, one allele's reads all below min_bq
        1900: dict(n=18, alt=9),                       # het, deeper than md_threshold
    }
    reads = []
    for pos, c in cols.items():
        q = c.get("q", 93)
        for k in range(c["n"]):
            subs, bq_at = {}, {pos: q}
            if k < c["alt"]:
                subs[pos] = a1[pos]
                bq_at[pos] = c.get("qalt", q)
            elif k < c["alt"] + c.get("alt2", 0):
                subs[pos] = a2[pos]
                bq_at[pos] = c.get("q2", q)
            reads.append(M.make_read(ref, pos - 70 + 3 * k, 120, subs, bq=93, bq_at=bq_at))
    b = _batch(ref, reads)
    recs, log = _both(ctx, b, [(1, 4000)], min_gq=10, min_bq=20, min_ref_count=2, min_alt_count=2, md_threshold=14)
    st = {int(r["tpos"]) - 1: (int(r["gt_state"]), int(r["status"])) for r in recs}
    print("filter cascade:", st, log)
    assert st == {500: (1, M.ST_PASS), 700: (1, M.ST_LOWGQ), 900: (3, M.ST_LOWBQ), 1100: (1, M.ST_LOWDEPTH), 1300: (3, M.ST_PASS),
                  1500: (2, M.ST_PASS), 1700: (2, M.ST_LOWBQ), 1900: (1, M.ST_HIGHDEPTH)}
    assert log[6:11] == [sum(s == x for _, s in st.values()) for x in (M.ST_PASS, M.ST_LOWGQ, M.ST_LOWBQ, M.ST_LOWDEPTH, M.ST_HIGHDEPTH)]
    r = recs[recs["tpos"] == 1501][0]
    assert chr(r["alt"]) == chr(r["gt0"]) and {chr(r["gt0"]), chr(r["gt1"])} == {a1[1500], a2[1500]}


def test_errors_then_a_good_contig(ctx):
    """Quality 0 in a candidate column: HIMUT_ERR_BQ0; a query N in an aligned position of a pile read: HIMUT_ERR_BASE;
    quality 0 outside every candidate column is no error; the same context runs a good contig right afterwards."""
    from himut_amd._ffi import HimutError
    ref, a1, _ = _contig()
    good = [M.make_read(ref, 100 + 13 * k, 600, {400: a1[400]} if k % 2 else {}, bq=93) for k in range(8)]
    want, wlog = M.run(_batch(ref, good), [(1, 4000)], **OPEN)
    for what, code in (("bq0", M.ERR_BQ0), ("n", M.ERR_BASE), ("bq0_elsewhere", 0)):
        reads = [dict(r) for r in good]
        if what == "bq0":
            reads[2]["bq"] = list(reads[2]["bq"]); reads[2]["bq"][400 - reads[2]["tstart"]] = 0
        elif what == "bq0_elsewhere":
            reads[2]["bq"] = list(reads[2]["bq"]); reads[2]["bq"][401 - reads[2]["tstart"]] = 0
        else:
            s = reads[3]["seq"]; k = 300 - reads[3]["tstart"]
            reads[3]["seq"] = s[:k] + "N" + s[k + 1:]
        b = _batch(ref, reads)
        if code:
            with pytest.raises(HimutError) as e:
                _germ(ctx, b, [(1, 4000)], **OPEN)
            assert e.value.code == code
            with pytest.raises(M.ModelError) as me:
                M.run(b, [(1, 4000)], **OPEN)
            assert me.value.code == code
        else:
            _both(ctx, b, [(1, 4000)], **OPEN)
        got, glog = _germ(ctx, _batch(ref, good), [(1, 4000)], **OPEN)
        M.assert_same(got, glog, want, wlog)


def test_argument_errors():
    from himut_amd import _ffi, gtlib
    ref, a1, _ = _contig()
    b = _batch(ref, [M.make_read(ref, 100, 600, {400: a1[400]})])
    with _ffi.Context(0) as c:
        for step in (lambda: c.set_gt_lut(*gtlib.build_tables(1e-3)), lambda: c.push_reads(b), lambda: c.set_chunks([(1, 4000)])):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_germline()
            assert e.value.code == 1
            step()
        c.run_germline()                       # himut_set_params was never called: not needed
        assert c.germline()[1][0] == 1


# ---- 3. a synthetic sample

def _sample(seed, length, **kw):
    from himut_amd import synth
    cfg = dict(seed=seed, contig_len=length, depth=20.0, read_len_mean=6000, read_len_sd=1200, read_len_min=2000,
               read_len_max=12000, snp_rate=1e-3, hetalt_frac=0.1, name="chrS")
    cfg.update(kw)
    return synth.generate(synth.SynthConfig(**cfg))


@pytest.fixture(scope="module")
def big():
    return _sample(71, 260_000).batch


@pytest.fixture(scope="module")
def big_model(big):
    return M.run(big, [(1, big.length)])


def _by_tpos(recs):
    return {int(r["tpos"]): r for r in recs}


@pytest.mark.parametrize("rates", ["default", "5e-4"])
def test_synthetic_sample(ctx, big, big_model, rates):
    """260 kb at depth 20 (two of chunkloci's tiles, a thousand 256-position blocks, the capture's 8192-cell and
    16 k-position steps): one region, chunkloci's tiles and random regions equal the model, and give the same record for
    every position they share."""
    from himut_amd import util as hutil
    if rates == "default":
        b, (want, wlog) = big, big_model
    else:
        b = _sample(72, 260_000, sub_rate=5e-4, ins_rate=5e-4, del_rate=5e-4).batch
        want, wlog = M.run(b, [(1, b.length)])
    one, olog = _germ(ctx, b, [(1, b.length)])
    M.assert_same(one, olog, want, wlog)
    assert olog[3] > 50 and olog[5] > 20 and olog[4] > 3 and olog[6] > 100
    tiles = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
    assert len(tiles) == 2
    t, tlog = _germ(ctx, b, tiles, push=False)
    # chunkloci's tiles start at tpos 0: everything but position 0 is the one region's
    assert tlog == olog and all(np.array_equal(t[k], one[k]) for k in M.FIELDS)
    rs = np.random.RandomState(5)
    cuts = rs.randint(1, b.length, 10)
    regions = [(int(min(x, y)), int(max(x, y))) for x, y in zip(cuts[0::2], cuts[1::2])]
    r, rlog = _both(ctx, b, regions)
    full = _by_tpos(one)
    assert 0 < len(r) < len(one)
    assert all(np.array_equal(x[k], full[int(x["tpos"])][k]) for x in r for k in M.FIELDS)


def test_call_records_have_their_germline_twin(ctx):
    """min_mapq = 0: every himut_run record with gt_state != 0 whose tpos is not its chunk's start has a germline record
    at that tpos with the same gt0, gt1, gt_state, gq, counts and bqsum (the call run's pile is the germline run's)."""
    big = _sample(76, 60_000, snp_rate=5e-3, sub_rate=2e-3).batch      # errors on top of SNP sites: records the call run keeps
    tiles = [(0, 20_000), (20_000, 45_000), (45_000, 60_000)]
    g, _ = _germ(ctx, big, tiles, report_homref=True)
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=0, qlen_upper_limit=1 << 20, md_threshold=60, min_bq=20, min_qv=0, min_mapq=0,
             min_sequence_identity=0.0, min_trim=0.0, max_mismatch_count=1 << 20, mismatch_window_size=0)
    ctx.set_params(**{k: v for k, v in p.items() if k in ("min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq",
                                                         "min_bq", "max_mismatch_count", "mismatch_window_size", "md_threshold",
                                                         "min_ref_count", "min_alt_count", "min_hap_count",
                                                         "min_sequence_identity", "min_trim")})
    ctx.set_site_set(0, np.zeros(0, np.uint64)); ctx.set_site_set(1, np.zeros(0, np.uint64))
    ctx.run()
    crecs = ctx.records()
    twin, n = _by_tpos(g), 0
    for r in crecs:
        if int(r["gt_state"]) == 0 or int(r["tpos"]) == tiles[int(r["chunk"])][0]:
            continue
        t = twin[int(r["tpos"])]
        assert all(np.array_equal(r[k], t[k]) for k in ("gt0", "gt1", "gt_state", "gq", "counts", "bqsum")), (r, t)
        n += 1
    assert n > 5


# ---- 4. context reuse

def test_context_reuse(ctx, big, big_model):
    """germline -> call -> germline; 260 kb -> 30 kb -> 260 kb; a first run that overflows the capacities it kept: each
    result equals the model's (what a fresh context gives), the call results in between equal a fresh context's."""
    from himut_amd.caller import Worker
    small = _sample(73, 30_000, depth=8.0).batch
    dense = _sample(74, 30_000, depth=40.0, sub_rate=2e-3).batch
    want = {"big": big_model, "small": M.run(small, [(1, small.length)]), "dense": M.run(dense, [(1, dense.length)])}
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=2000, qlen_upper_limit=12000, md_threshold=60)

    def call(w, b):
        w.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"], p["min_gq"],
                    p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"], p["md_threshold"],
                    p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"], False)
        return w.call_contig(b, [(0, b.length)])
    fresh = Worker(0)
    call_want = {"big": call(fresh, big), "small": call(fresh, small)}
    fresh.close()
    w = Worker(0)
    try:
        w._lut_prior = None
        seq = [("g", "small"), ("g", "big"), ("c", "big"), ("g", "big"), ("g", "small"), ("c", "small"), ("g", "dense"), ("g", "big"),
               ("c", "big"), ("g", "small")]
        reran = []
        for kind, name in seq:
            b = {"big": big, "small": small, "dense": dense}[name]
            if kind == "g":
                got, glog = _germ(w.ctx, b, [(1, b.length)])
                w._lut_prior = None
                M.assert_same(got, glog, *want[name])
                reran.append(w.ctx.stats()["reran"])
            else:
                recs, log = call(w, b)
                assert log == call_want[name][1] and all(np.array_equal(recs[k], call_want[name][0][k]) for k in recs.dtype.names)
        # the runs that followed a smaller contig overflowed what they kept and ran again with exact sizes
        assert reran[:3] == [0, 1, 0]
        st = w.ctx.stats()
        assert st["ms_total"] > 0 and st["n_records"] == len(want["small"][0])
    finally:
        w.close()


def test_alternation_over_the_shared_front(big, big_model, tmp_path):
    """germline, call --phase, germline, call, call on no reads, germline on 260 kb, call --phase on one context: the
    two kinds of run go through one column front and hand each other the bitmap, the scalars, the read windows and the
    mask (k_read_hap sits between the front's halves in the call run only).  Every germline result equals the model's,
    every call result a fresh context's."""
    from himut_amd import synth, vcflib
    from himut_amd.caller import Worker
    from himut_amd.readbatch import batch_from_records
    from tests.test_gpu_parity import _run_hip
    samples = {"small": _sample(77, 30_000, snp_rate=2e-3, som_rate=1e-4), "big": _sample(71, 260_000)}
    assert samples["big"].batch.tstart.tobytes() == big.tstart.tobytes() and samples["big"].batch.cs.tobytes() == big.cs.tobytes()
    batch = {"small": samples["small"].batch, "big": big, "none": batch_from_records("chrS", 30_000, [])}
    want = {"small": M.run(batch["small"], [(1, 30_000)]), "big": big_model}
    phased = {}
    for name, block in (("small", 6), ("big", 20)):
        pv = str(tmp_path / (name + ".vcf"))
        synth.write_phased_vcf(pv, samples[name], block=block)
        hb, hp, hs, c2c = vcflib.load_phased_hetsnps(pv, ["chrS"], {"chrS": batch[name].length})
        phased[name] = ((dict(hb["chrS"]), dict(hp["chrS"]), dict(hs["chrS"])), [(c[1], c[2]) for c in c2c["chrS"]])
    assert 3 <= len(phased["small"][1]) <= 12 and len(phased["big"][1]) > 3
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=2000, qlen_upper_limit=12000, md_threshold=60)

    def call(w, name, phase):
        if phase:
            sets, chunks = phased[name]
            return _run_hip(w, batch[name], chunks, p, None, None, sets)
        return _run_hip(w, batch[name], [(0, 10_000), (10_000, 30_000)], p)
    seq = [("g", "small", 0), ("c", "small", 1), ("g", "small", 0), ("c", "small", 0), ("c", "none", 0), ("g", "big", 0), ("c", "big", 1)]
    call_want = {}
    for kind, name, phase in seq:
        if kind == "c":
            fresh = Worker(0)
            call_want[name, phase] = call(fresh, name, phase)
            fresh.close()
    assert len(call_want["small", 1][0]) > 0 and len(call_want["big", 1][0]) > 0 and len(call_want["none", 0][0]) == 0
    assert (call_want["small", 1][0]["phase_set"] >= 0).any()
    w = Worker(0)
    try:
        for step, (kind, name, phase) in enumerate(seq):
            if kind == "g":
                got, glog = _germ(w.ctx, batch[name], [(1, batch[name].length)])
                w._lut_prior = None
                M.assert_same(got, glog, *want[name])
            else:
                recs, log = call(w, name, phase)
                assert log == call_want[name, phase][1] and recs.tobytes() == call_want[name, phase][0].tobytes(), (step, name, phase)
    finally:
        w.close()


def test_germline_stage_timing_levels(big):
    """himut_set_stage_timing for the germline run: level 2 reports the decode, the index, the capture and the
    evaluation, all inside the total; level 0 the total only."""
    from himut_amd import _ffi
    with _ffi.Context(0) as c:
        for level in (2, 0):
            c.set_stage_timing(level)
            _germ(c, big, [(1, big.length)])
            st = c.stats()
            stages = [st[k] for k in ("ms_parse", "ms_index", "ms_capture", "ms_eval")]
            print("germline stage times, level", level, st["ms_total"], stages)
            assert st["ms_total"] > 0
            if level == 2:
                assert all(x > 0 for x in stages) and st["ms_total"] >= sum(stages)
            else:
                assert all(st[k] == 0 for k in st if k.startswith("ms_") and k != "ms_total")


def test_ingest_path_equals_pushed_reads(ctx, tmp_path):
    """The device-side ingest (ingest_contig), with the cs tags of the file and with the text derived from CIGAR and the
    reference, gives the records of the pushed reads."""
    from himut_amd import bamio, synth
    from tests import cs_from_cigar
    s = synth.generate(synth.SynthConfig(seed=75, contig_len=60_000, depth=20.0, read_len_mean=6000, read_len_sd=1200,
                                         read_len_min=2000, read_len_max=12000, hetalt_frac=0.1, name="chrI"), want_ref=True)
    want, wlog = M.run(s.batch, [(1, s.batch.length)])
    tagged, bare = str(tmp_path / "t.bam"), str(tmp_path / "b.bam")
    bamio.write_bam(tagged, [s.batch], sample="S")
    cs_from_cigar.batch_bam(bare, s.batch, "M", sample="S")
    for path, derive in ((tagged, False), (bare, True)):
        st = bamio.BamStream(path, threads=2)
        if derive:
            bamio.set_contig_reference(ctx, bytes(s.ref))
        st.ingest_contig(ctx, "chrI", derive_cs=derive)
        st.close()
        _lut(ctx, 1 / (10 ** 3))
        ctx.set_chunks([(1, s.batch.length)])
        ctx.run_germline()
        got, glog = ctx.germline()
        M.assert_same(got, glog, want, wlog)
    ctx.ingest_derive_cs(0)


# ---- 5. the command line

def test_cli_germline_then_phase_then_call_phase(tmp_path):
    """`germline` on a two-contig BAM writes the model's VCF body byte for byte, --devices 0,0 the same bytes; `phase
    --vcf` on the file loads the model's PASS het records; `call --phase` runs on phase's output."""
    from himut_amd import __main__ as cli
    from himut_amd import bamio, bamlib, util as hutil, vcflib
    s1 = _sample(81, 210_000, name="chr2")
    s2 = _sample(82, 70_000, name="chr10")
    bam = str(tmp_path / "in.bam")
    bamio.write_bam(bam, [s2.batch, s1.batch], sample="SMP")
    batches = {"chr2": s1.batch, "chr10": s2.batch}
    sizes = {"chr10": 70_000, "chr2": 210_000}
    chrom_lst, c2c = hutil.load_loci(None, None, sizes)
    _ql, _qu, md = bamlib.get_thresholds(batches, chrom_lst, sizes)
    body, logs, het = [], {}, {}
    for c in chrom_lst:
        recs, logs[c] = M.run(batches[c], [(x[1], x[2]) for x in c2c[c]], md_threshold=md)
        body += M.vcf_lines(c, recs)
        het[c] = [(int(r["tpos"]), chr(r["ref"]), chr(r["gt1"])) for r in recs if r["gt_state"] == 1 and r["status"] == M.ST_PASS]
    out = {}
    cwd = os.getcwd()
    for name, dev in (("one", "0"), ("two", "0,0")):
        d = tmp_path / name
        d.mkdir()
        os.chdir(d)
        try:
            cli.main(["germline", "-i", bam, "-o", str(d / "germline.vcf"), "--devices", dev])
        finally:
            os.chdir(cwd)
        out[name] = open(d / "germline.vcf").read()
        assert [l for l in out[name].splitlines(True) if not l.startswith("#")] == body and len(body) > 150
        rows = [l.split() for l in open(d / "himut_germline.log")]
        assert rows[0] == chrom_lst + ["total"]
        assert [[int(x) for x in r[1:3]] for r in rows[1:]] == [[logs["chr2"][k], logs["chr10"][k]] for k in range(12)]
    assert out["one"].replace("/one/", "/two/") == out["two"]
    assert "##himut_command=himut germline -i {} ".format(bam) in out["one"] and out["one"].splitlines()[-len(body) - 1].endswith("\tSMP")
    g = str(tmp_path / "one" / "germline.vcf")
    for c in chrom_lst:
        assert vcflib.load_hetsnps(g, c, sizes[c])[0] == het[c] and len(het[c]) > 20
    phased = str(tmp_path / "phased.vcf")
    calls = str(tmp_path / "calls.vcf")
    os.chdir(tmp_path)
    try:
        cli.main(["phase", "-i", bam, "--vcf", g, "-o", phased])
        assert sum(1 for l in open(phased) if not l.startswith("#")) == sum(len(v) for v in het.values())
        assert any("|" in l.split("\t")[-1] for l in open(phased) if not l.startswith("#"))
        cli.main(["call", "-i", bam, "--phased_vcf", phased, "--phase", "-o", calls])
    finally:
        os.chdir(cwd)
    assert os.path.getsize(calls) > 0 and open(calls).read().startswith("##fileformat")
