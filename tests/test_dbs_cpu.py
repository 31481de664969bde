"""The dbs contract in plain Python (tests/dbs_model.py) against what each of its rules says on hand-built alignments
(tests/dbs_cases.py) and, on a synthetic sample, against the restated worker of `call` (oracle.call): every half of a
doublet record is the single-base record `call` gives with the mismatch window open.  Then the genotype of a half at
fp64 rounding boundaries: the columns of tests/golden/gt_edges.json and leaf_gtlib.json as halves of doublets
(gt_piles.build_dbs) give records whose half carries the fixture's gt, gq and state.  No GPU here; tests/test_gpu_dbs.py
and tests/test_gpu_gt_edges.py compare the run with this model."""
import collections
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import dbs_cases as C
from tests import dbs_model as M
from tests import gt_piles as G
from tests.test_callmap_cpu import EDGE_KINDS, LEAF_K, LEAF_PRIOR, edge_vectors, leaf_vectors, perturbed

CASES = C.rule_cases() + C.verdict_cases() + C.shape_cases()

# the synthetic sample's parameters: the read filters open (at this error rate identity 0.99 removes four reads in five),
# the window left to do its work at three mismatches beside the doublet, a depth threshold inside the sample's depths
SAMPLE_KW = dict(C.OPEN, min_bq=30, md_threshold=24, min_trim=0.01, max_mismatch_count=3, mismatch_window_size=20)


def sample(seed=72, **kw):
    from tests.test_gpu_germline import _sample
    return _sample(seed, 260_000, **kw).batch


@functools.lru_cache(maxsize=None)
def sample_model():
    """(batch, keyword parameters with the two site sets, records, log, dropped) of the 260 kb sample at sub_rate 5e-3.
    The site sets are taken from a first run without any: a half of every seventh PASS record each."""
    b = sample(sub_rate=5e-3)
    first, _ = M.run(b, [(1, b.length)], **SAMPLE_KW)
    ok = [r for r in first if M.STATUS[int(r["status"])] == "PASS"]
    key = lambda r, j: (int(r["tpos"] + j) << 4) | (M.BASES.index(chr(r["ref"][j])) << 2) | M.BASES.index(chr(r["alt"][j]))  # noqa: E731
    kw = dict(SAMPLE_KW, pon_keys=sorted(key(r, 0) for r in ok[0::7]), com_keys=sorted(key(r, 1) for r in ok[3::7]))
    dropped = []
    recs, log = M.run(b, [(1, b.length)], dropped=dropped, **kw)
    return b, kw, recs, log, dropped


def call_params(kw):
    return dict({k: v for k, v in kw.items() if k not in ("pon_keys", "com_keys")}, max_mismatch_count=1 << 20)


def assert_twins(recs, dropped, crecs):
    """Both single-base twins of every doublet record are among the call records with equal status, gq, genotype, state
    and counts; the germline half of a dropped doublet has none.  (Two candidates at one HetAltSite print one tuple:
    the call run keeps one record for them, whichever alt it names.)"""
    by_key, hetalt = {}, {}
    for r in crecs:
        by_key[int(r["tpos"]), chr(r["ref"]), chr(r["alt"])] = r
        if M.STATUS[int(r["status"])] == "HetAltSite":
            hetalt[int(r["tpos"])] = r
    for r in recs:
        for j in (0, 1):
            k = (int(r["tpos"]) + j, chr(r["ref"][j]), chr(r["alt"][j]))
            t = by_key.get(k)
            if t is None and M.STATUS[int(r["half_status"][j])] == "HetAltSite":
                t = hetalt.get(k[0])
            assert t is not None, k
            assert int(t["status"]) == int(r["half_status"][j]) and int(t["gq"]) == int(r["half_gq"][j]), (k, t, r)
            assert (int(t["gt0"]), int(t["gt1"]), int(t["gt_state"])) == (int(r["gt"][j][0]), int(r["gt"][j][1]), int(r["gt_state"][j]))
            assert np.array_equal(t["counts"], r["counts"][j]), (k, t, r)
            if t is by_key.get(k):
                assert int(t["bqsum"][M.BASES.index(k[2])]) == int(r["alt_bqsum"][j])
        assert int(r["gq"]) == min(int(x) for x in r["half_gq"])
    for tpos, refs, alts, hv in dropped:
        assert M.GERM in hv
        for j in (0, 1):
            if hv[j] == M.GERM:
                assert (tpos + j, refs[j], alts[j]) not in by_key


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rule(case):
    _name, b, regions, kw, expect = case
    recs, log = M.run(b, regions, **kw)
    expect(recs, log)
    assert log[18:] == [0, 0] and sum(log[7:18]) == len(recs) == log[5] - log[6]
    assert list(recs["tpos"]) == sorted(recs["tpos"])


def test_synthetic_sample_against_the_call_oracle():
    """The 260 kb sample at sub_rate 5e-3 holds 1583 doublet runs and 255 longer ones.  The floors are conditions on the
    input (enough records of enough kinds for the comparison to mean something), not measurements."""
    b, kw, recs, log, dropped = sample_model()
    assert log[1] == 1583 and log[2] == 255
    verdicts = {int(s) for s in recs["status"]}
    print("dbs sample:", len(recs), log, sorted(M.STATUS[v] for v in verdicts))
    assert len(recs) >= 200 and log[17] >= 20 and log[6] >= 5 and len(verdicts) >= 5
    assert len(dropped) == log[6] and log[3] > 0 and log[4] > 0
    crecs, _ = O.call(b, [(0, b.length)], call_params(kw), pon_keys=np.array(kw["pon_keys"], np.uint64),
                      com_keys=np.array(kw["com_keys"], np.uint64))
    assert_twins(recs, dropped, crecs)
    # keys in record order, each once
    keys = [(int(r["tpos"]), M.BASES.index(chr(r["alt"][0])), M.BASES.index(chr(r["alt"][1]))) for r in recs]
    assert keys == sorted(set(keys))


def test_default_rate_sample_has_germline_doublets():
    """Seed 71 at the generator's default rates: 19 doublet runs at 11 sites, adjacent germline SNPs among them."""
    b = sample(71)
    dropped = []
    recs, log = M.run(b, [(1, b.length)], dropped=dropped, **SAMPLE_KW)
    assert log[1] == 19 and log[5] == 11 and log[6] >= 5 and log[6] + len(recs) == 11
    crecs, _ = O.call(b, [(0, b.length)], call_params(SAMPLE_KW))
    assert_twins(recs, dropped, crecs)


def test_regions_never_shape_a_pile():
    """The records of any region list are the one-region records at the positions the list holds."""
    b, kw, recs, _log, _d = sample_model()
    rs = np.random.RandomState(5)
    cuts = rs.randint(1, b.length, 10)
    regions = [(int(min(x, y)), int(max(x, y))) for x, y in zip(cuts[0::2], cuts[1::2])]
    part, plog = M.run(b, regions, **kw)
    inside = np.array([any(s <= int(t) <= e for s, e in regions) for t in recs["tpos"]])
    assert 0 < len(part) < len(recs) and part.tobytes() == recs[inside].tobytes() and plog[:5] == _log[:5]


def test_record_dtype_and_writers():
    """The model's dtype is the binding's; vcflib.dbs_lines writes the model's lines; the log table has a row per counter."""
    from himut_amd import _ffi, vcflib
    assert M.DBS_RECORD_DTYPE == _ffi.DBS_RECORD_DTYPE and _ffi.DBS_RECORD_DTYPE.itemsize == 112 and 112 % 16 == 0
    _b, _kw, recs, log, _d = sample_model()
    lines = M.vcf_lines("chrS", recs)
    assert lines == vcflib.dbs_lines("chrS", recs) and len(lines) == len(recs)
    f = lines[0].rstrip("\n").split("\t")
    assert len(f) == 10 and len(f[3]) == 2 and len(f[4]) == 2 and f[8] == "GT:GQ:BQ:DP:AD:VAF" and f[6] in M.STATUS
    assert vcflib.DBS_LOG_ROWS == M.LOG_ROWS and len(M.LOG_ROWS) == 20 == len(log)


def test_header_is_calls_with_the_dbs_command():
    from himut_amd import vcflib
    args = ("in.bam", None, None, {"chr1": 1000}, None, None, 30, 60, 0, 100, 0.99, 20, 93, 0.01, 0, 20, 50, 3, 1, 1e-3, 1, "v", "o.vcf", "S")
    h = vcflib.get_dbs_vcf_header(*args).split("\n")
    c = vcflib.get_himut_vcf_header("in.bam", None, None, None, None, {"chr1": 1000}, None, None, 30, 60, 0, 100, 0.99, 20, 93, 0.01, 0,
                                    20, 50, 3, 1, 0, 1, 0, 1e-3, 0, False, False, False, False, "v", "o.vcf", "S").split("\n")
    assert len(h) == len(c)
    diff = [(a, b) for a, b in zip(h, c) if a != b]
    assert len(diff) == 1 and diff[0][0].startswith("##himut_command=himut dbs -i in.bam ") and diff[0][1].startswith("##himut_command=himut call ")


def test_cli_parser():
    from himut_amd.parse_args import parse_args
    _p, o = parse_args("v", ["dbs", "-i", "a.bam", "-o", "o.vcf"])
    assert (o.sub, o.bam, o.output, o.devices, o.cs_from_ref, o.ref) == ("dbs", "a.bam", "o.vcf", "0", False, None)
    assert (o.min_qv, o.min_mapq, o.min_sequence_identity, o.min_gq, o.min_bq, o.min_trim, o.max_mismatch_count,
            o.mismatch_window_size, o.min_ref_count, o.min_alt_count, o.germline_snv_prior) == (30, 60, 0.99, 20, 93, 0.01, 0, 20, 3, 1, 1e-3)
    assert not hasattr(o, "phase") and o.region is None and o.region_list is None and o.common_snps is None
    _p, o = parse_args("v", ["dbs", "-i", "a.bam", "-o", "o.vcf", "--devices", "0,1", "--region", "chr2", "--ref", "r.fa", "--cs_from_ref",
                             "--max_mismatch_count", "2", "--panel_of_normals", "p.vcf", "--common_snps", "c.vcf"])
    assert (o.devices, o.region, o.ref, o.cs_from_ref, o.max_mismatch_count, o.panel_of_normals, o.common_snps) == \
        ("0,1", "chr2", "r.fa", True, 2, "p.vcf", "c.vcf")
    with pytest.raises(SystemExit):
        parse_args("v", ["dbs", "-i", "a.bam", "-o", "o.vcf", "--phase"])
    with pytest.raises(SystemExit):
        parse_args("v", ["dbs", "-i", "a.bam", "-o", "o.vcf", "--cs_from_ref"])


def test_library_exports_the_dbs_run():
    import ctypes
    from himut_amd import _ffi, build
    lib = ctypes.CDLL(build.build_hip())
    assert hasattr(lib, "himut_run_dbs") and hasattr(lib, "himut_get_dbs")
    assert "himut_run_dbs" in _ffi.EXPORTS and "himut_get_dbs" in _ffi.EXPORTS
    lib.himut_run_dbs.restype = ctypes.c_int
    lib.himut_run_dbs.argtypes = [ctypes.c_void_p]
    assert lib.himut_run_dbs(None) != 0


# ---------------------------------------------------------------------------------------------- fp64 rounding boundaries
# kinds whose vectors hold a non-reference allele (the "order" vectors are pure-reference columns)
DBS_KINDS = tuple(k for k in EDGE_KINDS if k != "order")


@functools.lru_cache(maxsize=None)
def edge_doublets():
    """(vector index, alt, half, straddle) of every boundary candidate: each distinct non-reference allele of each
    vector as the doublet's allele, the vector as the first half and as the second; every fourth pair straddles two
    256-position blocks of the column index."""
    out = []
    for i, v in enumerate(edge_vectors()):
        for alt in G.alts_of(v):
            for half in (0, 1):
                out.append((i, alt, half, len(out) % 4 == 0))
    return out


def doublets_of(kind, half):
    return [d for d in edge_doublets() if edge_vectors()[d[0]]["kind"] == kind and d[2] == half]


@functools.lru_cache(maxsize=None)
def edge_doublet_model(i, alt, half, straddle):
    """(vector, pile, parameters, prior, records, log) of one boundary candidate in its own pile at its own prior with
    min_gq = k; computed once and left unchanged."""
    v = edge_vectors()[i]
    P = G.build_dbs([v], [alt], [half], orders=[G.ORDERS[i % 3]], straddle=[straddle])
    kw = G.dbs_params(v["k"], len(v["alleles"]))
    recs, log = M.run(P.batch, P.regions, prior=v["prior"], **kw)
    return v, P, kw, v["prior"], recs, log


@functools.lru_cache(maxsize=None)
def leaf_doublet_model():
    """The leaf vectors that hold a non-reference allele in one contig, one pair per 256 positions, halves alternating,
    the first non-reference allele of each as the doublet's: (vectors, pile, parameters, prior, records, log)."""
    vs = [v for v in leaf_vectors() if G.alts_of(v)]
    P = G.build_dbs(vs, [G.alts_of(v)[0] for v in vs], [i % 2 for i in range(len(vs))])
    kw = G.dbs_params(LEAF_K, max(len(v["alleles"]) for v in vs))
    recs, log = M.run(P.batch, P.regions, prior=LEAF_PRIOR, **kw)
    return vs, P, kw, LEAF_PRIOR, recs, log


def check_halves(recs, vs, P, min_gq):
    """Records (the model's or the device's) against the fixture: a record lies at a vector's pair only, once; the
    vector's half has the fixture's gt, gq and state, LowGQ exactly when a homref half's gq is below min_gq (each
    vector's own k if min_gq is None), and the companion half is a homref column at or above it.  Returns the vectors'
    half verdicts by kind."""
    at = {tpos: (v, half) for v, (tpos, half) in zip(vs, P.doublets)}
    assert len(at) == len(vs)
    seen = collections.defaultdict(list)
    for r in recs:
        v, h = at.pop(int(r["tpos"]))
        k = v["k"] if min_gq is None else min_gq
        got = ("".join(chr(x) for x in r["gt"][h]), int(r["half_gq"][h]), M.STATES[int(r["gt_state"][h])])
        assert got == (v["gt"], v["gq"], v["state"]), "{} as half {} at {}: (gt, gq, state) {} for {}".format(
            v["id"], h, int(r["tpos"]), got, (v["gt"], v["gq"], v["state"]))
        assert int(r["half_gq"][1 - h]) >= k and M.STATES[int(r["gt_state"][1 - h])] == "homref", v["id"]
        status = M.STATUS[int(r["half_status"][h])]
        if v["state"] == "homref":
            assert (status == "LowGQ") == (v["gq"] < k), "{} as half {}: status {} at gq {}, min_gq {}".format(
                v["id"], h, status, v["gq"], k)
        seen[v["kind"] if "kind" in v else "leaf"].append(status)
    return seen


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("kind", DBS_KINDS)
def test_gt_edges_doublets(kind, half):
    """Every (vector, alt) of the kind as that half: one candidate each, dropped as germline or a record whose half is
    the fixture's."""
    cands = doublets_of(kind, half)
    n_rec = 0
    for d in cands:
        v, P, _kw, _prior, recs, log = edge_doublet_model(*d)
        assert log[5] == 1 and log[6] + len(recs) == 1 and log[1] == 1, v["id"]
        check_halves(recs, [v], P, None)
        n_rec += len(recs)
    assert n_rec > 0


def test_gt_edges_doublet_counts():
    """452 candidates over the 136 vectors that hold a non-reference allele: 72 germline, 380 records, of every kind;
    the halves' verdicts cover the genotype's part of the cascade."""
    assert len({d[0] for d in edge_doublets()}) == 136 and sum(d[3] for d in edge_doublets()) == 113
    n_cand = n_germ = n_rec = 0
    kinds, verdicts = collections.Counter(), set()
    for d in edge_doublets():
        v, P, _kw, _prior, recs, log = edge_doublet_model(*d)
        n_cand, n_germ, n_rec = n_cand + log[5], n_germ + log[6], n_rec + len(recs)
        for r in recs:
            kinds[v["kind"]] += 1
            verdicts.add(M.STATUS[int(r["half_status"][P.doublets[0][1]])])
            assert (int(r["tpos"]) - 1) // 256 != int(r["tpos"]) // 256 if d[3] else True
    assert (n_cand, n_germ, n_rec) == (452, 72, 380)
    assert set(kinds) == set(DBS_KINDS) and 4 * n_rec >= 3 * n_cand
    assert verdicts == {"PASS", "LowGQ", "LowDepth", "HetSite", "HomAltSite"}


def test_leaf_vectors_doublets():
    """The 348 leaf columns with a non-reference allele in one contig: more than 256 candidates (two workgroups of
    k_dbs_eval), 209 germline, 139 records equal to the fixture, every second pair across a 256-position block."""
    vs, P, _kw, _prior, recs, log = leaf_doublet_model()
    assert P.spacing == 256 and (len(vs), log[5], log[6], len(recs)) == (348, 348, 209, 139) and log[5] > 256
    check_halves(recs, vs, P, LEAF_K)
    across = [(int(t) - 1) // 256 != int(t) // 256 for t in recs["tpos"]]
    assert any(across) and not all(across)
    assert [(t - 1) // 256 != t // 256 for t, _h in P.doublets] == [i % 2 == 1 for i in range(len(vs))]


def test_perturbed_sums_move_the_half():
    """The GPU test bites: a kernel that sums in reverse, in partial sums, with the prior first or in another base order
    changes (gt, state, gq, gq >= k) of 130 of the 136 columns."""
    moved = collections.Counter()
    for i in sorted({d[0] for d in edge_doublets()}):
        v = edge_vectors()[i]
        for how in G.PERTURBATIONS:
            w = perturbed(v, how)
            if (w["gt"], w["state"], w["gq"], w["gq"] >= v["k"]) != (v["gt"], v["state"], v["gq"], v["gq"] >= v["k"]):
                moved[v["kind"]] += 1
                break
    assert sum(moved.values()) == 130, moved
    for kind in ("gq_int", "cap99", "state", "qual"):
        assert moved[kind] > 0
