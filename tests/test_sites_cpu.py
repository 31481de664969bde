"""The sites contract in plain Python (tests/sites_model.py) against what each of its rules says on hand-built alignments
(tests/sites_cases.py) and, on a synthetic sample, against the restated worker of `call` (oracle.call): every call record
is the site record of its (tpos, ref, alt), and what `call` dropped as germline comes out Germline.  Then the host side of
`himut sites`: the TSV lines, the --unseen selection, the argument parser.  No GPU here; tests/test_gpu_sites.py compares
the run with this model."""
import functools
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import dbs_cases as C
from tests import dbs_model as D
from tests import sites_cases as S
from tests import sites_model as M

CASES = S.cases()
SAMPLE_KW = dict(C.OPEN, min_bq=30, md_threshold=24, min_mapq=20)


def sample(seed=91, length=200_000, **kw):
    from tests.test_gpu_germline import _sample
    return _sample(seed, length, **dict(dict(sub_rate=1e-3), **kw)).batch


def read_substitutions(b, passing=None):
    """The distinct (tpos, ref, alt) the non-secondary reads carry (cs2subindel's list: no N reference bases); passing:
    of the reads that pass call's read filters under these parameters only."""
    out = set()
    for i in range(b.n):
        if not int(b.flag[i]) & 0x100:
            info = D.ReadInfo(b, i)
            if passing is None or info.passes(passing):
                out.update((e[0], e[2], e[3]) for e in info.mismatch if e[1])
    return out


def key_of(s):
    return (s[0] << 4) | (M.BASES.index(s[1]) << 2) | M.BASES.index(s[2])


@functools.lru_cache(maxsize=None)
def sample_model():
    """(batch, sites, keyword parameters with the two site sets, records, log) of the 200 kb sample: the sites are the
    substitutions its reads carry plus as many random triples without any; the site sets hold every seventh PASS site."""
    b = sample()
    real = read_substitutions(b)
    rs, decoys = random.Random(4), set()
    while len(decoys) < len(real) // 2:
        p, r, a = rs.randrange(1, b.length + 300), rs.choice("ATGC"), rs.choice("ATGC")
        if r != a and (p, r, a) not in real:
            decoys.add((p, r, a))
    sites = sorted(real | decoys)
    first, _ = M.run(b, sites, **SAMPLE_KW)
    ok = [sites[int(r["site"])] for r in first if M.STATUS[int(r["status"])] == "PASS"]
    kw = dict(SAMPLE_KW, pon_keys=sorted(key_of(s) for s in ok[0::7]), com_keys=sorted(key_of(s) for s in ok[3::7]))
    recs, log = M.run(b, sites, **kw)
    return b, sites, kw, recs, log


def call_params(kw):
    return dict({k: v for k, v in kw.items() if k not in ("pon_keys", "com_keys")}, max_mismatch_count=1 << 20)


def assert_twins(sites, recs, crecs, carried):
    """Every call record is the site record of its (tpos, ref, alt) in status, gq, genotype, state, counts and the alt
    allele's quality sum; a substitution some proposing read carries that has no call record is Germline, or the second candidate
    of a HetAltSite (the call run keeps one record for the two).  Returns the number of Germline sites seen."""
    at = {s: r for s, r in zip(sites, recs)}
    have, hetalt = set(), set()
    for t in crecs:
        k = (int(t["tpos"]), chr(t["ref"]), chr(t["alt"]))
        r = at[k]
        have.add(k)
        if O.STATUS[int(t["status"])] == "HetAltSite":
            hetalt.add(k[0])
        assert M.STATUS[int(r["status"])] == O.STATUS[int(t["status"])] and int(r["gq"]) == int(t["gq"]), (k, t, r)
        assert (int(t["gt0"]), int(t["gt1"]), int(t["gt_state"])) == (int(r["gt"][0]), int(r["gt"][1]), int(r["gt_state"])), (k, t, r)
        assert np.array_equal(t["counts"], r["counts"]) and M.depth_of(r) == M.depth_of(t), (k, t, r)
        assert int(t["bqsum"][M.BASES.index(k[2])]) == int(r["alt_bqsum"]) and int(t["bqsum"][M.BASES.index(k[1])]) == int(r["ref_bqsum"])
    n_germ = 0
    for k in carried:
        if k in have or k not in at:
            continue
        st = M.STATUS[int(at[k]["status"])]
        assert st == "Germline" or (st == "HetAltSite" and k[0] in hetalt), (k, at[k])
        n_germ += st == "Germline"
    return n_germ


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rule(case):
    _name, b, sites, kw, expect = case
    recs, log = M.run(b, sites, **kw)
    if expect:
        expect(recs, log)
    assert len(recs) == len(sites) == log[0] == sum(log[1:14]) and log[16:] == [0] * 4
    assert [int(x) for x in recs["site"]] == list(range(len(sites))) and [int(x) for x in recs["tpos"]] == [s[0] for s in sites]
    assert log[15] == len({s[0] for s in sites if s[0] - 1 < M.span_of(b)})
    for r in recs:
        if M.STATUS[int(r["status"])] == "NoCoverage":
            assert M.depth_of(r) == 0 and (int(r["gq"]), int(r["gt_state"]), list(r["gt"])) == (0, 0, [0, 0])
        else:
            assert M.depth_of(r) > 0 and chr(r["gt"][0]) in M.BASES
        assert int(r["alt_hi"]) <= int(r["counts"][M.BASES.index(chr(r["alt"]))]) >= int(r["alt_mq"])


def test_every_status_has_a_case():
    seen = set()
    for _name, b, sites, kw, _e in S.status_cases():
        seen.update(S.statuses(M.run(b, sites, **kw)[0]))
    assert seen == set(M.STATUS) - {"Unphased"}


def test_synthetic_sample_against_the_call_oracle():
    """The floors are conditions on the input (enough records of enough kinds for the comparison to mean something), not
    measurements."""
    b, sites, kw, recs, log = sample_model()
    carried, proposed = read_substitutions(b), read_substitutions(b, dict(D.DEFAULTS, **call_params(kw)))
    crecs, _ = O.call(b, [(0, b.length)], call_params(kw), pon_keys=np.array(kw["pon_keys"], np.uint64),
                      com_keys=np.array(kw["com_keys"], np.uint64))
    n_germ = assert_twins(sites, recs, crecs, proposed)
    kinds = {M.STATUS[int(s)] for s in recs["status"]}
    print("sites sample:", len(sites), len(crecs), n_germ, log, sorted(kinds))
    assert len(sites) >= 2000 and len(crecs) >= 1000 and 20 <= n_germ <= log[2]
    assert {"PASS", "LowBQ", "NoCoverage", "Germline", "PanelOfNormal", "ComSnp", "HetSite", "IndelSite"} <= kinds
    # (a decoy names a random reference base: where its alt is the true base every read is an alt read)
    assert log[0] == len(sites) and log[14] >= len(carried) and carried <= set(sites) and log[15] <= len({s[0] for s in sites})


def test_record_dtype_and_log_rows():
    from himut_amd import _ffi, sites
    assert M.SITE_RECORD_DTYPE == _ffi.SITE_RECORD_DTYPE and _ffi.SITE_RECORD_DTYPE.itemsize == 64
    assert _ffi.SITE_STATUS_NAMES == M.STATUS and _ffi.STATUS_NAMES == O.STATUS
    assert sites.LOG_ROWS == M.LOG_ROWS and len(M.LOG_ROWS) == 20


VCF = """##fileformat=VCFv4.2
##contig=<ID=chrD,length=4000>
##contig=<ID=chrX,length=100>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS
chrD\t{p0}\t.\t{r0}\t{a0}\t.\tPASS\t.\tGT\t./.
chrD\t{p1}\t.\t{r1}\t{a1},{b1}\t.\tHetAltSite\t.\tGT\t./.
chrD\t{p2}\t.\t{r2}\t{a2}\t.\tLowBQ\t.\tGT\t./.
chrD\t{p3}\t.\t{r3}\t{a3}\t.\tPASS\t.\tGT\t./.
chrD\t{p4}\t.\t{r4}\t{a4}\t.\tPASS\t.\tGT\t./.
chrD\t700\t.\tAC\tA\t.\tPASS\t.\tGT\t./.
chrX\t5\t.\tA\tC\t.\tPASS\t.\tGT\t./.
"""


def hand_vcf(tmp_path):
    """A pile of twelve reads over 0-based 500 .. 520, read 0 with A1 at 500 and A2 at 510: line 0 is seen here, line 1
    (HetAlt, two sites) has one alt seen, lines 2 and 3 are unseen (line 2 is no PASS line), line 4 is not covered."""
    reads = S.stack(510, 12, {0: {500: C.A1[500], 510: C.A2[510]}})
    pos = (500, 510, 505, 515, 2000)
    f = {}
    for k, p in enumerate(pos):
        f["p{}".format(k)], f["r{}".format(k)], f["a{}".format(k)] = p + 1, C.REF[p], C.A1[p]
    f["b1"] = C.A2[510]
    path = tmp_path / "calls.vcf"
    path.write_text(VCF.format(**f))
    return C.batch(reads), str(path), pos


@pytest.mark.parametrize("all_filters", (False, True))
def test_load_sites_to_tsv_and_unseen(tmp_path, all_filters):
    from himut_amd import sites, support
    b, vcf, pos = hand_vcf(tmp_path)
    chrom2sites, skipped = support.load_sites(vcf, all_filters)
    assert skipped == 1 and set(chrom2sites) == {"chrD", "chrX"}
    lst = chrom2sites["chrD"]
    assert [s[0] - 1 for s in lst] == ([500, 505, 510, 510, 515, 2000] if all_filters else [500, 515, 2000])
    recs, _log = M.run(b, lst, **S.KW)
    lines = sites.format_rows("chrD", lst, recs)
    head = lines[0].split("\t")
    assert len(head) == len(sites.COLUMNS) == 21 and len(lines) == len(lst)
    # the seen PASS site: one alt read of quality 93 in twelve
    assert head == ["chrD", "501", C.REF[500], C.A1[500], "PASS", "PASS", C.REF[500] * 2, head[7], "12", "11", "1"] + \
        [str(int(x)) for x in recs[0]["counts"]] + ["93.0", "1", "1", "0.08"]
    last = lines[-1].split("\t")
    assert last[4:11] == ["PASS", "NoCoverage", ".", "0", "0", "0", "0"] and last[17:] == [".", "0", "0", "."]
    unseen = sites.unseen_sites(lst, recs, 10)
    assert unseen == ({(506, C.REF[505], C.A1[505]), (511, C.REF[510], C.A1[510]), (516, C.REF[515], C.A1[515])} if all_filters
                      else {(516, C.REF[515], C.A1[515])})
    assert sites.unseen_sites(lst, recs, 13) == set()
    out, missing = sites.select_unseen(vcf, all_filters, {"chrD": unseen}, {"chrD"}, "himut sites -i n.bam")
    data = [l for l in out if not l.startswith("#")]
    assert missing == 1 and out[:2] == VCF.splitlines(True)[:2] and out[3] == "##himut_sites_command=himut sites -i n.bam\n"
    assert out[4].startswith("#CHROM") and len([l for l in out if l.startswith("#")]) == 5
    # the HetAlt line needs both of its sites unseen: the A2 read keeps it out; the non-PASS line comes with --all_filters
    assert [int(l.split("\t")[1]) - 1 for l in data] == ([505, 515] if all_filters else [515])
    assert all(l in open(vcf).read().splitlines(True) for l in data)


def test_cli_parser():
    from himut_amd.parse_args import parse_args
    _p, o = parse_args("v", ["sites", "-i", "n.bam", "--sbs", "calls.vcf", "-o", "s.tsv"])
    assert (o.sub, o.bam, o.sbs, o.output, o.devices, o.cs_from_ref, o.ref, o.all_filters, o.unseen, o.min_depth) == \
        ("sites", "n.bam", "calls.vcf", "s.tsv", "0", False, None, False, None, 10)
    assert (o.min_gq, o.min_bq, o.min_mapq, o.min_ref_count, o.min_alt_count, o.germline_snv_prior) == (20, 93, 60, 3, 1, 1e-3)
    assert o.region is None and o.region_list is None and o.common_snps is None and o.panel_of_normals is None
    assert not hasattr(o, "phase") and not hasattr(o, "min_qv")
    _p, o = parse_args("v", ["sites", "-i", "n.bam", "--sbs", "c.vcf.bgz", "-o", "s.tsv", "--devices", "0,1", "--region", "chr2",
                             "--ref", "r.fa", "--cs_from_ref", "--all_filters", "--unseen", "u.vcf", "--min_depth", "15",
                             "--panel_of_normals", "p.vcf", "--common_snps", "c.vcf", "--min_bq", "30"])
    assert (o.devices, o.region, o.ref, o.cs_from_ref, o.all_filters, o.unseen, o.min_depth, o.panel_of_normals, o.common_snps,
            o.min_bq) == ("0,1", "chr2", "r.fa", True, True, "u.vcf", 15, "p.vcf", "c.vcf", 30)
    for bad in (["--phase"], ["--cs_from_ref"]):
        with pytest.raises(SystemExit):
            parse_args("v", ["sites", "-i", "n.bam", "--sbs", "c.vcf", "-o", "s.tsv"] + bad)
    with pytest.raises(SystemExit):
        parse_args("v", ["sites", "-i", "n.bam", "-o", "s.tsv"])


def test_library_exports_the_sites_run():
    import ctypes
    from himut_amd import _ffi, build
    lib = ctypes.CDLL(build.build_hip())
    assert hasattr(lib, "himut_run_sites") and hasattr(lib, "himut_get_sites")
    assert "himut_run_sites" in _ffi.EXPORTS and "himut_get_sites" in _ffi.EXPORTS
    lib.himut_run_sites.restype = ctypes.c_int
    lib.himut_run_sites.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64]
    assert lib.himut_run_sites(None, None, None, None, 0) != 0


# ---------------------------------------------------------------------------------------------- fp64 rounding boundaries
# The columns of tests/golden/leaf_gtlib.json and gt_edges.json as site columns (gt_piles.build): the site record carries
# the fixture's gt, gq and state, and a homref column is LowGQ exactly when its gq is below min_gq.

def vector_sites(vs, P):
    """One site per vector at its column: its first non-reference allele, or the base behind the reference base."""
    from tests import gt_piles as G
    out = []
    for v, c in zip(vs, P.cols):
        alts = G.alts_of(v)
        out.append((c[0] + 1, v["ref"], alts[0] if alts else M.BASES[(M.BASES.index(v["ref"]) + 1) % 4]))
    return out


@functools.lru_cache(maxsize=None)
def leaf_site_model():
    """The leaf vectors in one contig at prior 1e-3, min_gq 20: (vectors, pile, parameters, prior, sites, records, log)."""
    from tests import gt_piles as G
    from tests.test_callmap_cpu import LEAF_K, LEAF_PRIOR, leaf_vectors
    vs = list(leaf_vectors())
    P = G.build(vs)
    kw = G.dbs_params(LEAF_K, max(len(v["alleles"]) for v in vs))
    sites = vector_sites(vs, P)
    recs, log = M.run(P.batch, sites, prior=LEAF_PRIOR, **kw)
    return vs, P, kw, LEAF_PRIOR, sites, recs, log


@functools.lru_cache(maxsize=None)
def edge_site_model(i):
    """Boundary vector i in a pile of its own at its own prior with min_gq = its k; computed once and left unchanged."""
    from tests import gt_piles as G
    from tests.test_callmap_cpu import edge_vectors
    v = edge_vectors()[i]
    P = G.build([v], orders=[G.ORDERS[i % 3]])
    kw = G.dbs_params(v["k"], len(v["alleles"]))
    sites = vector_sites([v], P)
    recs, log = M.run(P.batch, sites, prior=v["prior"], **kw)
    return v, P, kw, v["prior"], sites, recs, log


def check_vectors(recs, vs, min_gq):
    """Site records (the model's or the device's) against the fixture.  Returns the statuses seen."""
    seen = set()
    assert len(recs) == len(vs)
    for r, v in zip(recs, vs):
        k = v["k"] if min_gq is None else min_gq
        status = M.STATUS[int(r["status"])]
        seen.add(status)
        if not v["alleles"]:
            assert status == "NoCoverage", v["id"]
            continue
        got = ("".join(chr(x) for x in r["gt"]), int(r["gq"]), M.STATES[int(r["gt_state"])])
        assert got == (v["gt"], v["gq"], v["state"]), "{}: (gt, gq, state) {} for {}".format(v["id"], got, (v["gt"], v["gq"], v["state"]))
        if v["state"] == "homref":
            assert (status == "LowGQ") == (v["gq"] < k), "{}: status {} at gq {}, min_gq {}".format(v["id"], status, v["gq"], k)
    return seen


def test_leaf_vectors_as_sites():
    vs, _P, _kw, _prior, sites, recs, log = leaf_site_model()
    from tests.test_callmap_cpu import LEAF_K
    seen = check_vectors(recs, vs, LEAF_K)
    assert len(sites) == 400 and log[0] == 400 and {"LowGQ", "Germline", "LowBQ"} <= seen, seen


def test_gt_edges_as_sites():
    from tests.test_callmap_cpu import edge_vectors
    seen, below, above = set(), 0, 0
    for i in range(len(edge_vectors())):
        v, _P, _kw, _prior, _sites, recs, _log = edge_site_model(i)
        seen |= check_vectors(recs, [v], None)
        if v["state"] == "homref":
            below, above = below + (v["gq"] < v["k"]), above + (v["gq"] >= v["k"])
    assert below > 5 and above > 5 and {"LowGQ", "Germline"} <= seen, (below, above, seen)
