"""The indels run's contract without a GPU: the plain-Python model (tests/indels_model.py) against what each rule says
on the hand-built alignments of tests/indels_cases.py, a property test of the left shift, the parser, the ABI table and the
VCF text.  The samples the GPU tests compare the run with are built (once) here."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import indels_cases as C
from tests import indels_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- samples shared with the GPU tests

def repeat_contig(rs, n):
    """A contig rich in repeats: homopolymers, di- and trinucleotide repeats, random stretches, lower case, the odd N."""
    parts, total = [], 0
    while total < n:
        k = rs.randint(0, 8)
        if k == 0:
            t = "ACGT"[rs.randint(4)] * rs.randint(3, 13)
        elif k == 1:
            t = "".join("ACGT"[x] for x in rs.randint(0, 4, 2)) * rs.randint(2, 8)
        elif k == 2:
            t = "".join("ACGT"[x] for x in rs.randint(0, 4, 3)) * rs.randint(2, 6)
        else:
            t = "".join("ACGT"[x] for x in rs.randint(0, 4, rs.randint(5, 40)))
        if rs.rand() < 0.1:
            t = t.lower()
        if rs.rand() < 0.03:
            t += "N" * rs.randint(1, 3)
        parts.append(t)
        total += len(t)
    return "".join(parts)[:n]


def _random_event(rs, ref, p):
    """An insertion (bases) or a deletion (length) for position p: short, often a copy of what follows (so that it shifts)."""
    L = int(rs.choice([1, 1, 1, 2, 2, 3, 4, 6, 9]))
    if rs.rand() < 0.5:
        return ("D", L)
    if rs.rand() < 0.6:
        s = ref[p:p + L].upper()
        if len(s) == L and all(b in "ACGT" for b in s):
            return ("I", s)
    s = "".join("ACGT"[x] for x in rs.randint(0, 4, L))
    if rs.rand() < 0.03:
        s = s[:-1] + "N"
    return ("I", s)


def random_round(seed):
    """(batch, regions, contig string, parameters) of one random round."""
    rs = np.random.RandomState(seed)
    n = int(rs.randint(700, 3000))
    ref = repeat_contig(rs, n)
    pool = {}
    for p in rs.randint(5, n - 20, 12):
        pool[int(p)] = _random_event(rs, ref, int(p))
    recs = []
    for _ in range(int(rs.randint(20, 201))):
        length = int(min(n - 1, rs.choice([100, 150, 300, 600, 1000, 2000])))
        start = int(rs.randint(0, n - length))
        end = start + length
        cand = {p: e for p, e in pool.items() if start <= p <= end and rs.rand() < 0.5}
        for p in rs.randint(start, end + 1, rs.poisson(length / 150.0)):
            cand.setdefault(int(p), _random_event(rs, ref, int(p)))
        ins, dels, free = {}, {}, start
        for p in sorted(cand):
            kind, v = cand[p]
            if p < free:
                continue
            if kind == "I":
                ins[p] = v
                if rs.rand() < 0.1 and p + 2 <= end:             # an insertion straight in front of a deletion
                    dels[p] = 2
                    free = p + 2
            elif p + v <= end:
                dels[p] = v
                free = p + v + (0 if rs.rand() < 0.1 else 1)     # now and then an event straight behind the deletion
        recs.append(C.read(ref, start, length, ins=ins, dels=dels, mapq=int(rs.choice([0, 10, 60, 60, 60])),
                           flag=int(rs.choice([0, 0, 0, 0, 16, 0x100, 0x800]))))
    cuts = sorted(int(x) for x in rs.randint(0, n, 4))
    regions = [(cuts[0], cuts[2]), (cuts[1], cuts[3])] if rs.rand() < 0.7 else [(0, n)]
    kw = dict(min_mapq=int(rs.choice([0, 20])), max_len=int(rs.choice([4, 50])), report_homref=bool(rs.rand() < 0.5),
              min_alt_count=int(rs.choice([1, 2])), min_gq=int(rs.choice([0, 20])))
    return C.batch(recs, n), regions, ref, kw


BOUNDARY_N, BOUNDARY_STEP = 60_000, 190


@functools.lru_cache(maxsize=None)
def boundary_sample():
    """A 60 kb contig with one locus for every (DP, n_alt), DP <= 24 and 1 <= n_alt <= DP: (batch, contig string, the
    model's alleles and counters (collect), the loci)."""
    loci = [(dp, na) for dp in range(1, 25) for na in range(1, dp + 1)]
    at = [200 + BOUNDARY_STEP * k for k in range(len(loci))]
    ref = C.contig(21, BOUNDARY_N, plant=[(p, "CAGTCA") for p in at])
    recs = []
    for p, (dp, na) in zip(at, loci):
        recs += C.cover(ref, dp, na, start=p - 50, length=110, dels={p + 3: 2})
    b = C.batch(recs, BOUNDARY_N)
    items, log = M.collect(b, [(0, BOUNDARY_N)], ref)
    assert [(it[3], it[1]) for it in items] == loci and [it[0][0] for it in items] == [p + 2 for p in at]
    return b, ref, items, log, loci


# ---- the model against what each rule says

@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_model_on_hand_built(case):
    _name, b, regions, ref, kw, expect = case
    recs, log = M.run(b, regions, ref, **kw)
    expect(recs, log)
    assert recs.dtype.itemsize == 64
    d = C.logd(log)
    assert d["alleles"] == d["homref"] + d["het"] + d["homalt"]
    assert d["het"] + d["homalt"] == d["PASS"] + d["LowGQ"] + d["LowDepth"] + d["HighDepth"]
    key = [(int(r["anchor"]), int(r["type"]), int(r["len"]), [M.BASES.index(x) for x in M.unpack_bases(r)]) for r in recs]
    assert key == sorted(key) and len(set(map(str, key))) == len(key)


def test_genotype_follows_the_stated_operations():
    lg = M.logs(0.01, 1e-4)
    for dp, na in ((12, 6), (12, 12), (12, 1), (24, 3), (1, 1)):
        state, gq, pls = M.genotype(dp - na, na, lg)
        want = []
        for prior, x, y in ((lg[3], lg[0], lg[1]), (lg[4], lg[2], lg[2]), (lg[5], lg[1], lg[0])):
            want.append(-10.0 * ((prior + (dp - na) * x) + na * y))
        assert pls == want
        assert state == min(range(3), key=lambda g: (want[g], g))
        assert gq == min(99, int(sorted(want)[1] - sorted(want)[0]))
    assert M.genotype(6, 6, lg)[0] == 1 and M.genotype(0, 12, lg)[0] == 2 and M.genotype(11, 1, lg)[0] == 0


def test_boundary_sample_covers_every_state():
    _b, _ref, items, log, loci = boundary_sample()
    recs, _ = M.evaluate(items, log, report_homref=True, min_gq=0)
    assert len(recs) == 300 and set(int(x) for x in recs["gt_state"]) == {0, 1, 2}
    assert len(set(int(x) for x in recs["gq"])) >= 20


# ---- the left shift

@pytest.mark.parametrize("seed", range(8))
def test_normalisation_keeps_the_change_and_is_leftmost(seed):
    """On random repeat-rich contigs: the shifted allele applied to the contig gives the string the raw one gives, and no
    further shift is possible except at the stated stops (the read's start, a byte outside ACGT; position 1 is the read's
    start at the contig's)."""
    rs = np.random.RandomState(100 + seed)
    ref = repeat_contig(rs, 1500)
    shifted = 0
    for _ in range(400):
        p = int(rs.randint(2, len(ref) - 12))
        kind, v = _random_event(rs, ref, p)
        ty, L, s = (M.DEL, v, "") if kind == "D" else (M.INS, len(v), v)
        if "N" in s:
            continue
        tstart = int(rs.choice([0, 0, max(0, p - int(rs.randint(1, 8)))]))
        if not tstart <= p - 1:
            continue
        q, t = M.normalise(ref, tstart, ty, p, L, s)
        assert tstart <= q - 1 and q <= p and len(t) == len(s)
        assert M.apply_allele(ref, ty, q, L, t) == M.apply_allele(ref, ty, p, L, s)
        shifted += q < p
        if q - 1 > tstart:                                       # not at the read's start: the next step must be refused
            c = M.ref_letter(ref, q - 1)
            if c is not None:
                assert c != (M.ref_letter(ref, q + L - 1) if ty == M.DEL else t[L - 1])
        q2, t2 = M.normalise(ref, tstart, ty, q, L, t)           # idempotent
        assert (q2, t2) == (q, t)
    assert shifted > 20


def test_random_rounds_build_and_hold_the_invariants():
    for seed in (0, 1, 2):
        b, regions, ref, kw = random_round(seed)
        assert 20 <= b.n <= 200
        recs, log = M.run(b, regions, ref, **kw)
        d = C.logd(log)
        assert d["events"] > 0 and all(int(r["n_alt"]) <= int(r["dp"]) for r in recs)
        assert all(any(s <= int(r["anchor"]) <= e for s, e in regions) for r in recs)


# ---- the parser, the ABI, the VCF text

def test_parser_defaults():
    from himut_amd.parse_args import parse_args
    _p, o = parse_args("x", ["indels", "-i", "in.bam", "--ref", "ref.fa", "-o", "out.vcf"])
    assert o.sub == "indels" and o.bam == "in.bam" and o.ref == "ref.fa" and o.output == "out.vcf"
    assert o.germline_indel_prior == 1 / (10 ** 4) and o.indel_error == 0.01 and o.max_indel_len == 50
    assert o.min_mapq == 0 and o.min_gq == 20 and o.min_ref_count == 2 and o.min_alt_count == 2
    assert o.cs_from_ref is False and o.region is None and o.region_list is None and o.devices == "0"
    with pytest.raises(SystemExit):
        parse_args("x", ["indels", "-i", "in.bam", "-o", "out.vcf"])                     # --ref is required
    with pytest.raises(SystemExit):
        parse_args("x", ["indels", "-i", "in.bam", "--ref", "r.fa", "-o", "o.vcf", "--max_indel_len", "65"])


def test_abi_declares_and_exports_the_two_entry_points():
    from himut_amd import _ffi, build
    text = open(os.path.join(ROOT, "include", "himut_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {name: params.count(",") + 1 for name, params in re.findall(r"^int\s+(himut_\w+)\(([^)]*)\);", text, flags=re.M)}
    lib = ctypes.CDLL(build.build_hip())
    for name in ("himut_run_indels", "himut_get_indels"):
        assert name in protos and hasattr(lib, name)
        restype, argtypes = _ffi._ABI[name]
        assert restype is ctypes.c_int and len(argtypes) == protos[name]
    assert _ffi.INDEL_RECORD_DTYPE == M.RECORD_DTYPE and _ffi.INDEL_RECORD_DTYPE.itemsize == 64
    assert ctypes.sizeof(_ffi.IndelParams) == 80
    assert tuple(_ffi.INDEL_LOG_NAMES) == M.LOG
    assert _ffi.indel_logs(0.01, 1e-4) == M.logs(0.01, 1e-4)
    lib.himut_run_indels.restype = ctypes.c_int
    lib.himut_run_indels.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.himut_run_indels(None, None) != 0


def test_vcf_text_of_a_hand_case():
    from himut_amd import vcflib
    name, b, regions, ref, kw, _e = [c for c in C.CASES if c[0] == "het_del"][0]
    recs, _ = M.run(b, regions, ref, **kw)
    gq = int(recs[0]["gq"])
    want = ["chrI\t1003\t.\tGTC\tG\t{0}\tPASS\t.\tGT:GQ:DP:AD:NO\t0/1:{0}:12:6,6:0\n".format(gq)]
    assert M.vcf_lines("chrI", recs, ref) == want == vcflib.indel_lines("chrI", recs, ref)
    name, b, regions, ref, kw, _e = [c for c in C.CASES if c[0] == "homalt_ins"][0]
    recs, _ = M.run(b, regions, ref, **kw)
    gq = int(recs[0]["gq"])
    want = ["chrI\t1003\t.\tG\tGTA\t{0}\tPASS\t.\tGT:GQ:DP:AD:NO\t1/1:{0}:12:0,12:0\n".format(gq)]
    assert M.vcf_lines("chrI", recs, ref) == want == vcflib.indel_lines("chrI", recs, ref)
    for c in C.CASES:                                            # every case: the package prints what the model prints
        recs, _ = M.run(c[1], c[2], c[3], **c[4])
        assert vcflib.indel_lines("chrI", recs, c[3]) == M.vcf_lines("chrI", recs, c[3])
    header = vcflib.get_indels_vcf_header("in.bam", None, None, {"chrI": 4000}, 0, 20, 2, 2, 100, 1e-4, 0.01, 50, 1, "v", "o.vcf",
                                          "sample", ref_file="ref.fa")
    assert "##fileformat=VCFv4.2" in header and "ID=NO," in header and "one line per allele" in header
    assert header.rstrip("\n").split("\n")[-1].startswith("#CHROM\tPOS")
