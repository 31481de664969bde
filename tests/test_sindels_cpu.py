"""The sindels run's contract without a GPU: the plain-Python model (tests/sindels_model.py) against what each rule says
on the hand-built alignments of tests/sindels_cases.py, the identities between the counters, the model's composition
under tests/chrom_islands.py (the premise of tests/test_gpu_sindels_coords.py), the parser, the ABI table and the VCF
text.  The samples the GPU tests compare the run with are built (once) here."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import chrom_islands as I
from tests import indels_model as M
from tests import sindels_cases as C
from tests import sindels_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model against what each rule says

@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_model_on_hand_built(case):
    _name, b, regions, ref, kw, expect = case
    kw, l_hit, l_err = C.table_of(kw)
    recs, log = S.run(b, regions, ref, l_hit, l_err, **kw)
    expect(recs, log)
    assert recs.dtype.itemsize == 64
    S.check_identities(log, len(recs))
    key = [(int(r["anchor"]), int(r["type"]), int(r["len"]), [M.BASES.index(x) for x in M.unpack_bases(r)]) for r in recs]
    assert key == sorted(key) and len(set(map(str, key))) == len(key)
    assert all(int(r["gt_state"]) == 0 and 1 <= int(r["n_prop"]) <= int(r["n_alt"]) <= int(r["dp"]) for r in recs)


def test_cases_cover_every_status_and_loss():
    seen, losses = set(), dict.fromkeys(("num_trim", "num_window", "num_lowbq", "num_germ_het", "num_germ_homalt"), 0)
    for _name, b, regions, ref, kw, _e in C.CASES:
        kw, l_hit, l_err = C.table_of(kw)
        recs, log = S.run(b, regions, ref, l_hit, l_err, **kw)
        seen |= set(int(x) for x in recs["status"])
        for k in losses:
            losses[k] += S.logd(log)[k]
    assert seen == set(S.FILTER_NAME) and all(losses.values()), (seen, losses)


# ---- seeded random rounds on synth reads (shared with the GPU test): the floors below hold for the model alone

ROUND_SEEDS = (401, 402, 403, 404)
ROUND_KW = dict(min_mapq=20, min_qv=20, min_bq=20, min_gq=20, min_ref_count=3, min_alt_count=1, max_run=2,
                min_sequence_identity=0.98, min_trim=0.01, mismatch_window_size=20, max_mismatch_count=0)
ROUND_FLOORS = dict(candidates=300, records=300)        # per round
# across the rounds: every loss and every status (synth plants no germline indels: the two germline drops are the hand-built
# cases' -- het among the islands too, whose rounds draw their events from a pool)
ROUND_NONZERO = ("num_trim", "num_window", "num_lowbq", "IndelSite", "Repeat", "LowGQ", "LowDepth", "HighDepth", "PASS")


@functools.lru_cache(maxsize=None)
def synth_round(seed):
    """(batch, regions, contig string, parameters, the model's records and counters) of one round: 30 kb, depth 8, indel
    rates around 2e-3; the depth threshold sits where some piles are above it."""
    from himut_amd import synth
    s = synth.generate(synth.SynthConfig(seed=seed, contig_len=30_000, depth=8.0, read_len_mean=6000, read_len_sd=1200,
                                         read_len_min=2000, read_len_max=12000, snp_rate=1e-3, sub_rate=2e-3, ins_rate=2e-3,
                                         del_rate=2e-3, name="chrS"), want_ref=True)
    b = s.batch
    ref = bytes(np.asarray(s.ref, np.uint8)).decode("ascii")
    regions = [(1, b.length)]
    kw = dict(ROUND_KW, md_threshold=10, min_gq=25 if seed % 2 else 20)
    recs, log = S.run(b, regions, ref, **kw)
    return b, regions, ref, kw, recs, log


def test_random_rounds_meet_their_floors():
    total = dict.fromkeys(S.LOG, 0)
    for seed in ROUND_SEEDS:
        _b, _regions, _ref, _kw, recs, log = synth_round(seed)
        d = S.logd(log)
        print(seed, len(recs), d)
        assert d["candidates"] >= ROUND_FLOORS["candidates"] and len(recs) >= ROUND_FLOORS["records"], (seed, d)
        for k in S.LOG:
            total[k] += d[k]
    assert all(total[k] > 0 for k in ROUND_NONZERO), total


# ---- composition under chrom_islands: the indels run's islands under this run's parameters

ISLAND_KW = dict(min_mapq=20, min_qv=30, min_bq=30, min_gq=0, min_ref_count=1, min_alt_count=1, max_run=3, max_len=50,
                 min_sequence_identity=0.9, min_trim=0.01, mismatch_window_size=5, max_mismatch_count=1)


def islands():
    from tests import test_chrom_islands_cpu as T
    return T.islands("indels")


@functools.lru_cache(maxsize=None)
def island_part(k, right, mode):
    """The model on island k alone inside its padding, under its own regions or the one region (0, padded length)."""
    b, regions, ref = I.isolated(islands()[k], I.PAD, right)
    return S.run(b, {"own": regions, "whole": [(0, b.length)]}[mode], I.letters(ref), **ISLAND_KW)


def want(offsets, last_at_end, whole=False, ks=None):
    ks = list(range(len(islands()))) if ks is None else list(ks)
    assert len(ks) == len(offsets)
    parts = [island_part(k, 0 if last_at_end and k == ks[-1] else I.PAD, "whole" if whole else "own") + (int(o) - I.PAD,)
             for k, o in zip(ks, offsets)]
    return I.expected(parts, "anchor")


@pytest.mark.parametrize("last_at_end", (False, True), ids=("padded_end", "last_at_end"))
def test_model_composes(last_at_end):
    from tests import test_chrom_islands_cpu as T
    n = len(islands())
    ks = list(range(n - 6, n) if last_at_end else range(0, n, 2))
    offsets, length = T.small_layout("indels", ks, last_at_end)
    b, regions, ref = I.compose([islands()[k] for k in ks], offsets, length)
    for whole in (False, True):
        got, glog = S.run(b, [(0, length)] if whole else regions, I.letters(ref), **ISLAND_KW)
        wanted, wlog = want(offsets, last_at_end, whole, ks)
        S.assert_same(got, glog, wanted, wlog)
        d = S.logd(glog)
        assert len(got) > 20 and d["proposing_events"] > 50 and d["num_germ_het"] > 0, d


# ---- the parser, the ABI, the VCF text

def test_parser_defaults():
    from himut_amd.parse_args import parse_args
    _p, o = parse_args("x", ["sindels", "-i", "in.bam", "--ref", "ref.fa", "-o", "out.vcf"])
    assert o.sub == "sindels" and o.bam == "in.bam" and o.ref == "ref.fa" and o.output == "out.vcf"
    _p, call = parse_args("x", ["call", "-i", "in.bam", "-o", "out.vcf"])
    for k in ("min_qv", "min_mapq", "min_sequence_identity", "min_gq", "min_bq", "min_ref_count", "min_alt_count", "min_trim",
              "max_mismatch_count", "mismatch_window_size", "germline_indel_prior"):
        assert getattr(o, k) == getattr(call, k), k
    assert o.indel_error == 0.01 and o.max_indel_len == 50 and o.max_run == 2 and o.error_table is None and o.min_spans == 1000
    assert o.cs_from_ref is False and o.region is None and o.region_list is None and o.devices == "0"
    with pytest.raises(SystemExit):
        parse_args("x", ["sindels", "-i", "in.bam", "-o", "out.vcf"])                    # --ref is required
    with pytest.raises(SystemExit):
        parse_args("x", ["sindels", "-i", "in.bam", "--ref", "r.fa", "-o", "o.vcf", "--max_indel_len", "65"])


def test_abi_declares_and_exports_the_entry_points():
    from himut_amd import _ffi, build
    text = open(os.path.join(ROOT, "include", "himut_hip.h")).read()
    assert re.search(r"HIMUT_ST_REPEAT\s*=\s*14", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {name: params.count(",") + 1 for name, params in re.findall(r"^int\s+(himut_\w+)\(([^)]*)\);", text, flags=re.M)}
    lib = ctypes.CDLL(build.build_hip())
    for name in ("himut_run_sindels", "himut_get_sindels", "himut_set_indel_error_table"):
        assert name in protos and hasattr(lib, name)
        restype, argtypes = _ffi._ABI[name]
        assert restype is ctypes.c_int and len(argtypes) == protos[name]
    assert _ffi.SINDEL_RECORD_DTYPE == S.RECORD_DTYPE and _ffi.SINDEL_RECORD_DTYPE.itemsize == 64
    for name in M.RECORD_DTYPE.names[:12]:                           # himut_indel_record's fields keep their offsets
        assert _ffi.SINDEL_RECORD_DTYPE.fields[name][1] == _ffi.INDEL_RECORD_DTYPE.fields[name][1], name
    assert _ffi.SINDEL_RECORD_DTYPE.fields["n_prop"][1] == _ffi.INDEL_RECORD_DTYPE.fields["reserved"][1]
    assert ctypes.sizeof(_ffi.SindelParams) == 120 and _ffi.ST_REPEAT == S.ST_REPEAT
    assert tuple(_ffi.SINDEL_LOG_NAMES) == S.LOG and _ffi.SINDEL_STATUS_NAMES == S.FILTER_NAME
    for f in (lib.himut_run_sindels, lib.himut_get_sindels):
        f.restype = ctypes.c_int
    lib.himut_run_sindels.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.himut_get_sindels.argtypes = [ctypes.c_void_p] * 4
    assert lib.himut_run_sindels(None, None) != 0 and lib.himut_get_sindels(None, None, None, None) != 0


def test_vcf_text_of_hand_cases():
    from himut_amd import vcflib
    case = {c[0]: c for c in C.CASES}
    _n, b, regions, ref, kw, _e = case["lone_del"]
    recs, _ = S.run(b, regions, ref, **kw)
    gq = int(recs[0]["gq"])
    assert vcflib.sindel_lines("chrI", recs, ref) == \
        ["chrI\t1003\t.\tGTC\tG\t{0}\tPASS\tRUN=T1;CLASS=other\tGT:GQ:DP:AD:NO:NP\t./.:{0}:12:11,1:0:1\n".format(gq)]
    _n, b, regions, ref, kw, _e = case["repeat_ins_run3"]
    recs, _ = S.run(b, regions, ref, **kw)
    gq = int(recs[0]["gq"])
    assert vcflib.sindel_lines("chrI", recs, ref) == \
        ["chrI\t1001\t.\tC\tCA\t{0}\tRepeat\tRUN=A3;CLASS=ins1\tGT:GQ:DP:AD:NO:NP\t./.:{0}:12:11,1:0:1\n".format(gq)]
    _n, b, regions, ref, kw, _e = case["repeat_run65"]
    recs, _ = S.run(b, regions, ref, **kw)
    assert "\tRepeat\tRUN=A65\t" in vcflib.sindel_lines("chrI", recs, ref)[0]
    header = vcflib.get_sindels_vcf_header("in.bam", None, None, {"chrI": 6000}, 30, 60, 100, 200, 0.99, 20, 93, 0.01, 0, 20, 50, 3,
                                           1, 1e-4, 0.01, 50, 2, 1, "v", "o.vcf", "sample", ref_file="ref.fa")
    for word in ("##FILTER=<ID=Repeat", "##FILTER=<ID=IndelSite", "##INFO=<ID=RUN", "##INFO=<ID=CLASS", "##FORMAT=<ID=NP",
                 "##candidates=not calls", "definitions chosen here", "himut sindels -i in.bam --ref ref.fa", "--max_run 2"):
        assert word in header, word
    assert len(vcflib.SINDEL_LOG_ROWS) == len(S.LOG) == 20
