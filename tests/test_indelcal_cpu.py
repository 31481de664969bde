"""The indelcal run's contract without a GPU: the plain-Python model (tests/indelcal_model.py) against what each rule says
on the hand-built alignments of tests/indelcal_cases.py, its invariants, the TSV writer, the loader and the table of
logs `indels --error_table` reads, the parser and the ABI table.  The random rounds the GPU tests compare the run with
are built here, and the seeds are chosen so that the model alone fills every column and every counter."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import indelcal_cases as C
from tests import indelcal_model as K
from tests import indels_model as M
from tests.indels_cases import batch, read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = tuple(range(40))


# ---- random rounds, shared with the GPU tests

def skewed_contig(rs, n):
    """A contig of runs: mostly one to four letters, now and then up to 30, rarely up to 70; lower case and the odd N."""
    parts, total, last = [], 0, ""
    while total < n:
        b = "ACGT"[rs.randint(4)]
        if b == last:
            continue
        x = rs.rand()
        k = int(rs.randint(1, 5)) if x < 0.80 else int(rs.randint(5, 31)) if x < 0.96 else int(rs.randint(31, 71))
        t = b * k
        if rs.rand() < 0.08:
            t = t.lower()
        if rs.rand() < 0.02:
            t += "N" * int(rs.randint(1, 3))
        parts.append(t)
        total += len(t)
        last = b
    return "".join(parts)[:n]


def _event_in_run(rs, ref, s, n):
    """An event somewhere in the run [s, s + n): mostly of the run's own letter, short."""
    p = int(s + rs.randint(0, n))
    b = ref[s].upper()
    x = rs.rand()
    if x < 0.45:
        return p, ("D", int(rs.choice([1, 1, 1, 2, 3, 5, n, n + 1])))
    if x < 0.85:
        return p, ("I", b * int(rs.choice([1, 1, 1, 2, 3, 4, 6])))
    s_ = "".join("ACGT"[k] for k in rs.randint(0, 4, int(rs.choice([1, 2, 3, 6]))))
    return p, ("I", s_[:-1] + "N" if rs.rand() < 0.1 else s_)


def random_round(seed):
    """(batch, regions, contig string, parameters) of one random round: event anchors are placed in runs, a pool of
    events is shared by many reads (variant anchors), every read adds a few of its own."""
    rs = np.random.RandomState(7000 + seed)
    n = int(rs.randint(600, 2600))
    ref = skewed_contig(rs, n)
    runs = sorted((s, k) for s, (k, _b) in K.runs_of(ref).items())
    pool = dict(_event_in_run(rs, ref, *runs[int(rs.randint(len(runs)))]) for _ in range(10))
    recs = []
    for _ in range(int(rs.randint(15, 121))):
        length = int(min(n - 1, rs.choice([60, 150, 300, 600, 1200])))
        start = int(rs.randint(0, n - length))
        end = start + length
        cand = {p: e for p, e in pool.items() if start <= p <= end and rs.rand() < 0.5}
        inside = [r for r in runs if start <= r[0] < end]
        for _k in range(int(rs.poisson(length / 120.0))):
            if inside:
                p, e = _event_in_run(rs, ref, *inside[int(rs.randint(len(inside)))])
                if start <= p <= end:
                    cand.setdefault(p, e)
        if rs.rand() < 0.05:
            cand[start] = ("I", "AC")                             # a leading insertion: no event
        ins, dels, free = {}, {}, start
        for p in sorted(cand):
            kind, v = cand[p]
            if p < free:
                continue
            if kind == "I":
                ins[p] = v
                if rs.rand() < 0.1 and p + 1 <= end:              # an insertion straight in front of a deletion
                    dels[p] = 1
                    free = p + 1
            elif p + v <= end:
                dels[p] = v
                free = p + v + 1
        recs.append(read(ref, start, length, ins=ins, dels=dels, mapq=int(rs.choice([0, 10, 60, 60, 60])),
                         flag=int(rs.choice([0, 0, 0, 0, 16, 0x100, 0x800]))))
    cuts = sorted(int(x) for x in rs.randint(0, n, 4))
    regions = [(cuts[0], cuts[2]), (cuts[1], cuts[3])] if rs.rand() < 0.6 else [(0, n)]
    kw = dict(min_mapq=int(rs.choice([0, 20])), max_len=int(rs.choice([4, 50])), min_alt_count=int(rs.choice([1, 2, 3])),
              vaf_permille=int(rs.choice([100, 250, 500])))
    return batch(recs, n), regions, ref, kw


# ---- the model against what each rule says

@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_model_on_hand_built(case):
    _name, b, regions, ref, kw, expect = case
    table, log = K.run(b, regions, ref, **kw)
    expect(table, log)
    K.check_invariants(table, log)


def test_random_rounds_cover_every_column_and_counter():
    """A condition on the seeds: over all rounds every table column and every counter is non-zero at least once, some
    round has an excluded run, runs of every length bin up to 70 occur."""
    cols, logs = np.zeros(len(K.COLUMNS), np.int64), np.zeros(len(K.LOG), np.int64)
    longest = 0
    for seed in SEEDS:
        b, regions, ref, kw = random_round(seed)
        assert 15 <= b.n <= 120
        table, log = K.run(b, regions, ref, **kw)
        K.check_invariants(table, log)
        cols += (table.sum(axis=0) > 0)
        logs += (np.array(log) > 0)
        longest = max(longest, max(k for k, _b in K.runs_of(ref).values()))
    assert (cols > 0).all(), dict(zip(K.COLUMNS, cols))
    assert (logs > 0).all(), dict(zip(K.LOG, logs))
    assert cols[K.col("excluded")] >= 1 and longest > K.MAX_RUN


def test_runs_of_and_classes():
    runs = K.runs_of("AAcgGGtNTTa")
    assert runs == {2: (1, "C"), 3: (3, "G"), 6: (1, "T"), 8: (2, "T")}          # AA has nothing in front, the last a nothing behind
    assert K.run_class("A", 1) == 0 and K.run_class("T", 1) == 32 and K.run_class("C", 31) == 126
    assert K.run_class("C", 32) == K.run_class("C", 64) == 127


# ---- the TSV, the loader, the logs

def _some_table():
    table = np.zeros((128, 10), np.int64)
    table[K.run_class("A", 3)] = [50, 2, 4000, 3, 1, 0, 2, 0, 0, 1]
    table[K.run_class("T", 40)] = [7, 1, 1000, 400, 90, 30, 250, 10, 2, 5]
    table[K.run_class("G", 9)] = [3, 0, 999, 5, 0, 0, 0, 0, 0, 0]
    return table


def test_tsv_writer_and_loader_round_trip(tmp_path):
    from himut_amd import indelcal
    table = _some_table()
    lines = indelcal.table_lines(table)
    assert lines == K.table_lines(table) and len(lines) == 129
    assert lines[0] == "base\trun\truns\texcluded\tspans\tdel1\tdel2\tdel3p\tins1\tins2\tins3p\tother\tdel_rate\tins_rate\n"
    assert lines[1 + 2] == "A\t3\t50\t2\t4000\t3\t1\t0\t2\t0\t0\t1\t0.001\t0.0005\n"
    assert lines[1] == "A\t1" + "\t0" * 10 + "\tNA\tNA\n"
    assert lines[1 + 32 + 31].startswith("T\t32+\t7\t1\t1000\t") and lines[1 + 32 + 31].endswith("\t{}\t{}\n".format(repr(520 / 1000), repr(262 / 1000)))
    path = tmp_path / "t.tsv"
    path.write_text("".join(lines))
    assert np.array_equal(indelcal.load_table(str(path)), table)
    path.write_text("".join(lines[:-1]))
    with pytest.raises(ValueError):
        indelcal.load_table(str(path))
    path.write_text("".join(lines).replace("A\t3\t", "A\t4\t", 1))
    with pytest.raises(ValueError):
        indelcal.load_table(str(path))


def test_error_logs_cap_fallback_and_formula():
    from himut_amd import _ffi, indelcal
    table = _some_table()
    hit, err = indelcal.error_logs(table, 0.01, min_spans=1000)
    want_hit, want_err = K.error_logs(table, 0.01, min_spans=1000)
    assert hit.shape == err.shape == (896,) == (_ffi.INDEL_ERROR_CELLS,) and list(hit) == want_hit and list(err) == want_err

    def e_of(b, n, column):
        return 10 ** err[K.run_class(b, n) * 7 + K.COLUMNS.index(column) - 3]
    assert err[K.run_class("A", 3) * 7] == math.log10(4 / 4002) and hit[K.run_class("A", 3) * 7] == math.log10(1 - 4 / 4002)
    assert err[K.run_class("T", 40) * 7] == math.log10(0.25) and hit[K.run_class("T", 40) * 7] == math.log10(0.75)   # 401 / 1002: capped
    assert math.isclose(e_of("T", 40, "ins1"), 0.25) and math.isclose(e_of("T", 40, "del2"), 91 / 1002)
    assert err[K.run_class("G", 9) * 7] == math.log10(0.01)                    # 999 spans: one short of --min_spans
    assert err[K.run_class("C", 5) * 7 + 6] == math.log10(0.01) and hit[0] == math.log10(0.99)
    hit2, err2 = indelcal.error_logs(table, 0.02, min_spans=999)
    assert err2[K.run_class("G", 9) * 7] == math.log10(6 / 1001) and err2[0] == math.log10(0.02)
    assert indelcal.vaf_permille(0.25) == 250 and indelcal.vaf_permille(1) == 1000
    with pytest.raises(ValueError):
        indelcal.vaf_permille(1.5)


def test_model_under_a_table_differs_only_where_the_table_does():
    from tests.test_indels_cpu import boundary_sample
    _b, ref, items, log, _loci = boundary_sample()
    cell = K.event_cell(ref, K.runs_of(ref), *items[0][0][:3], "")
    assert cell is not None and all(K.event_cell(ref, K.runs_of(ref), *it[0][:3], "")[:2] == cell[:2] for it in items)
    base, blog = M.evaluate(items, log, report_homref=True, min_gq=0)
    flat = K.error_logs(np.zeros((128, 10), np.int64), 0.01)
    same, slog = K.evaluate_with_table(items, log, ref, *flat, report_homref=True, min_gq=0)
    assert same.tobytes() == base.tobytes() and slog == blog
    table = np.zeros((128, 10), np.int64)
    table[cell[0]] = [1, 0, 5000] + [600 if k == cell[1] else 0 for k in range(7)]
    other, _ = K.evaluate_with_table(items, log, ref, *K.error_logs(table, 0.01), report_homref=True, min_gq=0)
    assert other.tobytes() != base.tobytes() and len(other) == len(base)


# ---- the parser, the ABI

def test_parser():
    from himut_amd.parse_args import parse_args
    _p, o = parse_args("x", ["indelcal", "-i", "in.bam", "--ref", "ref.fa", "-o", "out.tsv"])
    assert o.sub == "indelcal" and o.bam == "in.bam" and o.ref == "ref.fa" and o.output == "out.tsv"
    assert o.min_mapq == 0 and o.min_alt_count == 2 and o.germline_vaf == 0.25 and o.max_indel_len == 50
    assert o.cs_from_ref is False and o.region is None and o.region_list is None and o.devices == "0" and o.threads == 1
    with pytest.raises(SystemExit):
        parse_args("x", ["indelcal", "-i", "in.bam", "-o", "out.tsv"])                   # --ref is required
    with pytest.raises(SystemExit):
        parse_args("x", ["indelcal", "-i", "in.bam", "--ref", "r.fa", "-o", "o.tsv", "--max_indel_len", "65"])
    _p, o = parse_args("x", ["indels", "-i", "in.bam", "--ref", "ref.fa", "-o", "out.vcf"])
    assert o.error_table is None and o.min_spans == 1000
    _p, o = parse_args("x", ["indels", "-i", "in.bam", "--ref", "ref.fa", "-o", "out.vcf", "--error_table", "t.tsv", "--min_spans", "50"])
    assert o.error_table == "t.tsv" and o.min_spans == 50


def test_abi_declares_and_exports_the_three_entry_points():
    from himut_amd import _ffi, build
    lib = ctypes.CDLL(build.build_hip())
    for name in ("himut_run_indelcal", "himut_get_indelcal", "himut_set_indel_error_table"):
        assert hasattr(lib, name) and name in _ffi._ABI
    assert ctypes.sizeof(_ffi.IndelcalParams) == 32 and ctypes.sizeof(_ffi.IndelParams) == 80
    assert tuple(_ffi.INDELCAL_LOG_NAMES) == K.LOG and tuple(_ffi.INDELCAL_COLUMNS) == K.COLUMNS
    lib.himut_run_indelcal.restype = ctypes.c_int
    lib.himut_run_indelcal.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.himut_run_indelcal(None, None) != 0
    lib.himut_abi_version.restype = ctypes.c_int
    assert lib.himut_abi_version() == 2


def test_header_line_only_under_the_flag():
    from himut_amd import vcflib
    args = ("in.bam", None, None, {"chrI": 4000}, 0, 20, 2, 2, 100, 1e-4, 0.01, 50, 1, "v", "o.vcf", "sample")
    plain = vcflib.get_indels_vcf_header(*args, ref_file="ref.fa")
    tabled = vcflib.get_indels_vcf_header(*args, ref_file="ref.fa", error_table="t.tsv", min_spans=1000)
    assert "indel_error_table" not in plain
    extra = [l for l in tabled.split("\n") if l not in plain.split("\n")]
    assert len(extra) == 1 and extra[0].startswith("##indel_error_table=t.tsv --min_spans 1000")
    assert [l for l in tabled.split("\n") if l != extra[0]] == plain.split("\n")
