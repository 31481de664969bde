"""The plain model of the intervals run (tests/intervals_model.py) pinned to the reference, and the host side of
`himut intervals` (himut_amd/intervals.py): the BED parser, the bins, the derived columns, the command line.  CPU only;
tests/test_gpu_intervals.py holds the device against the same model."""
import numpy as np
import pytest

from tests import callmap_model as M
from tests import intervals_cases as K
from tests import intervals_model as IM
from tests.test_callmap_cpu import golden_result
from tests.test_oracle_golden import NORM_CASES


@pytest.mark.parametrize("case", NORM_CASES)
def test_model_is_pinned_to_the_reference(case):
    """One interval over the whole string: the reference's two histograms on the 32 keys, the sum of all its other keys
    in slot 32, and the rows of norm.log."""
    res, v, refseq = golden_result(case, None)
    row = IM.Map.of(res, refseq).row(0, len(refseq))
    assert np.array_equal(row["ref_tri"], IM.fold_tri(v["ref_tri2count"]))
    assert np.array_equal(row["ccs_tri"], IM.fold_tri(v["ccs_tri2count"]))
    for code in (2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13):
        assert int(row["bases"][code]) == v["log"][code], code
    assert int(row["positions"][6]) == 0 and int(row["bases"][6]) == 0
    assert int(row["entries"]) == res.state.shape[0] == int(row["positions"].sum()) == int(row["all_tri"].sum())
    assert int(row["ref_tri"].sum()) == int(row["positions"][M.CALLABLE])
    assert int(row["ccs_tri"].sum()) == int(row["bases"][M.CALLABLE])


def test_class_order_is_the_tallys():
    assert IM.TRI_KEYS[0] == "ACA" and IM.TRI_KEYS[4] == "ATA" and IM.TRI_KEYS[8] == "CCA" and IM.TRI_KEYS[31] == "TTT"
    assert IM.tri_class("ACGT", 1) == IM.CLASS_OF["ACG"]
    assert IM.tri_class("ACGT", 2) == IM.CLASS_OF["ACG"]             # CGT on the other strand
    assert IM.tri_class("ACGT", 0) == IM.OTHER and IM.tri_class("ACGT", 3) == IM.OTHER
    assert IM.tri_class("AcG", 1) == IM.OTHER and IM.tri_class("aCG", 1) == IM.OTHER and IM.tri_class("NAG", 1) == IM.OTHER


@pytest.mark.parametrize("case", ["boundary", "hetalt"])
def test_partitions_sum_to_the_whole_span(case):
    c = getattr(K, case)()
    lo, hi = K.span_of(c.scene.chunks)
    whole = c.map.row(lo, hi)
    assert int(whole["entries"]) == c.res.state.shape[0]
    for parts in (K.steps(lo, hi, 1000), K.partition(lo, hi, 5, 40), K.partition(lo, hi, 6, 3), [(lo, hi)],
                  [(lo - 50, lo + 1), (lo + 1, hi - 1), (hi - 1, hi + 50)]):
        assert IM.same(IM.total(c.map.rows(parts)), whole)


def test_the_other_slot_is_exercised():
    """boundary_scene: the neighbours of the N at 1000 and of the lower-case stretch 1010..1013 that are CALLABLE -- 999,
    1001, 1009 and 1014 -- have a key outside the 32, ten bases each."""
    c = K.boundary()
    lo, hi = K.span_of(c.scene.chunks)
    whole = c.map.row(lo, hi)
    assert int(whole["ref_tri"][IM.OTHER]) == 4 and int(whole["ccs_tri"][IM.OTHER]) == 40
    s0 = c.scene.chunks[0][0]
    others = [p for p in range(990, 1030) if c.map.cls[p - s0] == IM.OTHER and c.res.state[p - s0] == M.CALLABLE]
    assert others == [999, 1001, 1009, 1014]
    assert int(whole["all_tri"][IM.OTHER]) >= 4 + 5


def test_unordered_chunks_count_a_position_twice():
    c = K.hetalt_unordered()
    one, two = c.map.row(1400, 1500), c.map.row(1500, 1600)
    assert int(one["entries"]) == 100 and int(two["entries"]) == 200
    a, b = K.hetalt().map.row(1500, 1600), two
    assert all(np.array_equal(2 * a[f], b[f]) for f in IM.FIELDS)


def test_string_ends_land_in_other():
    c = K.string_ends()
    n = len(c.scene.ref)
    for s, e in ((0, 1), (n - 1, n)):
        r = c.map.row(s, e)
        assert int(r["entries"]) == 1 and int(r["all_tri"][IM.OTHER]) == 1 and int(r["all_tri"].sum()) == 1
    assert int(c.map.row(0, 2)["all_tri"][IM.OTHER]) == 1
    assert int(c.map.row(0, n)["positions"][M.CALLABLE]) > 0


# ---------------------------------------------------------------------------------------------- the host side
def test_tri_class_of_the_driver_is_the_models():
    from himut_amd import _ffi, intervals
    assert list(_ffi.INTERVAL_TRI_NAMES) == IM.TRI_NAMES
    ref = K.boundary().scene.ref
    for pos in list(range(0, 3)) + list(range(990, 1030)) + list(range(len(ref) - 3, len(ref))):
        assert intervals.tri_class(ref, pos) == IM.tri_class(ref, pos), pos


def test_bed_parser(tmp_path):
    from himut_amd import intervals
    bed = tmp_path / "t.bed"
    bed.write_text("# a comment\ntrack name=x\nbrowser position chr1:1-2\nchr1\t10\t20\texon1\textra\nchr1\t5\t9\n\n"
                   "chrUn\t0\t100\tabsent\nchr2\t7\t7\tempty\n")
    assert intervals.read_bed(str(bed)) == [("chr1", 10, 20, "exon1"), ("chr1", 5, 9, "."), ("chrUn", 0, 100, "absent"),
                                            ("chr2", 7, 7, "empty")]
    bad = tmp_path / "bad.bed"
    bad.write_text("chr1\t10\n")
    with pytest.raises(ValueError):
        intervals.read_bed(str(bad))


def test_bins_at_a_length_that_is_no_multiple():
    from himut_amd import intervals
    b = intervals.bin_intervals("chr3", 2450, 700)
    assert [(s, e) for _c, s, e, _n in b] == [(0, 700), (700, 1400), (1400, 2100), (2100, 2450)]
    assert all(c == "chr3" for c, _s, _e, _n in b) and b[3][3] == "chr3:2100-2450"
    assert [(s, e) for _c, s, e, _n in intervals.bin_intervals("c", 1400, 700)] == [(0, 700), (700, 1400)]
    assert intervals.bin_intervals("c", 0, 700) == []
    with pytest.raises(ValueError):
        intervals.bin_intervals("c", 10, 0)


def test_derived_columns_on_hand_made_rows():
    from himut_amd import intervals
    all_tri, ccs, sbs = [0] * 33, [0] * 33, [0] * 33
    all_tri[0], ccs[0], sbs[0] = 100, 50, 2          # 2 / 50 * 100 = 4
    all_tri[5], ccs[5], sbs[5] = 30, 40, 1           # 1 / 40 * 30 = 0.75
    all_tri[7], ccs[7], sbs[7] = 9, 0, 3             # no callable base in the class: uncallable
    all_tri[32], ccs[32], sbs[32] = 8, 12, 4         # other: uncallable, and out of the denominator
    n, unc, rate, burden = intervals.derived(all_tri, ccs, sbs)
    assert (n, unc) == (10, 7)
    assert rate == (10 - 7) / 90
    assert burden == 2 * (2 / 50 * 100 + 1 / 40 * 30)
    assert intervals.derived(all_tri, [0] * 32 + [12], sbs) == (10, 10, None, None)
    assert intervals.derived([0] * 33, [0] * 33, [0] * 33) == (0, 0, None, None)
    n, unc, rate, burden = intervals.derived(all_tri, ccs, [0] * 33)
    assert (n, unc, rate, burden) == (0, 0, 0.0, 0.0)
    row = np.zeros((), IM.ROW_DTYPE)
    row["all_tri"], row["ccs_tri"], row["entries"] = all_tri, ccs, 147
    row["positions"][13], row["bases"][13] = 60, 102
    lines = intervals.main_lines([("chr1", 10, 157, "x")], [row], [np.array(sbs)])
    assert lines[0] == "\t".join(intervals.HEADER) + "\n"
    assert lines[1] == "chr1\t10\t157\tx\t147\t147\t60\t102\t10\t7\t{}\t{}\n".format(repr(3 / 90), repr(9.5))
    assert intervals.main_lines([("chr1", 10, 157, "x")], [row], None)[1].endswith("\t60\t102\tNA\tNA\tNA\tNA\n")
    assert intervals.main_lines([("chr1", 9, 3, "x")], [np.zeros((), IM.ROW_DTYPE)], [np.zeros(33, np.int64)])[1] == \
        "chr1\t9\t3\tx\t0\t0\t0\t0\t0\t0\tNA\tNA\n"


def test_substitutions_go_to_every_interval_that_holds_them():
    from himut_amd import intervals
    ref = "TTACGTCCATnACTTTT"                                    # 3: ACG, 8: CAT (ATG on the other strand), 12: ACT
    pos, cls = intervals.sbs_classes("c", ref, [8, 3, 3, 12], ["A", "C", "C", "C"])
    assert pos.tolist() == [3, 3, 8, 12] and cls.tolist() == [IM.tri_class(ref, p) for p in (3, 3, 8, 12)]
    got = intervals.sbs_per_interval([0, 3, 4, 0, 9], [4, 4, 9, 17, 9], pos, cls)
    assert got.sum(axis=1).tolist() == [2, 2, 1, 4, 0]
    assert got[3][IM.CLASS_OF["ACG"]] == 2 and got[3][IM.CLASS_OF["ATG"]] == 1 and got[3][IM.CLASS_OF["ACT"]] == 1
    with pytest.raises(ValueError):
        intervals.sbs_classes("c", ref, [3], ["A"])
    assert intervals.sbs_classes("c", ref, [10], ["N"])[1].tolist() == [IM.OTHER]      # the upper-cased letter


def test_parse_args_wants_exactly_one_of_bed_and_bin_size():
    from himut_amd.parse_args import build_parser
    parser = build_parser("t")
    base = ["intervals", "-i", "in.bam", "--ref", "ref.fa", "-o", "out.tsv"]
    for extra in ([], ["--bed", "t.bed", "--bin_size", "1000"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + extra)
    o = parser.parse_args(base + ["--bed", "t.bed", "--tri", "tri.tsv", "--states", "st.tsv"])
    assert (o.sub, o.bed, o.bin_size, o.sbs, o.tri, o.states) == ("intervals", "t.bed", None, None, "tri.tsv", "st.tsv")
    o = parser.parse_args(base + ["--bin_size", "700", "--sbs", "calls.vcf", "--phase", "--min_bq", "50"])
    assert (o.bin_size, o.bed, o.sbs, o.phase, o.min_bq) == (700, None, "calls.vcf", True, 50)
    sub = parser._subparsers._group_actions[0].choices
    call = {a.dest: a for a in sub["callable"]._actions}
    mine = {a.dest: a for a in sub["intervals"]._actions}
    assert set(call) - {"callable_only", "summary"} <= set(mine)
    for dest in set(call) - {"callable_only", "summary", "help"}:
        a, b = call[dest], mine[dest]
        assert (a.option_strings, a.type, a.default, a.required) == (b.option_strings, b.type, b.default, b.required), dest


def test_the_driver_is_a_single_process(monkeypatch):
    from himut_amd import intervals
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError):
        intervals.dump_intervals(*([None] * 30))
