"""Hand-built alignments for the indels run's contract: one case per rule of the contract and per shape at which the
kernels can go wrong.  A case is (name, batch, regions, contig string, parameters, expect(records, log)); the CPU tests run
the model on them and check what each rule says, the GPU tests compare the run with the model byte for byte and check the
same statements."""
import numpy as np

from himut_amd.readbatch import batch_from_records
from tests import indels_model as M

N = 4000
ALL = [(0, N)]


def contig(seed, n=N, plant=()):
    """A random ACGT string with the given (position, string) planted."""
    rs = np.random.RandomState(seed)
    s = "".join("ACGT"[k] for k in rs.randint(0, 4, n))
    for pos, t in plant:
        s = s[:pos] + t + s[pos + len(t):]
    return s[:n]


def read(ref, start, length, ins=None, dels=None, bq=40, **extra):
    """A read record over ref[start:start + length]: ins {pos: bases in front of pos; pos == start + length trails}, dels
    {pos: length}.  The text is made of slices, so that thousands of reads cost little."""
    ins, dels = ins or {}, dels or {}
    end = start + length
    seq, cs = [], []
    run = 0
    p = start

    def flush():
        nonlocal run
        if run:
            cs.append(":{}".format(run))
            run = 0
    for pos in sorted(set(ins) | set(dels)):
        assert start <= pos <= end and pos >= p, (pos, p, start, end)
        if pos > p:
            seq.append(ref[p:pos].upper())
            run += pos - p
            p = pos
        if pos in ins:
            flush()
            cs.append("+" + ins[pos].lower())
            seq.append(ins[pos].upper())
        if pos in dels:
            assert pos + dels[pos] <= end
            flush()
            cs.append("-" + ref[pos:pos + dels[pos]].lower())
            p = pos + dels[pos]
    seq.append(ref[p:end].upper())
    run += end - p
    flush()
    s = "".join(seq)
    return dict(tstart=start, tend=end, qstart=0, seq=s, bq=[bq] * len(s), cs="".join(cs), **extra)


def batch(records, length=N, name="chrI"):
    records = sorted(records, key=lambda r: r["tstart"])        # coordinate sorted, as a BAM is
    return batch_from_records(name, length, records)


def cover(ref, n, carriers, start=900, length=300, **event):
    """n reads over [start, start + length), the first `carriers` with the event."""
    return [read(ref, start, length, **(event if k < carriers else {})) for k in range(n)]


def only(recs, **fields):
    assert len(recs) == 1, recs
    for k, v in fields.items():
        assert int(recs[0][k]) == v, (k, int(recs[0][k]), v)
    return recs[0]


def ok(*conds):
    assert all(conds), conds


def logd(log):
    return dict(zip(M.LOG, log))


def _cases():
    out = []

    def case(name, recs, ref, expect, regions=ALL, **kw):
        out.append((name, batch(recs, len(ref)), regions, ref, kw, expect))

    # ---- rules.  CAGTCA at 1000: deleting TC from 1003 and inserting TA in front of 1003 cannot shift
    ref = contig(1, plant=[(1000, "CAGTCA")])
    for n_car, state, nm in ((6, 1, "het"), (12, 2, "homalt")):
        case(nm + "_del", cover(ref, 12, n_car, dels={1003: 2}), ref,
             lambda r, l, n_car=n_car, state=state: only(r, anchor=1002, type=0, len=2, gt_state=state, dp=12, n_alt=n_car, n_other=0,
                                                         status=M.ST_PASS))
        case(nm + "_ins", cover(ref, 12, n_car, ins={1003: "TA"}), ref,
             lambda r, l, n_car=n_car, state=state: ok(M.unpack_bases(only(r, anchor=1002, type=1, len=2, gt_state=state, dp=12, n_alt=n_car,
                                                                             n_other=0, status=M.ST_PASS)) == "TA"))

    def one_in_twelve(r, l):
        assert len(r) == 0 and logd(l)["homref"] == 1 and logd(l)["alleles"] == 1 and logd(l)["PASS"] == 0
    case("one_in_twelve", cover(ref, 12, 1, dels={1003: 2}), ref, one_in_twelve)
    case("one_in_twelve_reported", cover(ref, 12, 1, dels={1003: 2}), ref,
         lambda r, l: only(r, anchor=1002, gt_state=0, n_alt=1, dp=12, status=M.ST_PASS), report_homref=True)
    case("low_gq", cover(ref, 12, 6, dels={1003: 2}), ref, lambda r, l: only(r, status=M.ST_LOWGQ), min_gq=100)
    case("low_depth_alt", cover(ref, 12, 6, dels={1003: 2}), ref, lambda r, l: only(r, status=M.ST_LOWDEPTH, n_alt=6), min_alt_count=7)
    case("low_depth_ref", cover(ref, 7, 6, dels={1003: 2}), ref, lambda r, l: only(r, gt_state=1, status=M.ST_LOWDEPTH), min_ref_count=2, min_gq=0)
    case("high_depth", cover(ref, 12, 6, dels={1003: 2}), ref, lambda r, l: only(r, status=M.ST_HIGHDEPTH), md_threshold=11)

    # ---- the shift.  C A*8 G at 1000: a deleted A anywhere in the run is the deletion of the first
    ref = contig(2, plant=[(1000, "C" + "A" * 8 + "G")])
    case("shift_homopolymer", [read(ref, 900, 300, dels={1001 + k % 8: 1}) for k in range(12)], ref,
         lambda r, l: only(r, anchor=1000, type=0, len=1, n_alt=12, dp=12, gt_state=2))
    # G (CA)*6 T: CA at any period, or AC one position off, is CA in front of the first C
    ref = contig(3, plant=[(1000, "G" + "CA" * 6 + "T")])
    recs = [read(ref, 900, 300, ins={1001 + 2 * (k % 6): "CA"}) for k in range(8)] + \
           [read(ref, 900, 300, ins={1002 + 2 * (k % 5): "AC"}) for k in range(6)]
    case("shift_rotation", recs, ref,
         lambda r, l: ok(M.unpack_bases(only(r, anchor=1000, type=1, len=2, n_alt=14, dp=14)) == "CA"))
    # C AAA N AAA G: the N stops the shift of a deletion behind it
    ref = contig(4, plant=[(1000, "CAAANAAAG")])
    recs = [read(ref, 900, 300, dels={1007: 1}) for _ in range(5)] + [read(ref, 900, 300, dels={1003: 1}) for _ in range(4)]

    def stop_n(r, l):
        assert [int(x) for x in r["anchor"]] == [1000, 1004] and [int(x) for x in r["n_alt"]] == [4, 5]
    case("shift_stop_n", recs, ref, stop_n)
    # lower case is compared like upper case: the shift goes through
    ref = contig(5, plant=[(1000, "caAaAg")])
    case("shift_lower_case", [read(ref, 900, 300, dels={1004: 1}) for _ in range(6)], ref, lambda r, l: only(r, anchor=1000, n_alt=6))
    # TTTTTT G at the contig's start under reads from 0: the anchor stops at position 1
    ref = contig(6, plant=[(0, "TTTTTTG")])
    case("shift_stop_position_1", [read(ref, 0, 300, dels={4: 1}) for _ in range(6)], ref, lambda r, l: only(r, anchor=0, n_alt=6, dp=6))
    # a read that starts inside the run anchors its deletion at its own start
    ref = contig(7, plant=[(1000, "C" + "A" * 8 + "G")])
    recs = [read(ref, 900, 300, dels={1006: 1}) for _ in range(6)] + [read(ref, 1004, 300, dels={1007: 1}) for _ in range(3)]

    def stop_read(r, l):
        assert [int(x) for x in r["anchor"]] == [1000, 1004] and [int(x) for x in r["n_alt"]] == [6, 3]
        assert [int(x) for x in r["dp"]] == [6, 9]
    case("shift_stop_read_start", recs, ref, stop_read, min_alt_count=1, report_homref=True)

    # ---- exactness: one anchor, strings that differ in one base
    ref = contig(8, plant=[(1000, "CAGTCA")])
    base = "T" * 12
    strings = [base] + [base[:k] + "C" + base[k + 1:] for k in range(12)]
    long_ = ["A" * 32 + x for x in "ATC"]
    recs = [read(ref, 900, 300, ins={1003: s}) for s in strings + long_ for _ in range(2)]

    def exact(r, l):
        assert len(r) == 16 and set(int(x) for x in r["anchor"]) == {1002}
        assert [M.unpack_bases(x) for x in r] == sorted(strings, key=lambda s: [M.BASES.index(b) for b in s]) + long_
        assert all(int(x) == 2 for x in r["n_alt"]) and all(int(x) == 30 for x in r["n_other"]) and all(int(x) == 32 for x in r["dp"])
    case("exact_strings", recs, ref, exact, report_homref=True)

    # ---- counting
    ref = contig(9, plant=[(1000, "C" + "A" * 8 + "G")])
    recs = cover(ref, 6, 3, dels={1002: 1}) + [read(ref, 900, 300, dels={1002: 1, 1006: 1})]

    def dup(r, l):
        only(r, anchor=1000, n_alt=4, dp=7)
        assert logd(l)["num_dup"] == 1 and logd(l)["events"] == 5
    case("count_dup", recs, ref, dup)
    ref = contig(10, plant=[(1000, "CAGTCA")])
    recs = cover(ref, 8, 4, dels={1003: 2}) + [read(ref, 900, 300, dels={1003: 2}, flag=0x100), read(ref, 900, 300, dels={1003: 2}, mapq=5),
                                               read(ref, 900, 300, flag=0x100), read(ref, 900, 300, mapq=5)]
    case("count_secondary_mapq", recs, ref, lambda r, l: only(r, n_alt=4, dp=8), min_mapq=20)
    # the anchor is 1002, the span end 1005: tstart 1002 in, 1003 out; tend 1006 in, 1005 out
    recs = cover(ref, 8, 4, dels={1003: 2}) + [read(ref, 1002, 200), read(ref, 1003, 200), read(ref, 800, 206), read(ref, 800, 205)]
    case("count_dp_edges", recs, ref, lambda r, l: only(r, n_alt=4, dp=10))
    recs = cover(ref, 6, 3, dels={1003: 2}) + [read(ref, 900, 300, ins={900: "GG"}), read(ref, 900, 300, ins={1200: "GG"}),
                                               read(ref, 900, 300, dels={900: 2}), read(ref, 900, 300, dels={1198: 2})]

    def edge(r, l):
        only(r, n_alt=3, dp=10)
        assert logd(l)["num_edge"] == 4 and logd(l)["events"] == 3
    case("count_edges", recs, ref, edge, report_homref=True)
    for ml in (50, 64):
        recs = [read(ref, 800, 500, dels={1003: ml}) for _ in range(3)] + [read(ref, 800, 500, dels={1003: ml + 1}) for _ in range(2)] + \
               [read(ref, 800, 500, ins={1003: "TC" * (ml // 2)}) for _ in range(3)] + [read(ref, 800, 500, ins={1003: "TC" * (ml // 2) + "T"}) for _ in range(2)]

        def longs(r, l, ml=ml):
            assert logd(l)["num_long"] == 4 and logd(l)["events"] == 6 and len(r) == 2
            assert all(int(x) == ml for x in r["len"]) and all(int(x) == 3 for x in r["n_alt"])
        case("count_max_len_{}".format(ml), recs, ref, longs, max_len=ml, report_homref=True)
    recs = cover(ref, 6, 3, ins={1003: "TA"}) + [read(ref, 900, 300, ins={1003: "TNA"})]

    def nbase(r, l):
        only(r, n_alt=3, dp=7, n_other=0)
        assert logd(l)["num_nbase"] == 1
    case("count_inserted_n", recs, ref, nbase, report_homref=True)

    # ---- shapes
    ref = contig(11, plant=[(1000, "CAGTCA"), (1020, "GACTTG")])
    case("shape_no_events", cover(ref, 12, 0), ref, lambda r, l: ok(len(r) == 0, list(l) == [0] * 13))
    case("shape_empty_batch", [], ref, lambda r, l: ok(len(r) == 0, list(l) == [0] * 13))
    many = {p: 1 for p in range(120, 120 + 12 * 40, 12)}        # 40 deletions: 81 segments
    more = {p: 1 for p in range(120, 120 + 12 * 140, 12)}       # 140 deletions: 281 segments
    recs = [read(ref, 100, 2000, dels=many) for _ in range(3)] + [read(ref, 100, 2000, dels=more) for _ in range(3)] + [read(ref, 100, 2000)]

    def segments(r, l):
        assert logd(l)["events"] == 3 * 40 + 3 * 140 and logd(l)["alleles"] >= 100
    case("shape_many_segments", recs, ref, segments, report_homref=True)
    for n in (70, 300):
        case("shape_locus_{}_reads".format(n), cover(ref, n, n // 2, dels={1003: 2}) + cover(ref, 5, 5, ins={1023: "TA"}), ref,
             lambda r, l, n=n: ok(len(r) == 2, int(r[0]["dp"]) == n + 5, int(r[0]["n_alt"]) == n // 2), report_homref=True)
    # GACGTCAG at 1020: TCA deleted from 1024 cannot shift; the anchor 1023 is the last position of its 256-block, the span
    # ends in the next; tend 1027 is out, 1028 in
    ref2 = contig(12, plant=[(1020, "GACGTCAG")])
    case("shape_block_edge", cover(ref2, 12, 6, dels={1024: 3}) + [read(ref2, 800, 227), read(ref2, 800, 228)], ref2,
         lambda r, l: only(r, anchor=1023, len=3, n_alt=6, dp=13))
    recs = cover(ref, 12, 6, dels={1003: 2})
    case("region_overlap", recs, ref, lambda r, l: ok(only(r, anchor=1002) is not None, logd(l)["alleles"] == 1),
         regions=[(900, 1002), (1002, 1100), (1000, 1005)])
    case("region_outside", recs, ref, lambda r, l: ok(len(r) == 0, logd(l)["events"] == 0), regions=[(0, 1001), (1003, N)])
    return out


CASES = _cases()
