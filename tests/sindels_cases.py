"""Hand-built alignments for the sindels run's contract: one case per rule of the contract and per shape at which the
kernels can go wrong.  A case is (name, batch, regions, contig string, parameters, expect(records, log)); a parameter
"table" ({(letter, run length, column): error}) is not the run's: it is the indel error table to set for the case.  The
CPU tests run the model on them and check what each rule says, the GPU tests compare the run with the model byte for byte
and check the same statements.

A batch keeps every read at a multiple of 32 bytes (readbatch.py), so no read starts at an odd offset of the quality
array; the bytes between two reads are set to 255 here, so that a sum that reads past a read's end or in front of its
start does not go unnoticed."""
import math

import numpy as np

from tests import indelcal_model as IC
from tests import indels_cases as C
from tests import indels_model as M
from tests import sindels_model as S

N = 6000
ALL = [(0, N)]
# the cases' own defaults: the reads' qualities are 40, so min_bq sits below them
KW = dict(min_mapq=20, min_qv=30, min_bq=30, min_gq=20, min_ref_count=3, min_alt_count=1, max_run=2,
          min_sequence_identity=0.99, min_trim=0.01, mismatch_window_size=20, max_mismatch_count=0)
DEL, INS = M.DEL, M.INS


def read(ref, start, length, ins=None, dels=None, subs=None, bq=40, clip=(0, 0), **extra):
    """indels_cases.read with substitutions (subs {pos: base}), soft clips (clip = bases in front, behind) and qualities
    per query base (bq: one number, or a function of the query length that returns the list)."""
    ins, dels, subs = ins or {}, dels or {}, subs or {}
    end = start + length
    seq, cs = ["A" * clip[0]], []
    run = 0
    p = start

    def flush():
        nonlocal run
        if run:
            cs.append(":{}".format(run))
            run = 0
    for pos in sorted(set(ins) | set(dels) | set(subs)):
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
            assert pos + dels[pos] <= end and pos not in subs
            flush()
            cs.append("-" + ref[pos:pos + dels[pos]].lower())
            p = pos + dels[pos]
        if pos in subs:
            assert subs[pos].upper() != ref[pos].upper() and pos < end
            flush()
            cs.append("*" + ref[pos].lower() + subs[pos].lower())
            seq.append(subs[pos].upper())
            p = pos + 1
    seq.append(ref[p:end].upper())
    run += end - p
    flush()
    seq.append("C" * clip[1])
    s = "".join(seq)
    return dict(tstart=start, tend=end, qstart=clip[0], seq=s, bq=bq(len(s)) if callable(bq) else [bq] * len(s),
                cs="".join(cs), **extra)


def batch(records, length=N, name="chrI"):
    b = C.batch(records, length, name)
    for i in range(b.n):                                             # the padding behind every read
        o, ql = int(b.qoff[i]), int(b.qlen[i])
        b.bq[o + ql:(o + ql + 31) & ~31] = 255
    return b


def plain(ref, n, start=900, length=300):
    return [read(ref, start, length) for _ in range(n)]


def low_at(*offsets, value=29):
    """Qualities of 40 with `value` at the given query offsets."""
    def f(qlen):
        out = [40] * qlen
        for o in offsets:
            out[o] = value
        return out
    return f


def at(recs, anchor, ty=None):
    """The records anchored at `anchor` (of one type)."""
    return [r for r in recs if int(r["anchor"]) == anchor and (ty is None or int(r["type"]) == ty)]


def one(recs, anchor, ty=None, **fields):
    got = at(recs, anchor, ty)
    assert len(got) == 1, (anchor, ty, recs)
    for k, v in fields.items():
        assert int(got[0][k]) == v, (k, int(got[0][k]), v)
    return got[0]


def none(recs, log, **counters):
    assert len(recs) == 0, recs
    d = S.logd(log)
    for k, v in counters.items():
        assert d[k] == v, (k, d[k], v)


def counts(log, **counters):
    d = S.logd(log)
    for k, v in counters.items():
        assert d[k] == v, (k, d[k], v)
    return True


def trim_bounds(qlen, min_trim=0.01):
    return math.floor(min_trim * qlen), math.ceil((1 - min_trim) * qlen)


def _cases():
    out = []

    def case(name, recs, ref, expect, regions=ALL, **kw):
        out.append((name, batch(recs, len(ref)), regions, ref, dict(KW, **kw), expect))

    # ---- CAGTCA at 1000: deleting TC from 1003 and inserting TA in front of 1003 cannot shift; the run behind the anchor
    # 1002 is one T, so neither is in a repeat
    ref = C.contig(31, N, plant=[(1000, "CAGTCA")])
    d, i_ = dict(dels={1003: 2}), dict(ins={1003: "TA"})
    case("lone_del", plain(ref, 11) + [read(ref, 900, 300, **d)], ref,
         lambda r, l: (one(r, 1002, type=0, len=2, status=S.ST_PASS, gt_state=0, dp=12, n_alt=1, n_other=0, n_prop=1, run_base=1,
                           run_len=1, class_col=6), counts(l, candidates=1, PASS=1, pile_reads=12, proposing_reads=12)))
    case("lone_ins", plain(ref, 11) + [read(ref, 900, 300, **i_)], ref,
         lambda r, l: C.ok(M.unpack_bases(one(r, 1002, type=1, len=2, status=S.ST_PASS, dp=12, n_alt=1, n_prop=1)) == "TA"))
    two = plain(ref, 10) + [read(ref, 900, 300, **d), read(ref, 900, 300, **d)]
    case("two_carriers_min_alt_1", two, ref, lambda r, l: one(r, 1002, status=S.ST_PASS, n_alt=2, n_prop=2, dp=12))
    case("two_carriers_min_alt_3", two, ref, lambda r, l: one(r, 1002, status=S.ST_LOWDEPTH, n_alt=2, n_prop=2), min_alt_count=3)

    # ---- the read filters, each alone: a good carrier and one the filter takes out; the pile keeps both
    def filtered(name, bad, n_prop, n_alt=2, dp=12, **kw):
        case(name, plain(ref, 10) + [read(ref, 900, 300, **d), bad], ref,
             lambda r, l: one(r, 1002, ty=0, n_alt=n_alt, n_prop=n_prop, dp=dp), **kw)
    qlen = 298
    filtered("qsum_exact", read(ref, 900, 300, bq=30, **d), 2)                                   # 30 * 298 = min_qv * qlen
    filtered("qsum_one_less_first", read(ref, 900, 300, bq=lambda n: [29] + [30] * (n - 1), **d), 1)
    filtered("qsum_one_less_last", read(ref, 900, 300, bq=lambda n: [30] * (n - 1) + [29], **d), 1)
    far = dict(dels={1003: 2, 1150: 1})                              # identity 297 / 300 against the good carrier's 298 / 300
    filtered("identity_at_cut", read(ref, 900, 300, **far), 2, min_sequence_identity=297 / 300.0)
    filtered("identity_below_cut", read(ref, 900, 300, **far), 1, min_sequence_identity=float(np.nextafter(297 / 300.0, 1.0)))
    longer = read(ref, 900, 310, **d)                                # qlen 308 against 298
    filtered("qlen_below_upper", longer, 2, qlen_upper_limit=309, qlen_lower_limit=297)
    filtered("qlen_at_upper", longer, 1, qlen_upper_limit=308, qlen_lower_limit=297)
    filtered("qlen_at_lower", longer, 1, qlen_upper_limit=309, qlen_lower_limit=qlen)
    filtered("mapq_below_cut", read(ref, 900, 300, mapq=19, **d), 1, n_alt=1, dp=11)
    filtered("mapq_at_cut", read(ref, 900, 300, mapq=20, **d), 2)

    # ---- the trim: the footprint's first base at floor(min_trim qlen) and one in front, its last at ceil((1 - min_trim)
    # qlen) and one behind
    for nm, ev, ty, qlen, width in (("del", d, 0, 298, 0), ("ins", i_, 1, 302, 2)):
        lo, hi = trim_bounds(qlen)
        for where, q, ok in (("start_at", lo + 1, True), ("start_inside", lo, False), ("end_at", hi - width, True),
                             ("end_inside", hi - width + 1, False)):
            carrier = read(ref, 1003 - q, 300, **ev)                 # q: the query offset of the event
            assert len(carrier["seq"]) == qlen
            case("trim_{}_{}".format(nm, where), plain(ref, 11, 720, 500) + [carrier], ref,
                 (lambda r, l, ty=ty: one(r, 1002, ty=ty, status=S.ST_PASS, n_prop=1)) if ok else
                 (lambda r, l: none(r, l, num_trim=1, events_proposing_reads=1, candidates=0)))

    # ---- the window: another entry of the read's mismatch list w and w + 1 away, on either side; the two branches of
    # get_mismatch_range at the read's ends; an insertion straight in front of a deletion
    def other(b):
        return "A" if b.upper() != "A" else "C"
    for nm, start, vetoes, passes in (("mid", 900, (1003 - 20, 1003 + 20), (1003 - 21, 1003 + 21)),
                                      ("read_start", 1003 - 10, (1003 + 30,), (1003 + 31,)),      # q = 10: qstart < 0
                                      ("read_end", 1003 - 288, (1003 - 30,), (1003 - 31,))):      # q = 288: qend > qlen
        for x in vetoes + passes:
            carrier = read(ref, start, 300, dels={1003: 2}, subs={x: other(ref[x])})
            case("window_{}_sub_{:+d}".format(nm, x - 1003), plain(ref, 11, 720, 600) + [carrier], ref,
                 (lambda r, l: none(r, l, num_window=1, candidates=0)) if x in vetoes else
                 (lambda r, l: one(r, 1002, status=S.ST_PASS, n_prop=1)))
    both = read(ref, 900, 300, ins={1003: "TA"}, dels={1003: 2})
    case("window_ins_del_0", plain(ref, 11) + [both], ref, lambda r, l: none(r, l, num_window=2, events_proposing_reads=2),
         min_sequence_identity=0.98)
    case("window_ins_del_1", plain(ref, 11) + [both], ref,
         lambda r, l: (one(r, 1002, ty=0, n_prop=1, n_other=0), one(r, 1002, ty=1, n_prop=1, n_other=0)), max_mismatch_count=1,
         min_sequence_identity=0.98)

    # ---- min_bq: one base below it at every position of the footprint and just outside it
    q = 103
    for off, ok in ((q - 2, True), (q - 1, False), (q, False), (q + 1, True)):
        case("lowbq_del_{:+d}".format(off - q), plain(ref, 11) + [read(ref, 900, 300, bq=low_at(off), **d)], ref,
             (lambda r, l: one(r, 1002, status=S.ST_PASS)) if ok else (lambda r, l: none(r, l, num_lowbq=1, candidates=0)))
    for L in (1, 32, 33, 64):
        s = ("TA" * 32)[:L]
        for off, ok in ((q - 2, True), (q - 1, False), (q, False), (q + L - 1, False), (q + L, False), (q + L + 1, True)):
            case("lowbq_ins{}_{:+d}".format(L, off - q), plain(ref, 11) + [read(ref, 900, 300, ins={1003: s}, bq=low_at(off))], ref,
                 (lambda r, l, L=L: one(r, 1002, ty=1, len=L, status=S.ST_PASS)) if ok else
                 (lambda r, l: none(r, l, num_lowbq=1, candidates=0)), max_len=64, min_sequence_identity=0.5)

    # ---- a soft-clipped read: query offsets count the clip
    case("soft_clip", plain(ref, 11) + [read(ref, 900, 300, clip=(7, 5), **d)], ref, lambda r, l: one(r, 1002, status=S.ST_PASS, n_prop=1))
    case("soft_clip_lowbq", plain(ref, 11) + [read(ref, 900, 300, clip=(7, 5), bq=low_at(q + 7), **d)], ref,
         lambda r, l: none(r, l, num_lowbq=1))

    # ---- the verdicts
    case("germ_het", plain(ref, 6) + [read(ref, 900, 300, **d) for _ in range(6)], ref, lambda r, l: none(r, l, candidates=1, num_germ_het=1))
    case("germ_homalt", [read(ref, 900, 300, **d) for _ in range(12)], ref, lambda r, l: none(r, l, candidates=1, num_germ_homalt=1))
    case("indel_site", plain(ref, 10) + [read(ref, 900, 300, **d), read(ref, 900, 300, **i_)], ref,
         lambda r, l: (one(r, 1002, ty=0, status=S.ST_INDEL, n_other=1), one(r, 1002, ty=1, status=S.ST_INDEL, n_other=1)))
    gq = M.genotype(11, 1, M.logs(0.01, 1e-4))[1]
    lone = plain(ref, 11) + [read(ref, 900, 300, **d)]
    case("precedence_low_gq", lone, ref, lambda r, l: one(r, 1002, status=S.ST_LOWGQ, gq=gq), min_gq=gq + 1, min_ref_count=12, md_threshold=5)
    case("precedence_gq_at_cut", lone, ref, lambda r, l: one(r, 1002, status=S.ST_LOWDEPTH), min_gq=gq, min_ref_count=12, md_threshold=5)
    case("precedence_low_depth_ref", lone, ref, lambda r, l: one(r, 1002, status=S.ST_LOWDEPTH), min_ref_count=12, md_threshold=5)
    case("precedence_ref_at_cut", lone, ref, lambda r, l: one(r, 1002, status=S.ST_HIGHDEPTH), min_ref_count=11, md_threshold=11)
    case("precedence_depth_at_cut", lone, ref, lambda r, l: one(r, 1002, status=S.ST_PASS), min_ref_count=11, md_threshold=12)

    # ---- Repeat: C AAA G at 1000; a deleted A is the deletion of the first, anchor 1000
    ref3 = C.contig(32, N, plant=[(1000, "CAAAG")])
    dA, iA, iT = dict(dels={1002: 1}), dict(ins={1002: "A"}), dict(ins={1001: "T"})
    case("repeat_del_run3", plain(ref3, 11) + [read(ref3, 900, 300, **dA)], ref3,
         lambda r, l: one(r, 1000, ty=0, status=S.ST_REPEAT, run_base=0, run_len=3, class_col=0))
    case("repeat_del_run3_max_run3", plain(ref3, 11) + [read(ref3, 900, 300, **dA)], ref3, lambda r, l: one(r, 1000, status=S.ST_PASS, run_len=3), max_run=3)
    case("repeat_ins_run3", plain(ref3, 11) + [read(ref3, 900, 300, **iA)], ref3,
         lambda r, l: one(r, 1000, ty=1, status=S.ST_REPEAT, run_len=3, class_col=3))
    case("repeat_other_ins_run3", plain(ref3, 11) + [read(ref3, 900, 300, **iT)], ref3,
         lambda r, l: one(r, 1000, ty=1, status=S.ST_PASS, run_len=3, class_col=6))
    ref2 = C.contig(33, N, plant=[(1000, "CAAG")])
    case("repeat_del_run2", plain(ref2, 11) + [read(ref2, 900, 300, **dA)], ref2, lambda r, l: one(r, 1000, status=S.ST_PASS, run_len=2, class_col=0))
    ref65 = C.contig(34, N, plant=[(1000, "C" + "A" * 65 + "G")])
    case("repeat_run65", plain(ref65, 11) + [read(ref65, 900, 300, dels={1030: 1})], ref65,
         lambda r, l: one(r, 1000, status=S.ST_REPEAT, run_base=0, run_len=65, class_col=255), max_run=1000, max_mismatch_count=1)

    # ---- the table: the cell's own error flips a verdict the constant does not
    case("table_constant", plain(ref2, 11) + [read(ref2, 900, 300, **dA)], ref2, lambda r, l: one(r, 1000, status=S.ST_PASS))
    case("table_cell", plain(ref2, 11) + [read(ref2, 900, 300, **dA)], ref2, lambda r, l: one(r, 1000, status=S.ST_LOWGQ),
         table={("A", 2, 0): 1e-6})
    case("table_other_cell", plain(ref2, 11) + [read(ref2, 900, 300, **dA)], ref2, lambda r, l: one(r, 1000, status=S.ST_PASS),
         table={("A", 3, 0): 1e-6, ("A", 2, 1): 1e-6})

    # ---- shapes.  The quality sum's head and tail: reads of every length at which the stream takes another path, their sum
    # exactly min_qv * qlen, then one less at the first or the last base; the longest all 93
    lens = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)

    def mixed(n, rs):                                                # qualities that add up to 40 n
        out = np.full(n, 40, np.int64)
        for _ in range(n // 2):
            a, b_, k = rs.randint(0, n), rs.randint(0, n), rs.randint(0, 20)
            if a != b_ and out[a] + k <= 93 and out[b_] - k >= 1:
                out[a] += k
                out[b_] -= k
        return [int(x) for x in out]
    for nm, delta_at in (("exact", None), ("less_first", 0), ("less_last", -1)):
        rs = np.random.RandomState(5)
        recs = []
        for n in lens:
            bq = mixed(n, rs)
            if delta_at is not None:
                bq[delta_at] -= 1
            recs.append(read(ref, 100 + 7 * n % 50, n, bq=lambda _n, bq=bq: bq))
        want = len(recs) if delta_at is None else 0
        case("sum_lengths_" + nm, recs, ref, lambda r, l, want=want: counts(l, pile_reads=len(lens), proposing_reads=want), min_qv=40)
    # the longest, all 93 under min_qv 93: the byte-parallel sums carry
    for nm, delta_at in (("exact", None), ("less_last", -1)):
        bq = [93] * 4097
        if delta_at is not None:
            bq[delta_at] -= 1
        case("sum_all_93_" + nm, [read(ref, 300, 4097, bq=lambda _n, bq=bq: bq)], ref,
             lambda r, l, want=int(delta_at is None): counts(l, pile_reads=1, proposing_reads=want), min_qv=93)

    # more than 16 segments: deletions and insertions 30 apart, on segments of every parity, far beyond the sixteenth
    many_d = {p: 1 for p in range(150, 150 + 30 * 40, 60)}
    many_i = {p: "G" for p in range(180, 180 + 30 * 40, 60)}
    carrier = read(ref, 100, 2000, dels=many_d, ins=many_i)

    def segments(r, l):
        counts(l, events_proposing_reads=40, candidates=40)
        assert len(r) == 40 and all(int(x) == 1 for x in r["n_prop"])
    case("shape_many_segments", plain(ref, 11, 100, 2000) + [carrier], ref, segments, min_sequence_identity=0.9)
    # a workgroup (sixteen reads) with more than 512 staged events
    case("shape_stage_overflow", [read(ref, 100, 2000, dels=many_d, ins=many_i) for _ in range(16)], ref,
         lambda r, l: counts(l, events=640, events_proposing_reads=640, proposing_events=640, candidates=40, num_germ_homalt=40),
         min_sequence_identity=0.9)
    # the proposing read is not the allele's first carrier in read order
    case("shape_second_carrier_proposes", plain(ref, 10) + [read(ref, 900, 300, bq=low_at(q), **d), read(ref, 900, 300, **d)], ref,
         lambda r, l: (one(r, 1002, n_alt=2, n_prop=1), counts(l, num_lowbq=1)))
    # a read that yields the allele twice: C A*8 G, two deleted As six apart; one of them, then both, propose
    ref8 = C.contig(35, N, plant=[(1000, "C" + "A" * 8 + "G")])
    twice = dict(dels={1002: 1, 1007: 1})
    case("shape_allele_twice", plain(ref8, 11) + [read(ref8, 900, 300, **twice)], ref8,
         lambda r, l: (one(r, 1000, n_alt=1, n_prop=1, status=S.ST_REPEAT, run_len=8), counts(l, proposing_events=2)), max_mismatch_count=1)
    case("shape_allele_twice_one_proposes", plain(ref8, 11) + [read(ref8, 900, 300, bq=low_at(102), **twice)], ref8,
         lambda r, l: (one(r, 1000, n_alt=1, n_prop=1), counts(l, proposing_events=1, num_lowbq=1)), max_mismatch_count=1)
    # two inserted strings at one anchor
    case("shape_two_strings", plain(ref, 10) + [read(ref, 900, 300, ins={1003: "TA"}), read(ref, 900, 300, ins={1003: "TC"})], ref,
         lambda r, l: C.ok([M.unpack_bases(x) for x in at(r, 1002)] == ["TA", "TC"], all(int(x["status"]) == S.ST_INDEL for x in r)))
    # GACGTCAG at 1020: the anchor 1023 is the last position of its 256-block
    refb = C.contig(36, N, plant=[(1020, "GACGTCAG")])
    case("shape_block_edge", plain(refb, 11) + [read(refb, 900, 300, dels={1024: 3})], refb, lambda r, l: one(r, 1023, len=3, dp=12, status=S.ST_PASS))
    case("region_overlap", lone, ref, lambda r, l: (one(r, 1002), counts(l, candidates=1, events=1)),
         regions=[(900, 1002), (1002, 1100), (1000, 1005)])
    case("region_outside", lone, ref, lambda r, l: none(r, l, events=0, candidates=0, proposing_events=1), regions=[(0, 1001), (1003, N)])
    case("shape_empty_batch", [], ref, lambda r, l: none(r, l, pile_reads=0))
    return out


def table_of(kw):
    """(parameters without "table", l_hit, l_err): the arrays of himut_set_indel_error_table for the case, None without."""
    kw = dict(kw)
    cells = kw.pop("table", None)
    if cells is None:
        return kw, None, None
    e0 = kw.get("indel_error", 0.01)
    hit = [math.log10(1 - e0)] * (IC.N_CLASSES * IC.N_EVCOLS)
    err = [math.log10(e0)] * (IC.N_CLASSES * IC.N_EVCOLS)
    for (letter, n, col), e in cells.items():
        k = IC.run_class(letter, n) * IC.N_EVCOLS + col
        hit[k], err[k] = math.log10(1 - e), math.log10(e)
    return kw, hit, err


CASES = _cases()
