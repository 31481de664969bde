"""Hand-built inputs for the rules of the dbs contract (tests/dbs_model.py), shared by the CPU tests (the model against
what each rule says) and the GPU tests (the run against the model).  A case is (name, batch, regions, keyword
parameters of dbs_model.run, expect) where expect(records, log) asserts what the rule says."""
import random

from tests import dbs_model as M

OPEN = dict(min_qv=0, min_mapq=0, min_sequence_identity=0.0, qlen_lower_limit=0, qlen_upper_limit=1 << 20, min_gq=20, min_bq=20,
            min_trim=0.0, max_mismatch_count=1 << 20, mismatch_window_size=20, md_threshold=1 << 30, min_ref_count=3,
            min_alt_count=1, min_hap_count=3)
N = 4000


def contig(n=N, seed=3):
    """(ref, a1, a2, a3): a random contig and per position its three other bases, in a fixed rotation."""
    rs = random.Random(seed)
    ref = "".join(rs.choice("ATGC") for _ in range(n))
    rot = [{p: "ATGC"[("ATGC".index(ref[p]) + k) % 4] for p in range(n)} for k in (1, 2, 3)]
    return ref, rot[0], rot[1], rot[2]


REF, A1, A2, A3 = contig()


def batch(recs, ref=REF, name="chrD"):
    from himut_amd.readbatch import batch_from_records
    return batch_from_records(name, len(ref), sorted(recs, key=lambda r: r["tstart"]))


def pile(p, n=12, carriers=1, length=300, bq=93, step=7, alt=(A1, A1), carrier_kw=None, other_subs=None, other_bq=20, **kw):
    """n reads over 0-based p and p + 1, the first `carriers` of them with the doublet (alt[0][p], alt[1][p + 1]); read k
    of the others carries other_subs[k], at quality other_bq.  (One substituted read of quality 93 in twelve leaves the
    column homref under the reference's arithmetic, two in ten do not: an error costs 3.1, a het read 0.3, the prior 3.)"""
    out = []
    for k in range(n):
        start = max(0, p - length // 2 + step * k - step * n // 2)
        if k < carriers:
            out.append(M.make_read(REF, start, length, {p: alt[0][p], p + 1: alt[1][p + 1]}, **dict(dict(kw, bq=bq), **(carrier_kw or {}))))
        else:
            subs = dict((other_subs or {}).get(k, {}))
            out.append(M.make_read(REF, start, length, subs, bq=bq, bq_at={x: other_bq for x in subs}, **kw))
    return out


def tposes(recs):
    return [int(x) for x in recs["tpos"]]


def status_of(recs):
    return [(M.STATUS[int(r["status"])], M.STATUS[int(r["half_status"][0])], M.STATUS[int(r["half_status"][1])]) for r in recs]


def _case(name, reads, expect, regions=((1, N),), pon=(), com=(), **kw):
    return name, batch(reads), [tuple(r) for r in regions], dict(dict(OPEN, **kw), pon_keys=list(pon), com_keys=list(com)), expect


def _key(tpos, ref, alt):
    return (tpos << 4) | ("ATGC".index(ref) << 2) | "ATGC".index(alt)


def rule_cases():
    """The cases of the doublet definition and the per-read rules."""
    out = []

    def add(*a, **kw):
        out.append(_case(*a, **kw))

    # a run of three gives no doublet and is counted once
    r = pile(500, carriers=0) + [M.make_read(REF, 400, 300, {500: A1[500], 501: A1[501], 502: A1[502]}, bq=93)]
    add("run_of_three", r, lambda recs, log: (len(recs), log[1], log[2]) == (0, 0, 1) or _fail(recs, log))
    # *ac*gt:1*ac*gt: two doublets one match apart
    r = pile(500, carriers=0) + [M.make_read(REF, 400, 300, {500: A1[500], 501: A1[501], 503: A1[503], 504: A1[504]}, bq=93)]
    add("two_doublets_one_apart", r, lambda recs, log: (tposes(recs), log[1], log[2]) == ([501, 504], 2, 0) or _fail(recs, log))
    # an insertion between the two bases: two entries that are not consecutive
    r = pile(500, carriers=0) + [M.make_read(REF, 400, 300, {500: A1[500], 501: A1[501]}, ins={501: "AC"}, bq=93)]
    add("insertion_between", r, lambda recs, log: (len(recs), log[1]) == (0, 0) or _fail(recs, log))
    # an insertion in front: the entry in front is no substitution; the first half's column holds the insertion
    r = pile(500, carriers=0) + [M.make_read(REF, 400, 300, {500: A1[500], 501: A1[501]}, ins={500: "AC"}, bq=93)]
    add("insertion_in_front", r, lambda recs, log: (tposes(recs), log[1]) == ([501], 1) and status_of(recs)[0][:2] == ("IndelSite", "IndelSite")
        or _fail(recs, log))
    # a deletion next to the doublet, behind and in front
    r = pile(500, carriers=0) + pile(900, carriers=0) + [M.make_read(REF, 400, 300, {500: A1[500], 501: A1[501]}, dels={502: 2}, bq=93),
                                                         M.make_read(REF, 800, 300, {900: A1[900], 901: A1[901]}, dels={898: 2}, bq=93)]
    add("deletion_next_to", r, lambda recs, log: (tposes(recs), log[1], status_of(recs)[0][0]) == ([501, 901], 2, "PASS") or _fail(recs, log))
    # N as the reference base of a neighbour: left out of the list, so the run is a run of two
    r = pile(500, carriers=0) + [M.make_read(REF, 400, 300, {499: A1[499], 500: A1[500], 501: A1[501]}, nref=(499,), bq=93),
                                 M.make_read(REF, 410, 300, {500: A2[500], 501: A2[501], 502: A2[502]}, nref=(502,), bq=93)]
    add("n_reference_neighbour", r, lambda recs, log: (tposes(recs), log[1], log[2]) == ([501, 501], 2, 0) or _fail(recs, log))
    # a doublet whose own first base names N: one substitution is left, no doublet
    r = pile(500, carriers=0) + [M.make_read(REF, 400, 300, {500: A1[500], 501: A1[501]}, nref=(500,), bq=93)]
    add("n_reference_own", r, lambda recs, log: (len(recs), log[1]) == (0, 0) or _fail(recs, log))
    # trim: qpos passes and qpos + 1 fails (and the mirror image at the front of the read)
    qlen, t = 300, 0.1
    q_hi = max(q for q in range(qlen) if not M.is_trimmed(q, qlen, t))
    q_lo = min(q for q in range(qlen) if not M.is_trimmed(q, qlen, t))
    assert M.is_trimmed(q_hi + 1, qlen, t) and M.is_trimmed(q_lo - 1, qlen, t) and q_lo > 1
    r = []
    for p, q in ((600, q_hi), (1000, q_hi - 1), (1400, q_lo - 1), (1800, q_lo)):
        r += pile(p, carriers=0) + [M.make_read(REF, p - q, qlen, {p: A1[p], p + 1: A1[p + 1]}, bq=93)]
    add("trim", r, lambda recs, log: (tposes(recs), log[1], log[3]) == ([1001, 1801], 4, 2) or _fail(recs, log), min_trim=t)
    # a leading soft clip counts in qpos: the clipped read's doublet is inside the trimmed range, the bare read's is not
    r = pile(600, carriers=0) + pile(1000, carriers=0)
    r += [M.make_read(REF, 598, 100, {600: A1[600], 601: A1[601]}, bq=93, softclip=("ACGTACGTAC", "")),
          M.make_read(REF, 998, 100, {1000: A1[1000], 1001: A1[1001]}, bq=93)]
    add("leading_soft_clip", r, lambda recs, log: (tposes(recs), log[3]) == ([601], 1) or _fail(recs, log), min_trim=0.05)
    # each branch of get_mismatch_range, a third mismatch on the window's last position inside and first position outside
    w, qlen = 20, 200
    r, want = [], []
    for p, q, off, inside in ((300, 100, 22, False), (500, 100, 21, True), (700, 100, -21, False), (900, 100, -20, True),      # middle
                              (1100, 5, 36, False), (1300, 5, 35, True), (1500, 5, -5, True),                                  # qstart < 0
                              (1700, 190, -31, False), (1900, 190, -30, True), (2100, 190, 9, True)):                          # qend > qlen
        s1, e1 = M.get_mismatch_range(p + 1, q, qlen, w)
        s2, e2 = M.get_mismatch_range(p + 2, q + 1, qlen, w)
        assert (min(s1, s2) <= p + off + 1 <= max(e1, e2)) == inside, (p, q, off)
        r += pile(p, carriers=0, length=400) + [M.make_read(REF, p - q, qlen, {p: A1[p], p + 1: A1[p + 1], p + off: A1[p + off]}, bq=93)]
        if not inside:
            want.append(p + 1)
    add("mismatch_range_branches", r, lambda recs, log, want=want: (tposes(recs), log[4]) == (want, 10 - len(want)) or _fail(recs, log),
        max_mismatch_count=0, mismatch_window_size=w)
    # an indel inside the window counts as a substitution does
    r = pile(500, carriers=0, length=400) + [M.make_read(REF, 400, 200, {500: A1[500], 501: A1[501]}, dels={510: 1}, bq=93)]
    add("window_counts_indels", r, lambda recs, log: (len(recs), log[4]) == (0, 1) or _fail(recs, log), max_mismatch_count=0)
    # read filters: each one removes the proposer, the pile keeps the read
    for name, ckw, kw in (("filter_mapq", dict(mapq=10), dict(min_mapq=20)), ("filter_qv", dict(), dict(min_qv=94)),
                          ("filter_identity", dict(), dict(min_sequence_identity=0.995)), ("filter_qlen", dict(), dict(qlen_upper_limit=300)),
                          ("filter_secondary", dict(flag=0x100), dict())):
        r = pile(500, carriers=1, mapq=60, carrier_kw=ckw)
        add(name, r, lambda recs, log: (len(recs), log[1]) == (0, 0) or _fail(recs, log), **kw)
    # a supplementary alignment is a read of its own
    r = pile(500, n=14, carriers=2, mapq=60, carrier_kw=dict(flag=0x800))
    add("supplementary_proposes", r, lambda recs, log: (tposes(recs), int(recs[0]["n_proposers"])) == ([501], 2) or _fail(recs, log),
        min_gq=0)
    return out


def verdict_cases():
    """Each verdict, the order of precedence between the halves, the joint counts."""
    out = []
    X = {500: A2[500], 501: A2[501]}

    def add(name, reads, want, check=None, **kw):
        def expect(recs, log, want=want, check=check):
            assert status_of(recs) == want, (status_of(recs), want, log)
            assert all(log[7 + M.VERDICTS.index(s[0])] >= 1 for s in want) and sum(log[7:18]) == len(recs)
            if check:
                check(recs, log)
        out.append(_case(name, reads, expect, **kw))

    def joint(both_alt, both_ref, one_alt, n_prop):
        def check(recs, log):
            r = recs[0]
            assert (int(r["both_alt"]), int(r["both_ref"]), int(r["one_alt"]), int(r["n_proposers"])) == (both_alt, both_ref, one_alt, n_prop), r
        return check
    add("pass", pile(500), [("PASS", "PASS", "PASS")], joint(1, 11, 0, 1))
    # a read carrying one half only: one_alt; it proposes nothing
    one = {9: {500: A1[500]}}
    add("one_alt", pile(500, other_subs=one), [("PASS", "PASS", "PASS")], joint(1, 10, 1, 1))
    # the halves pass on their own counts, the joint counts do not
    halves = {8: {500: A1[500]}, 9: {501: A1[501]}}
    add("low_depth_joint_alt", pile(500, other_subs=halves), [("LowDepth", "PASS", "PASS")], joint(1, 9, 2, 1), min_alt_count=2)
    halves = {10: {500: A2[500]}, 11: {501: A2[501]}}
    add("low_depth_joint_ref", pile(500, other_subs=halves), [("LowDepth", "PASS", "PASS")], joint(1, 9, 0, 1), min_ref_count=10)
    add("low_depth_halves", pile(500, n=3, carriers=1), [("LowDepth", "LowDepth", "LowDepth")], joint(1, 2, 0, 1), min_gq=0)
    add("high_depth", pile(500, n=14), [("HighDepth", "HighDepth", "HighDepth")], md_threshold=12)
    add("low_bq_second_half", pile(500, carrier_kw=dict(bq_at={501: 19})), [("LowBQ", "PASS", "LowBQ")])
    add("low_gq", pile(500, n=4, carriers=1), [("LowGQ", "LowGQ", "LowGQ")], min_gq=99)
    add("indel_first_half", pile(500, other_subs={}) + [M.make_read(REF, 380, 300, dels={500: 1}, bq=93)], [("IndelSite", "IndelSite", "PASS")])
    add("pon_second_half", pile(500), [("PanelOfNormal", "PASS", "PanelOfNormal")], pon=[_key(502, REF[501], A1[501])])
    add("com_first_half", pile(500), [("ComSnp", "ComSnp", "PASS")], com=[_key(501, REF[500], A1[500]), _key(501, REF[500], A2[500])])
    # germline states of a half that are not the doublet's own alleles
    het = {k: {500: A2[500]} for k in range(1, 7)}
    add("het_first_half", pile(500, other_subs=het, other_bq=93), [("HetSite", "HetSite", "PASS")])
    hom = {k: {501: A2[501]} for k in range(1, 12)}
    add("homalt_second_half", pile(500, n=12, carriers=1, other_subs=hom), [("HomAltSite", "PASS", "HomAltSite")], min_ref_count=0)
    hetalt = {k: {500: (A2 if k % 2 else A3)[500]} for k in range(1, 13)}
    add("hetalt_first_half", pile(500, n=13, other_subs=hetalt, other_bq=93), [("HetAltSite", "HetAltSite", "PASS")], min_ref_count=0)
    # the doublet itself is germline: both halves het with the doublet's alleles, no record
    def germ(recs, log):
        assert (len(recs), log[5], log[6]) == (0, 1, 1), log
    out.append(_case("germline_doublet", pile(500, n=12, carriers=6), germ))
    out.append(_case("germline_one_half", pile(500, n=12, carriers=1, other_subs={k: {501: A1[501]} for k in range(1, 7)}), germ))
    # precedence: the verdict that comes first in the order, whichever half holds it; the first half on a tie
    add("precedence_het_over_lowbq", pile(500, carrier_kw=dict(bq_at={500: 19}), other_subs={k: {501: A2[501]} for k in range(1, 7)}, other_bq=93),
        [("HetSite", "LowBQ", "HetSite")])
    add("precedence_lowbq_over_pon", pile(500, carrier_kw=dict(bq_at={501: 19})), [("LowBQ", "PanelOfNormal", "LowBQ")],
        pon=[_key(501, REF[500], A1[500])])
    add("precedence_pon_over_com", pile(500), [("PanelOfNormal", "ComSnp", "PanelOfNormal")], com=[_key(501, REF[500], A1[500])],
        pon=[_key(502, REF[501], A1[501])])
    add("precedence_indel_over_lowdepth", pile(500, n=2, carriers=1) + [M.make_read(REF, 380, 300, dels={501: 1}, bq=93)],
        [("IndelSite", "LowDepth", "IndelSite")], min_gq=0)
    # two alt pairs at one position: two candidates, in ATGC order of the alt alleles
    two = pile(500, carrier_kw=dict(bq=30)) + pile(500, n=1, bq=30, alt=(A2, A3)) + pile(500, n=1, bq=30, alt=(A1, A2))

    def pairs(recs, log):
        got = [("ATGC".index(chr(r["alt"][0])), "ATGC".index(chr(r["alt"][1]))) for r in recs]
        assert got == sorted(got) and len(set(got)) == 3 and tposes(recs) == [501] * 3 and log[5] == 3, (got, log)
    out.append(_case("two_alt_pairs", two, pairs, min_gq=0))
    return out


def shape_cases():
    """The shapes at which the kernels can go wrong (the model does not care)."""
    out = []

    def add(name, reads, want_tpos, regions=((1, N),), **kw):
        out.append(_case(name, reads, lambda recs, log, want=want_tpos: tposes(recs) == want or _fail(recs, log), regions=regions, **kw))
    # a doublet on either side of a 256-position block boundary, reads that end at it and reads that start at it: two
    # windows; carriers that start in different blocks name the same candidate
    r = [M.make_read(REF, 100 + 5 * k, 156 - 5 * k, bq=93) for k in range(6)]                       # end at 256: cover rpos 255 only
    r += [M.make_read(REF, 256, 200 + k, bq=93) for k in range(5)]                                  # start at 256
    r += [M.make_read(REF, 30, 400, {255: A1[255], 256: A1[256]}, bq=30), M.make_read(REF, 250, 400, {255: A1[255], 256: A1[256]}, bq=30)]
    r += [M.make_read(REF, 200 + 3 * k, 300, bq=93) for k in range(4)]
    add("block_boundary", r, [256])
    # tpos = 1 and the contig's last two positions
    r = [M.make_read(REF, 0, 200 + k, {0: A1[0], 1: A1[1]} if k < 1 else {}, bq=93) for k in range(8)]
    r += [M.make_read(REF, N - 200 - k, 200 + k, {N - 2: A1[N - 2], N - 1: A1[N - 1]} if k < 1 else {}, bq=93) for k in range(8)]
    add("contig_ends", r, [1, N - 1])
    # more than 64 mismatch entries, doublets on entries 15/16 and 63/64 (single substitutions two apart in between)
    subs, p, e, at = {}, 1000, 0, {}
    while e < 70:
        subs[p] = A1[p]
        if e in (15, 63):
            subs[p + 1] = A1[p + 1]
            at[e] = p
            e, p = e + 1, p + 1
        e, p = e + 1, p + 2
    first, second = at[15], at[63]
    r = [M.make_read(REF, 900 + 3 * k, 400, bq=93) for k in range(8)] + [M.make_read(REF, 950, 400, subs, bq=93)]
    add("entries_across_the_group_loop", r, [first + 1, second + 1])
    # a column deeper than a wave and than the in-flight batch
    add("deep_column", pile(2000, n=70, carriers=3, step=1), [2001])
    # more than 256 keys; the two proposers of one candidate sit on either side of key 256
    r = []
    for s in range(130):
        p = 300 + 25 * s
        r += [M.make_read(REF, p - 100 + k, 200, {p: A1[p], p + 1: A1[p + 1]} if k < 2 else {}, bq=30) for k in range(6)]
    add("keys_across_workgroups", r, [301 + 25 * s for s in range(130)])
    # regions: overlapping, abutting, out of order; a region that holds tpos + 1 and not tpos reports nothing
    r = pile(500) + pile(900) + pile(1300)
    add("regions_mixed", r, [501, 901], regions=((880, 1000), (400, 501), (501, 700), (450, 600), (1302, 1400), (2000, 2100)))
    add("regions_exclude_tpos", r, [], regions=((502, 800), (902, 1300)))
    add("regions_tpos_at_edges", r, [501, 901, 1301], regions=((501, 501), (1301, 1301), (600, 901)))
    return out


def order_cases():
    """Where the order of the records can go wrong across the eval kernel's workgroups of 256 sorted keys."""
    # one candidate proposed by 560 reads between two proposed by one read each: its run of equal keys is keys 1 .. 560,
    # the end of workgroup 0, all of workgroup 1 (which emits nothing) and the start of workgroup 2.  (A carrier of
    # quality 1 says next to nothing about its base: with 40 reference reads of quality 93 both halves stay homref.)
    r = pile(1000) + pile(2000, n=600, carriers=560, step=0, carrier_kw=dict(bq=1)) + pile(3000)

    def expect(recs, log):
        assert tposes(recs) == [1001, 2001, 3001] and [int(x) for x in recs["n_proposers"]] == [1, 560, 1], (recs, log)
    return [_case("deep_key_run", r, expect)]


def _fail(recs, log):
    raise AssertionError((recs, log))
