"""Hand-built inputs for the duplex contract (tests/duplex_model.py), shared by the CPU tests (the model against what
each rule says) and the GPU tests (the run against the model).  A case is (name, batch, mate, chunks, keyword parameters
of duplex_model.run, expect) where expect(records, ss, log-as-dict) asserts what the rule says (None: the shape alone
matters, the model is the expectation).  The reads of a molecule are named <movie>/<zmw>/ccs/fwd and .../rev, the
reverse-strand one with flag 0x10; mate[] is made from the names here, by the rule of himut_amd.duplex.mate_index."""
import random

import numpy as np

from tests import duplex_model as M
from tests.dbs_cases import A1, A2, A3, N, OPEN, REF
from tests.germline_model import make_read

# call's read filters open, the three event rules on: 5 % trimmed at either end, no other mismatch within 20 bases
KW = dict(OPEN, min_mapq=20, min_bq=20, min_trim=0.05, max_mismatch_count=0, mismatch_window_size=20)
WHOLE = [(0, N)]


def read(name, start, length, subs=(), alt=A1, bq=40, **kw):
    """A read over REF[start:start + length] with the substitutions alt[p] at the positions ``subs``."""
    return make_read(REF, start, length, {p: alt[p] for p in subs}, bq=bq, qname=name, **kw)


def mol(k, fwd, rev):
    """The two reads of molecule k: fwd and rev are (start, length, subs) or (start, length, subs, keywords of read)."""
    out = []
    for strand, spec, flag in (("fwd", fwd, 0), ("rev", rev, 0x10)):
        kw = dict(spec[3]) if len(spec) > 3 else {}
        out.append(read("m/{}/ccs/{}".format(k, strand), spec[0], spec[1], spec[2], flag=kw.pop("flag", flag), **kw))
    return out


def depth(p, n, length=300):
    """n clean reads without a mate over 0-based p."""
    return [read("bg/{}/ccs".format(p * 100 + k), max(0, p - length // 2 + 3 * k - n), length) for k in range(n)]


def pair_by_name(names, flag):
    """mate[] by the rule of duplex.mate_index, stated again: a stem pairs iff it has exactly one primary /fwd and
    exactly one primary /rev alignment."""
    stems = {}
    for i, q in enumerate(names):
        if q.endswith(("/fwd", "/rev")) and not int(flag[i]) & 0x900:
            stems.setdefault(q[:-4], {"/fwd": [], "/rev": []})[q[-4:]].append(i)
    mate = np.full(len(names), -1, np.int32)
    for s in stems.values():
        if len(s["/fwd"]) == 1 and len(s["/rev"]) == 1:
            a, b = s["/fwd"][0], s["/rev"][0]
            mate[a], mate[b] = b, a
    return mate


def build(recs, length=N, shift=0, name="chrX"):
    """(batch, mate) of the records, sorted by start; shift moves every read along the contig."""
    from himut_amd.readbatch import batch_from_records
    recs = sorted((dict(r, tstart=r["tstart"] + shift, tend=r["tend"] + shift) for r in recs), key=lambda r: r["tstart"])
    b = batch_from_records(name, length, recs)
    return b, pair_by_name(b.qnames, b.flag)


def _case(name, recs, expect=None, chunks=WHOLE, **kw):
    shift, length = kw.pop("shift", 0), kw.pop("length", N)
    b, mate = build(recs, length=length, shift=shift)
    return name, b, mate, list(chunks), dict(KW, **kw), expect


def _sites(recs):
    return [(int(r["tpos"]), chr(r["ref"]), chr(r["alt"])) for r in recs]


def cases():
    out = []

    def add(*a, **kw):
        out.append(_case(*a, **kw))

    # ---- the mates' overlap
    p = 500

    def full(recs, ss, d):
        assert _sites(recs) == [(p + 1, REF[p], A1[p])] and int(recs[0]["n_ds"]) == 1 and int(recs[0]["n_ss"]) == 0
        assert d["concordant"] == 2 and d["ds_events"] == 1 and sum(ss) == 0
        assert d["ds_bases"] == 285 - 15 + 1               # the offsets 15 .. 285 of 300 are not trimmed
    add("full_overlap", mol(0, (350, 300, [p]), (350, 300, [p])) + depth(p, 12), full)

    def partial(recs, ss, d):
        # the overlap is [1150, 1300): its first and its last base are double-strand events, the bases next to it nocover
        assert [s[0] for s in _sites(recs)] == [1151, 1300] and d["nocover"] == 2 and d["ds_events"] == 2
        assert d["ds_bases"] == 150 and d["ds_pairs_overlap"] == 1
    add("partial_overlap_edges", mol(0, (1000, 300, [1120, 1150, 1299]), (1150, 300, [1150, 1299, 1330])), partial, min_trim=0.0)

    def apart(recs, ss, d):
        assert len(recs) == 0 and d["nocover"] == 2 and d["ds_bases"] == 0 and d["ds_pairs_overlap"] == 0 and d["pairs_in_play"] == 1
    add("no_overlap", mol(0, (2000, 200, [2100]), (2300, 200, [2400])), apart)
    # overlaps of 1, 63, 64, 65 and 129 positions, nothing trimmed
    recs, want = [], 0
    for k, n in enumerate((1, 63, 64, 65, 129)):
        recs += mol(k, (600 * k + 100, 200, []), (600 * k + 300 - n, 200, []))
        want += n

    def widths(recs_, ss, d):
        assert d["ds_bases"] == want and d["ds_pairs_overlap"] == 5
    add("overlap_widths", recs, widths, min_trim=0.0)

    # ---- the mate's state
    def state(name, n_ds=0, **counts):
        def expect(recs, ss, d):
            assert len(recs) == n_ds and all(d[k] == v for k, v in counts.items()), (name, d)
        return expect
    add("mate_deletion", mol(0, (350, 300, [p]), (350, 300, [], dict(dels={p - 1: 3}))), state("del", **{"del": 1, "events": 1}))
    add("mate_insertion_in_front", mol(0, (350, 300, [p]), (350, 300, [p], dict(ins={p - 40: "ACG"}))) + depth(p, 8),
        state("ins", n_ds=1, concordant=2, ds_events=1))
    add("mate_soft_clip", mol(0, (350, 300, [p]), (350, 300, [p], dict(softclip=("ACGTACGTA", "TT")))) + depth(p, 8),
        state("clip", n_ds=1, concordant=2, ds_events=1))
    add("mate_low_bq", mol(0, (350, 300, [p]), (350, 300, [p], dict(bq_at={p: 19}))), state("lowbq", lowbq=1, num_lowbq=1, events=2))
    # p is base 5 of the reverse read (trimmed there: 5 % of 400 is 20), base 195 of the forward read
    add("mate_trimmed", mol(0, (3000, 400, [3195]), (3190, 400, [3195])), state("trim", trim=1, num_trim=1, events=2))
    add("mate_third_base", mol(0, (350, 300, [p]), (350, 300, [p], dict(alt=A2))), state("other", other=2, events=2))
    add("mate_reference", mol(0, (350, 300, [p]), (350, 300, [])), state("single", single=1, events=1, ss_events_in_chunk=1))

    # ---- candidates
    def two_molecules(recs, ss, d):
        assert [int(x) for x in recs["n_ds"]] == [2] and int(recs[0]["counts"]["ATGC".index(A1[p])]) == 4
    add("two_molecules_one_site", mol(0, (350, 300, [p]), (360, 300, [p])) + mol(1, (380, 300, [p]), (300, 300, [p])) + depth(p, 20),
        two_molecules)

    def two_sites(recs, ss, d):
        assert [s[0] for s in _sites(recs)] == [p + 1, p + 101] and [int(x) for x in recs["n_ds"]] == [1, 1]
    add("one_molecule_two_sites", mol(0, (350, 400, [p, p + 100]), (350, 400, [p, p + 100])) + depth(p + 50, 20, 400), two_sites)
    add("two_sites_in_one_window", mol(0, (350, 400, [p, p + 10]), (350, 400, [p, p + 10])), state("window", num_window=4, events=4))

    def unpaired(recs, ss, d):
        # a read without a mate and a read whose mate maps at 5 carry alt too; a read in play shows it on one strand
        assert [int(recs[0][k]) for k in ("n_ds", "n_ss", "n_alt_unpaired")] == [1, 1, 2] and d["pairs_notpile"] == 1
    add("alt_on_unpaired_reads", mol(0, (350, 300, [p]), (350, 300, [p])) + [read("lone/1/ccs", 400, 300, [p])] +
        mol(1, (420, 300, [p]), (430, 300, [], dict(mapq=5))) + mol(2, (300, 300, [p]), (310, 300, [])) + depth(p, 20), unpaired)

    def veto(recs, ss, d):
        # the reverse read has a second mismatch five bases on: its two events fail its window, the forward read's event is
        # concordant and vetoed by nothing but the mate's window
        assert len(recs) == 0 and d["num_window"] == 2 and d["concordant"] == 1 and d["num_mate_window"] == 1 and d["ds_events"] == 0
    add("vetoed_by_mates_window", mol(0, (350, 300, [p]), (350, 300, [p, p + 5])), veto)

    # ---- the single-strand spectrum: the forward read's own change, the reverse read's complemented
    q = 700

    def strands(recs, ss, d):
        want = [0] * 12
        want[M.SS_CLASSES.index(REF[p] + ">" + A1[p])] += 1
        want[M.SS_CLASSES.index(M.COMPLEMENT[REF[q]] + ">" + M.COMPLEMENT[A1[q]])] += 1
        assert list(ss) == want and d["single"] == 2
    add("single_strand_classes", mol(0, (350, 500, [p]), (350, 500, [q])), strands)

    # ---- chunks: [0, 1500) and [1500, 2000) share an edge, [2600, N) leaves a gap
    ev = [1499, 1500, 2100, 2599, 2600]
    recs = []
    for k, e in enumerate(ev):
        recs += mol(k, (e - 150, 300, [e]), (e - 140, 300, [e])) + mol(10 + k, (e - 100, 300, [e + 30]), (e - 90, 300, []))

    # (the single events sit at e + 30: 1529, 1530, 2629 and 2630 inside a chunk, 2130 in the gap)
    def chunked(recs_, ss, d):
        assert [s[0] for s in _sites(recs_)] == [1500, 1501, 2601] and d["ds_events"] == 5 and d["ds_events_in_chunk"] == 3
        assert d["single"] == 5 and sum(ss) == 4
    add("chunk_edges", recs, chunked, chunks=[(1500, 2000), (0, 1500), (2600, N)])

    # ---- past one wave's lanes: 80 substitutions and more than 160 segments in either read, the window open
    subs = list(range(1010, 3000, 25))
    dels = {s + 12: 1 for s in subs}

    def long_reads(recs_, ss, d):
        assert len(recs_) == 80 and d["ds_events"] == 80 and d["events"] == 160
    add("long_lists", mol(0, (1000, 2000, subs, dict(dels=dels)), (1000, 2000, subs, dict(dels=dels))), long_reads, max_mismatch_count=1 << 20,
        min_trim=0.0)

    # ---- call's read filters: a pair per cause (the first cause either read shows), one pair in play
    recs = mol(0, (350, 300, [p]), (350, 300, [p]))
    recs += mol(1, (350, 300, [p]), (350, 300, [p], dict(mapq=5)))                                 # not a pile read
    recs += mol(2, (350, 300, [p]), (350, 300, [p, p + 30, p + 60, p + 90, p + 120, p + 140, p - 30]))   # identity 293 / 300
    recs += mol(3, (350, 300, [p], dict(bq=24)), (350, 300, [p]))                                  # quality sum below 25 per base
    recs += mol(4, (350, 300, [p]), (440, 120, [p]))                                               # 120 bases: too short
    recs += mol(5, (350, 300, [p], dict(mapq=5)), (440, 120, [p], dict(bq=24)))                    # several causes: the first counts

    def filters(recs_, ss, d):
        assert (d["pairs"], d["pairs_in_play"], d["pairs_notpile"], d["pairs_identity"], d["pairs_lowqv"], d["pairs_qlen"]) == (6, 1, 2, 1, 1, 1)
        assert int(recs_[0]["n_ds"]) == 1 and int(recs_[0]["n_alt_unpaired"]) == 8 and d["pile_reads"] == 10 and d["proposing_reads"] == 6
    add("read_filters", recs, filters, min_sequence_identity=0.98, min_qv=25, qlen_lower_limit=150, qlen_upper_limit=1000)

    # ---- no pairs, no reads
    def lonely(recs_, ss, d):
        assert len(recs_) == 0 and d["pairs"] == 0 and d["events"] == 0 and d["reads"] == 12
    add("mate_all_minus_one", depth(p, 11) + [read("lone/0/ccs", 400, 300, [p])], lonely)

    def nothing(recs_, ss, d):
        assert len(recs_) == 0 and not any(d.values()) and not any(ss)
    add("empty_batch", [], nothing)

    # ---- the end of a 248 Mb contig
    far = 248_387_328 - N

    def chrom_end(recs_, ss, d):
        assert _sites(recs_) == [(far + 3801, REF[3800], A1[3800])] and d["ds_bases"] == 190 - 10 + 1
    add("chromosome_scale", mol(0, (3700, 200, [3800]), (3700, 200, [3800])) + depth(3800, 12, 200), chrom_end,
        shift=far, length=far + N, chunks=[(far + 3000, far + N)])
    return out


def random_case(seed, n_mol=24, n_lone=12, span=2600):
    """A seeded batch of molecules with random spans, substitutions (a third shared by both strands), insertions, deletions
    and qualities, some reads without a mate, under thresholds that bite; (batch, mate, chunks, keywords)."""
    rs = random.Random(seed)
    recs = []

    def spec(start, length, shared):
        subs = set(shared) | {rs.randrange(start, start + length) for _ in range(rs.randrange(0, 4))}
        subs = sorted(s for s in subs if start <= s < start + length)
        free = [x for x in range(start + 2, start + length - 2) if all(abs(x - s) > 3 for s in subs)]
        ins = {x: rs.choice(("A", "CG", "TTT")) for x in rs.sample(free, rs.randrange(0, 3))}
        dels = {x: rs.randrange(1, 3) for x in rs.sample(free, rs.randrange(0, 3)) if x not in ins}
        bq_at = {s: rs.choice((10, 30, 50)) for s in subs if rs.random() < 0.3}
        kw = dict(ins=ins, dels=dels, bq_at=bq_at, mapq=rs.choice((60,) * 9 + (10,)), alt=rs.choice((A1, A1, A1, A2)), bq=rs.choice((40,) * 9 + (22,)))
        return start, length, subs, kw
    for k in range(n_mol):
        s1, l1 = rs.randrange(0, span), rs.randrange(80, 700)
        s2, l2 = max(0, s1 + rs.randrange(-300, 300)), rs.randrange(80, 700)
        lo, hi = max(s1, s2), min(s1 + l1, s2 + l2)
        shared = [rs.randrange(lo, hi) for _ in range(rs.randrange(0, 5))] if lo < hi else []
        recs += mol(k, spec(s1, l1, shared), spec(s2, l2, shared))
    for k in range(n_lone):
        s, l = rs.randrange(0, span), rs.randrange(80, 700)
        st = spec(s, l, [])
        recs.append(read("lone/{}/ccs".format(k), st[0], st[1], st[2], **st[3]))
    b, mate = build(recs)
    cuts = sorted(rs.sample(range(100, N - 100), 4))
    chunks = [(0, cuts[0]), (cuts[0], cuts[1]), (cuts[2], cuts[3])]
    kw = dict(KW, min_bq=rs.choice((20, 35)), min_qv=rs.choice((0, 30)), min_sequence_identity=rs.choice((0.0, 0.97)),
              min_trim=rs.choice((0.0, 0.05)), max_mismatch_count=rs.choice((0, 1)), mismatch_window_size=rs.choice((5, 20)),
              qlen_lower_limit=rs.choice((0, 120)))
    return b, mate, chunks, kw
