"""Hand-built phased alignments for `call --phase` and `normcounts --phase`: one case per rule of the read's haplotype
(haplib.get_ccs_hap: k_read_hap) and of the haplotype vote (caller.py:552-603: k_eval_columns<true>, by column row and by
query name), and per shape at which the kernels can go wrong.  A case is (name, batch, chunks, phase sets, contig string,
parameter overrides, expect(records, log), tpos): `records` are the reference's twelve-field tuples, `log` its fifteen
counters, `tpos` the candidate a vote case decides (None where the case has none).  The haplotypes cannot be read back,
so every case makes the haplotype of its subject read decide something that can: the subject proposes the candidate (a
record if it is phased, none and one read fewer in num_ccs if not), or it is the reference-allele read that brings its
haplotype to min_hap_count (PASS against Unphased).

tests/golden/phase_edges.json holds what the reference gives for every case; the CPU tests check the oracle and
`expect` against it, the GPU tests the HIP run against the oracle, the golden and `expect`."""
from collections import namedtuple

import numpy as np

from himut_amd.readbatch import batch_from_records
from tests import util

N = 40960                 # a multiple of 256: the base behind the contig's last base is in no 256-block
CONTIG = "chrP"
BQ = 93
ALT = {"A": "C", "C": "G", "G": "T", "T": "A"}        # the alternative allele of a hetSNP and of a candidate
THIRD = {"A": "G", "C": "T", "G": "A", "T": "C"}      # an allele that is neither
FREE = (100, 700)         # no case puts a read or a chunk here: room for a pair of reads that only share a name

Case = namedtuple("Case", "name batch chunks phase_sets refseq overrides expect tpos")

PARAMS = dict(util.CALL_DEFAULTS, qlen_lower_limit=10, qlen_upper_limit=100_000, md_threshold=1000)


def params_of(case):
    p = dict(PARAMS)
    p.update(case.overrides)
    return p


def contig(seed, n=N):
    rs = np.random.RandomState(seed)
    return "".join("ACGT"[k] for k in rs.randint(0, 4, n))


def read(ref, start, length, subs=None, dels=None, ins=None, clip=0, flag=0, mapq=60, qname=None):
    """A read record over ref[start:start + length].  subs {pos: base}, dels {pos: length}, ins {pos: bases in front of
    pos}, all 0-based reference positions; a substitution inside a deletion is dropped.  clip: soft-clipped bases in front."""
    subs, dels, ins = subs or {}, dels or {}, ins or {}
    end = start + length
    seq, cs = [], []
    run = 0
    p = start

    def flush():
        nonlocal run
        if run:
            cs.append(":{}".format(run))
            run = 0
    for pos in sorted(set(subs) | set(dels) | set(ins)):
        if pos < p:
            assert pos in subs and pos not in dels and pos not in ins, pos    # a hetSNP inside a deletion
            continue
        assert start <= pos < end, (pos, start, end)
        seq.append(ref[p:pos])
        run += pos - p
        p = pos
        if pos in ins:
            assert pos > start and pos not in dels
            flush()
            cs.append("+" + ins[pos].lower())
            seq.append(ins[pos])
        if pos in dels:
            assert pos > start and pos + dels[pos] < end
            flush()
            cs.append("-" + ref[pos:pos + dels[pos]].lower())
            p = pos + dels[pos]
        elif pos in subs:
            assert subs[pos] != ref[pos]
            flush()
            cs.append("*" + ref[pos].lower() + subs[pos].lower())
            seq.append(subs[pos])
            p = pos + 1
    seq.append(ref[p:end])
    run += end - p
    flush()
    s = "ACGT" * (clip // 4) + "ACGT"[:clip % 4] + "".join(seq)
    rec = dict(tstart=start, tend=end, qstart=clip, seq=s, bq=[BQ] * len(s), cs="".join(cs), flag=flag, mapq=mapq)
    if qname is not None:
        rec["qname"] = qname
    return rec


def batch(records):
    """Coordinate sorted, as a BAM is; reads without a name get one of their own."""
    records = sorted((dict(r) for r in records), key=lambda r: r["tstart"])     # (copies: a record may serve several cases)
    for i, r in enumerate(records):
        r.setdefault("qname", "ccs/{}".format(i))
    return batch_from_records(CONTIG, N, records)


class Locus:
    """One phase set: hetSNPs at the 1-based positions `hpos`, `gts` the first GT field of each (random where not given).
    Haplotype 0 shows the reference allele where that field is 0, haplotype 1 where it is 1."""

    def __init__(self, ref, hpos, gts=None, seed=0, alleles=None):
        self.ref, self.hpos = ref, [int(p) for p in hpos]
        if gts is None:
            gts = "".join("01"[k] for k in np.random.RandomState(1000 + seed).randint(0, 2, len(self.hpos)))
        assert len(gts) == len(self.hpos)
        self.hbit = list(gts)
        self.hetsnp = [(p, ref[p - 1], ALT[ref[p - 1]]) for p in self.hpos]
        for i, (r, a) in (alleles or {}).items():       # VCF alleles of more than one base
            self.hetsnp[i] = (self.hpos[i], r, a)
        self.key = str(self.hpos[0])
        self.chunk = (self.hpos[0], self.hpos[-1])

    def p0(self, i):
        """0-based position of hetSNP i."""
        return self.hpos[i] - 1

    def shows(self, i, h):
        _, r, a = self.hetsnp[i]
        return r[0] if (self.hbit[i] == "0") == (h == 0) else a[0]

    def subs(self, h, start, end, flip=(), third=()):
        """What a read of haplotype h over [start, end) differs in from the contig: `flip` lists hetSNP indices at which
        it shows the other haplotype's allele, `third` those at which it shows a third allele."""
        out = {}
        for i, p in enumerate(self.hpos):
            if start < p <= end:
                b = THIRD[self.ref[p - 1]] if i in third else self.shows(i, h ^ (1 if i in flip else 0))
                if b != self.ref[p - 1]:
                    out[p - 1] = b
        return out

    def read(self, h, start, length, flip=(), third=(), subs=None, **kw):
        s = self.subs(h, start, start + length, flip, third)
        s.update(subs or {})
        return read(self.ref, start, length, subs=s, **kw)

    def bg(self, at, n0, n1, length=1000, before=500, **kw):
        """n0 + n1 clean reads of haplotype 0 / 1 over the position `at`."""
        return [self.read(h, at - before, length, **kw) for h, n in ((0, n0), (1, n1)) for _ in range(n)]

    def index_shown(self, h, want_alt, lo, hi):
        """The first hetSNP index in [lo, hi) at which haplotype h shows the alternative (want_alt) / reference allele."""
        for i in range(lo, hi):
            if (self.shows(i, h) != self.ref[self.p0(i)]) == want_alt:
                return i
        raise AssertionError("no such hetSNP")


def phase_sets(*loci):
    return ({L.key: list(L.hbit) for L in loci}, {L.key: list(L.hpos) for L in loci}, {L.key: list(L.hetsnp) for L in loci})


def som(ref, p):
    return {p: ALT[ref[p]]}


# ---- what a case states about the reference's (and the HIP run's) output

def at(records, tpos):
    return [r for r in records if r[1] == tpos]


def is_status(records, tpos, status, ps=None, **fields):
    """Exactly one record at tpos, with this status (and phase set, depth, ref_count, alt_count)."""
    rs = at(records, tpos)
    assert len(rs) == 1, (tpos, rs)
    r = rs[0]
    assert r[4] == status, r
    assert r[11] == (ps if status == "PASS" else "."), r
    idx = dict(depth=7, ref_count=8, alt_count=9)
    for k, v in fields.items():
        assert r[idx[k]] == v, (k, r)
    return r


def none_at(records, tpos):
    assert at(records, tpos) == [], at(records, tpos)


def _cases():
    out = []
    names = set()

    def case(name, recs, loci, expect, tpos=None, **overrides):
        assert name not in names, name
        names.add(name)
        loci = loci if isinstance(loci, (list, tuple)) else [loci]
        for r in recs:
            assert r["tend"] <= N and (r["tend"] <= FREE[0] or r["tstart"] >= FREE[1])
        out.append(Case(name, batch(recs), [L.chunk for L in loci], phase_sets(*loci), loci[0].ref, overrides, expect, tpos))

    # ------------------------------------------------------------------------------------------------------------
    # The haplotype of one read X.  `x(subs)` builds it with further substitutions, `h` is the haplotype it was built
    # from, `phased` what the rule says it gets.  Two cases each: X proposes the candidate (a record only if it is
    # phased; else one read fewer in num_ccs), and X is the reference-allele read that brings haplotype h to
    # min_hap_count = 3 (PASS only if X votes for h).
    def hap(name, L, x, h, phased, c0, counted=True, before=500, **ov):
        tpos = c0 + 1
        ref = L.ref

        def proposes(r, l):
            if phased:
                is_status(r, tpos, "PASS", L.key, depth=9.0, ref_count=8.0, alt_count=1.0)
                assert l[0] == 9, l
            else:
                none_at(r, tpos)
                assert l[0] == 8, l
        case("hap_" + name + "_proposes", L.bg(c0, 4, 4, before=before) + [x(som(ref, c0))], L, proposes, tpos, **ov)

        def tips(r, l):
            is_status(r, tpos, "PASS" if phased else "Unphased", L.key, ref_count=7.0 if counted else 6.0, alt_count=1.0)
        bgr = [L.read(0, c0 - min(450, before), 1000, third={i for i in range(len(L.hpos))})]     # unphased: for the genotype quality
        bgr += L.bg(c0, 2 if h == 0 else 3, 3 if h == 0 else 2, before=before) + [L.read(h, c0 - min(400, before), 1000, subs=som(ref, c0))]
        case("hap_" + name + "_tips", bgr + [x(None)], L, tips, tpos, **ov)

    ref = contig(1)
    L60 = Locus(ref, [5000 + 100 * i for i in range(60)], seed=1)
    I0 = 5

    def span(L, i0, k, c0):
        """A read over exactly the hetSNPs i0 .. i0 + k - 1 and the two bases at c0."""
        start = L.p0(i0) - 30
        end = max(L.hpos[i0 + k - 1] + 30, c0 + 31)
        return start, end - start

    # hetSNPs under the read: 1 is too few, 2 is enough; at 17, 33 and 48 the one disagreeing hetSNP takes every place
    # at which the sixteen lanes turn
    c0 = L60.p0(I0) + 50
    for k in (1, 2, 15, 16, 17, 31, 32, 33, 48):
        s, n = span(L60, I0, k, c0)
        ov = dict(min_sequence_identity=0.95) if k <= 2 else {}
        hap("count_{}".format(k), L60, lambda subs, s=s, n=n: L60.read(0, s, n, subs=subs), 0, k >= 2, c0, **ov)
        for j in (15, 16, 31, 32, 47):
            if k in (17, 33, 48) and j < k:
                hap("count_{}_off_{}".format(k, j), L60, lambda subs, s=s, n=n, j=j: L60.read(1, s, n, flip={I0 + j}, subs=subs),
                    1, False, c0)

    # the size of the whole set: the counted bisect runs over all of it
    for size in (2, 16, 17):
        Ls = Locus(ref, [5000 + 100 * i for i in range(size)], seed=10 + size)
        c0s = Ls.p0(0) + 50
        s, n = Ls.p0(0) - 300, 100 * size + 500
        hap("set_{}".format(size), Ls, lambda subs, Ls=Ls, s=s, n=n: Ls.read(1, s, n, subs=subs), 1, True, c0s)
        if size > 2:
            hap("set_{}_last_off".format(size), Ls, lambda subs, Ls=Ls, s=s, n=n: Ls.read(0, s, n, flip={size - 1}, subs=subs),
                0, False, c0s)
    L300 = Locus(ref, [5000 + 100 * i for i in range(300)], seed=3)
    for i0, k in ((137, 5), (160, 3), (283, 2)):
        c0s = L300.p0(i0) + 50
        s, n = span(L300, i0, k, c0s)
        ov = dict(min_sequence_identity=0.95)
        hap("set_300_from_{}".format(i0), L300, lambda subs, s=s, n=n: L300.read(i0 & 1, s, n, subs=subs), i0 & 1, True, c0s, **ov)
        hap("set_300_from_{}_off".format(i0), L300, lambda subs, s=s, n=n, i0=i0, k=k: L300.read(0, s, n, flip={i0 + k - 1}, subs=subs),
            0, False, c0s, **ov)

    # the read's ends: 1-based position tstart is out, tstart + 1 (the first base) in, tend (the last base) in, tend + 1 out;
    # once as the hetSNP that makes two, once as the only one that disagrees
    c0 = L60.p0(20) + 50
    for nm, lo, hi, in_ in (("start_out", L60.hpos[19], L60.hpos[20] + 80, False), ("start_in", L60.hpos[19] - 1, L60.hpos[20] + 80, True),
                            ("end_in", L60.p0(20) - 30, L60.hpos[21], True), ("end_out", L60.p0(20) - 30, L60.hpos[21] - 1, False)):
        hap("edge_" + nm + "_second", L60, lambda subs, lo=lo, hi=hi: L60.read(0, lo, hi - lo, subs=subs), 0, in_, c0,
            min_sequence_identity=0.95)
    for nm, lo, hi, fl, in_ in (("start_out", L60.hpos[18], L60.hpos[20] + 80, 18, False), ("start_in", L60.hpos[18] - 1, L60.hpos[20] + 80, 18, True),
                                ("end_in", L60.p0(19) - 30, L60.hpos[21], 21, True), ("end_out", L60.p0(19) - 30, L60.hpos[21] - 1, 21, False)):
        hap("edge_" + nm + "_off", L60, lambda subs, lo=lo, hi=hi, fl=fl: L60.read(1, lo, hi - lo, flip={fl}, subs=subs), 1, not in_, c0,
            min_sequence_identity=0.95)

    # what the read shows at one hetSNP of six (indices 30 .. 35; the candidate behind 32)
    c0 = L60.p0(32) + 50
    s, n = span(L60, 30, 6, c0)
    i_alt, i_ref = L60.index_shown(0, True, 33, 36), L60.index_shown(0, False, 33, 36)

    def shown(nm, phased, extra=None, **kw):
        hap("shows_" + nm, L60, lambda subs: L60.read(0, s, n, subs={**(extra or {}), **(subs or {})}, **kw), 0, phased, c0,
            min_sequence_identity=0.95)
    shown("clean", True)
    shown("ref_for_alt", False, flip={i_alt})
    shown("alt_for_ref", False, flip={i_ref})
    shown("third_allele", False, third={i_ref})
    shown("third_allele_for_alt", False, third={i_alt})
    shown("deleted", False, dels={L60.p0(34): 1})
    shown("deleted_inside", False, dels={L60.p0(34) - 2: 5})
    shown("behind_insertion", True, ins={L60.p0(34): "GATTA"})
    shown("behind_insertion_off", False, ins={L60.p0(i_ref): "GATTA"}, flip={i_ref})
    # the first and the last base of a match segment, between two substitutions
    p = L60.p0(i_ref)
    shown("segment_first_last", True, extra={p - 1: THIRD[ref[p - 1]], p + 1: THIRD[ref[p + 1]]})
    shown("segment_first", True, extra={p - 1: THIRD[ref[p - 1]]})
    shown("segment_last", True, extra={p + 1: THIRD[ref[p + 1]]})
    shown("behind_deletion", True, dels={L60.p0(34) - 3: 3})
    shown("before_deletion", True, dels={L60.p0(34) + 1: 3})
    shown("soft_clip", True, clip=37)
    shown("soft_clip_off", False, clip=37, flip={i_alt})
    shown("soft_clip_behind_deletion", True, clip=5, dels={L60.p0(34) - 3: 3, L60.p0(31) + 7: 2})
    # VCF alleles of more than one base at hetSNP 30: a two-base ref is no read's base, so only the alt can match, and
    # the other way round.  The background reads start behind hetSNP 30.
    r30 = ref[L60.p0(30)]
    for nm, alle in (("long_ref", (r30 + "G", ALT[r30])), ("long_alt", (r30, ALT[r30] + "G"))):
        for g in "01":
            gts = "".join(L60.hbit[:30]) + g + "".join(L60.hbit[31:])
            La = Locus(ref, L60.hpos, gts=gts, alleles={30: alle})
            for h in (0, 1):
                ok = (La.shows(30, h) != r30) == (nm == "long_ref")      # the read shows the allele of one base
                hap("shows_{}_gt{}_hap{}".format(nm, g, h), La, lambda subs, La=La, h=h: La.read(h, s, n, subs=subs), h, ok, c0, before=150)

    # the segment search: 1, 2, 3 and more than 200 segments, hetSNPs in the first, a middle and the last one.  The set's
    # fields are all 0, so a clean haplotype 0 read is one match segment.
    Lz = Locus(ref, [5000 + 100 * i for i in range(60)], gts="0" * 60)
    c0 = Lz.p0(10) + 50
    s, n = span(Lz, 10, 3, c0)

    def segs(nm, phased, h=0, i0=10, k=3, **kw):
        s_, n_ = span(Lz, i0, k, c0)
        hap("segments_" + nm, Lz, lambda subs: Lz.read(h, s_, n_, subs=subs, **kw), h, phased, c0,
            min_sequence_identity=0.9)
    segs("1", True)
    segs("2", True, ins={Lz.p0(11) - 20: "TT"})                       # match, insertion, match
    segs("2_first_off", False, ins={Lz.p0(11) - 20: "TT"}, flip={10})
    segs("3", True, dels={Lz.p0(11) - 20: 2})                         # match, deletion, match
    segs("3_middle", False, dels={Lz.p0(11): 1})                      # the deletion holds the hetSNP
    segs("3_last_off", False, dels={Lz.p0(11) - 20: 2}, third={12})
    many = {Lz.p0(i) + d: 1 for i in range(10, 57) for d in (5, 25, 78)}      # 141 deletions: 283 segments and more
    segs("many", True, h=1, k=48, dels=many)
    segs("many_h0", True, h=0, k=48, dels=many)
    for j in (0, 1, 23, 46, 47):
        segs("many_off_{}".format(j), False, h=1, k=48, dels=many, flip={10 + j})

    # a secondary read over a full set: no haplotype, no proposal, no vote, not in the pile
    c0 = L60.p0(32) + 50
    s, n = span(L60, 30, 6, c0)
    hap("secondary", L60, lambda subs: L60.read(0, s, n, subs=subs, flag=0x100), 0, False, c0, counted=False)
    hap("supplementary", L60, lambda subs: L60.read(0, s, n, subs=subs, flag=0x800), 0, True, c0)

    # ------------------------------------------------------------------------------------------------------------
    # Ten phase sets on one contig: A and B interleaved, C nested in D, S1 .. S6 under one read.
    ref = contig(2)
    A = Locus(ref, [2000 + 200 * i for i in range(10)], seed=21)
    B = Locus(ref, [2100 + 200 * i for i in range(10)], seed=22)
    D = Locus(ref, [6000 + 200 * i for i in range(16)], seed=23)
    C = Locus(ref, [7100, 7300, 7500], seed=24)
    S = [Locus(ref, [14000 + 400 * k + d for d in (0, 150, 300)], seed=30 + k) for k in range(6)]
    sets = [A, B, D, C] + S

    def carry(start, length, haps, subs=None, **kw):
        """A read that carries haplotype haps[i] (0, 1, or ("flip" | "third", h, hetSNP index)) in set i."""
        s = {}
        for L, h in zip(sets, haps):
            if isinstance(h, tuple):
                s.update(L.subs(h[1], start, start + length, **{h[0]: {h[2]}}))
            else:
                s.update(L.subs(h, start, start + length))
        s.update(subs or {})
        return read(ref, start, length, subs=s, **kw)
    recs = []
    for h in (0, 1):
        for _ in range(3):
            recs += [carry(1500, 3000, [h] * 10), carry(6500, 1600, [h] * 10), carry(13700, 2900, [h] * 10)]
    flipA, flipD = ("flip", 0, 3), ("flip", 0, 6)
    # R1: haplotype 0 in A, 1 in B, and with D's first hetSNP alone under it unphased in D
    recs.append(carry(1600, 4500, [0, 1, 0, 0] + [0] * 6, subs={3049: ALT[ref[3049]], 6049: ALT[ref[6049]]}))
    # R2: unphased in A (hetSNP 3 of A disagrees), 1 in B
    recs.append(carry(1700, 2600, [flipA, 1, 0, 0] + [0] * 6, subs=som(ref, 3249)))
    # R4: 0 in D, 1 in C;  R5: unphased in D, 1 in C
    recs.append(carry(6600, 1400, [0, 0, 0, 1] + [0] * 6, subs=som(ref, 7249)))
    recs.append(carry(6700, 1200, [0, 0, flipD, 1] + [0] * 6, subs=som(ref, 7449)))
    # two short reads under the long ones, inside C's read window: one ends at C's start (not fetched by C), one a base on
    recs.append(carry(6900, 200, [0] * 10, subs=som(ref, 7049)))
    recs.append(carry(6900, 201, [1] * 10, subs=som(ref, 7069)))
    # the long read: 0, 1, disagreeing, 0, third allele, 1 in S1 .. S6, a substitution in each
    Lh = [0, 1, ("flip", 0, 1), 0, ("third", 1, 2), 1]
    recs.append(carry(13800, 2700, [0] * 4 + Lh, subs={14075 + 400 * k - 1: ALT[ref[14075 + 400 * k - 1]] for k in range(6)}))

    def chunks10(r, l):
        is_status(r, 3050, "PASS", A.key, depth=8.0, alt_count=1.0)        # in A and in B's span: decided once, by A
        is_status(r, 3250, "PASS", B.key, depth=8.0)                       # proposed in B only
        none_at(r, 6050)                                                   # R1 has no haplotype in D
        is_status(r, 7250, "PASS", D.key, depth=8.0)
        is_status(r, 7450, "PASS", C.key, depth=8.0)
        none_at(r, 7050)
        none_at(r, 7070)
        for k, ok in enumerate((True, True, False, True, False, True)):
            if ok:
                is_status(r, 14075 + 400 * k, "PASS", S[k].key, depth=7.0, alt_count=1.0)
            else:
                none_at(r, 14075 + 400 * k)
    case("chunks_ten_sets", recs, sets, chunks10)

    # the same candidate in A and B, Unphased in A (haplotype 1 lacks a vote there): B does not look again
    recs = []
    for h, n in ((0, 3), (1, 2)):
        recs += [carry(1500, 3000, [h] * 10) for _ in range(n)]
    recs.append(carry(1500, 3000, [("flip", 1, 4), 1] + [0] * 8))          # haplotype 1 in B, none in A
    recs.append(carry(1600, 2800, [0, 1] + [0] * 8, subs=som(ref, 3049)))
    case("chunks_overlap_first_decides", recs, [A, B], lambda r, l: is_status(r, 3050, "Unphased", depth=7.0, ref_count=6.0), 3050)

    # ------------------------------------------------------------------------------------------------------------
    # The vote, unique names.  Twelve hetSNPs, the candidate behind hetSNP 5.
    ref = contig(3)

    def vote_locus(base=5000, seed=41, n=12, gts=None):
        return Locus(ref, [base + 100 * i for i in range(n)], seed=seed, gts=gts)
    V = vote_locus()
    c0 = V.p0(5) + 50
    tp = c0 + 1

    def proposer(L=V, h=0, c=c0, start=None, length=1000, **kw):
        return L.read(h, c - 400 if start is None else start, length, subs=som(L.ref, c), **kw)

    def vote(name, recs, status, L=V, tpos=tp, **kw):
        fields = {k: kw.pop(k) for k in ("depth", "ref_count", "alt_count") if k in kw}
        case("vote_" + name, recs, L, lambda r, l: is_status(r, tpos, status, L.key, **fields), tpos, **kw)

    unph = [V.read(0, c0 - 500, 1000, flip={4}), V.read(1, c0 - 450, 1000, flip={6}), V.read(0, c0 - 350, 1000, third={5}),
            V.read(1, c0 - 300, 1000, flip={3, 7})]
    for m in (1, 3):
        for a, b in ((m - 1, m), (m, m - 1), (m, m), (m - 1, m - 1)):
            ok = a >= m and b >= m
            vote("min_hap_{}_h0_{}_h1_{}".format(m, a, b), V.bg(c0, a, b) + unph * 2 + [proposer()], "PASS" if ok else "Unphased",
                 min_hap_count=m, depth=float(a + b + 9), ref_count=float(a + b + 8))
    vote("min_hap_0_none_phased", unph * 2 + [proposer()], "PASS", min_hap_count=0, ref_count=8.0)
    vote("min_hap_0_one_side", V.bg(c0, 3, 0) + unph + [proposer(h=1)], "PASS", min_hap_count=0)
    vote("min_hap_3_unphased_do_not_vote", V.bg(c0, 3, 2) + unph * 2 + [proposer()], "Unphased", ref_count=13.0)

    # a reference-allele read that ends on the candidate is in the column and casts no vote; one base more and it does
    for h in (0, 1):
        n0, n1 = (2, 3) if h == 0 else (3, 2)
        vote("ref_read_ends_at_candidate_h{}".format(h), V.bg(c0, n0, n1) + [V.read(h, c0 - 700, 701), proposer()], "Unphased", ref_count=6.0)
        vote("ref_read_ends_behind_candidate_h{}".format(h), V.bg(c0, n0, n1) + [V.read(h, c0 - 700, 702), proposer()], "PASS", ref_count=6.0)
    # the proposer's own end
    vote("proposer_ends_at_candidate", V.bg(c0, 4, 4) + [proposer(start=c0 - 700, length=701)], "Unphased", min_trim=0.0, alt_count=1.0)
    vote("proposer_ends_behind_candidate", V.bg(c0, 4, 4) + [proposer(start=c0 - 700, length=702)], "PASS", min_trim=0.0)
    vote("proposer_starts_at_candidate", V.bg(c0, 4, 4) + [proposer(start=c0, length=700)], "PASS", min_trim=0.0)

    # several reads with the alternative allele (the pile is deep enough for two of them to stay somatic)
    deep = V.bg(c0, 32, 32)
    vote("two_alt_same_haplotype", deep + [proposer(), proposer(start=c0 - 300)], "PASS", alt_count=2.0, depth=66.0)
    vote("two_alt_both_haplotypes", deep + [proposer(), proposer(h=1, start=c0 - 300)], "Unphased", alt_count=2.0)
    vote("two_alt_one_unphased", deep + [proposer(h=1), proposer(start=c0 - 300, flip={6})], "PASS", alt_count=2.0)
    vote("two_alt_one_ends_at_candidate", deep + [proposer(), proposer(h=1, start=c0 - 700, length=701)], "PASS", alt_count=2.0, min_trim=0.0)

    # the chunk's span.  A candidate on the set's first or last hetSNP: the reads there are all of the haplotype that
    # shows the reference allele, the proposer is of the other and its hetSNP allele is the candidate (min_hap_count 0).
    for end_, gts in (("start", "0" + "".join(V.hbit[1:])), ("end", "".join(V.hbit[:-1]) + "0")):
        E = vote_locus(gts=gts)
        i = 0 if end_ == "start" else 11
        ce = E.p0(i)
        near = [E.read(0, ce - 480 - 10 * k, 1000) for k in range(8)]
        prop = E.read(1, ce - 450, 1000)
        vote("candidate_at_chunk_" + end_, near + [prop], "PASS", E, ce + 1, min_hap_count=0, depth=9.0, ref_count=8.0, alt_count=1.0)
        vote("candidate_at_chunk_{}_min_hap_1".format(end_), near + [prop], "Unphased", E, ce + 1, min_hap_count=1)
        if end_ == "start":
            # tend == chunk start: in the column store, not fetched by the chunk; one base more and it is
            vote("read_ends_at_chunk_start", near + [prop, E.read(0, ce - 600, 601)], "PASS", E, ce + 1, min_hap_count=0, depth=9.0, ref_count=8.0)
            vote("read_ends_behind_chunk_start", near + [prop, E.read(0, ce - 600, 602)], "PASS", E, ce + 1, min_hap_count=0, depth=10.0, ref_count=9.0)
        else:
            # tstart == chunk end - 1: the last read the chunk fetches; one base on and it is not fetched
            vote("read_starts_at_chunk_end", near + [prop, E.read(0, ce, 600)], "PASS", E, ce + 1, min_hap_count=0, depth=10.0, ref_count=9.0)
            vote("read_starts_behind_chunk_end", near + [prop, E.read(0, ce + 1, 600)], "PASS", E, ce + 1, min_hap_count=0, depth=9.0, ref_count=8.0)

    # the last and the first position of a 256-block
    for rem in (255, 0):
        base = 5120 + rem - 50 - 500 + 1 + (256 if rem == 0 else 0)
        W = vote_locus(base=base, seed=43)
        cw = W.p0(5) + 50
        assert cw % 256 == rem
        vote("block_{}".format(rem), W.bg(cw, 3, 3) + [proposer(W, c=cw)], "PASS", W, cw + 1)
        vote("block_{}_short".format(rem), W.bg(cw, 3, 2) + [W.read(1, cw - 700, 701), proposer(W, c=cw)], "Unphased", W, cw + 1)
        vote("block_{}_just".format(rem), W.bg(cw, 3, 2) + [W.read(1, cw - 700, 702), proposer(W, c=cw)], "PASS", W, cw + 1)

    # ------------------------------------------------------------------------------------------------------------
    # The vote by name: a supplementary alignment shares a read's name.
    def named(name, recs, status, L=V, tpos=tp, **kw):
        fields = {k: kw.pop(k) for k in ("depth", "ref_count", "alt_count") if k in kw}
        case("name_" + name, recs, L, lambda r, l: is_status(r, tpos, status, L.key, **fields), tpos, **kw)

    def deepen(L, c):
        """Two unphased reference-allele reads: depth for the genotype quality, no votes."""
        return [L.read(0, c - 480, 1000, flip={4}), L.read(1, c - 470, 1000, third={6})]

    def two_three(L=V, c=c0, **kw):
        """2 + 3 reference-allele reads; the first read of haplotype 0 is named "wt"."""
        r = L.bg(c, 2, 3, **kw)
        r[0]["qname"] = "wt"
        return r + deepen(L, c)

    def three_two(L=V, c=c0):
        r = L.bg(c, 3, 2)
        r[0]["qname"] = "wt"
        return r + deepen(L, c)
    sup = dict(flag=0x800)
    # a partner that starts on the base behind the candidate: not in the column, votes by name
    named("proposers_partner_other_haplotype", V.bg(c0, 4, 4) + [proposer(qname="alt"), V.read(1, c0 + 1, 800, qname="alt", **sup)], "Unphased", depth=9.0)
    named("proposers_partner_same_haplotype", V.bg(c0, 4, 4) + [proposer(qname="alt"), V.read(0, c0 + 1, 800, qname="alt", **sup)], "PASS", depth=9.0)
    named("proposers_partner_unphased", V.bg(c0, 4, 4) + [proposer(qname="alt"), V.read(1, c0 + 1, 800, flip={7}, qname="alt", **sup)], "PASS")
    named("ref_reads_partner_votes_too", two_three() + [proposer(), V.read(0, c0 + 1, 800, qname="wt", **sup)], "PASS", depth=8.0)
    named("ref_reads_partner_votes_other_haplotype", three_two() + [proposer(), V.read(1, c0 + 1, 800, qname="wt", **sup)], "PASS", depth=8.0)
    named("ref_reads_partner_unphased", two_three() + [proposer(), V.read(0, c0 + 1, 800, flip={8}, qname="wt", **sup)], "Unphased")
    named("ref_reads_partner_starts_a_base_late", two_three() + [proposer(), V.read(0, c0 + 2, 800, qname="wt", **sup)], "Unphased")
    # a partner over the candidate too: in the column with the reference allele, and a second vote of its name
    named("ref_reads_partner_in_column", two_three() + [proposer(), V.read(0, c0 - 200, 800, qname="wt", **sup)], "PASS", depth=9.0, ref_count=8.0)
    # a partner that ends on the candidate is in the column and casts no vote
    named("ref_reads_partner_ends_at_candidate", two_three() + [proposer(), V.read(0, c0 - 700, 701, qname="wt", **sup)], "Unphased", ref_count=8.0)
    named("ref_reads_partner_ends_behind_candidate", two_three() + [proposer(), V.read(0, c0 - 700, 702, qname="wt", **sup)], "PASS", ref_count=8.0)
    # a partner that fails the read filters still votes; a secondary one does not
    named("partner_low_mapq", two_three() + [proposer(), V.read(0, c0 + 1, 800, qname="wt", mapq=3, **sup)], "PASS")
    named("partner_too_long", two_three() + [proposer(), V.read(0, c0 + 1, 1500, qname="wt", **sup)], "PASS", qlen_upper_limit=1200)
    named("partner_too_short", two_three() + [proposer(), V.read(0, c0 + 1, 400, qname="wt", **sup)], "PASS", qlen_lower_limit=500)
    named("partner_secondary", two_three() + [proposer(), V.read(0, c0 + 1, 800, qname="wt", flag=0x100)], "Unphased")
    named("partner_secondary_of_proposer", V.bg(c0, 4, 4) + [proposer(qname="alt"), V.read(1, c0 + 1, 800, qname="alt", flag=0x100)], "PASS")
    # one name in the column with both alleles: it counts among the reference-allele names, for both alignments
    named("both_alleles_one_name", V.bg(c0, 4, 4) + [proposer(qname="alt"), V.read(0, c0 - 200, 800, qname="alt", **sup)], "Unphased", depth=10.0, alt_count=1.0)
    named("both_alleles_one_name_of_ref_read", two_three() + [proposer(qname="wt")], "Unphased", depth=8.0)
    # the proposer's partner starts at the chunk's end: the chunk did not fetch it, and it has no haplotype
    E = vote_locus(gts="".join(V.hbit[:-1]) + "0")
    ce = E.p0(11)
    near = [E.read(0, ce - 480 - 10 * k, 1000) for k in range(8)]
    prop = E.read(1, ce - 450, 1000, qname="alt")
    named("partner_beyond_chunk", near + [prop, E.read(0, ce + 1, 600, qname="alt", **sup)], "PASS", E, ce + 1, min_hap_count=0)
    named("partner_last_fetched", near + [prop, E.read(0, ce, 600, qname="alt", **sup)], "Unphased", E, ce + 1, min_hap_count=0, depth=10.0)
    # the candidate on a block's last position: the partner starts in the next block, where only that block's window has it
    W = vote_locus(base=5120 + 255 - 50 - 500 + 1, seed=43)
    cw = W.p0(5) + 50
    named("partner_in_next_block", two_three(W, cw) + [proposer(W, c=cw), W.read(0, cw + 1, 800, qname="wt", **sup)], "PASS", W, cw + 1)
    named("partner_in_next_block_of_proposer", W.bg(cw, 4, 4) + [proposer(W, c=cw, qname="alt"), W.read(1, cw + 1, 800, qname="alt", **sup)],
          "Unphased", W, cw + 1)
    # the candidate on the last base of the contig's last read, which is the contig's last base and the set's last hetSNP
    Z = vote_locus(base=N - 1100, gts="".join(vote_locus(seed=44).hbit[:-1]) + "0")
    cz = N - 1
    zr = [Z.read(0, N - 1400 + 10 * k, 1400 - 10 * k) for k in range(8)]
    zr[0]["qname"] = "wt"
    zr.append(Z.read(1, N - 3000, 2000, qname="wt", **sup))
    named("candidate_on_last_base", zr + [Z.read(1, N - 1300, 1300)], "Unphased", Z, cz + 1, min_trim=0.0, min_hap_count=0, depth=9.0, alt_count=1.0)
    return out


CASES = _cases()
VOTE_BY_ROW = [c for c in CASES if c.name.startswith("vote_")]
VOTE_BY_NAME = [c for c in CASES if c.name.startswith("name_")]


def with_shared_pair(case):
    """The case's batch with two short reads more that share one name, on a stretch no chunk and no read touches: the
    batch's names are no longer unique and every candidate is voted on by name."""
    b = case.batch
    recs = []
    for i in range(b.n):
        recs.append(dict(tstart=int(b.tstart[i]), tend=int(b.tend[i]), qstart=int(b.qstart[i]), seq=b.query_sequence(i),
                         bq=list(b.query_qualities(i)), cs=b.cs_tag(i), flag=int(b.flag[i]), mapq=int(b.mapq[i]), qname=b.query_name(i)))
    recs += [read(case.refseq, FREE[0] + 50, 200, qname="pair"), read(case.refseq, FREE[0] + 300, 200, qname="pair", flag=0x800)]
    return batch(recs)
