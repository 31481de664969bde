"""Hand-built inputs for the hetSNP edge counts (himut_run_edges / k_edges, phaselib.get_edges): builders only, used by
the fixture generator (tests/golden/make_golden.py edges_blocks / edges_rules) and by tests/test_edges_cpu.py and
tests/test_gpu_edges.py.  Every batch is small on purpose -- a few hundred reads of at most about 600 bases -- and every
draw is seeded, so a rebuilt case equals the committed fixture.

blocks      reads that span exactly k hetSNPs: the 64-lane blocking of k_edges (k = 64, 65, 128, 129, ...)
spans       a hetSNP on tstart, tstart + 1, tend, tend + 1: the span rule tstart < pos1 <= tend
cs_geometry a hetSNP in, behind and between insertions and deletions: the query offset of its base
filters     base quality, mapping quality and flags at their boundaries; read counts that are no multiple of four
deep        hundreds of reads on the same edges: the atomic accumulation
rules       the last four on disjoint stretches of one contig (the edges_rules fixture)"""
import random
from collections import namedtuple

from himut_amd.readbatch import batch_from_records
from tests.germline_model import make_read

Case = namedtuple("Case", "name length ref records hets")

BLOCKS_FIXTURE_K = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130]
BLOCKS_LARGE_K = [193, 257]
BLOCKS_PARAMS = (20, 20)                                  # (min_bq, min_mapq) of the edges_blocks fixture
RULES_MIN_BQ = [0, 1, 20, 21, 93, 94]
RULES_MIN_MAPQ = [0, 20, 21, 255]


def batch_of(case):
    return batch_from_records(case.name, case.length, case.records)


def _other(base, k=1):
    """A base that is not ``base`` (nor N): the k-th behind it in ACGT."""
    return "ACGT"[("ACGT".index(base) + k) % 4] if base in "ACGT" else "ACGT"[k % 4]


def _random_ref(seed, length):
    rs = random.Random(seed)
    return "".join(rs.choice("ACGT") for _ in range(length))


def _sorted(records):
    return sorted(records, key=lambda r: r["tstart"])        # stable: equal starts keep the order they were built in


# ---------------------------------------------------------------------------------------------------------------
# blocks

def blocks(k_list):
    """One 1.5 kb contig, hetSNPs at pos1 = 101, 103, ...; one read per k that starts at 100 and spans exactly k of them
    (2k - 1 bases; k = 1: the one base on the first hetSNP, k = 0: the one base behind it).  At every hetSNP a read
    carries the reference base, the alt or a third base with quality 19, 20, 21 or 40, drawn from one seeded stream
    (no period), so every pair of one read adds at most one count and a missed, doubled or mis-broadcast pair shows."""
    ref = _random_ref(7001, 1500)
    n_het = max(list(k_list) + [2]) + 10
    assert 100 + 2 * n_het < len(ref)
    rs = random.Random(7002)
    hets = [(100 + 2 * g + 1, ref[100 + 2 * g], _other(ref[100 + 2 * g], rs.randint(1, 3))) for g in range(n_het)]
    records = []
    for k in k_list:
        rr = random.Random(7100 + k)
        if k == 0:
            records.append(make_read(ref, 101, 1, mapq=60, qname="k0"))
            continue
        subs, bq_at = {}, {}
        for g in range(k):
            pos = 100 + 2 * g
            what = rr.randrange(3)
            if what:
                subs[pos] = hets[g][2] if what == 1 else next(b for b in "ACGT" if b not in (hets[g][1], hets[g][2]))
            bq_at[pos] = rr.choice([19, 20, 21, 40])
        records.append(make_read(ref, 100, 2 * k - 1, subs=subs, bq_at=bq_at, mapq=60, qname="k{}".format(k)))
    return Case("chrB", len(ref), ref, _sorted(records), hets)


# ---------------------------------------------------------------------------------------------------------------
# the four rule cases share one contig; each has a stretch of its own

RULES_LEN = 3000
SPANS_AT, GEOMETRY_AT, FILTERS_AT, DEEP_AT = 100, 1000, 1400, 1600
_N_AT = (GEOMETRY_AT + 80, GEOMETRY_AT + 84)     # reference N (cs_geometry)


def rules_ref():
    ref = list(_random_ref(7003, RULES_LEN))
    for p in _N_AT:
        ref[p] = "N"
    return "".join(ref)


def _het(ref, pos0, k=1):
    return (pos0 + 1, ref[pos0], _other(ref[pos0], k))


def spans():
    """Twelve reads, each on a 60-base stretch of its own with three hetSNPs: a pair well inside the read and x, which
    lies on tstart (1-based: the base in front of the read, out), on tstart + 1 (the first base, in), on tend (the last
    base, in) or on tend + 1 (out) -- plain, with a 7-base leading and a 3-base trailing soft clip, and on a read that
    ends in an insertion.  The read carries the alt at x and at the second of the pair."""
    ref = rules_ref()
    records, hets = [], []
    n = 0
    for kind in ("plain", "clip", "ins"):
        for where in ("tstart", "tstart+1", "tend", "tend+1"):
            s0 = SPANS_AT + 60 * n
            n += 1
            if where.startswith("tstart"):
                x, p, q = s0 + 10, s0 + 20, s0 + 30
                start, end = (x + 1 if where == "tstart" else x), s0 + 45
            else:
                p, q, x = s0 + 10, s0 + 20, s0 + 40
                start, end = s0 + 3, (x + 1 if where == "tend" else x)
            hx, hp, hq = _het(ref, x), _het(ref, p), _het(ref, q, 2)
            hets += [hx, hp, hq]
            subs = {q: hq[2]}
            if start <= x < end:
                subs[x] = hx[2]
            kw = {}
            if kind == "clip":
                kw["softclip"] = ("".join(_other(ref[start + i], 2) for i in range(7)), "GAT")
            if kind == "ins":
                kw["ins"] = {end: "TGA"}
            records.append(make_read(ref, start, end - start, subs=subs, bq_at={x: 33, p: 34, q: 35}, mapq=60,
                                     qname="span_{}_{}".format(kind, where), **kw))
    return Case("chrR", RULES_LEN, ref, _sorted(records), sorted(hets))


GEOMETRY_SITES = {            # offset in the stretch -> what the position is for the reads that carry the indels
    5: "plain, in front of everything",
    10: "first of a 3-base deletion", 11: "middle of it", 12: "last of it", 13: "right behind the deletion",
    30: "right behind an insertion",
    45: "first of a deletion that directly follows an insertion (+ac-gt)", 46: "last of it", 47: "right behind the two",
    60: "substitution to the alt", 70: "substitution to a third base",
    80: "N in SEQ inside a match run over a reference N, hetSNP reference N",
    84: "the same, hetSNP reference A",
    95: "plain, behind everything",
}
_GEOMETRY_Q = [20, 21, 93, 40, 19, 1, 22, 20, 21, 19, 93, 20, 21, 40]


def cs_geometry():
    """Reads over one 120-base stretch whose hetSNPs lie on, in and behind insertions and deletions (GEOMETRY_SITES), in
    short and in long cs form, with and without the indels, one with a leading soft clip; the reads over the two
    reference Ns (N in SEQ, a match for the cs text) are reads of their own (names n_*), because no cs text derived from
    CIGAR and reference can say what theirs says.  Every hetSNP base has a quality of its own."""
    ref = rules_ref()
    g0 = GEOMETRY_AT
    offs = sorted(GEOMETRY_SITES)
    hets = []
    for o in offs:
        p = g0 + o
        hets.append((p + 1, "A", "G") if o == 84 else (p + 1, ref[p], _other(ref[p])))
    bq_at = {g0 + o: q for o, q in zip(offs, _GEOMETRY_Q)}
    alt = {g0 + o: h[2] for o, h in zip(offs, hets)}
    third = {p: next(b for b in "ACGT" if b not in (ref[p], alt[p])) for p in alt}
    indel = dict(ins={g0 + 30: "ACG", g0 + 45: "AC"}, dels={g0 + 10: 3, g0 + 45: 2})
    subs = {g0 + 60: alt[g0 + 60], g0 + 70: third[g0 + 70]}
    records = [
        # stops in front of the Ns: the reads the derived cs text can describe
        make_read(ref, g0, 78, subs=subs, bq_at=bq_at, mapq=60, qname="g_indel", **indel),
        make_read(ref, g0, 78, subs=subs, bq_at=bq_at, mapq=60, qname="g_indel_long", long_cs=True, **indel),
        make_read(ref, g0 + 2, 76, subs={**subs, g0 + 13: alt[g0 + 13], g0 + 47: alt[g0 + 47]}, bq_at=bq_at,
                  mapq=60, qname="g_indel_clip", softclip=("TTGCAGT", "CC"), **indel),
        make_read(ref, g0, 78, subs={g0 + 11: alt[g0 + 11], g0 + 30: alt[g0 + 30], g0 + 46: third[g0 + 46]}, bq_at=bq_at,
                  mapq=60, qname="g_plain"),
        make_read(ref, g0 + 4, 70, subs={g0 + 5: alt[g0 + 5], g0 + 45: alt[g0 + 45]}, bq_at=bq_at, mapq=60,
                  qname="g_plain_long", long_cs=True),
        # a deletion that ends the stretch's hetSNPs in front of it, then the Ns
        make_read(ref, g0 + 40, 70, subs={g0 + 95: alt[g0 + 95]}, bq_at=bq_at, mapq=60, qname="n_short",
                  ins={g0 + 45: "AC"}, dels={g0 + 45: 2}),
        make_read(ref, g0 + 55, 50, subs={g0 + 70: alt[g0 + 70]}, bq_at=bq_at, mapq=60, qname="n_long", long_cs=True),
    ]
    return Case("chrR", RULES_LEN, ref, _sorted(records), hets)


def filters():
    """Copies of one read over two hetSNPs, each kind with an allele pattern (and so a column of the edge) of its own:
    mapq 0 ... 255 (reference, reference), flags 0 ... 0x900 (alt, alt), the quality of the first hetSNP 1 ... 93
    (reference, alt) and of the second (alt, reference), the other end at 93.  Starts differ within every group of four reads, and the 22
    reads are no multiple of four."""
    ref = rules_ref()
    f0 = FILTERS_AT
    p, q = f0 + 8, f0 + 24
    hp, hq = _het(ref, p), _het(ref, q, 3)
    records = []

    def add(name, k, subs, **kw):
        start = f0 + k % 3
        records.append(make_read(ref, start, 30 + k % 4, subs=subs, qname=name, **kw))

    k = 0
    for mapq in (0, 19, 20, 21, 60, 255):
        add("f_mapq{}".format(mapq), k, {}, mapq=mapq)
        k += 1
    for flag in (0, 0x10, 0x100, 0x400, 0x800, 0x900):
        add("f_flag{:x}".format(flag), k, {p: hp[2], q: hq[2]}, mapq=60, flag=flag)
        k += 1
    for bq in (1, 19, 20, 21, 93):
        add("f_bq_first{}".format(bq), k, {q: hq[2]}, mapq=60, bq=93, bq_at={p: bq})
        add("f_bq_second{}".format(bq), k + 1, {p: hp[2]}, mapq=60, bq=93, bq_at={q: bq})
        k += 2
    assert len(records) % 4
    return Case("chrR", RULES_LEN, ref, _sorted(records), [hp, hq])


def deep():
    """300 identical reads over five hetSNPs with the reference allele, three with the alt, all qualities 40: every one of
    the ten edges ends with 300 in one column and 3 in another."""
    ref = rules_ref()
    d0 = DEEP_AT
    pos = [d0 + 3 + 4 * g for g in range(5)]
    hets = [_het(ref, p, 1 + g % 3) for g, p in enumerate(pos)]
    records = [make_read(ref, d0, 24, mapq=60, qname="d{}".format(i)) for i in range(300)]
    records += [make_read(ref, d0, 24, subs={p: h[2] for p, h in zip(pos, hets)}, mapq=60, qname="d_alt{}".format(i))
                for i in range(3)]
    return Case("chrR", RULES_LEN, ref, records, hets)


def rules(derivable_only=False):
    """spans, cs_geometry, filters and deep on their stretches of one contig, coordinate sorted.  ``derivable_only``:
    without the reads whose SEQ holds an N (an ingest that derives the cs text refuses them)."""
    parts = [spans(), cs_geometry(), filters(), deep()]
    records = _sorted([r for c in parts for r in c.records])
    if derivable_only:
        records = [r for r in records if "N" not in r["seq"]]
    hets = sorted(h for c in parts for h in c.hets)
    assert len({h[0] for h in hets}) == len(hets)
    return Case("chrR", RULES_LEN, parts[0].ref, records, hets)
