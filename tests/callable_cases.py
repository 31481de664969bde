"""Hand-built reads for the callable bits of `normcounts` (k_callable, normcounts.update_tri2count): builders only, used
by the fixture generator (tests/golden/make_golden.py callable_cases) and by tests/test_callable_cpu.py and
tests/test_gpu_callable.py.  Every read is written as a list of cs operations in QUERY order, so that an event sits at
the query offset -- the bit of the word -- a case asks for; nothing is drawn at run time but the contig's letters, and
those are seeded, so a rebuilt case equals the committed fixture.  Every case carries its own parameter sets (overrides
of BASE, whose filters let every read pass).

word_edges      one substitution, insertion or deletion at query offsets 0 ... 65, windows of 0 ... 33
read_start      the first match operation starts at 0, 1, w - 1, w, w + 1 (soft clip, leading substitution, leading insertion)
read_end        operations that start at qlen - w - 1 ... qlen - 1, qlen % 32 in 0, 1, 31
counts          0 ... 9 entries in a window against max_mismatch_count 0 ... 9; five entries near one word
indel_geometry  windows in reference coordinates across 300-base indels; +ac+gt, -gt+ac, +ac-gt, long-form cs
nsub            substitutions whose reference base is n
quality         qualities 1 ... 255 in every byte lane against min_bq 0 ... 255
trim            min_trim 0 ... 0.51 at query lengths where ceil((1 - t) qlen) != qlen - floor(t qlen)
padding         qlen % 32 in 0 ... 31, the mean quality exactly at and one point below min_qv
filters         one read failing each read filter at its boundary, between reads that pass
lists           256 / 257 list entries, 62 ... 66 segments, 128 and about 300 marked words
long            reads of 65,504, 65,536, 65,537 and 70,001 bases"""
import random
from collections import namedtuple

from himut_amd.readbatch import ReadBatch, batch_from_records

Case = namedtuple("Case", "name length ref records chunks params")

# every read passes; a case overrides what it is about
BASE = dict(min_qv=0, min_mapq=0, qlen_lower_limit=0, qlen_upper_limit=1 << 30, min_sequence_identity=0.0, min_gq=20,
            min_bq=1, min_trim=0.0, max_mismatch_count=0, mismatch_window_size=20, md_threshold=100000, min_ref_count=3,
            min_alt_count=1, min_hap_count=3, germline_snv_prior=1 / (10 ** 3))
DEFAULT_TRIM = 0.01
CONTIG = "chrK"

CASES = ("word_edges", "read_start", "read_end", "counts", "indel_geometry", "nsub", "quality", "trim", "padding",
         "filters", "lists", "long")
FIXTURE_CASES = tuple(c for c in CASES if c not in ("long", "filters", "padding"))


def params_of(overrides):
    p = dict(BASE)
    p.update(overrides)
    return p


def in_fixture(case_name, record):
    """The fixture leaves out three cases and the 256 / 257-entry reads of lists."""
    return case_name in FIXTURE_CASES and not record["qname"].startswith("entries_")


def batch_of(case, copies=1):
    """The case's batch; copies > 1: every read laid down that many times at the same start under distinct names."""
    records = case.records
    if copies > 1:
        records = [dict(r, qname="{}#{}".format(r["qname"], k)) for r in records for k in range(copies)]
    return batch_from_records(CONTIG, case.length, records)


def poison_padding(batch, value=255):
    """The batch with the bytes of bq behind each read's last base set to ``value``."""
    bq = batch.bq.copy()
    for i in range(batch.n):
        o, n = int(batch.qoff[i]), int(batch.qlen[i])
        bq[o + n:o + ((n + 31) & ~31)] = value
    return ReadBatch(name=batch.name, length=batch.length, tstart=batch.tstart, tend=batch.tend, qstart=batch.qstart,
                     qlen=batch.qlen, mapq=batch.mapq, flag=batch.flag, qid=batch.qid, qoff=batch.qoff, cs_off=batch.cs_off,
                     seq=batch.seq, bq=bq, cs=batch.cs, tp=batch.tp, qnames=batch.qnames)


def _random_ref(seed, length):
    rs = random.Random(seed)
    return "".join(rs.choice("ACGT") for _ in range(length))


def _other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


def read(ref, tstart, ops, qname, lead=0, trail=0, bq=40, bq_q=None, long_cs=False, **extra):
    """A read record from cs operations in query order: ("m", n) n matching bases, ("s",) a substitution, ("n",) a
    substitution whose cs names n as the reference base, ("i", n) an insertion, ("d", n) a deletion; lead / trail: soft
    clipped bases (in seq and bq, not in the cs text); bq: the quality of every base, or a function of the query offset;
    bq_q {query offset: quality} on top."""
    seq, cs = [], []
    p = tstart
    for k in range(lead):
        seq.append("ACGT"[k % 4])
    for op in ops:
        if op[0] == "m":
            if op[1] <= 0:
                continue
            run = ref[p:p + op[1]]
            assert len(run) == op[1], "contig too short"
            if cs and cs[-1][0] in ":=":                      # two match runs in a row are one operation
                prev = cs.pop()
                run0 = int(prev[1:]) if prev[0] == ":" else len(prev) - 1
                cs.append(("=" + ref[p - run0:p + op[1]]) if long_cs else ":{}".format(run0 + op[1]))
            else:
                cs.append(("=" + run) if long_cs else ":{}".format(op[1]))
            seq.extend(run)
            p += op[1]
        elif op[0] in "sn":
            alt = _other(ref[p])
            cs.append("*" + ("n" if op[0] == "n" else ref[p].lower()) + alt.lower())
            seq.append(alt)
            p += 1
        elif op[0] == "i":
            ins = "".join("ACGT"[(len(seq) + k) % 4] for k in range(op[1]))
            cs.append("+" + ins.lower())
            seq.extend(ins)
        elif op[0] == "d":
            cs.append("-" + ref[p:p + op[1]].lower())
            p += op[1]
        else:
            raise ValueError(op)
    for k in range(trail):
        seq.append("TGCA"[k % 4])
    n = len(seq)
    quals = [bq(q) for q in range(n)] if callable(bq) else [bq] * n
    for q, v in (bq_q or {}).items():
        quals[q] = v
    assert all(1 <= v <= 255 for v in quals)                  # (a quality of 0 in a piled column is an error of the run)
    return dict(tstart=tstart, tend=p, qstart=lead, seq="".join(seq), bq=quals, cs="".join(cs), qname=qname, **extra)


def _case(name, seed, length, build, params, chunks=None):
    ref = _random_ref(seed, length)
    records = build(ref)
    records = sorted(records, key=lambda r: r["tstart"])
    assert len({r["qname"] for r in records}) == len(records)
    assert max(r["tend"] for r in records) + 2 <= length
    return Case(name, length, ref, records, chunks or [(0, length)], [dict(p) for p in params])


class _Place:
    """Starts for the reads of a case: one after the other, three positions apart."""

    def __init__(self, first=10):
        self.t = first - 3

    def __call__(self):
        self.t += 3
        return self.t


# ---------------------------------------------------------------------------------------------------------------

WORD_EDGE_OFFSETS = (0, 1, 30, 31, 32, 33, 63, 64, 65)
WORD_EDGE_W = (0, 1, 5, 20, 31, 32, 33)


def word_edges():
    """200-base reads with one event: a substitution at query offset o, a two-base insertion whose first base is at o, a
    three-base deletion directly behind base o."""
    def build(ref):
        at, out = _Place(), []
        for o in WORD_EDGE_OFFSETS:
            out.append(read(ref, at(), [("m", o), ("s",), ("m", 199 - o)], "sub_{}".format(o)))
            out.append(read(ref, at(), [("m", o), ("i", 2), ("m", 198 - o)], "ins_{}".format(o)))
            out.append(read(ref, at(), [("m", o + 1), ("d", 3), ("m", 199 - o)], "del_{}".format(o)))
        return out
    return _case("word_edges", 9101, 400, build,
                 [dict(mismatch_window_size=w, max_mismatch_count=0) for w in WORD_EDGE_W])


READ_START_W = (5, 20)


def read_start():
    """The first match operation starts at query offset osq in 0, 1, w - 1, w, w + 1 for w = 5 and 20: behind a soft clip
    of osq bases, behind a clip of osq - 1 and a substitution, behind a clip and a leading insertion (a cs text that begins
    with +).  It is ended by a substitution d bases on (inside the first word, in a later word), by a deletion, or never:
    the bases of the operation see an entry behind them that is up to 2 w - osq reference positions away, and the entry
    in front of them (the leading substitution or insertion) from up to osq positions."""
    def build(ref):
        at, out = _Place(), []
        starts = sorted({x for w in READ_START_W for x in (0, 1, w - 1, w, w + 1)})
        for osq in starts:
            leads = [("clip", osq, [])]
            if osq >= 1:
                leads.append(("sub", osq - 1, [("s",)]))
                k = min(osq, 2)
                leads.append(("ins", osq - k, [("i", k)]))
            for lname, clip, head in leads:
                for tname, tail in (("sub8", [("m", 8), ("s",), ("m", 120)]), ("sub45", [("m", 45), ("s",), ("m", 90)]),
                                    ("sub12", [("m", 12), ("s",), ("m", 110)]), ("sub38", [("m", 38), ("s",), ("m", 95)]),
                                    ("del45", [("m", 45), ("d", 2), ("m", 90)]), ("none", [("m", 140)])):
                    out.append(read(ref, at(), head + tail, "start{}_{}_{}".format(osq, lname, tname), lead=clip))
        return out
    return _case("read_start", 9102, 1200, build,
                 [dict(mismatch_window_size=w, max_mismatch_count=m) for w in READ_START_W for m in (0, 1)])


READ_END_QLEN = (192, 193, 223)


def read_end():
    """Built for w = 20.  A substitution B at osq - 1 starts an operation at osq in qlen - 21, qlen - 20 (qe == qlen: the
    ordinary window), qlen - 19, qlen - 1; its window reaches ur = w + (osq + w - qlen) back, and a substitution A sits
    so that the bases up to osq + b (b = -1: none, 0, 2) see it.  In the del reads the operation is cut by a deletion
    sized so that a substitution C behind it is dr = qlen - osq reference positions from the operation's middle.  The
    clip reads end their alignment five bases in front of qlen."""
    w = 20

    def build(ref):
        at, out = _Place(), []
        for qlen in READ_END_QLEN:
            for osq in (qlen - w - 1, qlen - w, qlen - w + 1, qlen - 1):
                ur = w + (osq + w - qlen) if osq + w > qlen else w
                dr = qlen - osq if osq + w > qlen else w
                for b in (-1, 0, 2):
                    qa = osq + b - 1 - ur
                    out.append(read(ref, at(), [("m", qa), ("s",), ("m", osq - 2 - qa), ("s",), ("m", qlen - osq)],
                                    "end{}_{}_b{}".format(qlen, osq - qlen, b)))
                if qlen - osq >= 12:
                    k = 8
                    d = dr - 2 - k + k // 2
                    out.append(read(ref, at(), [("m", osq - 1), ("s",), ("m", k), ("d", d), ("m", 1), ("s",),
                                                ("m", qlen - osq - k - 2)], "end{}_{}_del".format(qlen, osq - qlen)))
            out.append(read(ref, at(), [("m", qlen - 5 - 12), ("s",), ("m", 11)], "end{}_clip".format(qlen), trail=5))
            out.append(read(ref, at(), [("m", qlen - 2), ("i", 2)], "end{}_ins".format(qlen)))
        return out
    return _case("read_end", 9103, 700, build,
                 [dict(mismatch_window_size=ww, max_mismatch_count=m, min_trim=t)
                  for ww in (19, 20, 21) for m in (1, 2) for t in (0.0, DEFAULT_TRIM)])


COUNTS_MAXMM = (0, 1, 2, 3, 4, 5, 7, 8, 9)


def _entries(k):
    """k list entries two reference positions apart: substitution, one-base insertion, one-base deletion, and (from the
    fourth on) an insertion directly followed by a substitution -- two entries with the same list position."""
    ops, n = [], 0
    while n < k:
        kind = ("s", "i", "d", "is")[len(ops) // 2 % 4]
        if kind == "is" and k - n >= 2:
            ops += [("i", 1), ("s",)]
            n += 2
        elif kind == "i":
            ops += [("i", 1)]
            n += 1
        elif kind == "d":
            ops += [("d", 1)]
            n += 1
        else:
            ops += [("s",)]
            n += 1
        ops += [("m", 1)]
    return ops


def counts():
    """400-base reads with k = 0 ... 9 entries packed from query offset 200 on (the bases around see 0 ... k of them),
    and two reads with four substitutions in front of the word of bases 192 ... 223 and a fifth whose list position is
    thi + 2 w + 1 and thi + 2 w + 2 (thi: the reference position of base 223; w = 20)."""
    def build(ref):
        at, out = _Place(), []
        for k in range(10):
            out.append(read(ref, at(), [("m", 200)] + _entries(k) + [("m", 170)], "entries{}".format(k)))
            out.append(read(ref, at(), [("m", 37)] + _entries(k) + [("m", 170)], "early{}".format(k)))
        for name, q5 in (("fifth_at", 263), ("fifth_behind", 264)):
            ops, q = [], 0
            for s in (160, 170, 180, 190, q5):
                ops += [("m", s - q), ("s",)]
                q = s + 1
            out.append(read(ref, at(), ops + [("m", 400 - q)], name))
        out.append(read(ref, at(), [("m", 150)] + [x for _ in range(6) for x in (("s",), ("m", 9))] + [("m", 190)], "six_subs"))
        return out
    return _case("counts", 9104, 700, build, [dict(max_mismatch_count=m) for m in COUNTS_MAXMM])


def indel_geometry():
    def build(ref):
        at, out = _Place(), []
        for long_cs in (False, True):
            sfx = "_long" if long_cs else ""
            out.append(read(ref, at(), [("m", 100), ("s",), ("m", 12), ("d", 300), ("m", 100)], "del300" + sfx, long_cs=long_cs))
            out.append(read(ref, at(), [("m", 100), ("s",), ("m", 12), ("i", 300), ("m", 100)], "ins300" + sfx, long_cs=long_cs))
            out.append(read(ref, at(), [("m", 100), ("i", 2), ("i", 2), ("m", 100)], "insins" + sfx, long_cs=long_cs))
            out.append(read(ref, at(), [("m", 100), ("d", 2), ("i", 2), ("m", 100)], "delins" + sfx, long_cs=long_cs))
            out.append(read(ref, at(), [("m", 100), ("i", 2), ("d", 2), ("m", 100)], "insdel" + sfx, long_cs=long_cs))
            out.append(read(ref, at(), [("m", 150), ("i", 3)], "ins_last" + sfx, long_cs=long_cs))
            out.append(read(ref, at(), [("m", 70), ("d", 25), ("m", 30), ("s",), ("m", 30), ("i", 25), ("m", 70)], "mixed" + sfx,
                            long_cs=long_cs))
        return out
    return _case("indel_geometry", 9105, 900, build,
                 [dict(mismatch_window_size=w, max_mismatch_count=m) for w in (20, 5) for m in (0, 1)])


def nsub():
    """Substitutions whose reference base is n: at bit 0 and bit 31 of a word, two adjacent, inside the first w bases, in
    front of a word whose first operation they start (bit 31 with w = 40: the operation behind starts within w of the
    read's start), beside an ordinary substitution on either side.  Ordinary substitutions 39 and 46 bases on tell which
    operation's window the bases in between have."""
    def build(ref):
        at, out = _Place(), []

        def one(name, q, extra=()):
            ops, pos = [], 0
            for s, kind in sorted([(q, "n")] + list(extra) + [(q + 39, "s"), (q + 46, "s")]):
                ops += [("m", s - pos), (kind,)]
                pos = s + 1
            out.append(read(ref, at(), ops + [("m", 300 - pos)], name))
        one("bit0", 64)
        one("bit31", 95)
        one("adjacent", 130, [(131, "n")])
        one("first_w", 5)
        one("front_of_word", 31)
        one("front_of_word2", 63)
        one("n_then_sub", 100, [(101, "s")])
        one("sub_then_n", 100, [(99, "s")])
        one("near_end", 240)
        one("first_base", 0)
        return out
    return _case("nsub", 9106, 500, build,
                 [dict(mismatch_window_size=w, max_mismatch_count=m) for w in (20, 40) for m in (0, 1)])


QUALITY_MIN_BQ = (0, 1, 20, 93, 127, 128, 129, 200, 255)
_Q_LOW = (1, 19, 20, 92, 93, 126, 127)
_Q_ALL = _Q_LOW + (128, 129, 199, 200, 254, 255)


def _lanes(values):
    """Every value in every byte lane of a dword: base q (lane q % 4 of dword q // 4) gets values[(q // 4 + q % 4) % n]."""
    return lambda q: values[(q // 4 + q % 4) % len(values)]


def quality():
    """320-base reads whose qualities run through 1, min_bq - 1, min_bq, 127, 128, 129, 255 (for every min_bq of the
    parameter sets) in each of the four byte lanes: below 128 only (the words without a high bit) and all of them; with no
    entry (every word is pass A's) and with substitutions every 80 bases (every word is pass B's; max_mismatch_count 9
    leaves the decision to the quality)."""
    def build(ref):
        at, out = _Place(), []
        subs = [("m", 40), ("s",), ("m", 79), ("s",), ("m", 79), ("s",), ("m", 79), ("s",), ("m", 39)]
        for name, values in (("low", _Q_LOW), ("all", _Q_ALL)):
            out.append(read(ref, at(), [("m", 320)], "passA_" + name, bq=_lanes(values)))
            out.append(read(ref, at(), subs, "passB_" + name, bq=_lanes(values)))
            out.append(read(ref, at(), [("m", 3)] + subs, "passB3_" + name, bq=_lanes(values)))
        return out
    return _case("quality", 9107, 500, build, [dict(min_bq=b, max_mismatch_count=9) for b in QUALITY_MIN_BQ])


TRIM_VALUES = (0.0, 0.01, 0.1, 0.35, 0.45, 0.5, 0.51)
TRIM_QLEN = (100, 101, 180, 199, 340)


def trim():
    """Reads of one match operation, and the same with a substitution on the first and the last base and in the middle (a
    substitution counts wherever it is)."""
    def build(ref):
        at, out = _Place(), []
        for n in TRIM_QLEN:
            out.append(read(ref, at(), [("m", n)], "plain{}".format(n)))
            out.append(read(ref, at(), [("s",), ("m", n // 2 - 1), ("s",), ("m", n - n // 2 - 2), ("s",)], "subs{}".format(n)))
            out.append(read(ref, at(), [("m", n - 14)], "clipped{}".format(n), lead=9, trail=5))
        return out
    return _case("trim", 9108, 500, build, [dict(min_trim=t, max_mismatch_count=3) for t in TRIM_VALUES])


PADDING_REST = (0, 1, 3, 4, 5, 31)
PADDING_MIN_QV = 30


def padding():
    """Reads of 96 + r bases: every quality 30 (the mean is min_qv exactly: the read stays), and with one base of 29 (one
    quality point short over the whole read: it goes).  The tests set the bytes of bq behind every read to 255."""
    def build(ref):
        at, out = _Place(), []
        for r in PADDING_REST:
            n = 96 + r
            out.append(read(ref, at(), [("m", n)], "exact{}".format(r), bq=30))
            out.append(read(ref, at(), [("m", n)], "below{}".format(r), bq=30, bq_q={n - 1: 29}))
            out.append(read(ref, at(), [("m", 50), ("s",), ("m", n - 51)], "exact_sub{}".format(r), bq=30))
            out.append(read(ref, at(), [("m", 50), ("s",), ("m", n - 51)], "below_sub{}".format(r), bq=30, bq_q={0: 29}))
        return out
    return _case("padding", 9109, 400, build, [dict(min_qv=PADDING_MIN_QV, min_bq=b) for b in (1, 30)])


FILTER_PARAMS = dict(min_mapq=20, qlen_lower_limit=99, qlen_upper_limit=401, min_sequence_identity=0.9, min_qv=25)
FILTER_CHUNKS = [(0, 1000), (1400, 3000)]


def filters():
    """One read failing each read filter at its boundary, each between two reads that pass: mapping quality 19 against
    20; query lengths 99 and 401 against the strict limits (100 and 400 pass); identity 89 / 100 against 0.9 (90 / 100
    passes); mean quality 2499 / 100 against 25; the secondary flag; a read that ends where the second chunk starts and
    one that starts where the first one ends (fetched by no chunk; one base further either way and it is)."""
    def build(ref):
        at, out = _Place(), []

        def ok(name, **kw):
            out.append(read(ref, at(), [("m", 60), ("s",), ("m", 139)], name, **kw))

        def ident(name, nsub):
            out.append(read(ref, at(), [x for _ in range(nsub) for x in (("s",), ("m", 2))] + [("m", 100 - 3 * nsub)], name))
        ok("pass0")
        ok("mapq19", mapq=19)
        ok("mapq20", mapq=20)
        out.append(read(ref, at(), [("m", 99)], "qlen99"))
        out.append(read(ref, at(), [("m", 100)], "qlen100"))
        out.append(read(ref, at(), [("m", 401)], "qlen401"))
        out.append(read(ref, at(), [("m", 400)], "qlen400"))
        ident("ident89", 11)
        ident("ident90", 10)
        out.append(read(ref, at(), [("m", 100)], "qv_below", bq=25, bq_q={7: 24}))
        out.append(read(ref, at(), [("m", 100)], "qv_exact", bq=25))
        ok("secondary", flag=0x100)
        ok("supplementary", flag=0x800)
        ok("pass1")
        out.append(read(ref, 1000, [("m", 400)], "between_chunks"))
        out.append(read(ref, 999, [("m", 400)], "in_first_chunk"))
        out.append(read(ref, 1001, [("m", 400)], "in_second_chunk"))
        ok("pass2")
        return out
    return _case("filters", 9110, 3000, build, [dict(FILTER_PARAMS), dict(FILTER_PARAMS, min_trim=DEFAULT_TRIM)],
                 chunks=FILTER_CHUNKS)


def lists():
    """The lists of a read in LDS and in memory: 256 and 257 list entries (substitutions ten bases apart); 61 ... 65
    insertions and 30 ... 33 deletions (62 ... 66 gapless pieces; with the deletions' own entries 61 ... 67 segments).
    Pass B's rounds: a read of 128 words with a substitution every 60 bases (every word marked: one round of exactly
    128), of 129 words (two rounds) and of 300 words (three)."""
    def build(ref):
        at, out = _Place(), []

        def every(n_events, gap, event, name, tail=40):
            ops = [("m", 40)]
            for _ in range(n_events):
                ops += [event, ("m", gap)]
            out.append(read(ref, at(), ops + [("m", tail)], name))
        every(256, 9, ("s",), "entries_256")
        every(257, 9, ("s",), "entries_257")
        for n in (61, 62, 63, 64, 65):
            every(n, 30, ("i", 1), "pieces_ins{}".format(n))
        for n in (30, 31, 32, 33):
            every(n, 60, ("d", 2), "pieces_del{}".format(n))
        for words in (128, 129, 300):
            n = words * 32
            ops, q = [], 0
            for s in range(30, n - 1, 60):
                ops += [("m", s - q), ("s",)]
                q = s + 1
            out.append(read(ref, at(), ops + [("m", n - q)], "marked_{}".format(words)))
        return out
    return _case("lists", 9111, 10000, build, [dict(max_mismatch_count=m) for m in (0, 1)])


LONG_QLEN = (65504, 65536, 65537, 70001)


def long():
    """Reads of 2047 words, 2048 words (the longest the bitmap of marked words holds), 2049 words and 70,001 bases (every
    word the exact way), with an event about every 2,000 bases, a substitution on the second base and events in the last
    word."""
    def build(ref):
        out = []
        for k, n in enumerate(LONG_QLEN):
            ops, q = [("m", 1), ("s",)], 2
            for j, s in enumerate(range(1500, n - 2100, 2000)):
                s += 7 * j
                ops += [("m", s - q)]
                kind = j % 3
                if kind == 0:
                    ops += [("s",)]
                    q = s + 1
                elif kind == 1:
                    ops += [("i", 2)]
                    q = s + 2
                else:
                    ops += [("d", 3)]
                    q = s
            ops += [("m", n - 9 - q), ("s",), ("m", 5), ("s",), ("m", 2)]
            out.append(read(ref, 10 + k, ops, "long_{}".format(n)))
            assert len(out[-1]["seq"]) == n
        return out
    return _case("long", 9112, 72000, build,
                 [dict(max_mismatch_count=0), dict(max_mismatch_count=1, min_trim=DEFAULT_TRIM, mismatch_window_size=33)])


def build(name):
    return globals()[name]()
