"""Inputs and checks for the tests of the grouped cs decode (k_parse_cs, himut_reads.h): reads built from operation
lists over a reference string, the hand-made batches that hold the places where a decode of several reads per wave can go
wrong, seeded random batches of short reads with many errors (1-12 reads share a group), a plain model of the group plan,
and the comparison of two copied-out read passes (Context.read_pass)."""
import bisect

import numpy as np

from himut_amd.readbatch import batch_from_records

# the plan's constants (himut_reads.h): tile bytes, the longest tag of a multi-read group, reads per group
GROUP_T, GROUP_LONG, GROUP_MAX = 768, 257, 64
MARK_CAP = 128

_OTHER = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}


def reference(rng, length):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, length))


def read_from_ops(ref, tstart, ops, rng, lead_clip=0, trail_clip=0, bq=93, **extra):
    """A record for batch_from_records.  ops: ("m", n) short-form match, ("=", n) long-form match, ("s", k) substitution
    to the k-th other base, ("n", base) substitution whose reference base cs names as n, ("i", bases) insertion,
    ("d", n) deletion."""
    t, cs, seq = tstart, [], ["".join("ACGT"[i] for i in rng.integers(0, 4, lead_clip))]
    for op, v in ops:
        if op == "m":
            cs.append(":%d" % v); seq.append(ref[t:t + v]); t += v
        elif op == "=":
            cs.append("=" + ref[t:t + v]); seq.append(ref[t:t + v]); t += v
        elif op == "s":
            alt = _OTHER[ref[t]][v % 3]
            cs.append("*" + ref[t].lower() + alt.lower()); seq.append(alt); t += 1
        elif op == "n":
            cs.append("*n" + v.lower()); seq.append(v); t += 1
        elif op == "i":
            cs.append("+" + v.lower()); seq.append(v)
        elif op == "d":
            cs.append("-" + ref[t:t + v].lower()); t += v
        else:
            raise ValueError(op)
    seq.append("".join("ACGT"[i] for i in rng.integers(0, 4, trail_clip)))
    seq = "".join(seq)
    assert t <= len(ref)
    rec = dict(tstart=tstart, tend=t, qstart=lead_clip, seq=seq, bq=[bq] * len(seq), cs="".join(cs))
    rec.update(extra)
    return rec


def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def random_ops(rng, span, rate, long_form=False):
    """Operations over about `span` reference bases with an error event about every 1 / rate bases; now and then two
    events with nothing between them, an indel at the very start or the very end."""
    ops, left = [], span
    m = "=" if long_form else "m"
    if rng.random() < 0.06:
        ops.append(("i", _bases(rng, 2)) if rng.random() < 0.5 else ("d", 2))
    while left > 0:
        n = int(min(left, max(1, rng.geometric(min(1.0, rate)))))
        ops.append((m, n)); left -= n
        if left <= 0:
            break
        for _ in range(1 if rng.random() < 0.8 else int(rng.integers(2, 4))):
            k = rng.random()
            if k < 0.5 and left > 0:
                ops.append(("s", int(rng.integers(0, 3)))); left -= 1
            elif k < 0.75:
                ops.append(("i", _bases(rng, int(rng.integers(1, 4)))))
            elif left > 3:
                d = int(rng.integers(1, 4)); ops.append(("d", d)); left -= d
    if rng.random() < 0.06:
        ops.append(("i", _bases(rng, 1)) if rng.random() < 0.5 else ("d", 1))
    return ops


def random_batch(seed, n_reads=None, name="chrD"):
    """Tens to a few hundred reads of 60-2,000 bases on a contig of 5-50 kb; the rates vary from read to read, so tags of a
    few bytes (many reads per group) sit beside tags of several hundred."""
    rng = np.random.default_rng(seed)
    length = int(rng.integers(5_000, 50_000))
    ref = reference(rng, length)
    n = int(n_reads or rng.integers(30, 300))
    starts = np.sort(rng.integers(0, length - 2100, n))
    recs = []
    for ts in starts:
        span = int(rng.choice([60, 90, 150, 400, 900, 2000]) * rng.uniform(0.7, 1.0))
        rate = float(rng.choice([0.002, 0.01, 0.03, 0.1, 0.3]))
        ops = random_ops(rng, span, rate, long_form=rng.random() < 0.05)
        clip = int(rng.integers(1, 30)) if rng.random() < 0.2 else 0
        recs.append(read_from_ops(ref, int(ts), ops, rng, lead_clip=clip, trail_clip=clip // 2,
                                  bq=int(rng.choice([93, 93, 40])), mapq=int(rng.choice([60, 60, 60, 20])),
                                  flag=int(rng.choice([0, 0, 0, 0, 16, 0x100 if rng.random() < 0.3 else 0]))))
    return batch_from_records(name, length, recs), ref


# ---- the hand-made batches: name -> (records, reference).  Reads of a few bytes of text each share one group unless the
# case says otherwise.

def _short(ref, rng, ts, ops=None, **kw):
    return read_from_ops(ref, ts, ops or [("m", 40), ("s", 1), ("m", 30)], rng, **kw)


def trap_batches():
    rng = np.random.default_rng(11)
    ref = reference(rng, 30_000)
    S = lambda ts, ops=None, **kw: _short(ref, rng, ts, ops, **kw)
    out = {}
    out["secondary_in_group"] = [S(100), dict(S(120), flag=0x100, cs="!!bad bytes!!"), S(140), S(160)]
    out["double_insertion"] = [S(100), S(110, [("m", 20), ("i", "A"), ("i", "CG"), ("m", 20)]), S(120)]
    out["starts_with_indel"] = [S(100, [("i", "AC"), ("m", 30)]), S(105, [("d", 3), ("m", 30)]), S(110, [("i", "A"), ("d", 2), ("m", 9)]), S(130)]
    out["ends_with_indel"] = [S(100, [("m", 30), ("i", "AC")]), S(105, [("m", 30), ("d", 3)]), S(110, [("m", 5), ("s", 0), ("i", "T")]),
                              S(120, [("m", 9), ("d", 1), ("i", "GG")]), S(130, [("m", 9), ("i", "G"), ("i", "G")]), S(140)]
    out["n_reference"] = [S(100), S(110, [("m", 10), ("n", "A"), ("m", 5), ("s", 2), ("n", "C"), ("n", "G"), ("m", 3)]), S(120, [("n", "T"), ("m", 8)]),
                          S(130)]
    out["long_form_per_read"] = [S(100), S(110, [("=", 25), ("s", 1), ("=", 10)]), S(120), S(130, [("m", 5), ("=", 5)])]
    # a read of more than MARK_CAP substitutions (387 bytes and more: a group of one) between short ones
    out["many_substitutions"] = [S(100), S(110, [("s", i) for i in range(MARK_CAP + 9)]), S(120), S(130)]
    # a long read between two short ones, short ones behind it
    out["long_between_short"] = [S(100), S(105), S(110, random_ops(rng, 1500, 0.2)), S(120), S(125), S(130)]
    # the operation counts 64, 65 and 128 in a group, and a head that is operation 64 (the first of the second round)
    def ops_n(k):        # k operations: matches and substitutions in turn
        return [("m", 2) if i % 2 == 0 else ("s", i) for i in range(k)]
    out["ops_64"] = [S(100, ops_n(31)), S(110, ops_n(33))]
    out["ops_65"] = [S(100, ops_n(32)), S(110, ops_n(33))]
    out["ops_128"] = [S(100, ops_n(64)), S(110, ops_n(3)), S(120, ops_n(61))]
    out["head_is_op_64"] = [S(100, ops_n(30)), S(110, ops_n(34)), S(120, [("d", 2), ("m", 5)]), S(130, [("i", "A"), ("m", 5)])]
    # indels on both sides of a round boundary: the open read's run crosses it
    out["run_across_rounds"] = [S(100, ops_n(60) + [("i", "A"), ("m", 3), ("s", 0), ("m", 2), ("m", 2), ("d", 2), ("m", 4)]),
                                S(110, ops_n(62) + [("m", 5), ("d", 1), ("m", 5)]), S(120)]
    # the filters known before the qualities: one read of a group fails mapq, one the query length, one the identity
    out["filters_per_read"] = [S(100), S(105, mapq=3), S(110), S(115, [("m", 4), ("s", 0), ("s", 1), ("s", 2), ("m", 4)]), S(120),
                               S(125, [("m", 200), ("s", 1), ("m", 100)]), S(130)]
    out["one_read"] = [S(100)]
    out["two_reads"] = [S(100), S(100)]
    # exactly GROUP_MAX reads in a tile and one more: tags of ten bytes
    tiny = lambda ts: S(ts, [("m", 10), ("s", 0), ("m", 100)])     # ":10*xy:100": ten bytes
    out["tile_of_64"] = [tiny(100 + i) for i in range(GROUP_MAX)] + [S(400, random_ops(rng, 1200, 0.3))] + [tiny(500 + i) for i in range(GROUP_MAX + 1)]
    out["tile_of_65_first"] = [tiny(100 + i) for i in range(GROUP_MAX + 1)]
    # a group whose text is PB = 1,024 bytes: the last tag starts at the tile's last byte and is GROUP_LONG bytes long
    pad = lambda ts, nbytes: S(ts, [("m", 11), ("i", "A" * (nbytes - 4))])      # ":11+aaaa...": nbytes bytes
    last = S(160, [("m", 10)] + [("s", i) for i in range(80)] + [("i", "A" * (GROUP_LONG - 3 - 240 - 1))])
    assert len(last["cs"]) == GROUP_LONG, len(last["cs"])
    out["text_of_1024"] = [pad(100, 200), pad(110, 200), pad(120, 200), pad(130, GROUP_T - 1 - 600), last, S(170), S(180)]
    return {k: (v, ref) for k, v in out.items()}


def batch_of(records, ref, name="chrT"):
    return batch_from_records(name, len(ref), sorted(records, key=lambda r: r["tstart"]))


# ---- the group plan, restated

def plan_groups(cs_off):
    """[(first, end)] of the groups k_group_flags makes of cs_off."""
    off = [int(x) for x in cs_off]
    n = len(off) - 1
    first = []
    for r in range(n):
        start = r == 0
        if not start:
            a, b, e = off[r - 1], off[r], off[r + 1]
            start = a // GROUP_T != b // GROUP_T or e - b > GROUP_LONG or b - a > GROUP_LONG
            if not start:
                start = (r - bisect.bisect_left(off, (b // GROUP_T) * GROUP_T, 0, r)) % GROUP_MAX == 0
        if start:
            first.append(r)
    return list(zip(first, first[1:] + [n]))


def plan_counters(batch, mode=0):
    """The three counters the plan decides: groups, groups of several reads, reads planned for the per-read path (groups of
    one, groups that hold a secondary read, groups whose text is in long form)."""
    if mode == 1:
        return [batch.n, 0, batch.n]
    groups = plan_groups(batch.cs_off)
    sec = (np.asarray(batch.flag) & 0x100) != 0
    for a, b in groups:
        assert b - a <= GROUP_MAX and (b - a == 1 or int(batch.cs_off[b]) - int(batch.cs_off[a]) <= 1024)
    eq = lambda a, b: 61 in batch.cs[int(batch.cs_off[a]):int(batch.cs_off[b])]      # long form: a '=' in the group's text
    return [len(groups), sum(1 for a, b in groups if b - a > 1),
            sum(b - a for a, b in groups if b - a == 1 or sec[a:b].any() or eq(a, b))]


# ---- two read passes compared

def exact_marks(batch, rp, params):
    """The bitmap the decode owes: the substitutions (mismatch entries with bit 4 set) of the reads that pass mapq, the
    query length limits and the identity."""
    want = set()
    for r in range(batch.n):
        if not (rp["rflag"][r] & 4) or int(batch.mapq[r]) < params["min_mapq"]:
            continue
        if not (params["qlen_lower_limit"] < int(batch.qlen[r]) < params["qlen_upper_limit"]):
            continue
        s = (int(batch.cs_off[r]) >> 1) + r
        for k in range(int(rp["nmis"][r])):
            if int(rp["mq"][s + k]) & 16:
                want.add(int(rp["mis"][s + k]) - 1)
    return want


def bits_set(bits):
    w = np.flatnonzero(bits)
    return set(int(32 * i + j) for i in w for j in range(32) if (int(bits[i]) >> j) & 1)


def assert_same_read_pass(batch, a, b, what=""):
    """Every array of two copied-out read passes, entry by entry where a read owns the entry."""
    for k in ("nseg", "nmis", "nnsub", "rflag", "meta"):
        d = np.flatnonzero(a[k] != b[k])
        assert not len(d), "{}: {} differs at read {}: {} | {}".format(what, k, int(d[0]), a[k][d[0]], b[k][d[0]])
    for r in range(batch.n):
        s = (int(batch.cs_off[r]) >> 1) + r
        top = (int(batch.cs_off[r + 1]) >> 1) - (int(batch.cs_off[r]) >> 1)
        ns, nm, nn = int(a["nseg"][r]), int(a["nmis"][r]), int(a["nnsub"][r])
        assert np.array_equal(a["segs"][s:s + ns], b["segs"][s:s + ns]), "{}: segments of read {}: {} | {}".format(
            what, r, a["segs"][s:s + ns], b["segs"][s:s + ns])
        assert np.array_equal(a["mis"][s:s + nm], b["mis"][s:s + nm]), "{}: mismatch positions of read {}".format(what, r)
        assert np.array_equal(a["mq"][s:s + nm], b["mq"][s:s + nm]), "{}: mismatch entries of read {}".format(what, r)
        for k in range(nn):
            assert a["mq"][s + top - k] == b["mq"][s + top - k], "{}: N substitution {} of read {}".format(what, k, r)
