"""The duplex run's contract (include/himut_hip.h, himut_run_duplex) in plain Python over a
ReadBatch, written from the contract's text: a cs walk of its own for the substitution list, the mismatch list and the
identity; call's read filters; the pairs in play; a read's own rules on an event; the mate's state; the double-strand
events and the candidates; the single-strand spectrum; the denominator; the forty counters and their identities.  The
first 64 bytes of a record are the sites model's record of the candidate (tests/sites_model.py), the segments of a read
are the haplotag model's (tests/haplotag_model.py).  Nothing of the package is imported.  It is the checker of every GPU
test."""
import bisect
import math

import numpy as np

from tests import haplotag_model as H
from tests import sites_model as S

RECORD_DTYPE = np.dtype(S.SITE_RECORD_DTYPE.descr + [("n_ds", "<u4"), ("n_ss", "<u4"), ("n_alt_unpaired", "<u4"),
                                                     ("reserved2", "<u4")])
assert RECORD_DTYPE.itemsize == 80
BASES = "ATGC"                                            # the allele order of the records
LOG = ("reads", "pile_reads", "proposing_reads", "pairs", "pairs_in_play", "pairs_notpile", "pairs_identity", "pairs_lowqv",
       "pairs_qlen", "events", "num_trim", "num_window", "num_lowbq", "nocover", "del", "lowbq", "trim", "concordant", "single",
       "other", "num_mate_window", "ds_events", "ds_events_in_chunk", "ss_events_in_chunk", "ds_bases", "ds_pairs_overlap",
       "candidates", "Germline") + tuple(S.VERDICTS) + ("reserved",)
assert len(LOG) == 40
SS_CLASSES = tuple(a + ">" + b for a in "ACGT" for b in "ACGT" if a != b)
STATES = ("nocover", "del", "lowbq", "trim", "concordant", "single", "other")
CAUSES = ("pairs_notpile", "pairs_identity", "pairs_lowqv", "pairs_qlen")
COMPLEMENT = {"A": "T", "T": "A", "G": "C", "C": "G"}
DEFAULTS = S.DEFAULTS


def get_mismatch_range(tpos, qpos, qlen, window):                     # bamlib.py:245-258
    qstart, qend = qpos - window, qpos + window
    if qstart < 0:
        urange, drange = window + qstart, window + abs(qstart)
    elif qend > qlen:
        urange, drange = window + abs(qend - qlen), qlen - qpos
    else:
        urange = drange = window
    return tpos - urange, tpos + drange


def is_trimmed(qpos, qlen, min_trim):                                 # bamlib.py:222-242
    return qpos < math.floor(min_trim * qlen) or qpos > math.ceil((1 - min_trim) * qlen)


class Read:
    """Read i from its cs text: subs [(p, ref, alt, q)] with p 0-based and q the query offset -- cs2subindel's list
    (cslib.py:47-64), letters upper-cased, a reference base N left out; positions, that list's 1-based positions with the
    insertions' and deletions' among them; the identity (bamlib.py:47-63); the segments; SEQ and the qualities."""

    def __init__(self, batch, i):
        cs = batch.cs_tag(i)
        self.i = i
        self.tstart, self.tend, self.qlen = int(batch.tstart[i]), int(batch.tend[i]), int(batch.qlen[i])
        self.flag, self.mapq = int(batch.flag[i]), int(batch.mapq[i])
        self.seq = batch.query_sequence(i)
        self.bq = [int(x) for x in batch.query_qualities(i)]
        self.segs = H.segments(cs, self.tstart, int(batch.qstart[i]))
        self.subs, self.positions = [], []
        t, q, k, match, mism = self.tstart, int(batch.qstart[i]), 0, 0, 0
        while k < len(cs):
            j = k + 1
            while j < len(cs) and cs[j] not in ":*+-=":
                j += 1
            kind, body = cs[k], cs[k + 1:j]
            if kind == ":":
                match += int(body); t += int(body); q += int(body)
            elif kind == "=":
                match += len(body); t += len(body); q += len(body)
            elif kind == "*":
                mism += 1
                if body[0].upper() != "N":
                    self.positions.append(t + 1)
                    self.subs.append((t, body[0].upper(), body[1].upper(), q))
                t += 1; q += 1
            elif kind == "+":
                mism += len(body)
                self.positions.append(t + 1)
                q += len(body)
            else:
                mism += len(body)
                self.positions.append(t + 1)
                t += len(body)
            k = j
        self.identity = match / float(match + mism) if match + mism else 0.0

    def verdict(self, p):
        """None: the read proposes (a pile read that passes caller.py:310-317); else the first cause it does not."""
        if self.flag & 0x100 or self.mapq < p["min_mapq"]:
            return "pairs_notpile"
        if self.identity < p["min_sequence_identity"]:
            return "pairs_identity"
        if sum(self.bq) < p["min_qv"] * self.qlen:
            return "pairs_lowqv"
        if not p["qlen_lower_limit"] < self.qlen < p["qlen_upper_limit"]:
            return "pairs_qlen"
        return None

    def crowded(self, pos, q, p):
        """The mismatch window of the entry at 0-based pos, query offset q, holds more than max_mismatch_count others."""
        s, e = get_mismatch_range(pos + 1, q, self.qlen, p["mismatch_window_size"])
        return bisect.bisect_right(self.positions, e) - bisect.bisect_left(self.positions, s) - 1 > p["max_mismatch_count"]

    def own_rule(self, pos, q, p):
        """The first of its own rules the event fails: "num_trim", "num_window", "num_lowbq", or None."""
        if is_trimmed(q, self.qlen, p["min_trim"]):
            return "num_trim"
        if self.crowded(pos, q, p):
            return "num_window"
        if self.bq[q] < p["min_bq"]:
            return "num_lowbq"
        return None

    def base_at(self, pos, p):
        """What the read holds at 0-based pos inside [tstart, tend): ("del" | "lowbq" | "trim", None) or ("base", q)."""
        for t0, t1, q0, deleted in self.segs:
            if t0 <= pos < t1:
                if deleted:
                    return "del", None
                q = q0 + pos - t0
                if self.bq[q] < p["min_bq"]:
                    return "lowbq", q
                if is_trimmed(q, self.qlen, p["min_trim"]):
                    return "trim", q
                return "base", q
        raise H.CoverError(pos)

    def state_for(self, pos, ref, alt, p):
        """(the state of this read as the mate of an event (pos, ref, alt), its query offset there)."""
        if not self.tstart <= pos < self.tend:
            return "nocover", None
        what, q = self.base_at(pos, p)
        if what != "base":
            return what, q
        b = self.seq[q]
        return ("concordant" if b == alt else "single" if b == ref else "other"), q


def check_mate(mate, n):
    """The rules of mate[]; ValueError names the one that broke."""
    if len(mate) != n:
        raise ValueError("mate must have an entry per read")
    for i, m in enumerate(mate):
        m = int(m)
        if m == -1:
            continue
        if m < -1 or m >= n:
            raise ValueError("mate[{}] lies outside -1..n-1".format(i))
        if m == i:
            raise ValueError("mate[{}] is the read itself".format(i))
        if int(mate[m]) != i:
            raise ValueError("mate[mate[{}]] is not {}".format(i, i))


def ss_class(ref, alt, flag):
    if flag & 0x10:
        ref, alt = COMPLEMENT[ref], COMPLEMENT[alt]
    return SS_CLASSES.index(ref + ">" + alt)


def run(batch, mate, chunks, prior=1 / (10 ** 3), pon_keys=(), com_keys=(), **kw):
    """(records, ss[12], log[40]) of the batch under mate[] and the chunks [(start, end)]."""
    p = dict(DEFAULTS, **kw)
    n = batch.n if batch is not None else 0
    check_mate(mate, n)
    chunks = [(int(s), int(e)) for s, e in chunks]

    def inside(pos):
        return any(s <= pos < e for s, e in chunks)
    log = dict.fromkeys(LOG, 0)
    reads = [Read(batch, i) for i in range(n)]
    verdicts = [r.verdict(p) for r in reads]
    log["reads"] = n
    log["pile_reads"] = sum(v != "pairs_notpile" for v in verdicts)
    log["proposing_reads"] = sum(v is None for v in verdicts)
    play = [False] * n
    for i in range(n):
        m = int(mate[i])
        if m < 0:
            continue
        play[i] = verdicts[i] is None and verdicts[m] is None
        if m > i:
            log["pairs"] += 1
            if play[i]:
                log["pairs_in_play"] += 1
            else:                                          # the first cause, in the order of CAUSES, that either read shows
                log[min((v for v in (verdicts[i], verdicts[m]) if v), key=CAUSES.index)] += 1
    ss = [0] * 12
    n_ds, n_ss, n_unp = {}, {}, {}
    for i in range(n):
        if not play[i]:
            continue
        a, b = reads[i], reads[int(mate[i])]
        for pos, ref, alt, q in a.subs:
            log["events"] += 1
            failed = a.own_rule(pos, q, p)
            if failed:
                log[failed] += 1
                continue
            state, qb = b.state_for(pos, ref, alt, p)
            log[state] += 1
            key = (pos + 1, BASES.index(ref), BASES.index(alt))
            if state == "single":
                n_ss[key] = n_ss.get(key, 0) + 1
                if inside(pos):
                    ss[ss_class(ref, alt, a.flag)] += 1
            if state != "concordant":
                continue
            if b.crowded(pos, qb, p):
                log["num_mate_window"] += 1
            elif i < b.i:                                  # seen from both reads, counted from the lower
                log["ds_events"] += 1
                if inside(pos):
                    log["ds_events_in_chunk"] += 1
                    n_ds[key] = n_ds.get(key, 0) + 1
    for i in range(n):
        if verdicts[i] == "pairs_notpile" or play[i]:
            continue
        for pos, ref, alt, _q in reads[i].subs:
            key = (pos + 1, BASES.index(ref), BASES.index(alt))
            n_unp[key] = n_unp.get(key, 0) + 1
    # the denominator
    for i in range(n):
        m = int(mate[i])
        if not (play[i] and m > i):
            continue
        a, b = reads[i], reads[m]
        count = 0
        for pos in range(max(a.tstart, b.tstart), min(a.tend, b.tend)):
            if inside(pos) and a.base_at(pos, p)[0] == "base" and b.base_at(pos, p)[0] == "base":
                count += 1
        log["ds_bases"] += count
        log["ds_pairs_overlap"] += count > 0
    log["ss_events_in_chunk"] = sum(ss)
    keys = sorted(n_ds)
    sites = [(pos1, BASES[r], BASES[a]) for pos1, r, a in keys]
    srecs, slog = S.run(batch, sites, prior=prior, pon_keys=pon_keys, com_keys=com_keys, **p)
    log["candidates"] = len(keys)
    assert slog[1] == 0, "a candidate has a read over it"
    log["Germline"] = slog[2]
    for k, v in enumerate(S.VERDICTS):
        log[v] = slog[3 + k]
    out = np.zeros(len(keys), RECORD_DTYPE)
    for name in S.SITE_RECORD_DTYPE.names:
        out[name] = srecs[name]
    out["n_ds"] = [n_ds[k] for k in keys]
    out["n_ss"] = [n_ss.get(k, 0) for k in keys]
    out["n_alt_unpaired"] = [n_unp.get(k, 0) for k in keys]
    log = [log[k] for k in LOG]
    check_identities(out, ss, log)
    return out, ss, log


def logd(log):
    return dict(zip(LOG, (int(x) for x in log)))


def check_identities(recs, ss, log):
    """The identities between the counters the contract states."""
    d = logd(log)
    assert d["pairs"] == d["pairs_in_play"] + sum(d[k] for k in CAUSES), d
    assert d["events"] == d["num_trim"] + d["num_window"] + d["num_lowbq"] + sum(d[k] for k in STATES), d
    assert d["concordant"] == 2 * d["ds_events"] + d["num_mate_window"], d
    assert d["candidates"] == d["Germline"] + sum(d[v] for v in S.VERDICTS) == len(recs), d
    assert d["ss_events_in_chunk"] == sum(int(x) for x in ss) and d["ds_events_in_chunk"] == int(np.sum(recs["n_ds"])), d
    assert d["proposing_reads"] <= d["pile_reads"] <= d["reads"] and 2 * d["pairs"] <= d["reads"] and d["reserved"] == 0
    assert d["ds_events_in_chunk"] <= d["ds_events"] and d["ds_pairs_overlap"] <= d["pairs_in_play"]
    for r in recs:                                         # every read the three counts name carries alt in the pile
        assert int(r["counts"][BASES.index(chr(r["alt"]))]) >= 2 * int(r["n_ds"]) + int(r["n_ss"]) + int(r["n_alt_unpaired"]), r
        assert int(r["n_ds"]) >= 1 and int(r["reserved2"]) == 0
    return d


def assert_same(got, want):
    """(records, ss, log) against (records, ss, log): the counters, field by field, then the bytes."""
    (grecs, gss, glog), (wrecs, wss, wlog) = got, want
    assert [int(x) for x in glog] == [int(x) for x in wlog], (logd(glog), logd(wlog))
    assert [int(x) for x in gss] == [int(x) for x in wss], (gss, wss)
    assert len(grecs) == len(wrecs), (len(grecs), len(wrecs))
    for name in RECORD_DTYPE.names:
        assert np.array_equal(grecs[name], wrecs[name]), (name, grecs[name][:8], wrecs[name][:8])
    assert grecs.tobytes() == wrecs.tobytes()
