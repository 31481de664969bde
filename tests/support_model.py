"""The support run's contract (include/himut_hip.h, himut_run_support) in plain Python over
a ReadBatch, written from the contract's text: a cs scanner of its own, the mismatch window, and the rows and site
counts as numpy arrays of SUPPORT_ROW_DTYPE.  tests/test_support_cpu.py pins it to the reference's recorded results."""
import bisect
import math

import numpy as np

from himut_amd._ffi import SUPPORT_ROW_DTYPE

OP_STARTS = ":*+-="


def cs_operations(text):
    """[(kind, payload)] of a cs text: an operation begins at one of ``: * + - =`` and its payload runs up to the next
    such byte (payload bytes are digits or letters, never one of the five)."""
    ops, k = [], 0
    if text and text[0] not in OP_STARTS:
        raise ValueError("cs text does not begin with an operation: " + text[:16])
    while k < len(text):
        j = k + 1
        while j < len(text) and text[j] not in OP_STARTS:
            j += 1
        kind, payload = text[k], text[k + 1:j]
        ok = (payload.isdigit() if kind == ":" else len(payload) == 2 and payload.isalpha() and payload.islower()
              if kind == "*" else payload.isalpha()) and payload.isascii()
        if not ok:
            raise ValueError("malformed cs operation: " + text[k:j])
        ops.append((kind, payload))
        k = j
    return ops


def cs_walk(batch, i):
    """Of read i, in cs order: its substitutions [(pos1, ref, alt, qpos)] -- letters upper-cased, those whose reference
    base is N left out, qpos counted from the start of SEQ (the leading soft clip included) -- and the 1-based
    positions of its mismatch list: those substitutions plus one entry per insertion and per deletion operation, an
    indel standing at the position of the reference base that follows the aligned run in front of it."""
    t, q = int(batch.tstart[i]), int(batch.qstart[i])
    subs, mismatches = [], []
    for kind, payload in cs_operations(batch.cs_tag(i)):
        if kind == ":":
            t += int(payload); q += int(payload)
        elif kind == "=":
            t += len(payload); q += len(payload)
        elif kind == "*":
            ref, alt = payload.upper()
            if ref != "N":
                subs.append((t + 1, ref, alt, q))
                mismatches.append(t + 1)
            t += 1; q += 1
        else:
            mismatches.append(t + 1)
            if kind == "+":
                q += len(payload)
            else:
                t += len(payload)
    return subs, mismatches


def mismatch_range(pos1, qpos, qlen, w):
    """The window [s, e] of reference positions the contract counts mismatches in: w to either side of pos1, shifted
    back inside the read where it would leave it.  Too close to the start of the read (qpos < w): what is missing on
    the left, w - qpos, is cut off there and added on the right.  Else too close to its end (qpos + w > qlen): the
    right side ends with the read, qlen - qpos, and the overhang qpos + w - qlen is added on the left."""
    if qpos < w:
        return pos1 - qpos, pos1 + w + (w - qpos)
    if qpos + w > qlen:
        return pos1 - w - (qpos + w - qlen), pos1 + (qlen - qpos)
    return pos1 - w, pos1 + w


def window_mismatches(mismatches, pos1, qpos, qlen, w):
    """Entries of the sorted mismatch list inside the window, the substitution itself not counted."""
    s, e = mismatch_range(pos1, qpos, qlen, w)
    return bisect.bisect_right(mismatches, e) - bisect.bisect_left(mismatches, s) - 1


def could_propose(row, p):
    """Whether the read of ``row`` passes the read and substitution filters of the call run under the parameters ``p``
    (tests.util.params_of): mapping quality, mean base quality, query length, the trimmed read ends -- the first
    floor(min_trim * qlen) and everything behind ceil((1 - min_trim) * qlen) -- and the mismatch window."""
    qlen, qpos = int(row["qlen"]), int(row["qpos"])
    return (int(row["mapq"]) >= p["min_mapq"] and int(row["bq_sum"]) / qlen >= p["min_qv"] and
            p["qlen_lower_limit"] < qlen < p["qlen_upper_limit"] and
            math.floor(p["min_trim"] * qlen) <= qpos <= math.ceil((1 - p["min_trim"]) * qlen) and
            int(row["window_mismatches"]) <= p["max_mismatch_count"])


def support(batch, sites, min_mapq=0, mismatch_window_size=20):
    """(rows ascending by (site, read), site_counts[n_sites, 2] = cover, alt_reads) of ``sites`` = [(pos1, ref, alt)]
    with pos1 non-decreasing."""
    pos = np.array([s[0] for s in sites], np.int64)
    assert np.all(np.diff(pos) >= 0)
    counts = np.zeros((len(sites), 2), np.int32)
    by_triple = {}
    for k, s in enumerate(sites):
        by_triple.setdefault((int(s[0]), s[1], s[2]), []).append(k)
    per_site = [[] for _ in sites]
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100 or int(batch.mapq[i]) < min_mapq:
            continue
        ts, te, qlen = int(batch.tstart[i]), int(batch.tend[i]), int(batch.qlen[i])
        lo, hi = np.searchsorted(pos, ts, "right"), np.searchsorted(pos, te, "right")   # tstart <= pos1 - 1 < tend
        counts[lo:hi, 0] += 1
        if lo == hi:
            continue
        subs, mismatches = cs_walk(batch, i)
        bq = np.asarray(batch.query_qualities(i), np.int64)
        for (pos1, ref, alt, qpos) in subs:
            for k in by_triple.get((pos1, ref, alt), ()):
                row = np.zeros((), SUPPORT_ROW_DTYPE)
                row["site"], row["read"], row["qid"] = k, i, int(batch.qid[i])
                row["tstart"], row["tend"], row["qlen"] = ts, te, qlen
                row["flag"], row["mapq"], row["bq"], row["qpos"] = int(batch.flag[i]), int(batch.mapq[i]), int(bq[qpos]), qpos
                row["bq_sum"], row["n_sub"], row["n_indel"] = int(bq.sum()), len(subs), len(mismatches) - len(subs)
                row["window_mismatches"] = window_mismatches(mismatches, pos1, qpos, qlen, mismatch_window_size)
                per_site[k].append(row)
                counts[k, 1] += 1
    flat = [r for rows in per_site for r in rows]
    rows = np.array(flat, SUPPORT_ROW_DTYPE) if flat else np.zeros(0, SUPPORT_ROW_DTYPE)
    return rows, counts


def assert_same(got, want):
    """(rows, site_counts) against (rows, site_counts), field by field."""
    (grows, gcounts), (wrows, wcounts) = got, want
    assert np.array_equal(np.asarray(gcounts), np.asarray(wcounts)), "site counts differ"
    assert grows.dtype == SUPPORT_ROW_DTYPE and grows.shape == wrows.shape, (grows.shape, wrows.shape)
    for name in SUPPORT_ROW_DTYPE.names:
        assert np.array_equal(grows[name], wrows[name]), "rows differ in " + name
