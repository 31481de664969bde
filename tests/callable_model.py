"""Which query bases count in `normcounts`, in plain Python: normcounts.update_tri2count (normcounts.py:65-110) over
cslib.cs2tuple / cs2subindel (cslib.py:13-64) and bamlib.get_mismatch_range, get_trimmed_range, is_trimmed
(bamlib.py:222-258), behind the read filters of normcounts.py:292-311.  Dictionaries, lists and bisect, a tokenizer of
its own, nothing of k_callable or the C oracle.

``callable_bits`` gives what himut_debug_norm_callable reads back: ``live`` per read and one bit per query base, bit
q & 31 of word (qoff[r] + q) >> 5, q from offset 0 of the query.  A read that fails a filter, or that no chunk
fetches, has no bit set.  ``rules`` switches single rules to a deliberately wrong variant: tests/test_callable_cpu.py
uses them to show that the hand-built reads of tests/callable_cases.py tell the right rule from the wrong one."""
import bisect
import math
import re

import numpy as np

# one switch per rule under test; every one of them makes the model wrong
RULES = ("window_at_base",   # the window get_mismatch_range gives for the base itself, not for the start of its match operation
         "list_0based",      # the mismatch list holds 0-based positions (tpos, not tpos + 1)
         "sub_tested",       # a substitution counts only if it passes the three tests of a match base
         "nsub_listed",      # a substitution whose reference base is n is in the mismatch list
         "nsub_same_op",     # ... and the match bases behind it keep the window of the operation in front of it
         "bq_le",            # bq <= min_bq is low quality, in place of bq < min_bq
         "trim_strict",      # qpos <= floor(t qlen) or qpos >= ceil((1 - t) qlen) is trimmed
         "minus_one",        # the count less one, as in the call path's is_mismatch_conflict (bamlib.py:266-282)
         "dr_w_at_start",    # an operation that starts within w of the read's start reaches w downstream, not w - qs
         "qe_ge",            # qe >= qlen in place of qe > qlen
         "trim_end_floor")   # the trimmed end is qlen - floor(t qlen), not ceil((1 - t) qlen)

_TOKEN = re.compile(r":[0-9]+|\*[a-z][a-z]|[=+\-][A-Za-z]+")


def cs_tuples(cs):
    """cslib.cs2tuple without the bases: [(state, ref, ref_len, alt_len)], state 1 match, 2 substitution, 3 insertion,
    4 deletion; ref is the (upper-case) reference base of a substitution, "" otherwise."""
    out = []
    assert "".join(_TOKEN.findall(cs)) == cs, cs
    for tok in _TOKEN.findall(cs):
        body = tok[1:]
        if tok[0] == "=":
            out.append((1, "", len(body), len(body)))
        elif tok[0] == ":":
            out.append((1, "", int(body), int(body)))
        elif tok[0] == "*":
            out.append((2, body[0].upper(), 1, 1))
        elif tok[0] == "+":
            out.append((3, "", 0, len(body)))
        else:
            out.append((4, "", len(body), 0))
    return out


def mismatch_positions(tstart, tuples, rules=()):
    """cs2subindel's mismatch_lst positions: 1-based; a substitution whose reference base is N is left out."""
    lst = []
    tpos = tstart
    for state, ref, ref_len, _alt_len in tuples:
        if state == 2 and (ref != "N" or "nsub_listed" in rules):
            lst.append(tpos if "list_0based" in rules else tpos + 1)
        elif state == 3 or state == 4:
            lst.append(tpos if "list_0based" in rules else tpos + 1)
        tpos += ref_len
    return lst


def mismatch_range(tpos, qpos, qlen, window, rules=()):
    """bamlib.get_mismatch_range."""
    qstart, qend = qpos - window, qpos + window
    if qstart < 0:
        urange = window + qstart
        drange = window if "dr_w_at_start" in rules else window + abs(qstart)
    elif (qend >= qlen) if "qe_ge" in rules else (qend > qlen):
        urange = window + abs(qend - qlen)
        drange = qlen - qpos
    else:
        urange = window
        drange = window
    return tpos - urange, tpos + drange


def trimmed_range(qlen, min_trim, rules=()):
    """bamlib.get_trimmed_range."""
    lo = math.floor(min_trim * qlen)
    hi = qlen - lo if "trim_end_floor" in rules else math.ceil((1 - min_trim) * qlen)
    return lo, hi


def is_trimmed(qpos, lo, hi, rules=()):
    if "trim_strict" in rules:
        return qpos <= lo or qpos >= hi
    return qpos < lo or qpos > hi


def counted(tstart, qstart, qlen, bq, cs, p, rules=()):
    """update_tri2count of one read: {reference position (0-based): query offset} of the bases that count."""
    rules = set(rules)
    assert rules <= set(RULES), rules - set(RULES)
    w, maxmm, min_bq = p["mismatch_window_size"], p["max_mismatch_count"], p["min_bq"]
    tuples = cs_tuples(cs)
    mis = mismatch_positions(tstart, tuples, rules)
    lo, hi = trimmed_range(qlen, p["min_trim"], rules)
    out = {}
    rpos, qpos = tstart, qstart
    op_rpos, op_qpos = None, None                  # (nsub_same_op: the operation in front of an n substitution goes on)
    for state, ref, ref_len, alt_len in tuples:
        if state == 1:
            if "nsub_same_op" in rules and op_rpos is not None:
                t0, q0 = op_rpos, op_qpos
            else:
                t0, q0 = rpos, qpos
            ts, te = mismatch_range(t0, q0, qlen, w, rules)
            for j in range(ref_len):
                if "window_at_base" in rules:
                    ts, te = mismatch_range(rpos + j, qpos + j, qlen, w, rules)
                    shift = 0
                else:
                    shift = rpos + j - t0
                count = bisect.bisect_right(mis, te + shift) - bisect.bisect_left(mis, ts + shift)
                if "minus_one" in rules:
                    count -= 1
                low = bq[qpos + j] <= min_bq if "bq_le" in rules else bq[qpos + j] < min_bq
                if low:
                    continue
                if count > maxmm:
                    continue
                if is_trimmed(qpos + j, lo, hi, rules):
                    continue
                assert rpos + j not in out
                out[rpos + j] = qpos + j
            op_rpos, op_qpos = t0, q0
        elif state == 2:
            keep = True
            if "sub_tested" in rules:
                ts, te = mismatch_range(rpos, qpos, qlen, w, rules)
                count = bisect.bisect_right(mis, te) - bisect.bisect_left(mis, ts) - 1
                keep = not (bq[qpos] < min_bq or count > maxmm or is_trimmed(qpos, lo, hi, rules))
            if keep:
                assert rpos not in out                    # a substitution and a match never share a position
                out[rpos] = qpos
            if not ("nsub_same_op" in rules and ref == "N"):
                op_rpos = None
        else:
            op_rpos = None
        rpos += ref_len
        qpos += alt_len
    return out


def identity(cs):
    """BAM.get_blast_sequence_identity (bamlib.py:47-63)."""
    match = mismatch = 0
    for state, _ref, ref_len, alt_len in cs_tuples(cs):
        if state == 1:
            match += ref_len
        elif state == 2 or state == 3:
            mismatch += alt_len
        else:
            mismatch += ref_len
    return match / float(match + mismatch)


def read_is_live(batch, i, chunks, p):
    """The read filters of normcounts.py:292-311 without --phase, and "some chunk fetches the read" (:292: start <
    tend and end > tstart)."""
    if int(batch.flag[i]) & 0x100:
        return False
    tstart, tend, qlen = int(batch.tstart[i]), int(batch.tend[i]), int(batch.qlen[i])
    if not any(s < tend and e > tstart for s, e in chunks):
        return False
    q = [int(x) for x in batch.query_qualities(i)]
    if sum(q) / float(len(q)) < p["min_qv"]:
        return False
    if int(batch.mapq[i]) < p["min_mapq"]:
        return False
    if identity(batch.cs_tag(i)) < p["min_sequence_identity"]:
        return False
    if not (p["qlen_lower_limit"] < qlen and qlen < p["qlen_upper_limit"]):
        return False
    return True


def read_counted(batch, i, p, rules=()):
    return counted(int(batch.tstart[i]), int(batch.qstart[i]), int(batch.qlen[i]),
                   [int(x) for x in batch.query_qualities(i)], batch.cs_tag(i), p, rules)


def callable_bits(batch, chunks, p, rules=()):
    """(live uint8[n], words uint32[len(bq) / 32]) in the layout of himut_debug_norm_callable."""
    live = np.zeros(batch.n, np.uint8)
    words = [0] * (int(batch.bq.shape[0]) >> 5)
    for i in range(batch.n):
        if not read_is_live(batch, i, chunks, p):
            continue
        live[i] = 1
        qoff = int(batch.qoff[i])
        for _rpos, q in read_counted(batch, i, p, rules).items():
            words[(qoff + q) >> 5] |= 1 << (q & 31)
    return live, np.array(words, np.uint64).astype(np.uint32)


def first_difference(batch, got_live, got_words, want_live, want_words):
    """None, or a line that names the first read and query base at which two results differ."""
    for i in range(batch.n):
        if int(got_live[i]) != int(want_live[i]):
            return "read {} ({}): live {} != {}".format(i, batch.query_name(i), int(got_live[i]), int(want_live[i]))
        qoff, qlen = int(batch.qoff[i]), int(batch.qlen[i])
        a, b = got_words[qoff >> 5:(qoff + qlen + 31) >> 5], want_words[qoff >> 5:(qoff + qlen + 31) >> 5]
        if not np.array_equal(a, b):
            k = int(np.flatnonzero(a != b)[0])
            x = int(a[k]) ^ int(b[k])
            q = 32 * k + (x & -x).bit_length() - 1
            return "read {} ({}): query base {} (word {}, bit {}; qlen {}): got {}, want {}; words {:08x} != {:08x}".format(
                i, batch.query_name(i), q, k, q & 31, qlen, (int(a[k]) >> (q & 31)) & 1, (int(b[k]) >> (q & 31)) & 1,
                int(a[k]), int(b[k]))
    if not np.array_equal(got_words, want_words):
        k = int(np.flatnonzero(got_words != want_words)[0])
        return "word {} outside every read: {:08x} != {:08x}".format(k, int(got_words[k]), int(want_words[k]))
    return None
