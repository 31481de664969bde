"""The haplotag run's contract (include/himut_hip.h, himut_run_haplotag) in plain Python
over a ReadBatch, written from the contract's text: a cs walk of its own, the classification of a read at a hetSNP, the
choice of the set, the verdict, the tallies per hetSNP and the counters, as numpy arrays of the two 32-byte layouts; and
the lines `himut haplotag` writes.  Nothing of the package is imported.  It is the checker of every GPU test."""
import numpy as np

ROW_DTYPE = np.dtype([("read", "<i4"), ("set", "<i4"), ("n0", "<u4"), ("n1", "<u4"), ("n_other", "<u4"), ("n_del", "<u4"),
                      ("n_lowbq", "<u4"), ("n_sets", "<u2"), ("hap", "u1"), ("status", "u1")])
SNP_DTYPE = np.dtype([(k, "<u4") for k in ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq", "agree", "disagree", "pad")])
assert ROW_DTYPE.itemsize == 32 and SNP_DTYPE.itemsize == 32

ASSIGNED, NOT_IN_PILE, NO_SNP, NO_VOTE, LOW_SUPPORT, CONFLICT = range(6)
STATUS_NAMES = ("Assigned", "NotInPile", "NoSnp", "NoVote", "LowSupport", "Conflict")
LOG_NAMES = ("reads", "pile", "hap0", "hap1", "NoSnp", "NoVote", "LowSupport", "Conflict", "multi_set", "votes", "other",
             "del", "lowbq")
READ_COLUMNS = ("chrom", "qname", "start", "end", "strand", "mapq", "PS", "HP", "status", "n_h1", "n_h2", "n_other", "n_del",
                "n_lowbq", "n_sets")
SNP_COLUMNS = ("chrom", "pos", "ref", "alt", "gt", "PS", "depth", "n_ref", "n_alt", "n_other", "n_del", "n_lowbq", "agree",
               "disagree")


class CoverError(Exception):
    """A spanned position that no segment of the read holds (HIMUT_ERR_COVER)."""


def segments(cs, tstart, qstart):
    """[(t0, t1, q0, deleted)] of a cs text: the stretches of the reference the read is aligned to, base by base from
    query offset q0 (counted from the start of SEQ), and the stretches it deletes."""
    out, t, q, k = [], tstart, qstart, 0
    while k < len(cs):
        j = k + 1
        while j < len(cs) and cs[j] not in ":*+-=":
            j += 1
        kind, payload = cs[k], cs[k + 1:j]
        if kind == ":":
            n = int(payload)
            out.append((t, t + n, q, False)); t += n; q += n
        elif kind == "=":
            n = len(payload)
            out.append((t, t + n, q, False)); t += n; q += n
        elif kind == "*":
            out.append((t, t + 1, q, False)); t += 1; q += 1
        elif kind == "+":
            q += len(payload)
        elif kind == "-":
            out.append((t, t + len(payload), q, True)); t += len(payload)
        else:
            raise ValueError("cs text: " + cs[k:j])
        k = j
    return out


def look(segs, seq, bq, rpos, ref, alt, min_bq):
    """What the read shows at the 0-based position: "del", "lowbq", 0 (ref), 1 (alt) or "other" -- the first rule that
    matches, in this order."""
    for t0, t1, q0, deleted in segs:
        if t0 <= rpos < t1:
            if deleted:
                return "del"
            q = q0 + rpos - t0
            if int(bq[q]) < min_bq:
                return "lowbq"
            return 0 if seq[q] == ref else 1 if seq[q] == alt else "other"
    raise CoverError(rpos)


def check_snps(snps, n_sets=None):
    """The rules of the hetSNP list [(pos1, ref, alt, bit, set)]; ValueError names the one that broke."""
    for k, (pos, ref, alt, bit, st) in enumerate(snps):
        if pos < 1 or (k and pos <= snps[k - 1][0]):
            raise ValueError("pos1 must be 1-based and strictly ascending")
        if ref not in tuple("ACGT") or alt not in tuple("ACGT") or ref == alt:
            raise ValueError("ref and alt must be different upper-case letters of ACGT")
        if bit not in (0, 1):
            raise ValueError("bit must be 0 or 1")
        if st < 0 or (n_sets is not None and st >= n_sets):
            raise ValueError("set out of range")


def haplotag(batch, snps, min_mapq=0, min_bq=20, min_snps=1, min_agree_permille=800, n_sets=None):
    """(rows, snp rows, the thirteen counters) of the hetSNPs [(pos1, ref, alt, bit, set)] on the batch's reads."""
    if min_snps < 1 or not 501 <= min_agree_permille <= 1000:
        raise ValueError("parameter out of range")
    check_snps(snps, n_sets)
    n = batch.n if batch is not None else 0
    rows = np.zeros(n, ROW_DTYPE)
    out = np.zeros(len(snps), SNP_DTYPE)
    log = dict.fromkeys(LOG_NAMES, 0)
    votes_at = []                                       # (read, hetSNP, haplotype voted for)
    for i in range(n):
        row = rows[i]
        row["read"], row["set"], row["hap"] = i, -1, 2
        log["reads"] += 1
        if int(batch.flag[i]) & 0x100 or int(batch.mapq[i]) < min_mapq:
            row["status"] = NOT_IN_PILE
            continue
        log["pile"] += 1
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        spanned = [k for k, s in enumerate(snps) if ts <= s[0] - 1 < te]
        if not spanned:
            row["status"] = NO_SNP
            log["NoSnp"] += 1
            continue
        segs = segments(batch.cs_tag(i), ts, int(batch.qstart[i]))
        seq, bq = batch.query_sequence(i), batch.query_qualities(i)
        per_set = {}                                    # set -> [n0, n1, other, del, lowbq]
        everywhere = [0, 0, 0, 0, 0]
        for k in spanned:
            pos, ref, alt, bit, st = snps[k]
            what = look(segs, seq, bq, pos - 1, ref, alt, min_bq)
            tally = per_set.setdefault(st, [0, 0, 0, 0, 0])
            if what in (0, 1):
                h = what ^ bit
                out[k]["n_ref" if what == 0 else "n_alt"] += 1
                tally[h] += 1
                everywhere[0] += 1
                votes_at.append((i, k, h))
            else:
                slot = {"other": 2, "del": 3, "lowbq": 4}[what]
                out[k][("n_other", "n_del", "n_lowbq")[slot - 2]] += 1
                tally[slot] += 1
                everywhere[slot] += 1
        log["votes"] += everywhere[0]; log["other"] += everywhere[2]; log["del"] += everywhere[3]; log["lowbq"] += everywhere[4]
        voted = sorted(s for s, t in per_set.items() if t[0] + t[1] > 0)
        row["n_sets"] = min(len(voted), 65535)
        if len(voted) >= 2:
            log["multi_set"] += 1
        if not voted:
            row["status"] = NO_VOTE
            row["n_other"], row["n_del"], row["n_lowbq"] = everywhere[2:]
            log["NoVote"] += 1
            continue
        best = max(voted, key=lambda s: (per_set[s][0] + per_set[s][1], -s))
        n0, n1, no, nd, nl = per_set[best]
        row["set"], row["n0"], row["n1"], row["n_other"], row["n_del"], row["n_lowbq"] = best, n0, n1, no, nd, nl
        if n0 + n1 < min_snps:
            row["status"] = LOW_SUPPORT
            log["LowSupport"] += 1
        elif n0 == n1 or max(n0, n1) * 1000 < min_agree_permille * (n0 + n1):
            row["status"] = CONFLICT
            log["Conflict"] += 1
        else:
            row["status"] = ASSIGNED
            row["hap"] = 0 if n0 > n1 else 1
            log["hap0" if n0 > n1 else "hap1"] += 1
    for i, k, h in votes_at:
        if int(rows[i]["status"]) == ASSIGNED and int(rows[i]["set"]) == snps[k][4]:
            out[k]["agree" if h == int(rows[i]["hap"]) else "disagree"] += 1
    return rows, out, [log[k] for k in LOG_NAMES]


def depth(snp_rows):
    """The spanning pile depth of every hetSNP."""
    return sum(snp_rows[k].astype(np.int64) for k in ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq"))


def assert_same(got, want):
    """(rows, snp rows, counters) against (rows, snp rows, counters): field by field, then the bytes."""
    (grows, gsnps, glog), (wrows, wsnps, wlog) = got, want
    assert grows.shape == wrows.shape and gsnps.shape == wsnps.shape, (grows.shape, wrows.shape, gsnps.shape, wsnps.shape)
    for name in ROW_DTYPE.names:
        assert np.array_equal(grows[name], wrows[name]), ("rows differ in " + name, grows[name].tolist(), wrows[name].tolist())
    for name in SNP_DTYPE.names:
        assert np.array_equal(gsnps[name], wsnps[name]), ("hetSNP rows differ in " + name, gsnps[name].tolist(), wsnps[name].tolist())
    assert list(glog) == list(wlog), (glog, wlog)
    assert grows.tobytes() == wrows.tobytes() and gsnps.tobytes() == wsnps.tobytes()


def check_identities(snps, rows, snp_rows, log):
    """What holds of every result: the counters' sums and the per-hetSNP bounds."""
    reads, pile, hap0, hap1, nosnp, novote, low, conflict, multi, votes, other, dele, lowbq = log
    assert reads == len(rows) and pile == int(np.sum(rows["status"] != NOT_IN_PILE))
    assert pile == hap0 + hap1 + nosnp + novote + low + conflict
    assert hap0 == int(np.sum((rows["status"] == ASSIGNED) & (rows["hap"] == 0)))
    assert hap1 == int(np.sum((rows["status"] == ASSIGNED) & (rows["hap"] == 1)))
    assert multi == int(np.sum(rows["n_sets"] >= 2))
    assert votes == int(snp_rows["n_ref"].sum() + snp_rows["n_alt"].sum())
    assert (other, dele, lowbq) == tuple(int(snp_rows[k].sum()) for k in ("n_other", "n_del", "n_lowbq"))
    assert np.all(snp_rows["agree"] + snp_rows["disagree"] <= snp_rows["n_ref"] + snp_rows["n_alt"])
    assert np.all(snp_rows["pad"] == 0)
    out = rows[rows["status"] == NOT_IN_PILE]
    assert all(np.all(out[k] == 0) for k in ("n0", "n1", "n_other", "n_del", "n_lowbq", "n_sets")) and np.all(out["set"] == -1)


# ---- the lines of `himut haplotag`

def read_lines(chrom, batch, rows, set_names, name_of=None):
    """One line per read: chrom qname start end strand mapq PS HP status n_h1 n_h2 n_other n_del n_lowbq n_sets; start is
    1-based, HP is hap + 1 or ".", PS the chosen set's name or "."."""
    out = []
    for r in rows:
        i = int(r["read"])
        qname = name_of(i) if name_of else batch.query_name(i)
        ps = set_names[int(r["set"])] if int(r["set"]) >= 0 else "."
        hp = str(int(r["hap"]) + 1) if int(r["hap"]) < 2 else "."
        out.append("\t".join(str(x) for x in (
            chrom, qname, int(batch.tstart[i]) + 1, int(batch.tend[i]), "-" if int(batch.flag[i]) & 0x10 else "+",
            int(batch.mapq[i]), ps, hp, STATUS_NAMES[int(r["status"])], int(r["n0"]), int(r["n1"]), int(r["n_other"]),
            int(r["n_del"]), int(r["n_lowbq"]), int(r["n_sets"]))))
    return out


def snp_lines(chrom, snps, snp_rows, set_names):
    """One line per hetSNP: chrom pos ref alt gt PS depth n_ref n_alt n_other n_del n_lowbq agree disagree."""
    out = []
    for (pos, ref, alt, bit, st), r in zip(snps, snp_rows):
        counts = [int(r[k]) for k in ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq")]
        out.append("\t".join(str(x) for x in [chrom, pos, ref, alt, "1|0" if bit else "0|1", set_names[st], sum(counts)] + counts +
                             [int(r["agree"]), int(r["disagree"])]))
    return out
