"""The dbs run's contract (himut_run_dbs) in plain Python: nothing of the device side.

A read batch, a region list, call's parameters, a prior and the two site sets in; doublet records, the twenty counters
and the VCF body out.  The mismatch list of a read is cslib.cs2subindel's, rebuilt from the cs operations
(oracle.cs_ops); piles are germline_model.PileRead's, in file order; every half goes through oracle.germ_gt (the
reference's gtlib.get_germ_gt; get_germ_gq(som_gt, ...) is called with a two-letter string that equals no base, so its
number is get_germ_gt's: oracle.germ_gq, the normcounts form that leaves a base out, is not the one) and through the
non-phased cascade of caller.py:332-550, restated below."""
import bisect
import math

import numpy as np

from oracle import oracle as O
from tests.germline_model import DEL, ERR_BASE, ERR_BQ0, NONE, OTHER, ModelError, PileRead, make_read  # noqa: F401

DBS_RECORD_DTYPE = np.dtype([("tpos", "<i4"), ("gq", "<i4"), ("ref", "u1", (2,)), ("alt", "u1", (2,)), ("status", "u1"),
                             ("half_status", "u1", (2,)), ("pad0", "u1"), ("gt_state", "u1", (2,)), ("gt", "u1", (2, 2)),
                             ("pad1", "u1", (2,)), ("half_gq", "<i4", (2,)), ("counts", "<u4", (2, 6)),
                             ("alt_bqsum", "<u4", (2,)), ("both_alt", "<u4"), ("both_ref", "<u4"), ("one_alt", "<u4"),
                             ("n_proposers", "<u4"), ("pad2", "<u4", (2,))])
BASES = "ATGC"
STATES = ["homref", "het", "hetalt", "homalt"]
STATUS = O.STATUS                                   # HIMUT_ST_* in code order
ST = {name: k for k, name in enumerate(STATUS)}
# the order of precedence between the halves, then the verdicts only the joint counts give; log[7 + k] counts VERDICTS[k]
PRECEDENCE = ["HetSite", "HetAltSite", "HomAltSite", "IndelSite", "LowGQ", "LowBQ", "PanelOfNormal", "ComSnp"]
VERDICTS = PRECEDENCE + ["LowDepth", "HighDepth", "PASS"]
LOG_ROWS = ["num_ccs", "num_dbs_runs", "num_mbs", "num_trimmed", "num_mismatch_conflict", "num_dbs", "num_germ"] + \
           ["num_" + v for v in VERDICTS] + ["reserved0", "reserved1"]
GERM = -1
DEFAULTS = dict(min_qv=30, min_mapq=60, qlen_lower_limit=0, qlen_upper_limit=1 << 30, min_sequence_identity=0.99, min_gq=20,
                min_bq=93, min_trim=0.01, max_mismatch_count=0, mismatch_window_size=20, md_threshold=1 << 30,
                min_ref_count=3, min_alt_count=1, min_hap_count=3)


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


class ReadInfo:
    """What the proposals need of read i: cs2subindel's mismatch_lst as (pos1, is_sub, ref, alt, qpos), the identity."""

    def __init__(self, batch, i):
        t, q = int(batch.tstart[i]), int(batch.qstart[i])
        self.mismatch = []
        match = mism = 0
        for state, ref_len, alt_len, ref, alt in O.cs_ops(batch, i):
            ref, alt = ref.upper(), alt.upper()
            if state == 1:
                match += ref_len
            elif state == 2:
                mism += alt_len
                if ref != "N":
                    self.mismatch.append((t + 1, True, ref, alt, q))
            elif state == 3:
                mism += alt_len
                self.mismatch.append((t + 1, False, "", "", q))
            elif state == 4:
                mism += ref_len
                self.mismatch.append((t + 1, False, "", "", q))
            t += ref_len
            q += alt_len
        self.identity = match / float(match + mism)
        self.qlen = int(batch.qlen[i])
        o = int(batch.qoff[i])
        self.bq = batch.bq[o:o + self.qlen]
        self.mapq = int(batch.mapq[i])

    def passes(self, p):                                              # caller.py:310-317
        if self.qlen and float(np.mean(self.bq)) < p["min_qv"]:
            return False
        if self.mapq < p["min_mapq"] or self.identity < p["min_sequence_identity"]:
            return False
        return p["qlen_lower_limit"] < self.qlen < p["qlen_upper_limit"]

    def runs(self):
        """The maximal runs of consecutive entries that are substitutions at consecutive positions: (first entry, length)."""
        m, out, e = self.mismatch, [], 0
        while e < len(m):
            if not m[e][1]:
                e += 1
                continue
            n = 1
            while e + n < len(m) and m[e + n][1] and m[e + n][0] == m[e][0] + n:
                n += 1
            out.append((e, n))
            e += n
        return out


def is_germ_gt(ref, alt, gt, state, counts):                          # caller.py:111-147
    if state == "het":
        return ref + alt == gt
    if state == "hetalt":
        return sum(counts[:4]) == counts[BASES.index(gt[0])] + counts[BASES.index(gt[1])] and alt in gt
    if state == "homalt":
        return counts[BASES.index(ref)] == 0 and gt.count(alt) == 2
    return alt == gt[0]


def half(col, tpos, ref, alt, p, prior, pon, com):
    """The verdict of call's non-phased cascade for (tpos, ref, alt) on the column: (status or GERM, gq, gt, state index,
    counts[6], the alt allele's quality sum)."""
    counts, alleles, bqs, altq, alt_hi = [0] * 6, [], [], 0, False
    ai = BASES.index(alt)
    for cell, q, ins in col:
        if ins:
            counts[4] += 1
        if cell < 4:
            if q == 0:
                raise ModelError(ERR_BQ0)
            counts[cell] += 1
            alleles.append(cell)
            bqs.append(q)
            if cell == ai:
                altq += q
                alt_hi = alt_hi or q >= p["min_bq"]
        elif cell == DEL:
            counts[5] += 1
        elif cell == OTHER:
            raise ModelError(ERR_BASE)
    gt, gq, state, _pl = O.germ_gt(ref, alleles, bqs, prior)
    depth = counts[0] + counts[1] + counts[2] + counts[3] + counts[5]
    key = (tpos << 4) | (BASES.index(ref) << 2) | ai
    if is_germ_gt(ref, alt, gt, state, counts):
        status = GERM
    elif state != "homref":
        status = ST[{"het": "HetSite", "hetalt": "HetAltSite", "homalt": "HomAltSite"}[state]]
    elif counts[4] or counts[5]:
        status = ST["IndelSite"]
    elif gq < p["min_gq"]:
        status = ST["LowGQ"]
    elif not alt_hi:
        status = ST["LowBQ"]
    elif key in pon:
        status = ST["PanelOfNormal"]
    elif key in com:
        status = ST["ComSnp"]
    elif not (counts[BASES.index(ref)] >= p["min_ref_count"] and counts[ai] >= p["min_alt_count"]):
        status = ST["LowDepth"]
    elif depth > p["md_threshold"]:
        status = ST["HighDepth"]
    else:
        status = ST["PASS"]
    return status, gq, gt, STATES.index(state), counts, altq


def run(batch, regions, prior=1 / (10 ** 3), pon_keys=(), com_keys=(), dropped=None, **kw):
    """(records, log[20]).  Raises ModelError where the run returns HIMUT_ERR_BASE / _BQ0.  dropped: a list that takes
    (tpos, refs, alts, [half verdicts]) of the candidates dropped as germline."""
    p = dict(DEFAULTS, **kw)
    regions = [(int(s), int(e)) for s, e in regions]
    pon, com = {int(k) for k in pon_keys}, {int(k) for k in com_keys}
    log = [0] * 20
    piles, fetched_bad, proposers = [], False, {}
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100:
            continue
        r = PileRead(batch, i)
        # the germline run's rule: an aligned base outside ATGC in a read some region fetches
        if r.bad_base and any(s < r.tend and e > r.tstart for s, e in regions):
            fetched_bad = True
        piles.append(r)
        info = ReadInfo(batch, i)
        if not info.passes(p):
            continue
        log[0] += 1
        m, w = info.mismatch, p["mismatch_window_size"]
        positions = [x[0] for x in m]
        for e, n in info.runs():
            if n == 1:
                continue
            if n > 2:
                log[2] += 1
                continue
            log[1] += 1
            tpos, qpos = m[e][0], m[e][4]
            if is_trimmed(qpos, info.qlen, p["min_trim"]) or is_trimmed(qpos + 1, info.qlen, p["min_trim"]):
                log[3] += 1
                continue
            s1, e1 = get_mismatch_range(tpos, qpos, info.qlen, w)
            s2, e2 = get_mismatch_range(tpos + 1, qpos + 1, info.qlen, w)
            inside = bisect.bisect_right(positions, max(e1, e2)) - bisect.bisect_left(positions, min(s1, s2))
            if inside - 2 > p["max_mismatch_count"]:
                log[4] += 1
                continue
            if not any(s <= tpos <= e_ for s, e_ in regions):
                continue
            cand = (tpos, BASES.index(m[e][3]), BASES.index(m[e + 1][3]), m[e][2] + m[e + 1][2])
            proposers[cand] = proposers.get(cand, 0) + 1
    if fetched_bad:
        raise ModelError(ERR_BASE)
    cands = sorted(proposers)
    need = sorted({c[0] - 1 for c in cands} | {c[0] for c in cands})       # 0-based column positions
    cols = {pos: [] for pos in need}
    for k, r in enumerate(piles):                                        # file order = fetch order
        for pos in need[bisect.bisect_left(need, r.tstart):bisect.bisect_right(need, r.tend)]:
            j = pos - r.tstart
            if r.cell[j] != NONE or r.ins[j]:
                cols[pos].append((int(r.cell[j]), int(r.bq[j]), bool(r.ins[j]), k))
    out = []
    for cand in cands:
        tpos, a0, a1, refs = cand
        alts = BASES[a0] + BASES[a1]
        log[5] += 1
        hv = [half([c[:3] for c in cols[tpos - 1 + j]], tpos + j, refs[j], alts[j], p, prior, pon, com) for j in (0, 1)]
        if hv[0][0] == GERM or hv[1][0] == GERM:
            log[6] += 1
            if dropped is not None:
                dropped.append((tpos, refs, alts, [hv[0][0], hv[1][0]]))
            continue
        cell0 = {k: c for c, _q, _i, k in cols[tpos - 1] if c < 4}
        cell1 = {k: c for c, _q, _i, k in cols[tpos] if c < 4}
        both_alt = both_ref = one_alt = 0
        for k in set(cell0) | set(cell1):
            x, y = cell0.get(k, NONE), cell1.get(k, NONE)
            is0, is1 = x == a0, y == a1
            both_alt += is0 and is1
            one_alt += is0 != is1
            both_ref += x == BASES.index(refs[0]) and y == BASES.index(refs[1])
        rank = [PRECEDENCE.index(STATUS[h[0]]) if STATUS[h[0]] in PRECEDENCE else 8 for h in hv]
        if min(rank) < 8:
            status = hv[0][0] if rank[0] <= rank[1] else hv[1][0]
        elif both_ref < p["min_ref_count"] or both_alt < p["min_alt_count"]:
            status = ST["LowDepth"]
        elif ST["HighDepth"] in (hv[0][0], hv[1][0]):
            status = ST["HighDepth"]
        else:
            status = ST["PASS"]
        log[7 + VERDICTS.index(STATUS[status])] += 1
        out.append((tpos, min(hv[0][1], hv[1][1]), [ord(x) for x in refs], [ord(x) for x in alts], status,
                    [hv[0][0], hv[1][0]], 0, [hv[0][3], hv[1][3]], [[ord(x) for x in hv[0][2]], [ord(x) for x in hv[1][2]]],
                    [0, 0], [hv[0][1], hv[1][1]], [hv[0][4], hv[1][4]], [hv[0][5], hv[1][5]], both_alt, both_ref, one_alt,
                    proposers[cand], [0, 0]))
    return (np.array(out, DBS_RECORD_DTYPE) if out else np.zeros(0, DBS_RECORD_DTYPE)), log


def vcf_lines(chrom, recs):
    """The data lines of the records of one contig, in vcflib._body_line's format with two-letter REF and ALT: BQ the alt
    quality sum of both columns over both alt counts, DP the smaller half depth, AD both_ref,both_alt, VAF both_alt / DP."""
    out = []
    for r in recs:
        ref, alt = "".join(chr(x) for x in r["ref"]), "".join(chr(x) for x in r["alt"])
        c = [[int(x) for x in h] for h in r["counts"]]
        dp = min(h[0] + h[1] + h[2] + h[3] + h[5] for h in c)
        n_alt = c[0][BASES.index(alt[0])] + c[1][BASES.index(alt[1])]
        bq = (int(r["alt_bqsum"][0]) + int(r["alt_bqsum"][1])) / float(n_alt) if n_alt else 0.0
        sample = "./.:{}:{:0.1f}:{:0.0f}:{:0.0f},{:0.0f}:{:.2f}".format(int(r["gq"]), bq, float(dp), float(r["both_ref"]),
                                                                      float(r["both_alt"]), int(r["both_alt"]) / float(dp))
        out.append("{}\t{}\t.\t{}\t{}\t.\t{}\t.\tGT:GQ:BQ:DP:AD:VAF\t{}\n".format(chrom, int(r["tpos"]), ref, alt,
                                                                              STATUS[int(r["status"])], sample))
    return out


def assert_same(got, got_log, want, want_log):
    assert [int(x) for x in got_log] == [int(x) for x in want_log], (got_log, want_log)
    assert len(got) == len(want), (len(got), len(want))
    for name in DBS_RECORD_DTYPE.names:
        assert np.array_equal(got[name], want[name]), name
    assert got.tobytes() == want.tobytes()
