"""The germline run's contract (himut_run_germline) in plain Python: nothing of the device side.

A read batch, a region list, a prior and the run's parameters in; records, the twelve counters and the VCF body out.
Candidate positions and reference bases come from the cs operations (oracle.cs_ops), piles are built in file order
as numpy arrays per read, every candidate column goes through oracle.germ_gt (the reference's gtlib.get_germ_gt), and
the FILTER cascade is applied to what it returns."""
import bisect

import numpy as np

from oracle import oracle as O

RECORD_DTYPE = np.dtype([("tpos", "<i4"), ("chunk", "<i4"), ("phase_set", "<i4"), ("gq", "<i4"), ("ref", "u1"),
                         ("alt", "u1"), ("gt0", "u1"), ("gt1", "u1"), ("status", "u1"), ("gt_state", "u1"),
                         ("flags", "u1"), ("pad", "u1"), ("counts", "<u4", (6,)), ("bqsum", "<u4", (4,))])
BASES = "ATGC"
STATES = ["homref", "het", "hetalt", "homalt"]
ST_PASS, ST_LOWBQ, ST_LOWGQ, ST_LOWDEPTH, ST_HIGHDEPTH = 0, 1, 2, 9, 10        # HIMUT_ST_*
FILTER_NAME = {ST_PASS: "PASS", ST_LOWBQ: "LowBQ", ST_LOWGQ: "LowGQ", ST_LOWDEPTH: "LowDepth", ST_HIGHDEPTH: "HighDepth"}
LOG_SLOT = {ST_PASS: 6, ST_LOWGQ: 7, ST_LOWBQ: 8, ST_LOWDEPTH: 9, ST_HIGHDEPTH: 10}
ERR_CS, ERR_BASE, ERR_BQ0 = 3, 4, 5                                            # HIMUT_ERR_*
DEFAULTS = dict(min_mapq=0, min_gq=20, min_bq=20, min_ref_count=2, min_alt_count=2, md_threshold=1 << 30,
                report_homref=False)
NONE, OTHER, DEL = 7, 4, 5
_NIB2ALLELE = np.full(16, OTHER, np.uint8)
for _n, _a in ((1, 0), (8, 1), (4, 2), (2, 3)):
    _NIB2ALLELE[_n] = _a


class ModelError(Exception):
    def __init__(self, code):
        super().__init__("germline model error {}".format(code))
        self.code = code


class PileRead:
    """One pile read over [tstart, tend]: per reference position its cell (allele 0-3, OTHER, DEL, NONE), quality and
    whether an insertion precedes the position (update_allelecounts, caller.py:44-72); its substitutions (pos, ref)."""

    def __init__(self, batch, i):
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        n = te - ts + 1                                         # a trailing insertion is counted at tend
        self.tstart, self.tend = ts, te
        self.cell = np.full(n, NONE, np.uint8)
        self.bq = np.zeros(n, np.uint8)
        self.ins = np.zeros(n, bool)
        self.subs = []
        self.bad_base = False
        o, ql = int(batch.qoff[i]), int(batch.qlen[i])
        packed = batch.seq[o >> 1:(o + ql + 1) >> 1]
        nib = np.empty(packed.shape[0] * 2, np.uint8)
        nib[0::2] = packed >> 4
        nib[1::2] = packed & 15
        alle = _NIB2ALLELE[nib[:ql]]
        q = batch.bq[o:o + ql]
        t, qp = ts, int(batch.qstart[i])
        for state, ref_len, alt_len, ref, alt in O.cs_ops(batch, i):
            k = t - ts
            if state == 1:
                self.cell[k:k + ref_len] = alle[qp:qp + ref_len]
                self.bq[k:k + ref_len] = q[qp:qp + ref_len]
            elif state == 2:
                self.cell[k] = BASES.index(alt.upper())
                self.bq[k] = q[qp]
                self.subs.append((t, ref.upper()))
            elif state == 3:
                self.ins[k] = True
            elif state == 4:
                self.cell[k:k + ref_len] = DEL
            t += ref_len
            qp += alt_len
        self.bad_base = bool(np.any(self.cell == OTHER))


def in_regions(regions, tpos):
    return any(s <= tpos <= e for s, e in regions)


def run(batch, regions, prior=1 / (10 ** 3), **kw):
    """(records, log[12]).  Raises ModelError where the run returns HIMUT_ERR_CS / _BASE / _BQ0."""
    p = dict(DEFAULTS, **kw)
    regions = [(int(s), int(e)) for s, e in regions]
    # the non-secondary reads in file order; the pile reads among them (mapq)
    reads, fetched_bad = [], False
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100:
            continue
        r = PileRead(batch, i)
        # a base outside ATGC in an aligned position of a read some region fetches (start < tend, end > tstart): KeyError
        # in the reference's pile, whatever the read's mapping quality (the capture's tail, as in the call run)
        if r.bad_base and any(s < r.tend and e > r.tstart for s, e in regions):
            fetched_bad = True
        if int(batch.mapq[i]) >= p["min_mapq"]:
            reads.append(r)
    if fetched_bad:
        raise ModelError(ERR_BASE)
    refs = {}
    for r in reads:
        for pos, ref in r.subs:
            refs.setdefault(pos, set()).add(ref)
    cand = sorted(pos for pos in refs if in_regions(regions, pos + 1))
    cols = {pos: [] for pos in cand}
    for r in reads:                                              # file order = fetch order
        for pos in cand[bisect.bisect_left(cand, r.tstart):bisect.bisect_right(cand, r.tend)]:
            k = pos - r.tstart
            if r.cell[k] != NONE or r.ins[k]:
                cols[pos].append((int(r.cell[k]), int(r.bq[k]), bool(r.ins[k])))
    log = [0] * 12
    out = []
    for pos in cand:
        names = refs[pos]
        if "N" in names:
            if len(names) > 1:
                raise ModelError(ERR_CS)
            log[1] += 1
            continue
        if len(names) > 1:
            raise ModelError(ERR_CS)
        ref = next(iter(names))
        counts, bqsum, alleles, bqs, hi = [0] * 6, [0] * 4, [], [], [False] * 4
        for cell, q, ins in cols[pos]:
            if ins:
                counts[4] += 1
            if cell < 4:
                if q == 0:
                    raise ModelError(ERR_BQ0)
                counts[cell] += 1
                bqsum[cell] += q
                alleles.append(cell)
                bqs.append(q)
                if q >= p["min_bq"]:
                    hi[cell] = True
            elif cell == DEL:
                counts[5] += 1
            elif cell == OTHER:
                raise ModelError(ERR_BASE)
        gt, gq, state, _pl = O.germ_gt(ref, alleles, bqs, prior)
        st = STATES.index(state)
        log[0] += 1
        log[2 + st] += 1
        alts = [b for b in gt if b != ref]
        if st == 3:
            alts = alts[:1]
        status = ST_PASS
        if st != 0:
            depth = counts[0] + counts[1] + counts[2] + counts[3] + counts[5]
            ai = [BASES.index(a) for a in alts]
            if gq < p["min_gq"]:
                status = ST_LOWGQ
            elif not all(hi[a] for a in ai):
                status = ST_LOWBQ
            elif any(counts[a] < p["min_alt_count"] for a in ai) or \
                    (st == 1 and counts[BASES.index(ref)] < p["min_ref_count"]):
                status = ST_LOWDEPTH
            elif depth > p["md_threshold"]:
                status = ST_HIGHDEPTH
            log[LOG_SLOT[status]] += 1
        if st == 0 and not p["report_homref"]:
            continue
        out.append((pos + 1, -1, -1, gq, ord(ref), ord(alts[0]) if alts else ord(ref), ord(gt[0]), ord(gt[1]), status,
                    st, 0, 0, counts, bqsum))
    return np.array(out, RECORD_DTYPE) if out else np.zeros(0, RECORD_DTYPE), log


def vcf_lines(chrom, recs):
    """The data lines of the records of one contig: chrom, tpos, ".", ref, ALT, gq, FILTER, ".", GT:GQ:DP:AD:VAF, sample."""
    out = []
    for r in recs:
        st = int(r["gt_state"])
        if st == 0:
            continue
        c = [int(x) for x in r["counts"]]
        dp = c[0] + c[1] + c[2] + c[3] + c[5]
        ref, g0, g1 = chr(r["ref"]), chr(r["gt0"]), chr(r["gt1"])
        alts, gt = {1: ([g1], "0/1"), 2: ([g0, g1], "1/2"), 3: ([g0], "1/1")}[st]
        ad = ",".join(str(c[BASES.index(b)]) for b in [ref] + alts)
        vaf = ",".join("{:.2f}".format(c[BASES.index(b)] / dp) for b in alts)
        out.append("\t".join([chrom, str(int(r["tpos"])), ".", ref, ",".join(alts), str(int(r["gq"])),
                              FILTER_NAME[int(r["status"])], ".", "GT:GQ:DP:AD:VAF",
                              "{}:{}:{}:{}:{}".format(gt, int(r["gq"]), dp, ad, vaf)]) + "\n")
    return out


FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "flags", "pad", "counts",
          "bqsum")


def assert_same(got, got_log, want, want_log):
    assert [int(x) for x in got_log] == [int(x) for x in want_log], (got_log, want_log)
    assert len(got) == len(want), (len(got), len(want))
    for name in FIELDS:
        assert np.array_equal(got[name], want[name]), name


def make_read(ref, start, length, subs=None, ins=None, dels=None, bq=40, bq_at=None, long_cs=False, nref=(),
              softclip=("", ""), **extra):
    """A read record (readbatch.batch_from_records) over ref[start:start + length]: subs {pos: base}, ins {pos: bases
    inserted in front of pos; pos == start + length is a trailing insertion}, dels {pos: deleted length}, bq_at {pos:
    quality of the base at pos}; nref: substituted positions whose cs names n as the reference base; softclip: the
    (leading, trailing) soft-clipped bases, which go into seq / bq (quality ``bq``) and set qstart; the cs text has none
    of them."""
    subs, ins, dels, bq_at = subs or {}, ins or {}, dels or {}, bq_at or {}
    seq, quals, cs, run = [], [], [], []

    def flush():
        if run:
            cs.append(("=" + "".join(run)) if long_cs else ":{}".format(len(run)))
            run.clear()
    p, end = start, start + length
    while p < end:
        if p in ins:
            flush()
            cs.append("+" + ins[p].lower())
            seq.extend(ins[p]); quals.extend([bq] * len(ins[p]))
        if p in dels:
            flush()
            cs.append("-" + ref[p:p + dels[p]].lower())
            p += dels[p]
            continue
        if p in subs:
            flush()
            cs.append("*" + ("n" if p in nref else ref[p].lower()) + subs[p].lower())
            seq.append(subs[p])
        else:
            run.append(ref[p])
            seq.append(ref[p])
        quals.append(bq_at.get(p, bq))
        p += 1
    flush()
    if end in ins:
        cs.append("+" + ins[end].lower())
        seq.extend(ins[end]); quals.extend([bq] * len(ins[end]))
    lead, trail = softclip
    return dict(tstart=start, tend=end, qstart=len(lead), seq=lead + "".join(seq) + trail,
                bq=[bq] * len(lead) + quals + [bq] * len(trail), cs="".join(cs), **extra)
