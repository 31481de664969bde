"""The bqcal run's contract (Row 8; himut_run_bqcal) in plain Python: nothing of the device side.

A read batch, the contig's string, a region list (0-based, half open), a prior and the run's parameters in; match[256],
mismatch[256] and the twelve counters out.  Piles are built in file order as numpy arrays per read (germline_model's
PileRead: update_allelecounts), every swept column that reaches step 4 goes through oracle.germ_gt (the reference's
gtlib.get_germ_gt), and the column's bases are counted as the reference's script counts them."""
import ctypes
import math

import numpy as np

from tests.germline_model import BASES, DEL, ERR_BASE, ERR_BQ0, NONE, ModelError, PileRead
from oracle import oracle as O

STATES = ["homref", "het", "hetalt", "homalt"]
DEFAULTS = dict(min_mapq=0, min_gq=20, md_threshold=1 << 30)
BLOCK = 2048                    # positions of a region laid out at a time


class Genotyper:
    """oracle.germ_gt at one prior with the tables built once: a sweep asks for tens of thousands of columns."""

    def __init__(self, prior):
        self._tables = O.build_lut(prior)
        self._lut = O._Lut(*[O._ptr(t) for t in self._tables])
        self._fn = O.lib().orc_germ_gt

    def __call__(self, ref, alleles, quals):
        """alleles (himut indices A0 T1 G2 C3) and qualities in fetch order -> (gt, gq, state)."""
        a, b = np.ascontiguousarray(alleles, np.uint8), np.ascontiguousarray(quals, np.uint8)
        g0, g1, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        pl = (ctypes.c_double * 10)()
        gq = self._fn(ctypes.c_int(ord(ref)), ctypes.c_int32(a.shape[0]), O._ptr(a), O._ptr(b), ctypes.byref(self._lut),
                      ctypes.byref(g0), ctypes.byref(g1), ctypes.byref(st), pl)
        if gq < 0:
            raise O.OracleError(-gq)
        return chr(g0.value) + chr(g1.value), gq, STATES[st.value]


def run(batch, refseq, regions, prior=1 / (10 ** 3), **kw):
    """(match[256], mismatch[256], log[12]).  Raises ModelError where the run returns HIMUT_ERR_BASE / _BQ0."""
    p = dict(DEFAULTS, **kw)
    regions = [(int(s), int(e)) for s, e in regions]
    reads, fetched_bad = [], False
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100:
            continue
        r = PileRead(batch, i)
        # a base outside ATGC in an aligned position of a read some region fetches: KeyError in the script's pile,
        # whatever the read's mapping quality (the germline run's rule)
        if r.bad_base and any(s < r.tend and e > r.tstart for s, e in regions):
            fetched_bad = True
        if int(batch.mapq[i]) >= p["min_mapq"]:
            reads.append(r)
    if fetched_bad:
        raise ModelError(ERR_BASE)
    match, mismatch, log = np.zeros(256, np.int64), np.zeros(256, np.int64), [0] * 12
    germ_gt = Genotyper(prior)
    verdicts = {}               # (ref, alleles, qualities) -> (gt, gq, state): neighbouring columns often look alike
    bq0 = False
    for s, e in regions:
        for b0 in range(s, e, BLOCK):
            b1 = min(b0 + BLOCK, e)
            rows = [r for r in reads if r.tstart < b1 and r.tend >= b0]          # file order = fetch order
            cell = np.full((len(rows), b1 - b0), NONE, np.uint8)
            qual = np.zeros((len(rows), b1 - b0), np.uint8)
            ins = np.zeros((len(rows), b1 - b0), bool)
            for k, r in enumerate(rows):
                lo, hi = max(r.tstart, b0), min(r.tend + 1, b1)                  # (a trailing insertion sits at tend)
                cell[k, lo - b0:hi - b0] = r.cell[lo - r.tstart:hi - r.tstart]
                qual[k, lo - b0:hi - b0] = r.bq[lo - r.tstart:hi - r.tstart]
                ins[k, lo - b0:hi - b0] = r.ins[lo - r.tstart:hi - r.tstart]
            for pos in range(b0, b1):
                log[0] += 1
                ref = refseq[pos]
                if ref not in BASES:
                    log[1] += 1
                    continue
                col = cell[:, pos - b0]
                base = col < 4
                alleles, quals = col[base], qual[:, pos - b0][base]
                n_del, n_ins = int(np.count_nonzero(col == DEL)), int(np.count_nonzero(ins[:, pos - b0]))
                if alleles.shape[0] + n_del >= p["md_threshold"]:
                    log[2] += 1
                    continue
                if n_ins != 0 or n_del != 0:
                    log[3] += 1
                    continue
                if np.any(quals == 0):
                    bq0 = True                                                   # log10(0) in the reference
                    continue
                key = (ref, alleles.tobytes(), quals.tobytes())
                if key not in verdicts:
                    verdicts[key] = germ_gt(ref, alleles, quals)
                gt, gq, state = verdicts[key]
                if gq < p["min_gq"]:
                    log[4] += 1
                    continue
                log[5 + STATES.index(state)] += 1
                in_gt = np.zeros(4, bool)
                in_gt[[BASES.index(b) for b in gt]] = True
                own = in_gt[alleles]
                if own.all():
                    if alleles.shape[0]:
                        log[9] += 1
                    match += np.bincount(quals, minlength=256)
                else:
                    log[10] += 1
                    mismatch += np.bincount(quals[~own], minlength=256)
    if bq0:
        raise ModelError(ERR_BQ0)
    return match, mismatch, log


def table_text(match, mismatch):
    """The script's table (dump_empirical_bq_score): rows 1 .. 93 always, then a row per quality above 93 that has a
    count; pq as the script formats it, NA when either count is 0."""
    out = ["bq\tmismatch\tmatch\tpq\n"]
    for bq in range(1, 256):
        m, mm = int(match[bq]), int(mismatch[bq])
        if bq > 93 and m == 0 and mm == 0:
            continue
        pq = "{}".format(-10 * math.log10(mm / float(m))) if m != 0 and mm != 0 else "NA"
        out.append("{}\t{}\t{}\t{}\n".format(bq, mm, m, pq))
    return "".join(out)
