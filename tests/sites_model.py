"""The sites run's contract (himut_run_sites) in plain Python: nothing of the device side.

A read batch, a site list [(pos1, ref, alt)], call's parameters, a prior and the two site sets in; one record per site in
input order and the twenty counters out.  Piles are germline_model.PileRead's, in file order, over every read with flag
0x100 clear whatever its mapq; a site with depth > 0 goes through dbs_model.half -- oracle.germ_gt (the reference's
gtlib.get_germ_gt), is_germ_gt and the non-phased cascade of caller.py:332-550 -- and the half's GERM becomes the status
Germline; a site with depth 0 is NoCoverage and no genotype is taken.

What "LowBQ" means for a site without an alt read: the cascade asks for an alt read with bq >= min_bq, there is none, so
the site is LowBQ unless an earlier rule (Germline, the three genotype states, IndelSite, LowGQ) holds.  A deep clean
homref column with no alt read is therefore LowBQ, never PASS: `call` can only say PASS of a substitution it saw."""
import bisect

import numpy as np

from tests import dbs_model as M
from tests.germline_model import DEL, ERR_BASE, ERR_BQ0, NONE, OTHER, ModelError, PileRead, make_read  # noqa: F401

SITE_RECORD_DTYPE = np.dtype([("site", "<i4"), ("tpos", "<i4"), ("ref", "u1"), ("alt", "u1"), ("status", "u1"),
                              ("gt_state", "u1"), ("gt", "u1", (2,)), ("pad", "u1", (2,)), ("gq", "<i4"),
                              ("counts", "<u4", (6,)), ("alt_bqsum", "<u4"), ("ref_bqsum", "<u4"), ("alt_hi", "<u4"),
                              ("alt_mq", "<u4"), ("reserved", "<u4")])
BASES = "ATGC"
STATES = M.STATES
STATUS = list(M.STATUS) + ["Germline", "NoCoverage"]      # HIMUT_ST_* in code order
ST = {name: k for k, name in enumerate(STATUS)}
assert ST["Germline"] == 12 and ST["NoCoverage"] == 13
VERDICTS = M.VERDICTS                                     # log[3 + k] counts VERDICTS[k]
LOG_ROWS = ["num_sites", "num_NoCoverage", "num_Germline"] + ["num_" + v for v in VERDICTS] + \
           ["num_alt_seen", "num_positions", "reserved0", "reserved1", "reserved2", "reserved3"]
DEFAULTS = M.DEFAULTS


def span_of(batch):
    """The positions the bitmap covers: 0 .. span - 1; 0 for a batch without reads (nothing is indexed)."""
    if batch.n == 0:
        return 0
    return 256 * ((int(np.max(batch.tend)) >> 8) + 2)


def run(batch, sites, prior=1 / (10 ** 3), pon_keys=(), com_keys=(), **kw):
    """(records, log[20]).  Raises ModelError where the run returns HIMUT_ERR_BASE / _BQ0."""
    p = dict(DEFAULTS, **kw)
    pon, com = {int(k) for k in pon_keys}, {int(k) for k in com_keys}
    sites = [(int(s[0]), s[1], s[2]) for s in sites]
    span = span_of(batch)
    need = sorted({pos1 - 1 for pos1, _r, _a in sites if pos1 - 1 < span})         # 0-based column positions
    cols = {pos: [] for pos in need}
    for i in range(batch.n):                                             # file order = fetch order
        if int(batch.flag[i]) & 0x100:
            continue
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        lo, hi = bisect.bisect_left(need, ts), bisect.bisect_right(need, te)
        if lo == hi:
            continue
        r = PileRead(batch, i)
        for pos in need[lo:hi]:
            j = pos - r.tstart
            if r.cell[j] != NONE or r.ins[j]:
                cols[pos].append((int(r.cell[j]), int(r.bq[j]), bool(r.ins[j]), int(batch.mapq[i])))
    log = [0] * 20
    log[15] = len(need)
    out = []
    for k, (pos1, ref, alt) in enumerate(sites):
        col = cols.get(pos1 - 1, [])
        ri, ai = BASES.index(ref), BASES.index(alt)
        counts, refq, altq, alt_hi, alt_mq = [0] * 6, 0, 0, 0, 0
        for cell, q, ins, mapq in col:
            counts[4] += ins
            if cell < 4:
                if q == 0:
                    raise ModelError(ERR_BQ0)
                counts[cell] += 1
                if cell == ri:
                    refq += q
                if cell == ai:
                    altq += q
                    alt_hi += q >= p["min_bq"]
                    alt_mq += mapq >= p["min_mapq"]
            elif cell == DEL:
                counts[5] += 1
            elif cell == OTHER:
                raise ModelError(ERR_BASE)
        depth = counts[0] + counts[1] + counts[2] + counts[3] + counts[5]
        if depth == 0:
            status, gq, gt, state = ST["NoCoverage"], 0, [0, 0], 0
        else:
            status, gq, g, state, hcounts, haltq = M.half([c[:3] for c in col], pos1, ref, alt, p, prior, pon, com)
            assert hcounts == counts and haltq == altq
            if status == M.GERM:
                status = ST["Germline"]
            gt = [ord(x) for x in g]
        log[0] += 1
        if status == ST["NoCoverage"]:
            log[1] += 1
        elif status == ST["Germline"]:
            log[2] += 1
        else:
            log[3 + VERDICTS.index(STATUS[status])] += 1
        log[14] += counts[ai] >= 1
        out.append((k, pos1, ord(ref), ord(alt), status, state, gt, [0, 0], gq, counts, altq, refq, alt_hi, alt_mq, 0))
    return (np.array(out, SITE_RECORD_DTYPE) if out else np.zeros(0, SITE_RECORD_DTYPE)), log


def depth_of(r):
    c = [int(x) for x in r["counts"]]
    return c[0] + c[1] + c[2] + c[3] + c[5]


def assert_same(got, got_log, want, want_log):
    assert [int(x) for x in got_log] == [int(x) for x in want_log], (got_log, want_log)
    assert len(got) == len(want), (len(got), len(want))
    for name in SITE_RECORD_DTYPE.names:
        if not np.array_equal(got[name], want[name]):
            bad = [k for k in range(len(got)) if not np.array_equal(got[name][k], want[name][k])][:5]
            raise AssertionError((name, [(got[k], want[k]) for k in bad]))
    assert got.tobytes() == want.tobytes()
