"""The sindels run's contract (himut_run_sindels) in plain Python: nothing of the device side,
nothing of the package.

It builds on the indels run's model (tests/indels_model.py): the pile reads, the raw events with their three rules, the
left shift, the alleles with n_alt, n_other and DP and the genotype are that model's (collect, raw_events, normalise,
genotype); the class of an allele against the homopolymer run behind its anchor is the indelcal model's (event_cell).
What is stated here: call's read filters on a pile read, the three rules on a raw event of a proposing read, the
candidates and the verdict cascade."""
import bisect
import math

import numpy as np

from tests import indelcal_model as IC
from tests import indels_model as M

RECORD_DTYPE = np.dtype([("anchor", "<i4"), ("len", "<i4"), ("type", "u1"), ("status", "u1"), ("gt_state", "u1"),
                         ("pad0", "u1"), ("gq", "<i4"), ("dp", "<u4"), ("n_alt", "<u4"), ("n_other", "<u4"),
                         ("pad1", "<u4"), ("bases", "u1", (16,)), ("n_prop", "<u4"), ("run_base", "u1"), ("run_len", "u1"),
                         ("class_col", "u1"), ("pad2", "u1"), ("reserved", "<u4", (2,))])
assert RECORD_DTYPE.itemsize == 64
BASES = M.BASES
ST_PASS, ST_LOWGQ, ST_INDEL, ST_LOWDEPTH, ST_HIGHDEPTH, ST_REPEAT = 0, 2, 3, 9, 10, 14       # HIMUT_ST_*
FILTER_NAME = {ST_PASS: "PASS", ST_LOWGQ: "LowGQ", ST_INDEL: "IndelSite", ST_LOWDEPTH: "LowDepth",
               ST_HIGHDEPTH: "HighDepth", ST_REPEAT: "Repeat"}
LOG = ("events", "num_edge", "num_long", "num_nbase", "pile_reads", "proposing_reads", "events_proposing_reads", "num_trim",
       "num_window", "num_lowbq", "proposing_events", "candidates", "num_germ_het", "num_germ_homalt", "IndelSite",
       "Repeat", "LowGQ", "LowDepth", "HighDepth", "PASS")
LOG_SLOT = {ST_INDEL: 14, ST_REPEAT: 15, ST_LOWGQ: 16, ST_LOWDEPTH: 17, ST_HIGHDEPTH: 18, ST_PASS: 19}
RUN_MAX = IC.MAX_RUN
DEFAULTS = dict(min_mapq=20, min_gq=20, min_ref_count=3, min_alt_count=1, md_threshold=1 << 30, max_len=50, max_run=2,
                min_qv=30, indel_error=0.01, germline_indel_prior=1 / (10 ** 4), qlen_lower_limit=-1,
                qlen_upper_limit=(1 << 31) - 1, min_bq=93, mismatch_window_size=20, max_mismatch_count=0,
                min_sequence_identity=0.99, min_trim=0.01)


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
    """What the rules need of read i, from its cs text: the raw events as (type, p, L, s, q) in indels_model.raw_events'
    order, q the query offset of the event's entry in cs2subindel's mismatch list (cslib.py:47-64); that list's positions;
    the identity (bamlib.py:47-63); the qualities of the whole query."""

    def __init__(self, batch, i):
        cs = bytes(batch.cs[int(batch.cs_off[i]):int(batch.cs_off[i + 1])]).decode("latin-1")
        seq = M.query(batch, i)
        t, q = int(batch.tstart[i]), int(batch.qstart[i])
        self.events, self.positions = [], []
        match = mism = 0
        prev_ins = False
        for op in M._OP.findall(cs):
            k, body = op[0], op[1:]
            if k == ":":
                n = int(body)
                match += n; t += n; q += n
            elif k == "=":
                match += len(body); t += len(body); q += len(body)
            elif k == "*":
                mism += 1
                if body[0].upper() != "N":
                    self.positions.append(t + 1)
                t += 1; q += 1
            elif k == "+":
                mism += len(body)
                self.positions.append(t + 1)
                s = seq[q:q + len(body)]
                if prev_ins:
                    ty, p, L, s0, q0 = self.events.pop()
                    self.events.append((M.INS, p, L + len(body), s0 + s, q0))
                else:
                    self.events.append((M.INS, t, len(body), s, q))
                q += len(body)
            else:
                mism += len(body)
                self.positions.append(t + 1)
                self.events.append((M.DEL, t, len(body), "", q))
                t += len(body)
            prev_ins = k == "+"
        assert [e[:4] for e in self.events] == M.raw_events(batch, i)
        self.identity = match / float(match + mism)
        self.qlen = int(batch.qlen[i])
        o = int(batch.qoff[i])
        self.bq = [int(x) for x in batch.bq[o:o + self.qlen]]
        self.mapq = int(batch.mapq[i])

    def proposes(self, p):                                            # caller.py:310-317
        if self.identity < p["min_sequence_identity"]:
            return False
        if sum(self.bq) < p["min_qv"] * self.qlen:
            return False
        if self.mapq < p["min_mapq"]:
            return False
        return p["qlen_lower_limit"] < self.qlen < p["qlen_upper_limit"]

    def event_rule(self, ty, pos, L, q, p):
        """The first rule the raw event fails: "num_trim", "num_window", "num_lowbq", or None."""
        qa, qb = q - 1, (q + L if ty == M.INS else q)
        if is_trimmed(qa, self.qlen, p["min_trim"]) or is_trimmed(qb, self.qlen, p["min_trim"]):
            return "num_trim"
        s, e = get_mismatch_range(pos + 1, q, self.qlen, p["mismatch_window_size"])
        if bisect.bisect_right(self.positions, e) - bisect.bisect_left(self.positions, s) - 1 > p["max_mismatch_count"]:
            return "num_window"
        assert 0 <= qa and qb < self.qlen                             # Row 12's edge rule: an aligned base on either side
        if any(b < p["min_bq"] for b in self.bq[qa:qb + 1]):
            return "num_lowbq"
        return None


def run_at(refseq, s):
    """(n, letter) of the homopolymer run that starts at s, n = RUN_MAX + 1 for anything longer; (0, None) where none
    starts: no position in front of s, no letter at s, or the same letter in front of it."""
    u = refseq.upper()
    if s < 1 or s >= len(u) or u[s] not in BASES or u[s - 1] == u[s]:
        return 0, None
    n = 1
    while n <= RUN_MAX and s + n < len(u) and u[s + n] == u[s]:
        n += 1
    return n, u[s]


def proposals(batch, regions, refseq, p):
    """({allele: set of proposing reads}, the counters 4..10 by name)."""
    log = dict.fromkeys(LOG[4:11], 0)
    out = {}
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100 or int(batch.mapq[i]) < p["min_mapq"]:
            continue
        log["pile_reads"] += 1
        info = ReadInfo(batch, i)
        if not info.proposes(p):
            continue
        log["proposing_reads"] += 1
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        for ty, pos, L, s, q in info.events:
            end = pos if ty == M.INS else pos + L
            if not (ts <= pos - 1 and end < te) or L > p["max_len"] or any(b not in BASES for b in s):
                continue
            log["events_proposing_reads"] += 1
            failed = info.event_rule(ty, pos, L, q, p)
            if failed:
                log[failed] += 1
                continue
            log["proposing_events"] += 1
            npos, ns = M.normalise(refseq, ts, ty, pos, L, s)
            out.setdefault((npos - 1, ty, L, tuple(BASES.index(b) for b in ns)), set()).add(i)
    return out, log


def collect(batch, regions, refseq, **kw):
    """What does not depend on the genotype's and the verdict's parameters: (indels_model.collect's alleles and counters,
    the proposals and theirs)."""
    p = dict(DEFAULTS, **kw)
    regions = [(int(s), int(e)) for s, e in regions]
    return M.collect(batch, regions, refseq, min_mapq=p["min_mapq"], max_len=p["max_len"]) + proposals(batch, regions, refseq, p)


def run(batch, regions, refseq, l_hit=None, l_err=None, **kw):
    """(records, log[20]); l_hit, l_err: the table of himut_set_indel_error_table (None: the constant)."""
    return evaluate(collect(batch, regions, refseq, **kw), refseq, l_hit, l_err, **kw)


def evaluate(collected, refseq, l_hit=None, l_err=None, **kw):
    """(records, log[20]) of collect's alleles and proposals under the genotype's and the verdict's parameters."""
    p = dict(DEFAULTS, **kw)
    items, ilog, props, plog = collected
    log = dict.fromkeys(LOG, 0)
    log.update(plog, events=ilog[0], num_edge=ilog[2], num_long=ilog[3], num_nbase=ilog[4])
    lg = M.logs(p["indel_error"], p["germline_indel_prior"])
    runs = IC.runs_of(refseq)
    out = []
    for allele, n_alt, n_other, dp in items:
        if allele not in props:
            continue
        a, ty, L, codes = allele
        s = "".join(BASES[c] for c in codes)
        log["candidates"] += 1
        n_run, letter = run_at(refseq, a + 1)
        cell = IC.event_cell(refseq, runs, a, ty, L, s)
        own = lg
        if l_hit is not None and cell is not None:
            own = (l_hit[cell[0] * IC.N_EVCOLS + cell[1]], l_err[cell[0] * IC.N_EVCOLS + cell[1]]) + tuple(lg[2:])
        state, gq, _pls = M.genotype(dp - n_alt, n_alt, own)
        if state != 0:
            log["num_germ_het" if state == 1 else "num_germ_homalt"] += 1
            continue
        if n_other > 0:
            status = ST_INDEL
        elif n_run > RUN_MAX or (cell is not None and cell[1] != 6 and n_run > p["max_run"]):
            status = ST_REPEAT
        elif gq < p["min_gq"]:
            status = ST_LOWGQ
        elif n_alt < p["min_alt_count"] or dp - n_alt - n_other < p["min_ref_count"]:
            status = ST_LOWDEPTH
        elif dp > p["md_threshold"]:
            status = ST_HIGHDEPTH
        else:
            status = ST_PASS
        log[LOG[LOG_SLOT[status]]] += 1
        out.append((a, L, ty, status, 0, 0, gq, dp, n_alt, n_other, 0, M.pack_bases(s), len(props[allele]),
                    BASES.index(letter) if n_run else 0, n_run, 255 if cell is None else cell[1], 0, [0, 0]))
    log = [log[k] for k in LOG]
    check_identities(log, len(out))
    return (np.array(out, RECORD_DTYPE) if out else np.zeros(0, RECORD_DTYPE)), log


def check_identities(log, n_records):
    """The identities between the counters the contract states."""
    d = dict(zip(LOG, log))
    assert d["events_proposing_reads"] == d["num_trim"] + d["num_window"] + d["num_lowbq"] + d["proposing_events"], d
    verdicts = sum(d[k] for k in ("IndelSite", "Repeat", "LowGQ", "LowDepth", "HighDepth", "PASS"))
    assert d["candidates"] == d["num_germ_het"] + d["num_germ_homalt"] + verdicts and verdicts == n_records, d
    assert d["proposing_reads"] <= d["pile_reads"]
    return d


def logd(log):
    return dict(zip(LOG, log))


def assert_same(got, got_log, want, want_log):
    assert [int(x) for x in got_log] == [int(x) for x in want_log], (logd(got_log), logd(want_log))
    assert len(got) == len(want), (len(got), len(want))
    for name in RECORD_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (name, got[name][:8], want[name][:8])
    assert got.tobytes() == want.tobytes()
