"""The indelcal run's contract (himut_run_indelcal) in plain Python, and the indels run's
under an error table (himut_set_indel_error_table): nothing of the device side, nothing of the package.

It builds on the indels run's model (tests/indels_model.py): the pile reads, the raw events, the left shift and an
allele's n_alt and DP are that model's (collect, raw_events, normalise), the genotype under a table is its genotype with
the allele's own logs.  Runs are found by walking the upper-cased string, spans by looking at every pile read, events are
classified from the string alone: no histogram, no bitmap, no windows."""
import math

import numpy as np

from tests import indels_model as M

BASES = M.BASES
COLUMNS = ("runs", "excluded", "spans", "del1", "del2", "del3p", "ins1", "ins2", "ins3p", "other")
LOG = ("events", "num_edge", "num_long", "num_nbase", "anchors", "variant_anchors", "events_variant", "num_offrun",
       "num_partial", "events_counted", "runs", "runs_excluded", "runs_long", "spans")
N_CLASSES, N_EVCOLS, MAX_RUN = 128, 7, 64
DEFAULTS = dict(min_mapq=0, max_len=50, min_alt_count=2, vaf_permille=250)


def run_class(b, n):
    return BASES.index(b) * 32 + min(n, 32) - 1


def col(name):
    return COLUMNS.index(name)


def runs_of(refseq):
    """{s: (n, letter)} of every run: a maximal stretch of one letter of ACGT (upper-cased) with a position on both sides."""
    u = refseq.upper()
    out = {}
    i = 0
    while i < len(u):
        j = i
        while j < len(u) and u[j] == u[i]:
            j += 1
        if u[i] in BASES and i >= 1 and j < len(u):
            out[i] = (j - i, u[i])
        i = j
    return out


def events_of(batch, regions, refseq, min_mapq, max_len):
    """([(a, type, L, s, tend of the read)] of the collected events in read order, the pile as [(tstart, tend)])."""
    out, pile = [], []
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100 or int(batch.mapq[i]) < min_mapq:
            continue
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        pile.append((ts, te))
        for ty, pos, L, s in M.raw_events(batch, i):
            end = pos if ty == M.INS else pos + L
            if not (ts <= pos - 1 and end < te) or L > max_len or any(b not in BASES for b in s):
                continue
            pos, s = M.normalise(refseq, ts, ty, pos, L, s)
            if M.in_regions(regions, pos - 1):
                out.append((pos - 1, ty, L, s, te))
    return out, pile


def event_cell(refseq, runs, a, ty, L, s):
    """(class, event column 0..6, n) of an event or allele from the string alone, None where it is off run."""
    u = refseq.upper()
    if a + 1 >= len(u) or u[a + 1] not in BASES or u[a] == u[a + 1]:
        return None
    if a + 1 not in runs or runs[a + 1][0] > MAX_RUN:         # the run reaches the end of the string, or is long
        return None
    n, b = runs[a + 1]
    if ty == M.DEL:
        k = min(L, 3) - 1 if L <= n else 6
    else:
        k = 3 + min(L, 3) - 1 if all(x == b for x in s) else 6
    return run_class(b, n), k, n


def run(batch, regions, refseq, **kw):
    """(table int64[128, 10], log[14])."""
    p = dict(DEFAULTS, **kw)
    regions = [(int(s), int(e)) for s, e in regions]
    items, ilog = M.collect(batch, regions, refseq, min_mapq=p["min_mapq"], max_len=p["max_len"])
    variant = set(al[0] for al, n_alt, _no, dp in items
                  if n_alt >= p["min_alt_count"] and n_alt * 1000 >= p["vaf_permille"] * dp)
    events, pile = events_of(batch, regions, refseq, p["min_mapq"], p["max_len"])
    assert len(events) == ilog[0]
    table = np.zeros((N_CLASSES, len(COLUMNS)), np.int64)
    log = dict.fromkeys(LOG, 0)
    log.update(events=ilog[0], num_edge=ilog[2], num_long=ilog[3], num_nbase=ilog[4],
               anchors=len(set(al[0] for al, *_ in items)), variant_anchors=len(variant))
    runs = runs_of(refseq)
    starts, ends = np.array([ts for ts, _te in pile], np.int64), np.array([te for _ts, te in pile], np.int64)
    for s, (n, b) in sorted(runs.items()):
        if not M.in_regions(regions, s - 1):
            continue
        if n > MAX_RUN:
            log["runs_long"] += 1
            continue
        c = run_class(b, n)
        table[c][0] += 1
        if s - 1 in variant:
            table[c][1] += 1
            continue
        table[c][2] += int(np.count_nonzero((starts <= s - 1) & (s + n < ends)))    # every pile read is looked at
    for a, ty, L, s, te in events:
        if a in variant:
            log["events_variant"] += 1
            continue
        cell = event_cell(refseq, runs, a, ty, L, s)
        if cell is None:
            log["num_offrun"] += 1
        elif not a + 1 + cell[2] < te:
            log["num_partial"] += 1
        else:
            table[cell[0]][3 + cell[1]] += 1
    log["events_counted"] = int(table[:, 3:].sum())
    log["runs"], log["runs_excluded"], log["spans"] = (int(table[:, k].sum()) for k in range(3))
    return table, [log[k] for k in LOG]


def check_invariants(table, log):
    d = dict(zip(LOG, log))
    assert d["events"] == d["events_variant"] + d["num_offrun"] + d["num_partial"] + d["events_counted"], d
    assert int(table[:, 3:].sum()) == d["events_counted"]
    assert [int(table[:, k].sum()) for k in range(3)] == [d["runs"], d["runs_excluded"], d["spans"]]
    assert (table >= 0).all() and (table[:, 1] <= table[:, 0]).all() and d["variant_anchors"] <= d["anchors"] <= d["events"]
    assert all(int(table[c][2]) == 0 for c in range(N_CLASSES) if table[c][0] == table[c][1])
    return d


def assert_same(got_table, got_log, want_table, want_log):
    assert [int(x) for x in got_log] == [int(x) for x in want_log], (dict(zip(LOG, got_log)), dict(zip(LOG, want_log)))
    got_table, want_table = np.asarray(got_table), np.asarray(want_table)
    assert got_table.shape == want_table.shape == (N_CLASSES, len(COLUMNS))
    bad = [(c, COLUMNS[k], int(got_table[c][k]), int(want_table[c][k])) for c, k in zip(*np.nonzero(got_table != want_table))]
    assert not bad, bad[:8]


# ---- the TSV

def table_lines(table):
    out = ["base\trun\t" + "\t".join(COLUMNS) + "\tdel_rate\tins_rate\n"]
    for c in range(N_CLASSES):
        row = [int(x) for x in table[c]]
        run_len = c % 32 + 1
        cells = [BASES[c // 32], str(run_len) if run_len < 32 else "32+"] + [str(x) for x in row]
        for first in (3, 6):
            cells.append(repr((row[first] + row[first + 1] + row[first + 2]) / row[2]) if row[2] else "NA")
        out.append("\t".join(cells) + "\n")
    return out


# ---- the indels run under a table

def error_logs(table, indel_error, min_spans=1000):
    """(l_hit[896], l_err[896]): e = min((count + 1) / (spans + 2), 0.25) per class and event column, indel_error for a
    class with fewer than min_spans spans."""
    hit, err = [], []
    for c in range(N_CLASSES):
        for k in range(N_EVCOLS):
            e = indel_error
            if int(table[c][2]) >= min_spans:
                e = min((int(table[c][3 + k]) + 1) / (int(table[c][2]) + 2), 0.25)
            hit.append(math.log10(1 - e))
            err.append(math.log10(e))
    return hit, err


def evaluate_with_table(items, base_log, refseq, l_hit, l_err, **kw):
    """M.evaluate with the per-read terms of every allele taken from its cell of the table, the constant where it has
    none: (records, log[13])."""
    p = dict(M.DEFAULTS, **kw)
    lg = M.logs(p["indel_error"], p["germline_indel_prior"])
    runs = runs_of(refseq)
    log = list(base_log)
    out = []
    for (a, ty, L, codes), n_alt, n_other, dp in items:
        cell = event_cell(refseq, runs, a, ty, L, "".join(BASES[c] for c in codes))
        own = lg if cell is None else (l_hit[cell[0] * N_EVCOLS + cell[1]], l_err[cell[0] * N_EVCOLS + cell[1]]) + tuple(lg[2:])
        n_non = dp - n_alt
        state, gq, _pls = M.genotype(n_non, n_alt, own)
        log[1] += 1
        log[6 + state] += 1
        status = M.ST_PASS
        if state != 0:
            if gq < p["min_gq"]:
                status = M.ST_LOWGQ
            elif n_alt < p["min_alt_count"] or (state == 1 and n_non < p["min_ref_count"]):
                status = M.ST_LOWDEPTH
            elif dp > p["md_threshold"]:
                status = M.ST_HIGHDEPTH
            log[M.LOG_SLOT[status]] += 1
        if state == 0 and not p["report_homref"]:
            continue
        out.append((a, L, ty, status, state, 0, gq, dp, n_alt, n_other, 0, M.pack_bases("".join(BASES[c] for c in codes)),
                    [0, 0, 0, 0]))
    return (np.array(out, M.RECORD_DTYPE) if out else np.zeros(0, M.RECORD_DTYPE)), log
