#!/usr/bin/env python3
"""One of the added runs against its baseline run of the same build in one process, on bench.py's workload (the
chr20-sized contig, 30x, reads resident): the baseline (himut_run for dbs, indels, germline, sites, support, haplotag and
duplex -- the last on the workload's reads each doubled as its own opposite-strand mate, the call step on the same reads;
himut_run_normcounts for bqcal and callable; himut_run_indels for indelcal and sindels; himut_run_callable for intervals, whose
tally runs over four interval sets) and the run alternate on the same reads for the same number of warm steps.
Device ms of each from the runs' own hipEvents with the per-stage split (timing level 2), min, max and median of the
totals, records, candidates and column slots of each, and what RUNS below adds for the run.  --wall N then times N calls
of the run alone from the host and hashes its records and counters.  Prints one JSON line.

    python tools/bench_runs.py <run> [--steps K] [--warmup W] [--contig-len N] [--depth D] [--wall N] [--out profiles/x.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_total", "ms_parse", "ms_index", "ms_capture", "ms_emit", "ms_eval", "ms_finalize")
BASELINES = {"call": ("call step", 20, 5), "normcounts": ("normcounts run", 10, 3),     # its name in `metric`, steps, warm-up
             "indels": ("indels run", 20, 5), "callable": ("callable run", 10, 3)}
COPY_CEILING_GBS = 6300.0          # DESIGN: what a device-to-device copy reaches on this part


def workload(contig_len, depth, want_ref):
    """bench.py's contig with everything a run reads resident in a configured Worker's context, stage timing 2; with
    want_ref the reference string is set and `tab` is the normcounts alt order."""
    import bench
    from himut_amd import bamlib, caller, normcounts, synth, util as hutil
    sample = synth.generate(synth.SynthConfig(seed=2, contig_len=contig_len, depth=depth, name="chr20"), want_ref=want_ref)
    b = sample.batch
    chunks = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
    ql, qu, md = bamlib.get_thresholds({b.name: b}, [b.name], {b.name: b.length})
    pon, com = bench.make_side_sets(sample, 100)
    w = caller.Worker(0)

    def configure(max_mismatch_count=0):
        w.configure(30, 60, ql, qu, 0.99, 20, 93, 0.01, max_mismatch_count, 20, md, 3, 1, 3, 1 / (10 ** 3), False)
    configure()
    ctx = w.ctx
    ctx.set_chunks(chunks)
    ctx.set_site_set(0, pon)
    ctx.set_site_set(1, com)
    ctx.push_reads(b)
    tab = None
    if want_ref:
        refseq = bytes(sample.ref)
        chars, cls = normcounts.tri_classes(refseq)
        ctx.set_reference(refseq, cls, len(chars))
        tab = normcounts.alt_order_table(bench.NORM_ALT_ORDER)
    ctx.set_stage_timing(2)
    return SimpleNamespace(sample=sample, b=b, chunks=chunks, ql=ql, qu=qu, md=md, w=w, ctx=ctx, tab=tab, configure=configure)


def alternate(legs, steps, warmup):
    """legs: ordered (name, step), step() makes one run and returns its stats.  Every leg once per round, in order, for
    warmup + steps rounds; name -> the stats of the rounds after the warm-up."""
    acc = {name: [] for name, _ in legs}
    for k in range(warmup + steps):
        for name, step in legs:
            st = step()
            if k >= warmup:
                acc[name].append(st)
    return acc


def summarise(rows):
    """One leg's stats as the line reports them."""
    tot = [r["ms_total"] for r in rows]
    d = {k: float(np.mean([r[k] for r in rows])) for k in STAGES}
    d.update(ms_total_min=float(np.min(tot)), ms_total_max=float(np.max(tot)), ms_total_median=float(np.median(tot)),
             reran=int(sum(r["reran"] for r in rows)), records=int(rows[-1]["n_records"]),
             candidates=int(rows[-1]["n_candidates"]), column_slots=int(rows[-1]["column_slots"]))
    return d


def call_sites(R):
    """The sites of the sites and support runs: the call run's records, one per (tpos, ref, alt), by position."""
    R.ctx.run()
    recs = R.ctx.records()
    key = np.unique(np.stack([recs["tpos"].astype(np.int64), recs["ref"].astype(np.int64), recs["alt"].astype(np.int64)], 1), axis=0)
    key = key[key[:, 1] != key[:, 2]]
    R.pos1, R.ref, R.alt = key[:, 0].astype(np.int32), key[:, 1].astype(np.uint8), key[:, 2].astype(np.uint8)


# ---- the runs: prepare(R) returns the run alone as a callable; legs(R, run), where the alternation is not baseline
# then run; extras(R, out, acc, res) adds the run's own fields, res being what the run's getter returned after the loop.
# R: W (the workload), ctx, a (the arguments) and what prepare leaves for extras.

def dbs_prepare(R):
    return R.ctx.run_dbs


def dbs_legs(R, run):
    def leg(max_mismatch_count, go):            # --max-mismatch-count opens the dbs run's window, the call step keeps 0
        def step():
            R.W.configure(max_mismatch_count)
            go()
            return R.ctx.stats()
        return step
    return [("call", leg(0, R.ctx.run)), ("dbs", leg(R.a.max_mismatch_count, run))]


def dbs_extras(R, out, acc, res):
    out["dbs_max_mismatch_count"] = R.a.max_mismatch_count
    out["log"] = dict(zip(("reads", "runs", "mbs", "trimmed", "window", "candidates", "germ", "HetSite", "HetAltSite", "HomAltSite",
                           "IndelSite", "LowGQ", "LowBQ", "PanelOfNormal", "ComSnp", "LowDepth", "HighDepth", "PASS"), res[1][:18]))


def indels_prepare(R):
    return lambda: R.ctx.run_indels(min_mapq=0, min_gq=20, min_ref_count=2, min_alt_count=2, md_threshold=R.W.md, max_len=50)


def indels_extras(R, out, acc, res):
    from himut_amd import _ffi
    recs, log = res
    out["note"] = "the synthetic reads carry indel errors and no germline indels: time and counts, not recall"
    out["log"] = dict(zip(_ffi.INDEL_LOG_NAMES, log))
    out["events"], out["alleles"], out["records"] = int(log[0]), int(log[1]), int(len(recs))


def indelcal_prepare(R):
    return lambda: R.ctx.run_indelcal(min_mapq=0, max_len=50, min_alt_count=2, vaf_permille=250)


def indelcal_legs(R, run):
    return [("indels", stepper(R, indels_prepare(R))), ("indelcal", stepper(R, run))]


def indelcal_extras(R, out, acc, res):
    import bench
    from himut_amd import _ffi
    table, log = res
    d, rows = out["indelcal"], acc["indelcal"]
    out["note"] = ("the synthetic reference is iid and the reads carry indel errors and no germline indels: its runs are short "
                   "and every rate is the generator's; time and counts, not calibration quality")
    out["log"] = dict(zip(_ffi.INDELCAL_LOG_NAMES, log))
    # the kernels behind the ordered events: ms_hap the bitmap's clearing and the variant marks, ms_eval the event pass,
    # ms_finalize the span sweep
    d["stages"] = {"decode": d["ms_parse"], "events": d["ms_emit"], "sort_order": d["ms_index"],
                   "mark": float(np.mean([r["ms_hap"] for r in rows])), "event_pass": d["ms_eval"], "span_sweep": d["ms_finalize"]}
    # the sweep's bytes: a reference byte per position, and per 256-position block the 32-byte metadata of its window reads
    st = rows[-1]
    reads_staged = st["n_reads"] + st["read_bases"] / 256.0      # a read is in the window of every block it touches
    alg = 1.0 * st["positions"] + 32.0 * reads_staged
    d["sweep_algorithmic_bytes"] = alg
    d["sweep_algorithmic_GBs"] = alg / 1e9 / (d["ms_finalize"] * 1e-3) if d["ms_finalize"] > 0 else None
    d["sweep_hbm_frac"] = d["sweep_algorithmic_GBs"] / bench.HBM_PEAK_GBS if d["sweep_algorithmic_GBs"] else None
    d["Mbp_per_s"] = st["positions"] / 1e6 / (d["ms_total"] * 1e-3)
    out["runs_by_length"] = {str(n + 1): int(table[:, 0].reshape(4, 32)[:, n].sum()) for n in range(32) if table[:, 0].reshape(4, 32)[:, n].sum()}
    out["column_totals"] = dict(zip(_ffi.INDELCAL_COLUMNS, (int(x) for x in table.sum(axis=0))))


def sindels_prepare(R):
    """call's thresholds (the workload's) and the CLI's defaults of the run's own."""
    W = R.W
    return lambda: R.ctx.run_sindels(min_mapq=60, min_gq=20, min_ref_count=3, min_alt_count=1, md_threshold=W.md, max_len=50,
                                     max_run=2, min_qv=30, qlen_lower_limit=W.ql, qlen_upper_limit=W.qu, min_bq=93,
                                     mismatch_window_size=20, max_mismatch_count=0, min_sequence_identity=0.99, min_trim=0.01)


def sindels_legs(R, run):
    return [("indels", stepper(R, indels_prepare(R))), ("sindels", stepper(R, run))]


def sindels_extras(R, out, acc, res):
    from himut_amd import _ffi
    recs, log = res
    d, rows = out["sindels"], acc["sindels"]
    out["note"] = ("the synthetic reads carry indel errors and no somatic or germline indels: every candidate is an error; "
                   "time and counts, neither recall nor precision")
    out["log"] = dict(zip(_ffi.SINDEL_LOG_NAMES, log))
    out["status"] = {_ffi.SINDEL_STATUS_NAMES[int(s)]: int(n) for s, n in zip(*np.unique(recs["status"], return_counts=True))}
    for name in ("indels", "sindels"):
        out[name]["ms_total_series"] = [round(float(r["ms_total"]), 3) for r in acc[name]]
    # ms_hap: the window index and k_sindel_reads (every quality byte of the pile reads once); the window index alone is
    # what the indels leg has between the decode and its events, inside its ms_emit
    hap = float(np.mean([r["ms_hap"] for r in rows]))
    d["stages"] = {"decode": d["ms_parse"], "window_index_and_read_verdicts": hap, "events": d["ms_emit"],
                   "sort_order": d["ms_index"], "eval": d["ms_eval"], "compaction": d["ms_finalize"]}
    st = rows[-1]
    d["read_verdict_bytes"] = float(st["read_bases"])               # a quality byte per query base
    d["read_verdict_GBs_upper_ms"] = hap                            # the window index shares the span: the rate is a lower bound
    d["read_verdict_GBs"] = st["read_bases"] / 1e9 / (hap * 1e-3) if hap > 0 else None
    d["read_verdict_copy_frac"] = d["read_verdict_GBs"] / COPY_CEILING_GBS if d["read_verdict_GBs"] else None


def germline_prepare(R):
    return lambda: R.ctx.run_germline(min_mapq=0, min_gq=20, min_bq=20, min_ref_count=2, min_alt_count=2, md_threshold=R.W.md)


def germline_extras(R, out, acc, res):
    import bench
    recs, log = res
    sample, cs_bytes = R.W.sample, int(R.W.b.cs.shape[0])
    for name, rows in acc.items():              # the capture's algorithmic bytes over its time, as bench.py prices them
        d, st = out[name], rows[-1]
        d["marked_or_candidates"] = d["candidates"]
        cap_bytes = bench.algorithmic_bytes("ms_capture", dict(st, n_candidates=st["n_candidates"] if name == "call" else 0), cs_bytes)
        d["capture_algorithmic_GBs"] = cap_bytes / 1e9 / (d["ms_capture"] * 1e-3) if d["ms_capture"] > 0 else None
    out["log"] = dict(zip(("positions", "nref", "homref", "het", "hetalt", "homalt", "PASS", "LowGQ", "LowBQ", "LowDepth",
                           "HighDepth"), log[:11]))
    # recall among PASS records: the generator's het (gt 1, 2) and hom-alt (gt 3) SNPs; tri-allelic sites (gt 4) apart
    ok = recs[recs["status"] == 0]
    called = {int(t): int(s) for t, s in zip(ok["tpos"], ok["gt_state"])}
    truth = {int(p) + 1: int(g) for p, g in zip(sample.snp_pos, sample.snp_gt)}
    het = [t for t, g in truth.items() if g in (1, 2)]
    hom = [t for t, g in truth.items() if g == 3]
    out["truth"] = {"het": len(het), "hom": len(hom), "tri": sum(g == 4 for g in truth.values()),
                    "het_recall": sum(called.get(t) == 1 for t in het) / max(1, len(het)),
                    "hom_recall": sum(called.get(t) == 3 for t in hom) / max(1, len(hom)),
                    "pass_not_true": sum(t not in truth for t in called), "pass": len(called)}


def sites_prepare(R):
    call_sites(R)
    return lambda: R.ctx.run_sites(R.pos1, R.ref, R.alt)


def sites_extras(R, out, acc, res):
    out["n_sites"] = int(R.pos1.shape[0])
    out["log"] = dict(zip(("sites", "NoCoverage", "Germline", "HetSite", "HetAltSite", "HomAltSite", "IndelSite", "LowGQ", "LowBQ",
                           "PanelOfNormal", "ComSnp", "LowDepth", "HighDepth", "PASS", "alt_seen", "positions"), res[1][:16]))


def support_prepare(R):
    call_sites(R)
    return lambda: R.ctx.run_support(R.pos1, R.ref, R.alt, min_mapq=0, mismatch_window_size=20)


def support_extras(R, out, acc, res):
    rows, counts = res
    n = int(R.pos1.shape[0])
    out["sites"] = n
    out["support"].update(rows=int(rows.shape[0]), rows_per_site=rows.shape[0] / max(1, n),
                          sites_without_rows=int((counts[:, 1] == 0).sum()),
                          mean_cover=float(counts[:, 0].mean()) if counts.shape[0] else 0.0)


def bqcal_prepare(R):
    return lambda: R.ctx.run_bqcal(min_mapq=0, min_gq=20, md_threshold=R.W.md)


def bqcal_extras(R, out, acc, res):
    import bench
    match, mismatch, log = res
    d, st = out["bqcal"], acc["bqcal"][-1]
    out["md_threshold"] = int(R.W.md)
    sweep_ms = d["ms_eval"]                                 # behind the decode: the base check, the tiles, k_bqcal
    alg = 1.5 * st["read_bases"] + 1.0 * st["positions"]    # a cell nibble and a quality byte per pile cell, 1 B per position
    d["sweep_algorithmic_bytes"] = alg
    d["sweep_algorithmic_GBs"] = alg / 1e9 / (sweep_ms * 1e-3) if sweep_ms > 0 else None
    d["sweep_hbm_frac"] = alg / 1e9 / (sweep_ms * 1e-3) / bench.HBM_PEAK_GBS if sweep_ms > 0 else None
    d["Mbp_per_s"] = st["positions"] / 1e6 / (d["ms_total"] * 1e-3)
    out["log"] = dict(zip(("swept", "not_ACGT", "depth", "indel", "low_gq", "homref", "het", "hetalt", "homalt", "only_matches",
                           "mismatches"), log[:11]))
    out["match_total"], out["mismatch_total"] = int(match.sum()), int(mismatch.sum())
    out["bq93"] = {"match": int(match[93]), "mismatch": int(mismatch[93])}


def callable_prepare(R):
    return lambda: R.ctx.run_callable(R.W.tab)


def callable_legs(R, run):
    ctx, tab = R.ctx, R.W.tab

    def tile():                                 # the whole contig through k_norm_tile (himut_debug_normcounts sweep = 1)
        ctx.debug_normcounts(sweep=1)
        ctx.run_normcounts(tab)
        st = ctx.stats()
        ctx.debug_normcounts()
        R.norm_log = ctx.normcounts()[2]
        return st
    return [baseline_leg(R, "normcounts"), ("normcounts_tile", tile), ("callable", stepper(R, run))]


def callable_extras(R, out, acc, res):
    from himut_amd import normcounts
    runs, log = res
    for name, rows in acc.items():
        out[name]["ms_total_series"] = [round(float(r["ms_total"]), 3) for r in rows]
    c, last, tile = out["callable"], acc["callable"][-1], out["normcounts_tile"]
    npos, nruns = int(last["positions"]), int(last["n_records"])
    c["stages"] = {"read_pass": c["ms_index"], "map_sweep": c["ms_eval"], "compaction": c["ms_capture"], "tail": c["ms_finalize"]}
    out["md_threshold"], out["positions"], out["runs"] = int(R.W.md), npos, nruns
    out["map_sweep_over_tile_sweep"] = c["ms_eval"] / tile["ms_eval"] if tile["ms_eval"] > 0 else None
    comp_bytes = 2 * 3.0 * npos + 40.0 * nruns             # the map twice; per run 16 B of bounds and a 24-byte record
    c["compaction_bytes"] = comp_bytes
    c["compaction_GBs"] = comp_bytes / 1e9 / (c["ms_capture"] * 1e-3) if c["ms_capture"] > 0 else None
    c["compaction_copy_frac"] = c["compaction_GBs"] / COPY_CEILING_GBS if c["compaction_GBs"] else None
    out["log"] = dict(zip(normcounts.NORM_LOG_ROWS, log))
    out["log_equals_normcounts"] = log == R.norm_log
    out["state_positions"] = {str(s): int((runs["end"][runs["state"] == s].astype(np.int64) - runs["start"][runs["state"] == s]).sum())
                              for s in sorted(set(runs["state"].tolist()))}


def intervals_sets(length):
    """name of the leg -> (start, end) of its intervals on a contig of ``length``: one interval over the contig, 1 Mb bins,
    10 kb bins, 200,000 intervals of 200 positions at seeded starts."""
    def bins(width):
        start = np.arange(0, length, width, dtype=np.int64)
        return start.astype(np.int32), np.minimum(start + width, length).astype(np.int32)
    seeded = np.random.RandomState(14).randint(0, max(1, length - 200), 200_000).astype(np.int32)
    return {"intervals": (np.zeros(1, np.int32), np.full(1, length, np.int32)), "intervals_1Mb": bins(1_000_000),
            "intervals_10kb": bins(10_000), "intervals_200x200k": (seeded, seeded + 200)}


def intervals_prepare(R):
    R.sets = intervals_sets(int(R.W.b.length))
    R.ctx.run_callable(R.W.tab)                 # the map the tally reads; every round of the loop makes it again
    return lambda: R.ctx.run_intervals(*R.sets["intervals"])


def intervals_legs(R, run):
    def tally(name):
        return stepper(R, lambda: R.ctx.run_intervals(*R.sets[name]))
    # (the one-row set last: what the line's getter fetches behind the loop)
    return [("callable", stepper(R, callable_prepare(R)))] + [(name, tally(name)) for name in reversed(list(R.sets))]


def intervals_extras(R, out, acc, res):
    """Per set: the rows' SHA-1, the entries its intervals cover, and the bytes per second of the tally on 4 B per covered
    entry (state, count, letter) against the copy ceiling."""
    for name, (start, end) in R.sets.items():
        R.ctx.run_intervals(start, end)
        rows = R.ctx.intervals()
        d = out[name]
        d["ms_total_series"] = [round(float(r["ms_total"]), 4) for r in acc[name]]
        d["intervals"], d["entries"] = int(rows.shape[0]), int(rows["entries"].sum())
        d["rows_sha1"] = hashlib.sha1(rows.tobytes()).hexdigest()
        d["tally_bytes"] = 4.0 * d["entries"]
        d["tally_GBs"] = d["tally_bytes"] / 1e9 / (d["ms_total_median"] * 1e-3) if d["ms_total_median"] > 0 else None
        d["tally_copy_frac"] = d["tally_GBs"] / COPY_CEILING_GBS if d["tally_GBs"] else None
    out["callable"]["ms_total_series"] = [round(float(r["ms_total"]), 3) for r in acc["callable"]]
    out["positions"] = int(acc["callable"][-1]["positions"])


def haplotag_prepare(R):
    """The synthetic sample's hetSNPs in synth.write_phased_vcf's default blocks: runs of 200 hetSNPs per phase set."""
    s = R.W.sample
    het = (s.snp_gt == 1) | (s.snp_gt == 2)
    pos1, first = np.unique(s.snp_pos[het].astype(np.int64) + 1, return_index=True)
    R.hsnps = (pos1.astype(np.int32), s.snp_ref[het][first].astype(np.uint8), s.snp_alt[het][first].astype(np.uint8),
               (s.snp_gt[het][first] == 1).astype(np.uint8), (np.arange(pos1.shape[0]) // 200).astype(np.int32))
    return lambda: R.ctx.run_haplotag(*R.hsnps, min_mapq=0, min_bq=20, min_snps=1, min_agree_permille=800)


def haplotag_extras(R, out, acc, res):
    from himut_amd import _ffi
    rows, snps, log = res
    d, st = out["haplotag"], acc["haplotag"][-1]
    d["ms_total_series"] = [round(float(r["ms_total"]), 4) for r in acc["haplotag"]]
    d["stages"] = {"clear_and_decode": d["ms_parse"], "rows_and_tallies": d["ms_eval"]}
    out["hetsnps"], out["sets"] = int(R.hsnps[0].shape[0]), int(R.hsnps[4].max(initial=-1)) + 1
    out["log"] = dict(zip(_ffi.HAPLOTAG_LOG_NAMES, log))
    out["assigned_frac"] = (log[2] + log[3]) / max(1, log[1])
    out["hetsnps_per_pile_read"] = (log[9] + log[10] + log[11] + log[12]) / max(1, log[1])
    out["hetsnps_disagreeing"] = int((snps["disagree"] > snps["agree"]).sum())
    behind = d["ms_eval"]                                   # k_haplotag: per (read, hetSNP) pair a segment search and a base
    d["pairs_per_us"] = out["hetsnps_per_pile_read"] * log[1] / (behind * 1e3) if behind > 0 else None
    d["reads_per_us"] = st["n_reads"] / (d["ms_total"] * 1e3) if d["ms_total"] > 0 else None


def doubled(b):
    """(batch, mate): the batch with every read twice, one behind the other; the copy, with flag 0x10 flipped, is the
    read's opposite-strand mate."""
    from himut_amd.readbatch import ReadBatch
    n = b.n
    rep = {k: np.repeat(getattr(b, k), 2) for k in ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "tp")}
    rep["flag"][1::2] ^= 0x10
    block = np.diff(np.append(b.qoff, b.bq.shape[0]))            # padded bases of each read
    csn = np.diff(b.cs_off)
    qoff = np.concatenate([[0], np.cumsum(np.repeat(block, 2))[:-1]]).astype(np.int64)
    cs_off = np.concatenate([[0], np.cumsum(np.repeat(csn, 2))]).astype(np.int64)
    seq, bq, cs = np.zeros(2 * b.seq.shape[0], np.uint8), np.zeros(2 * b.bq.shape[0], np.uint8), np.zeros(2 * b.cs.shape[0], np.uint8)
    for i in range(n):
        o, w, c, l = int(b.qoff[i]), int(block[i]), int(b.cs_off[i]), int(csn[i])
        for k in (2 * i, 2 * i + 1):
            bq[qoff[k]:qoff[k] + w] = b.bq[o:o + w]
            seq[qoff[k] >> 1:(qoff[k] + w) >> 1] = b.seq[o >> 1:(o + w) >> 1]
            cs[cs_off[k]:cs_off[k] + l] = b.cs[c:c + l]
    d = ReadBatch(name=b.name, length=b.length, qid=np.arange(2 * n, dtype=np.int32), qoff=qoff, cs_off=cs_off, seq=seq, bq=bq, cs=cs, **rep)
    d.validate()
    return d, (np.arange(2 * n, dtype=np.int32) ^ 1)


def duplex_prepare(R):
    """The workload's reads doubled (the pile is twice --depth: run the row with --depth 15 for bench.py's 30x), call's
    thresholds taken again from the doubled reads; the call leg runs on the same reads."""
    from himut_amd import bamlib
    W = R.W
    R.d, R.mate = doubled(W.b)
    ql, qu, md = bamlib.get_thresholds({R.d.name: R.d}, [R.d.name], {R.d.name: R.d.length})
    W.w.configure(30, 60, ql, qu, 0.99, 20, 93, 0.01, 0, 20, md, 3, 1, 3, 1 / (10 ** 3), False)
    R.ctx.push_reads(R.d)
    return lambda: R.ctx.run_duplex(R.mate)


def duplex_extras(R, out, acc, res):
    from himut_amd import _ffi
    recs, ss, log = res
    d, rows = out["duplex"], acc["duplex"]
    out["note"] = ("every read is doubled as its own opposite-strand mate, so every sequencing error is concordant: the row gives "
                   "time and counts, not a mutation rate")
    out["reads"] = int(R.d.n)
    out["log"] = dict(zip(_ffi.DUPLEX_LOG_NAMES, log))
    out["ss"] = dict(zip(_ffi.DUPLEX_SS_CLASSES, ss))
    out["status"] = {_ffi.SITE_STATUS_NAMES[int(s)]: int(n) for s, n in zip(*np.unique(recs["status"], return_counts=True))}
    for name in ("call", "duplex"):
        out[name]["ms_total_series"] = [round(float(r["ms_total"]), 3) for r in acc[name]]
    # ms_hap: the reads' verdicts, the events, the denominator, the keys' sort and encoding, the tallies, with the host's
    # waits for the two counts; the capture is the front's
    hap = float(np.mean([r["ms_hap"] for r in rows]))
    d["stages"] = {"decode": d["ms_parse"], "pair_kernels_and_waits": hap, "column_index": d["ms_index"], "capture": d["ms_capture"],
                   "eval": d["ms_eval"], "tail": d["ms_finalize"]}
    # the pair kernels' bytes: a quality byte per query base for the verdicts, and per position of a pair's overlap a quality
    # byte of either read (here: every read's whole span twice)
    st = rows[-1]
    d["pair_bytes"] = 2.0 * st["read_bases"]
    d["pair_GBs"] = d["pair_bytes"] / 1e9 / (hap * 1e-3) if hap > 0 else None
    d["pair_copy_frac"] = d["pair_GBs"] / COPY_CEILING_GBS if d["pair_GBs"] else None


def _run(baseline, want_ref, prepare, extras, legs=None):
    return SimpleNamespace(baseline=baseline, want_ref=want_ref, prepare=prepare, extras=extras, legs=legs)


RUNS = {"dbs": _run("call", False, dbs_prepare, dbs_extras, dbs_legs),
        "indels": _run("call", True, indels_prepare, indels_extras),
        "indelcal": _run("indels", True, indelcal_prepare, indelcal_extras, indelcal_legs),
        "sindels": _run("indels", True, sindels_prepare, sindels_extras, sindels_legs),
        "germline": _run("call", False, germline_prepare, germline_extras),
        "sites": _run("call", False, sites_prepare, sites_extras),
        "support": _run("call", False, support_prepare, support_extras),
        "bqcal": _run("normcounts", True, bqcal_prepare, bqcal_extras),
        "callable": _run("normcounts", True, callable_prepare, callable_extras, callable_legs),
        "intervals": _run("callable", True, intervals_prepare, intervals_extras, intervals_legs),
        "haplotag": _run("call", False, haplotag_prepare, haplotag_extras),
        "duplex": _run("call", False, duplex_prepare, duplex_extras)}


def stepper(R, run):
    def step():
        run()
        return R.ctx.stats()
    return step


def baseline_leg(R, baseline):
    return baseline, stepper(R, R.ctx.run if baseline == "call" else lambda: R.ctx.run_normcounts(R.W.tab))


def wall(R, name, run, n):
    """n calls of the run alone on the capacities the loop left, timed from the host (every run ends in a host
    synchronise); a SHA-1 of what the run's getter returns then: its records and counters."""
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) * 1e3)
    h = hashlib.sha1()
    for part in getattr(R.ctx, name)():
        h.update(np.ascontiguousarray(part).tobytes())
    return {"wall_calls": n, "wall_ms_median": float(np.median(ms)), "wall_ms_min": float(np.min(ms)),
            "wall_ms_max": float(np.max(ms)), "digest": h.hexdigest()}


def line(name, W, a):
    """The JSON line of run `name` on workload W (built with the reference if the run needs it) for the arguments a."""
    spec = RUNS[name]
    text, steps, warmup = BASELINES[spec.baseline]
    steps, warmup = (steps if a.steps is None else a.steps), (warmup if a.warmup is None else a.warmup)
    R = SimpleNamespace(W=W, ctx=W.ctx, a=a)
    W.configure()                               # a workload may serve several lines: the dbs run's window back to 0
    run = spec.prepare(R)
    legs = spec.legs(R, run) if spec.legs else [baseline_leg(R, spec.baseline), (name, stepper(R, run))]
    acc = alternate(legs, steps, warmup)
    out = {"metric": "{} run against the {}, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(name, text, a.depth),
           "steps": steps, "warmup": warmup, "reads": int(W.b.n), "contig_len": int(W.b.length)}
    for leg, rows in acc.items():
        out[leg] = summarise(rows)
    out["{}_over_{}".format(name, spec.baseline)] = out[name]["ms_total"] / out[spec.baseline]["ms_total"]
    spec.extras(R, out, acc, getattr(W.ctx, name)())
    if a.wall:
        out.update(wall(R, name, run, a.wall))
    return out


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("run", choices=sorted(RUNS))
    ap.add_argument("--steps", type=int, default=None, help="default 20 against the call step, 10 against normcounts")
    ap.add_argument("--warmup", type=int, default=None, help="default 5 against the call step, 3 against normcounts")
    ap.add_argument("--contig-len", type=int, default=64_444_167)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--max-mismatch-count", type=int, default=0, help="of the dbs run (mismatches in the window, the doublet aside)")
    ap.add_argument("--wall", type=int, default=0, metavar="N", help="then N host-timed calls of the run alone, and a digest of its result")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    return ap


def main():
    a = parser().parse_args()
    out = line(a.run, workload(a.contig_len, a.depth, RUNS[a.run].want_ref), a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
