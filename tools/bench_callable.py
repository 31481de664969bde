#!/usr/bin/env python3
"""The callable run against the normcounts run of the same build in one process, on bench.py's workload (the chr20-sized
contig, 30x, reads resident): three runs alternate on the same reads, chunks and reference string for the same number
of warm steps -- himut_run_normcounts, himut_run_normcounts with the whole contig through k_norm_tile
(himut_debug_normcounts sweep = 1), and himut_run_callable.  Device ms of each from the runs' own hipEvents (timing
level 2); for the callable run the stages: read pass, map sweep, run compaction, tail.  The map sweep against the
sweep = 1 normcounts sweep (the same work plus 3 B stored per position); the compaction's bytes -- the map read twice, 3 B
per position each time, and the records written -- over its time, and their fraction of the copy ceiling; the run
count and the fourteen counters, which must equal the normcounts run's.  Prints one JSON line.

    python tools/bench_callable.py [--steps 10] [--warmup 3] [--contig-len N] [--depth D] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_total", "ms_parse", "ms_index", "ms_capture", "ms_eval", "ms_finalize")
COPY_CEILING_GBS = 6300.0          # DESIGN: what a device-to-device copy reaches on this part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--contig-len", type=int, default=64_444_167)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    import numpy as np
    import bench
    from himut_amd import bamlib, caller, normcounts, synth, util as hutil
    sample = synth.generate(synth.SynthConfig(seed=2, contig_len=a.contig_len, depth=a.depth, name="chr20"), want_ref=True)
    b = sample.batch
    chunks = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
    ql, qu, md = bamlib.get_thresholds({b.name: b}, [b.name], {b.name: b.length})
    pon, com = bench.make_side_sets(sample, 100)
    w = caller.Worker(0)
    w.configure(30, 60, ql, qu, 0.99, 20, 93, 0.01, 0, 20, md, 3, 1, 3, 1 / (10 ** 3), False)
    ctx = w.ctx
    ctx.set_chunks(chunks)
    ctx.set_site_set(0, pon)
    ctx.set_site_set(1, com)
    ctx.push_reads(b)
    refseq = bytes(sample.ref)
    chars, cls = normcounts.tri_classes(refseq)
    ctx.set_reference(refseq, cls, len(chars))
    tab = normcounts.alt_order_table(bench.NORM_ALT_ORDER)
    ctx.set_stage_timing(2)
    acc = {"normcounts": [], "normcounts_tile": [], "callable": []}
    for k in range(a.warmup + a.steps):
        ctx.run_normcounts(tab)
        sn = ctx.stats()
        ctx.debug_normcounts(sweep=1)
        ctx.run_normcounts(tab)
        st = ctx.stats()
        ctx.debug_normcounts()
        norm_log = ctx.normcounts()[2]
        ctx.run_callable(tab)
        sc = ctx.stats()
        if k >= a.warmup:
            acc["normcounts"].append(sn)
            acc["normcounts_tile"].append(st)
            acc["callable"].append(sc)
    runs, log = ctx.callable()
    out = {"metric": "callable run against the normcounts run, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(a.depth),
           "steps": a.steps, "warmup": a.warmup, "reads": int(b.n), "contig_len": int(b.length), "md_threshold": int(md)}
    for name, rows in acc.items():
        d = {k: float(np.mean([r[k] for r in rows])) for k in STAGES}
        d["ms_total_series"] = [round(float(r["ms_total"]), 3) for r in rows]
        d["ms_total_median"] = float(np.median([r["ms_total"] for r in rows]))
        d["reran"] = int(sum(r["reran"] for r in rows))
        out[name] = d
    c = out["callable"]
    last = acc["callable"][-1]
    npos, nruns = int(last["positions"]), int(last["n_records"])
    c["stages"] = {"read_pass": c["ms_index"], "map_sweep": c["ms_eval"], "compaction": c["ms_capture"], "tail": c["ms_finalize"]}
    out["positions"], out["runs"] = npos, nruns
    out["callable_over_normcounts"] = c["ms_total"] / out["normcounts"]["ms_total"]
    out["map_sweep_over_tile_sweep"] = c["ms_eval"] / out["normcounts_tile"]["ms_eval"] if out["normcounts_tile"]["ms_eval"] > 0 else None
    comp_bytes = 2 * 3.0 * npos + 40.0 * nruns             # the map twice; per run 16 B of bounds and a 24-byte record
    c["compaction_bytes"] = comp_bytes
    c["compaction_GBs"] = comp_bytes / 1e9 / (c["ms_capture"] * 1e-3) if c["ms_capture"] > 0 else None
    c["compaction_copy_frac"] = c["compaction_GBs"] / COPY_CEILING_GBS if c["compaction_GBs"] else None
    out["log"] = dict(zip(normcounts.NORM_LOG_ROWS, log))
    out["log_equals_normcounts"] = log == norm_log
    out["state_positions"] = {str(s): int((runs["end"][runs["state"] == s].astype(np.int64) - runs["start"][runs["state"] == s]).sum())
                              for s in sorted(set(runs["state"].tolist()))}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
