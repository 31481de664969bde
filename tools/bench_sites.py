#!/usr/bin/env python3
"""The sites run against the call step of the same build in one process, on bench.py's workload (the chr20-sized
contig, 30x, reads resident): himut_run and himut_run_sites alternate on the same reads for the same number of warm
steps, the sites run's sites being the call run's own records (about 400 k).  Device ms of each from the runs' own
hipEvents with the per-stage split (timing level 2; the sites run's ms_index holds k_sites_mark and the column index,
ms_eval is k_sites_eval, ms_finalize the totals), column slots and records of each, the sites run's counters.  Prints
one JSON line.

    python tools/bench_sites.py [--steps 20] [--warmup 5] [--contig-len N] [--depth D] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_total", "ms_parse", "ms_index", "ms_capture", "ms_emit", "ms_eval", "ms_finalize")
LOG_ROWS = ("sites", "NoCoverage", "Germline", "HetSite", "HetAltSite", "HomAltSite", "IndelSite", "LowGQ", "LowBQ", "PanelOfNormal",
            "ComSnp", "LowDepth", "HighDepth", "PASS", "alt_seen", "positions")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--contig-len", type=int, default=64_444_167)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    import numpy as np
    import bench
    from himut_amd import bamlib, caller, synth, util as hutil
    sample = synth.generate(synth.SynthConfig(seed=2, contig_len=a.contig_len, depth=a.depth, name="chr20"))
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
    ctx.set_stage_timing(2)
    ctx.run()
    recs = ctx.records()
    # the sites: the call run's records, one per (tpos, ref, alt), by position
    key = np.unique(np.stack([recs["tpos"].astype(np.int64), recs["ref"].astype(np.int64), recs["alt"].astype(np.int64)], 1), axis=0)
    key = key[key[:, 1] != key[:, 2]]
    pos1, ref, alt = key[:, 0].astype(np.int32), key[:, 1].astype(np.uint8), key[:, 2].astype(np.uint8)
    acc = {"call": [], "sites": []}
    for k in range(a.warmup + a.steps):
        ctx.run()
        sc = ctx.stats()
        ctx.run_sites(pos1, ref, alt)
        ss = ctx.stats()
        if k >= a.warmup:
            acc["call"].append(sc)
            acc["sites"].append(ss)
    _recs, log = ctx.sites()
    out = {"metric": "sites run against the call step, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(a.depth),
           "steps": a.steps, "warmup": a.warmup, "reads": int(b.n), "contig_len": int(b.length), "n_sites": int(pos1.shape[0])}
    for name, runs in acc.items():
        st = runs[-1]
        d = {k: float(np.mean([r[k] for r in runs])) for k in STAGES}
        d["ms_total_min"] = float(np.min([r["ms_total"] for r in runs]))
        d["ms_total_max"] = float(np.max([r["ms_total"] for r in runs]))
        d["column_slots"] = int(st["column_slots"])
        d["records"] = int(st["n_records"])
        d["reran"] = int(sum(r["reran"] for r in runs))
        out[name] = d
    out["sites_over_call"] = out["sites"]["ms_total"] / out["call"]["ms_total"]
    out["log"] = dict(zip(LOG_ROWS, log[:16]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
