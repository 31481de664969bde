#!/usr/bin/env python3
"""The dbs run against the call step of the same build in one process, on bench.py's workload (the chr20-sized contig,
30x, reads resident): himut_run and himut_run_dbs alternate on the same reads for the same number of warm steps.  Device
ms of each from the runs' own hipEvents with the per-stage split (timing level 2), candidates, column slots and records of
each, the dbs run's twenty counters.  `call`'s parameters for both; --max-mismatch-count opens the dbs run's window (the
call step keeps 0).  Prints one JSON line.

    python tools/bench_dbs.py [--steps 20] [--warmup 5] [--contig-len N] [--depth D] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_total", "ms_parse", "ms_index", "ms_capture", "ms_emit", "ms_eval", "ms_finalize")
LOG_ROWS = ("reads", "runs", "mbs", "trimmed", "window", "candidates", "germ", "HetSite", "HetAltSite", "HomAltSite", "IndelSite",
            "LowGQ", "LowBQ", "PanelOfNormal", "ComSnp", "LowDepth", "HighDepth", "PASS")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--contig-len", type=int, default=64_444_167)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--max-mismatch-count", type=int, default=0, help="of the dbs run (mismatches in the window, the doublet aside)")
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
    ctx = w.ctx
    ctx.set_chunks(chunks)
    ctx.set_site_set(0, pon)
    ctx.set_site_set(1, com)
    ctx.push_reads(b)
    ctx.set_stage_timing(2)

    def configure(max_mismatch_count):
        w.configure(30, 60, ql, qu, 0.99, 20, 93, 0.01, max_mismatch_count, 20, md, 3, 1, 3, 1 / (10 ** 3), False)
    acc = {"call": [], "dbs": []}
    for k in range(a.warmup + a.steps):
        configure(0)
        ctx.run()
        sc = ctx.stats()
        configure(a.max_mismatch_count)
        ctx.run_dbs()
        sd = ctx.stats()
        if k >= a.warmup:
            acc["call"].append(sc)
            acc["dbs"].append(sd)
    _recs, log = ctx.dbs()
    out = {"metric": "dbs run against the call step, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(a.depth),
           "steps": a.steps, "warmup": a.warmup, "reads": int(b.n), "contig_len": int(b.length),
           "dbs_max_mismatch_count": a.max_mismatch_count}
    for name, rows in acc.items():
        st = rows[-1]
        d = {k: float(np.mean([r[k] for r in rows])) for k in STAGES}
        d["ms_total_min"] = float(np.min([r["ms_total"] for r in rows]))
        d["ms_total_max"] = float(np.max([r["ms_total"] for r in rows]))
        d["candidates"] = int(st["n_candidates"])
        d["column_slots"] = int(st["column_slots"])
        d["records"] = int(st["n_records"])
        d["reran"] = int(sum(r["reran"] for r in rows))
        out[name] = d
    out["dbs_over_call"] = out["dbs"]["ms_total"] / out["call"]["ms_total"]
    out["log"] = dict(zip(LOG_ROWS, log[:18]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
