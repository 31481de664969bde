#!/usr/bin/env python3
"""The germline run against the call step of the same build in one process, on bench.py's workload (the chr20-sized
contig, 30x, reads resident): himut_run and himut_run_germline alternate on the same reads for the same number of warm
steps.  Device ms of each from the runs' own hipEvents with the per-stage split (timing level 2), marked positions and
column slots of each, records per state, recall of the generator's true het and hom SNPs among the PASS records and the
PASS records that are no true SNP (reported, not asserted), the capture's algorithmic bytes over its time as bench.py
prices them.  Prints one JSON line.

    python tools/bench_germline.py [--steps 20] [--warmup 5] [--contig-len N] [--depth D] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_total", "ms_parse", "ms_index", "ms_capture", "ms_emit", "ms_eval", "ms_finalize")


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
    gkw = dict(min_mapq=0, min_gq=20, min_bq=20, min_ref_count=2, min_alt_count=2, md_threshold=md)
    acc = {"call": [], "germline": []}
    for k in range(a.warmup + a.steps):
        ctx.run()
        sc = ctx.stats()
        ctx.run_germline(**gkw)
        sg = ctx.stats()
        if k >= a.warmup:
            acc["call"].append(sc)
            acc["germline"].append(sg)
    recs, log = ctx.germline()
    cs_bytes = int(b.cs.shape[0])
    out = {"metric": "germline run against the call step, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(a.depth),
           "steps": a.steps, "warmup": a.warmup, "reads": int(b.n), "contig_len": int(b.length)}
    for name, rows in acc.items():
        st = rows[-1]
        d = {k: float(np.mean([r[k] for r in rows])) for k in STAGES}
        d["ms_total_min"] = float(np.min([r["ms_total"] for r in rows]))
        d["ms_total_max"] = float(np.max([r["ms_total"] for r in rows]))
        d["marked_or_candidates"] = int(st["n_candidates"])
        d["column_slots"] = int(st["column_slots"])
        d["records"] = int(st["n_records"])
        d["reran"] = int(sum(r["reran"] for r in rows))
        cap_bytes = bench.algorithmic_bytes("ms_capture", dict(st, n_candidates=st["n_candidates"] if name == "call" else 0), cs_bytes)
        d["capture_algorithmic_GBs"] = cap_bytes / 1e9 / (d["ms_capture"] * 1e-3) if d["ms_capture"] > 0 else None
        out[name] = d
    out["germline_over_call"] = out["germline"]["ms_total"] / out["call"]["ms_total"]
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
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
