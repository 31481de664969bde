#!/usr/bin/env python3
"""The indels run against the call step of the same build in one process, on bench.py's workload (the chr20-sized
contig, 30x, reads resident): himut_run and himut_run_indels alternate on the same reads for the same number of warm
steps.  Device ms of each from the runs' own hipEvents with the per-stage split (timing level 2: for the indels run
ms_parse is the decode, ms_emit the events, ms_index their sort and exact order, ms_eval the evaluation, ms_finalize the
compaction), events, alleles and records of the indels run.  The synthetic reads carry indel errors but no germline
indels: this reports time and counts, not recall.  Prints one JSON line.

    python tools/bench_indels.py [--steps 20] [--warmup 5] [--contig-len N] [--depth D] [--out profiles/x.json]
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
    from himut_amd import _ffi, bamlib, caller, normcounts, synth, util as hutil
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
    ctx.set_stage_timing(2)
    ikw = dict(min_mapq=0, min_gq=20, min_ref_count=2, min_alt_count=2, md_threshold=md, max_len=50)
    acc = {"call": [], "indels": []}
    for k in range(a.warmup + a.steps):
        ctx.run()
        sc = ctx.stats()
        ctx.run_indels(**ikw)
        si = ctx.stats()
        if k >= a.warmup:
            acc["call"].append(sc)
            acc["indels"].append(si)
    recs, log = ctx.indels()
    out = {"metric": "indels run against the call step, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(a.depth),
           "note": "the synthetic reads carry indel errors and no germline indels: time and counts, not recall",
           "steps": a.steps, "warmup": a.warmup, "reads": int(b.n), "contig_len": int(b.length)}
    for name, rows in acc.items():
        d = {k: float(np.mean([r[k] for r in rows])) for k in STAGES}
        d["ms_total_min"] = float(np.min([r["ms_total"] for r in rows]))
        d["ms_total_max"] = float(np.max([r["ms_total"] for r in rows]))
        d["records"] = int(rows[-1]["n_records"])
        d["reran"] = int(sum(r["reran"] for r in rows))
        out[name] = d
    out["indels_over_call"] = out["indels"]["ms_total"] / out["call"]["ms_total"]
    out["log"] = dict(zip(_ffi.INDEL_LOG_NAMES, log))
    out["events"], out["alleles"], out["records"] = int(log[0]), int(log[1]), int(len(recs))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
