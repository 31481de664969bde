#!/usr/bin/env python3
"""The bqcal run against the normcounts run of the same build in one process, on bench.py's workload (the chr20-sized
contig, 30x, reads resident): himut_run_bqcal and himut_run_normcounts alternate on the same reads, regions and reference
string for the same number of warm steps.  Device ms of each from the runs' own hipEvents with the per-stage split
(timing level 2), their ratio, the bqcal run's algorithmic bytes (1.5 B per read base: a cell nibble and a quality byte
per pile cell, plus 1 B per reference position) over the sweep's time and their fraction of the HBM peak, the twelve
counters and the table's row at BQ 93.  Prints one JSON line.

    python tools/bench_bqcal.py [--steps 10] [--warmup 3] [--contig-len N] [--depth D] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("ms_total", "ms_parse", "ms_index", "ms_capture", "ms_eval", "ms_finalize")
LOG = ("swept", "not_ACGT", "depth", "indel", "low_gq", "homref", "het", "hetalt", "homalt", "only_matches", "mismatches")


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
    acc = {"normcounts": [], "bqcal": []}
    for k in range(a.warmup + a.steps):
        ctx.run_normcounts(tab)
        sn = ctx.stats()
        ctx.run_bqcal(min_mapq=0, min_gq=20, md_threshold=md)
        sb = ctx.stats()
        if k >= a.warmup:
            acc["normcounts"].append(sn)
            acc["bqcal"].append(sb)
    match, mismatch, log = ctx.bqcal()
    out = {"metric": "bqcal run against the normcounts run, device ms (chr20-sized contig, {:.0f}x, reads resident)".format(a.depth),
           "steps": a.steps, "warmup": a.warmup, "reads": int(b.n), "contig_len": int(b.length), "md_threshold": int(md)}
    for name, rows in acc.items():
        d = {k: float(np.mean([r[k] for r in rows])) for k in STAGES}
        d["ms_total_min"] = float(np.min([r["ms_total"] for r in rows]))
        d["ms_total_max"] = float(np.max([r["ms_total"] for r in rows]))
        d["reran"] = int(sum(r["reran"] for r in rows))
        out[name] = d
    st = acc["bqcal"][-1]
    out["bqcal_over_normcounts"] = out["bqcal"]["ms_total"] / out["normcounts"]["ms_total"]
    sweep_ms = out["bqcal"]["ms_eval"]                      # behind the decode: the base check, the tiles, k_bqcal
    alg = 1.5 * st["read_bases"] + 1.0 * st["positions"]
    out["bqcal"]["sweep_algorithmic_bytes"] = alg
    out["bqcal"]["sweep_algorithmic_GBs"] = alg / 1e9 / (sweep_ms * 1e-3) if sweep_ms > 0 else None
    out["bqcal"]["sweep_hbm_frac"] = alg / 1e9 / (sweep_ms * 1e-3) / bench.HBM_PEAK_GBS if sweep_ms > 0 else None
    out["bqcal"]["Mbp_per_s"] = st["positions"] / 1e6 / (out["bqcal"]["ms_total"] * 1e-3)
    out["log"] = dict(zip(LOG, log[:11]))
    out["match_total"], out["mismatch_total"] = int(match.sum()), int(mismatch.sum())
    out["bq93"] = {"match": int(match[93]), "mismatch": int(mismatch[93])}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
