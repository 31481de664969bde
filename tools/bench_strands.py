"""himut_strand_tricounts against himut_ref_tricounts on one resident string: a seeded 64 Mb string (about 5 % soft-masked,
0.5 % N) with about 20,000 random genes (lengths 200 to --gene_len letters, either strand, overlaps as they fall: with
the default 3,000 about two fifths of the string lie in genes and the list has some 35,000 segments; with 60,000 the
genes cover nearly everything and join into a few hundred), the two calls alternated in one process.
himut_ref_tricounts' kernel makes the same pass over the string without the segment lookup and with 32 bins instead of
128: it is the yardstick.

Reports, per call over --reps alternations after one warm-up of each: the device time of each kernel between its call's
events (himut_get_stats), the calls as the host sees them, the bytes per second the strand pass reads, and a SHA-1 of
the 128 bins; the bins summed over the categories must equal the yardstick's.  Prints one JSON line.

    python tools/bench_strands.py [--length N] [--genes N] [--gene_len L] [--reps K]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_string(rs, n):
    seq = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, n, dtype=np.uint8)]
    for s, l in zip(rs.randint(0, n, n // 40000 + 1), rs.randint(500, 3500, n // 40000 + 1)):
        seq[s:s + l] |= 0x20
    for s, l in zip(rs.randint(0, n, n // 200000 + 1), rs.randint(100, 1900, n // 200000 + 1)):
        seq[s:s + l] = ord("N")
    return seq


def make_genes(rs, n, count, longest):
    start = rs.randint(0, n, count)
    length = rs.randint(200, longest + 1, count)
    strand = rs.randint(0, 2, count)
    return [(int(s), int(s + l), "+-"[k]) for s, l, k in zip(start, length, strand)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=64 << 20)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--gene_len", type=int, default=3000, help="the longest gene; lengths are uniform from 200")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=384)
    a = ap.parse_args()
    from himut_amd import caller, normcounts, strands
    rs = np.random.RandomState(a.seed)
    raw = make_string(rs, a.length).tobytes()
    seg_start, seg_mask = strands.segments(make_genes(rs, a.length, a.genes, a.gene_len), a.length)
    ctx = caller._worker_for(0).ctx
    chars, cls256 = normcounts.tri_classes(raw)
    ctx.set_reference(raw, cls256, len(chars))
    ctx.set_strands(seg_start, seg_mask)
    flat, tri = ctx.ref_tricounts(), ctx.strand_tricounts()        # buffers, code objects
    kernel = {"ref": [], "strand": []}
    host = {"ref": [], "strand": []}
    for _ in range(a.reps):
        for name, call in (("ref", ctx.ref_tricounts), ("strand", ctx.strand_tricounts)):
            t0 = time.perf_counter()
            out = call()
            host[name].append((time.perf_counter() - t0) * 1e3)
            kernel[name].append(ctx.stats()["ms_total"])
            if not np.array_equal(out, flat if name == "ref" else tri):
                raise SystemExit("bench_strands: a repeated call gave other bins")
    folded = np.array([flat[f * 16 + m * 4 + l] for f in range(4) for m in (1, 3) for l in range(4)], np.int64)
    if not np.array_equal(tri.sum(axis=0), folded):
        raise SystemExit("bench_strands: the strand bins do not sum to himut_ref_tricounts' bins")
    med = {k: float(np.median(v)) for k, v in kernel.items()}
    res = {"metric": "himut_strand_tricounts", "string_bytes": int(a.length), "genes": int(a.genes), "gene_len": int(a.gene_len),
           "segments": int(seg_start.shape[0]), "reps": a.reps,
           "strand_kernel_ms": round(med["strand"], 4), "strand_kernel_ms_min": round(float(np.min(kernel["strand"])), 4),
           "strand_kernel_ms_max": round(float(np.max(kernel["strand"])), 4),
           "ref_kernel_ms": round(med["ref"], 4), "ref_kernel_ms_min": round(float(np.min(kernel["ref"])), 4),
           "ref_kernel_ms_max": round(float(np.max(kernel["ref"])), 4),
           "ratio": round(med["strand"] / med["ref"], 3) if med["ref"] > 0 else None,
           "strand_gb_per_s": round(a.length / (med["strand"] * 1e6), 1) if med["strand"] > 0 else None,
           "strand_call_host_ms": round(float(np.median(host["strand"])), 3),
           "ref_call_host_ms": round(float(np.median(host["ref"])), 3),
           "per_category": [int(x) for x in tri.sum(axis=1)],
           "digest": hashlib.sha1(tri.tobytes()).hexdigest()}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
