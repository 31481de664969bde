"""himut_id83_classify on a synthetic contig: a seeded 64 Mb string made resident once, and 1,000,000 indel alleles
classified per call.  The alleles have the mix of the read generator's indels (himut_amd/csrc/synth.cpp): anchors uniform
over the string, lengths 1, 2 and 3 equally likely, half deletions and half insertions of random bases; --planted puts a
share of them into planted tandem repeats (units of 1-6 letters, up to 40 copies) with lengths up to 64, the alleles that
make a thread scan far.  About 5 % of the string is soft-masked and 0.5 % is N.

Reports, per call over --reps calls after one warm-up: the device time of k_id83 between the call's events, the upload of
the list in front of it (both from himut_get_stats), the whole call as the host sees it, and a SHA-1 of the bins and the
classes.  Prints one JSON line.

    python tools/bench_spectra.py [--length N] [--alleles N] [--planted SHARE] [--reps K]
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
    """(the string as uint8, the starts and lengths of the planted repeats)."""
    seq = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, n, dtype=np.uint8)]
    nrep = max(1, n // 2000)
    starts = np.sort(rs.randint(0, max(1, n - 300), nrep))
    units = rs.randint(1, 7, nrep)
    copies = rs.randint(2, 41, nrep)
    for s, u, c in zip(starts, units, copies):
        seq[s:s + u * c] = np.tile(seq[s:s + u], c)[:max(0, min(u * c, n - s))]
    for s, l in zip(rs.randint(0, n, n // 40000 + 1), rs.randint(500, 3500, n // 40000 + 1)):
        seq[s:s + l] |= 0x20
    for s, l in zip(rs.randint(0, n, n // 200000 + 1), rs.randint(100, 1900, n // 200000 + 1)):
        seq[s:s + l] = ord("N")
    return seq, starts, units * copies


def make_alleles(rs, n_string, n, planted, starts, spans):
    """(anchor, type, len, bases) of n alleles."""
    anchor = rs.randint(0, n_string - 70, n).astype(np.int32)
    length = rs.randint(1, 4, n).astype(np.int32)
    k = int(n * planted)
    if k:
        pick = rs.randint(0, starts.shape[0], k)
        anchor[:k] = np.minimum(starts[pick] + rs.randint(0, 8, k) - 1, n_string - 70).clip(0)
        length[:k] = np.minimum(rs.randint(1, 65, k), np.maximum(1, spans[pick])).astype(np.int32)
    typ = (rs.rand(n) < 0.5).astype(np.uint8)
    bases = rs.randint(0, 256, (n, 16), dtype=np.uint8)
    order = rs.permutation(n)
    return anchor[order], typ[order], length[order], np.ascontiguousarray(bases[order])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=64 << 20)
    ap.add_argument("--alleles", type=int, default=1_000_000)
    ap.add_argument("--planted", type=float, default=0.0, help="share of the alleles placed in planted repeats, lengths up to 64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=83)
    a = ap.parse_args()
    from himut_amd import caller, normcounts
    rs = np.random.RandomState(a.seed)
    seq, starts, spans = make_string(rs, a.length)
    alleles = make_alleles(rs, a.length, a.alleles, a.planted, starts, spans)
    ctx = caller._worker_for(0).ctx
    raw = seq.tobytes()
    chars, cls256 = normcounts.tri_classes(raw)
    t0 = time.perf_counter()
    ctx.set_reference(raw, cls256, len(chars))
    set_reference_ms = (time.perf_counter() - t0) * 1e3
    ctx.id83_classify(*alleles)                                # buffers, code object
    kernel, upload, host = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        cls, bins = ctx.id83_classify(*alleles)
        host.append((time.perf_counter() - t0) * 1e3)
        st = ctx.stats()
        kernel.append(st["ms_total"])
        upload.append(st["ms_parse"])
    res = {"metric": "himut_id83_classify", "string_bytes": int(a.length), "alleles": int(a.alleles), "planted": a.planted,
           "reps": a.reps, "kernel_ms": round(float(np.median(kernel)), 4), "kernel_ms_min": round(float(np.min(kernel)), 4),
           "kernel_ms_max": round(float(np.max(kernel)), 4), "upload_ms": round(float(np.median(upload)), 4),
           "call_host_ms": round(float(np.median(host)), 3), "set_reference_ms": round(set_reference_ms, 1),
           "alleles_per_us_kernel": round(a.alleles / (float(np.median(kernel)) * 1e3), 1),
           "classified": int(bins[:83].sum()), "num_nbase": int(bins[83]), "num_range": int(bins[84]),
           "digest": hashlib.sha1(bins.tobytes() + cls.tobytes()).hexdigest()}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
