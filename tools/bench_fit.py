"""himut_fit_exposures on a synthetic spectrum: a seeded 96 x 30 signature matrix (columns summing to 1, a fifth of the
entries 0), N = 10,000 mutations drawn from a mixture of five of the signatures, B = 1000 bootstrap replicates, T = 1000
EM iterations.

Reports, per call over --reps calls after one warm-up: the device time of k_fit_resample and of k_fit_em between the
call's events and the upload in front of them (himut_get_stats), the whole call as the host sees it, the LDS a workgroup of
k_fit_em took and whether S was in it, and a SHA-1 of the exposures' bytes.  Beside it, unless --no-numpy, the same
computation as vectorised numpy on this machine's CPU -- the draws as uint64 array arithmetic, searchsorted and bincount,
the EM as two matrix products an iteration over all replicates at once -- with its time and the largest relative
difference from the device's exposures (numpy's products sum in another order, so the last bits differ).  Prints one JSON
line.

    python tools/bench_fit.py [--channels C] [--signatures K] [--mutations N] [--bootstrap B] [--iters T] [--reps R] [--lds-budget BYTES]
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


def make_problem(rs, C, K, N):
    """(sig[C, K], counts[C]): the matrix through fit.normalise_columns, the counts a multinomial draw from a mixture."""
    from himut_amd import fit
    raw = rs.rand(C, K) ** 3
    raw[rs.rand(C, K) < 0.2] = 0.0
    raw[0, :] += 1e-3
    rows, _ = fit.normalise_columns(raw.tolist(), ["s{}".format(k) for k in range(K)])
    sig = np.array(rows, np.float64).reshape(C, K)
    w = np.zeros(K)
    w[rs.choice(K, min(5, K), replace=False)] = rs.dirichlet(np.ones(min(5, K)))
    p = sig @ w
    return sig, rs.multinomial(N, p / p.sum()).astype(np.int64)


def numpy_resample(counts, n_boot, seed):
    """The replicates' counts [n_boot + 1, C] by the definition's generator, as array arithmetic."""
    N, C = int(counts.sum()), counts.shape[0]
    out = np.zeros((n_boot + 1, C), np.int64)
    out[0] = counts
    prefix = np.cumsum(counts)
    i = np.arange(N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for b in range(1, n_boot + 1):
            z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(1) + (np.uint64(b) << np.uint64(32)) + i)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            j = ((z >> np.uint64(32)) * np.uint64(N)) >> np.uint64(32)
            out[b] = np.bincount(np.searchsorted(prefix, j.astype(np.int64), side="right"), minlength=C)
    return out


def numpy_em(sig, reps, iters):
    """The exposures [R, K] of the replicates' counts [R, C]: two matrix products an iteration."""
    m = reps.astype(np.float64)
    e = np.full((reps.shape[0], sig.shape[1]), float(reps[0].sum()) / sig.shape[1])
    sig_t = np.ascontiguousarray(sig.T)
    for _ in range(iters):
        r = e @ sig_t
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where((m == 0) | (r == 0.0), 0.0, m / r)
        e *= q @ sig
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=96)
    ap.add_argument("--signatures", type=int, default=30)
    ap.add_argument("--mutations", type=int, default=10_000)
    ap.add_argument("--bootstrap", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--lds-budget", type=int, default=0, help="himut_debug_fit's LDS budget of a workgroup of k_fit_em in bytes (0: the default)")
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy computation on the CPU")
    a = ap.parse_args()
    from himut_amd import caller
    rs = np.random.RandomState(a.seed)
    sig, counts = make_problem(rs, a.channels, a.signatures, a.mutations)
    ctx = caller._worker_for(0).ctx
    ctx.debug_fit(0, a.lds_budget)
    ctx.fit_exposures(sig, counts, n_boot=a.bootstrap, seed=a.seed, iters=a.iters)          # buffers, code objects
    resample, em, upload, host = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        expo, res = ctx.fit_exposures(sig, counts, n_boot=a.bootstrap, seed=a.seed, iters=a.iters)
        host.append((time.perf_counter() - t0) * 1e3)
        st = ctx.stats()
        resample.append(st["ms_hap"]); em.append(st["ms_eval"]); upload.append(st["ms_parse"])
    med = lambda v: round(float(np.median(v)), 4)
    out = {"metric": "himut_fit_exposures", "channels": a.channels, "signatures": a.signatures, "mutations": int(counts.sum()),
           "bootstrap": a.bootstrap, "iters": a.iters, "reps": a.reps, "resample_kernel_ms": med(resample),
           "em_kernel_ms": med(em), "em_kernel_ms_min": round(float(np.min(em)), 4), "em_kernel_ms_max": round(float(np.max(em)), 4),
           "upload_ms": med(upload), "call_host_ms": med(host), "replicates_per_workgroup": int(st["n_records"]), "em_workgroups": int(st["n_unique_positions"]),
           "em_lds_bytes": int(st["column_slots"]), "sig_in_lds": bool(st["positions"]),
           "em_gflops": round(4.0 * a.channels * a.signatures * a.iters * (a.bootstrap + 1) / (float(np.median(em)) * 1e6), 1),
           "digest": hashlib.sha1(expo.tobytes()).hexdigest()}
    if not a.no_numpy:
        t0 = time.perf_counter()
        reps = numpy_resample(counts, a.bootstrap, a.seed)
        t1 = time.perf_counter()
        e = numpy_em(sig, reps, a.iters)
        t2 = time.perf_counter()
        scale = np.maximum(np.abs(expo), 1e-300)
        out.update({"numpy_resample_ms": round((t1 - t0) * 1e3, 1), "numpy_em_ms": round((t2 - t1) * 1e3, 1),
                    "numpy_counts_equal": bool(np.array_equal(reps, res)),
                    "numpy_max_rel_diff": float(np.max(np.abs(e - expo) / scale * (np.abs(expo) > 1e-6)))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
