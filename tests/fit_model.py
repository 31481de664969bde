"""The definition of `himut fit` (include/himut_hip.h) a second time, in plain Python: integers
masked to 64 bits for the generator, Python floats in explicit loops for the EM.  No numpy reductions, no library call.

Python's float is IEEE fp64 and `*`, `+`, `/` on it are correctly rounded single operations (CPython does not contract
them), so the exposures this model gives are the ones the definition fixes to the bit."""
import bisect
import math

MASK = (1 << 64) - 1


def draw(seed, b, i, N):
    """The channel-independent part of draw i of replicate b: j in 0..N-1."""
    z = (seed + 0x9E3779B97F4A7C15 * (1 + (b << 32) + i)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return ((z >> 32) * N) >> 32


def resample(counts, b, seed):
    """The counts of replicate b: replicate 0 is ``counts``; draw i lands in the smallest c whose inclusive prefix sum
    exceeds j."""
    counts = [int(x) for x in counts]
    if b == 0:
        return counts
    N = sum(counts)
    prefix, s = [], 0
    for m in counts:
        s += m
        prefix.append(s)
    out = [0] * len(counts)
    seed &= MASK
    for i in range(N):
        out[bisect.bisect_right(prefix, draw(seed, b, i, N))] += 1     # the first c with prefix[c] > j
    return out


def em_steps(sig, counts, N, iters):
    """Yields e (a list of K floats) after each of ``iters`` iterations.  ``sig``: C rows of K floats; ``N``: the total the
    start is taken from (a replicate's own sum, which is the spectrum's)."""
    C, K = len(sig), len(sig[0])
    e = [float(N) / float(K)] * K
    for _ in range(iters):
        q = [0.0] * C
        for c in range(C):
            r = 0.0
            row = sig[c]
            for k in range(K):
                r = r + row[k] * e[k]
            q[c] = 0.0 if counts[c] == 0 or r == 0.0 else float(counts[c]) / r
        for k in range(K):
            g = 0.0
            for c in range(C):
                g = g + sig[c][k] * q[c]
            e[k] = e[k] * g
        yield list(e)


def em(sig, counts, N, iters):
    e = None
    for e in em_steps(sig, counts, N, iters):
        pass
    return e


def fit(sig, counts, n_boot=0, seed=1, iters=1000):
    """(exposures, resampled): n_boot + 1 rows each, as himut_fit_exposures defines them.  ``sig`` may be nested lists or an
    array with tolist()."""
    sig = sig.tolist() if hasattr(sig, "tolist") else [list(r) for r in sig]
    counts = [int(x) for x in counts]
    N = sum(counts)
    expo, res = [], []
    for b in range(n_boot + 1):
        m = resample(counts, b, seed)
        res.append(m)
        expo.append(em(sig, m, N, iters))
    return expo, res


def loglik(sig, counts, e):
    """sum over c of m[c] * log(r[c]) - r[c], r = S e; -inf where a channel with mutations has r == 0."""
    s = 0.0
    for row, m in zip(sig, counts):
        r = 0.0
        for x, y in zip(row, e):
            r = r + x * y
        if m and r <= 0.0:
            return -math.inf
        s += (m * math.log(r) if m else 0.0) - r
    return s
