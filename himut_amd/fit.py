"""`himut fit`: which signatures explain a spectrum and how much of each, with bootstrap intervals (no counterpart in
the reference, whose workflow sends the user to external tools at this point).

The spectrum is any table this package writes (`sbs96`, `sbs1536`, `sbs384` / `sbs192`, `id83`, `dbs78`, `normcounts`);
the signatures are a tab-separated matrix in COSMIC's layout.  The files are parsed and the matrix is prepared on the
host; the fit of the spectrum and of every bootstrap replicate runs on the device (himut_fit_exposures).  There is no CPU
implementation: without the HIP library the command raises.

THE DEFINITION is this package's (include/himut_hip.h):

* Inputs: integer counts m[c], c < C, N their sum; a non-negative matrix S[c][k], k < K, whose columns each sum to 1.
* Fit: multiplicative EM for the Poisson / multinomial mixture, T iterations, no early stop.  Start e[k] = N / K.  Step 1,
  for every c: r[c] = sum over k of S[c][k] * e[k], summed sequentially in ascending k from 0.0, and
  q[c] = 0.0 if m[c] == 0 or r[c] == 0.0, else m[c] / r[c].  Step 2, for every k: g = sum over c of S[c][k] * q[c], summed
  sequentially in ascending c from 0.0, and e[k] = e[k] * g.  All arithmetic is fp64, one multiply and one add per term,
  nothing contracted.  The orders are the specification: the exposures are defined to the bit.
* Bootstrap: replicate 0 is m.  Replicate b (1 <= b <= B) draws N mutations; draw i (0 <= i < N) takes
  z = seed + 0x9E3779B97F4A7C15 * (1 + b * 2^32 + i), z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9,
  z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z ^= z >> 31 (all mod 2^64), j = ((z >> 32) * N) >> 32, and lands in the
  smallest c whose inclusive prefix sum of m exceeds j; a channel with m[c] == 0 is never drawn.  Each replicate is fitted
  as above with the same N.
* Limits: 1 <= C <= 1536, 1 <= K <= 96, 0 <= N < 2^31, 0 <= B <= 100,000, 1 <= T <= 100,000.

Around the call, on the host: rows are matched by label; with opportunities w the matrix becomes S'[c][k] = S[c][k] * w[c],
renormalised per column, so the fit runs in the sample's space; channels in which every selected signature is 0 are set
aside and their counts reported as unexplained; columns are normalised by `prepare`, summing in ascending channel order.
"""
import math

import numpy as np

MAX_C, MAX_K, MAX_BOOT, MAX_ITERS = 1536, 96, 100000, 100000
LOG_ROWS = ("channels", "channels_set_aside", "signatures", "N", "replicates", "iterations")
NORMCOUNTS_RATIOS = ("ref_tri_ratio", "ref_ccs_tri_ratio")


class FitError(ValueError):
    """What is wrong with an input file of `himut fit`; the command prints it and exits with status 1."""


class Spectrum:
    """A spectrum table: ``labels`` and ``counts`` in file order; ``header`` and ``rows``, the table's own fields (what
    --opp normcounts reads); ``label_column``."""

    def __init__(self, labels, counts, header, rows, label_column):
        self.labels, self.counts, self.header, self.rows, self.label_column = labels, counts, header, rows, label_column


def read_spectrum(path):
    """Any table this package writes.  The header is the first line that has a field named ``counts``, the label column
    is the one just before it, lines before the header are skipped (the `normcounts` table's command line)."""
    header, labels, counts, rows = None, [], [], []
    with open(path) as fh:
        for line in fh:
            f = line.rstrip("\r\n").split("\t")
            if header is None:
                if "counts" in f:
                    header = f
                    at = f.index("counts")
                    if at == 0:
                        raise FitError("{}: no label column in front of the counts column".format(path))
                continue
            if not line.strip():
                continue
            if len(f) <= at:
                raise FitError("{}: a line with fewer fields than its header: {!r}".format(path, line.rstrip("\r\n")))
            try:
                n = int(f[at])
            except ValueError:
                raise FitError("{}: the count of {} is not an integer: {!r}".format(path, f[at - 1], f[at]))
            if n < 0:
                raise FitError("{}: the count of {} is negative".format(path, f[at - 1]))
            labels.append(f[at - 1]); counts.append(n); rows.append(f)
    if header is None:
        raise FitError("{}: no header line with a field named counts".format(path))
    seen = set()
    for k in labels:
        if k in seen:
            raise FitError("{}: label {} appears twice".format(path, k))
        seen.add(k)
    return Spectrum(labels, counts, header, rows, at - 1)


def _number(path, text, what):
    try:
        x = float(text)
    except ValueError:
        raise FitError("{}: {} is not a number: {!r}".format(path, what, text))
    if not math.isfinite(x) or x < 0.0:
        raise FitError("{}: {} is negative or not finite: {!r}".format(path, what, text))
    return x


def read_signatures(path, select=None):
    """(labels, names, rows): a tab-separated matrix in COSMIC's layout, the first column the labels and each further
    column a signature; ``rows[i][k]`` is label i's entry of signature ``names[k]``.  ``select`` keeps the named columns,
    in the order given."""
    with open(path) as fh:
        lines = [ln.rstrip("\r\n") for ln in fh if ln.strip()]
    if not lines:
        raise FitError("{}: empty".format(path))
    head = lines[0].split("\t")
    names = head[1:]
    if not names:
        raise FitError("{}: no signature column".format(path))
    if len(set(names)) != len(names):
        raise FitError("{}: a signature name appears twice".format(path))
    if select is None:
        cols = list(range(len(names)))
    else:
        cols = []
        for s in select:
            if s not in names:
                raise FitError("{}: no signature named {}".format(path, s))
            if names.index(s) in cols:
                raise FitError("--select names {} twice".format(s))
            cols.append(names.index(s))
    labels, rows, seen = [], [], set()
    for ln in lines[1:]:
        f = ln.split("\t")
        if len(f) != len(head):
            raise FitError("{}: the row of {} has {} fields, the header has {}".format(path, f[0], len(f), len(head)))
        if f[0] in seen:
            raise FitError("{}: label {} appears twice".format(path, f[0]))
        seen.add(f[0])
        labels.append(f[0])
        rows.append([_number(path, f[1 + k], "{} of {}".format(names[k], f[0])) for k in cols])
    return labels, [names[k] for k in cols], rows


def read_opportunities(path):
    """{label: weight} of a table of label and weight, tab-separated; a first line whose weight is not a number is taken
    as the header."""
    out = {}
    with open(path) as fh:
        for i, line in enumerate(fh):
            if not line.strip():
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 2:
                raise FitError("{}: a line without a weight: {!r}".format(path, line.rstrip("\r\n")))
            if i == 0:
                try:
                    float(f[1])
                except ValueError:
                    continue
            if f[0] in out:
                raise FitError("{}: label {} appears twice".format(path, f[0]))
            out[f[0]] = _number(path, f[1], "the weight of {}".format(f[0]))
    return out


def normcounts_weights(spectrum, path="-i"):
    """{label: 1 / (ref_tri_ratio * ref_ccs_tri_ratio)} from a `normcounts` table's own columns: how strongly the callable
    bases over-represent the channel's trinucleotide relative to the genome.  A trinucleotide without a callable base (a
    ratio of 0) has weight 0."""
    for k in NORMCOUNTS_RATIOS:
        if k not in spectrum.header:
            raise FitError("--opp normcounts: {} is not a normcounts table (no column {})".format(path, k))
    a, b = (spectrum.header.index(k) for k in NORMCOUNTS_RATIOS)
    out = {}
    for label, f in zip(spectrum.labels, spectrum.rows):
        if len(f) <= max(a, b):
            raise FitError("{}: the row of {} has no {} / {}".format(path, label, *NORMCOUNTS_RATIOS))
        d = _number(path, f[a], "ref_tri_ratio of " + label) * _number(path, f[b], "ref_ccs_tri_ratio of " + label)
        out[label] = 0.0 if d == 0.0 else 1.0 / d
    return out


class Prepared:
    """What `prepare` hands to the fit: ``labels`` / ``counts`` of the channels kept, ``sig`` ([C, K] float64, columns
    summing to 1: the matrix in the sample's space), ``names``; ``aside`` (label, count) of the channels set aside;
    ``scale[k]`` = sum over c of S[c][k] * w[c] for the column-normalised S over every matched channel (1.0 without
    weights); ``weighted``."""

    def __init__(self, labels, counts, sig, names, aside, scale, weighted, all_labels, all_counts):
        self.labels, self.counts, self.sig, self.names, self.aside, self.scale = labels, counts, sig, names, aside, scale
        self.weighted, self.all_labels, self.all_counts = weighted, all_labels, all_counts

    @property
    def N(self):
        return sum(self.counts)

    @property
    def unexplained(self):
        return sum(n for _k, n in self.aside)


def normalise_columns(rows, names):
    """(rows with every column divided by its sum, the sums): each sum taken in ascending row order from 0.0.  A column
    whose sum is 0 is an error that names it."""
    K = len(names)
    sums = [0.0] * K
    for row in rows:
        for k in range(K):
            sums[k] += row[k]
    for k in range(K):
        if sums[k] == 0.0:
            raise FitError("signature {} sums to 0 over the spectrum's channels".format(names[k]))
    return [[row[k] / sums[k] for k in range(K)] for row in rows], sums


def prepare(labels, counts, sig_labels, names, sig_rows, weights=None):
    """The spectrum (``labels``, ``counts``) and the signature matrix (``sig_labels``, ``names``, ``sig_rows`` as
    read_signatures gives them) as a Prepared.  Rows are matched by label, in the spectrum's order; a label missing on
    either side is an error that names it.  The columns are normalised (normalise_columns); with ``weights`` ({label:
    w}) S'[c][k] = S[c][k] * w[c] is normalised again and ``scale`` keeps the divisors.  Channels in which every column
    of the result is 0 are set aside."""
    at = {k: i for i, k in enumerate(sig_labels)}
    for k in labels:
        if k not in at:
            raise FitError("label {} of the spectrum is not in the signature matrix".format(k))
    have = set(labels)
    for k in sig_labels:
        if k not in have:
            raise FitError("label {} of the signature matrix is not in the spectrum".format(k))
    K = len(names)
    if not 1 <= K <= MAX_K:
        raise FitError("{} signatures: the fit takes 1..{}".format(K, MAX_K))
    rows, _sums = normalise_columns([sig_rows[at[k]] for k in labels], names)
    scale = [1.0] * K
    if weights is not None:
        for k in labels:
            if k not in weights:
                raise FitError("label {} of the spectrum has no opportunity weight".format(k))
        rows, scale = normalise_columns([[x * weights[k] for x in row] for k, row in zip(labels, rows)], names)
    keep = [i for i, row in enumerate(rows) if any(x != 0.0 for x in row)]
    kept = set(keep)
    aside = [(labels[i], counts[i]) for i in range(len(labels)) if i not in kept]
    if not 1 <= len(keep) <= MAX_C:
        raise FitError("{} channels: the fit takes 1..{}".format(len(keep), MAX_C))
    sig = np.array([rows[i] for i in keep], np.float64).reshape(len(keep), K)
    return Prepared([labels[i] for i in keep], [int(counts[i]) for i in keep], sig, list(names), aside, scale,
                    weights is not None, list(labels), [int(x) for x in counts])


def reconstruct(sig, e):
    """r[c] = sum over k of sig[c][k] * e[k], ascending k from 0.0, as Python floats."""
    out = []
    for row in sig.tolist():
        r = 0.0
        for s, x in zip(row, e):
            r += s * x
        out.append(r)
    return out


def cosine(a, b):
    """The cosine similarity of two vectors, summed in ascending order; 0.0 when either is all zero."""
    ab = aa = bb = 0.0
    for x, y in zip(a, b):
        ab += float(x) * y; aa += float(x) * float(x); bb += y * y
    return 0.0 if aa == 0.0 or bb == 0.0 else ab / (math.sqrt(aa) * math.sqrt(bb))


def loglik(counts, recon):
    """The Poisson log-likelihood without its constant: sum over c of m[c] * log(r[c]) - r[c]; -inf where a channel with
    mutations is reconstructed as 0."""
    s = 0.0
    for m, r in zip(counts, recon):
        if m and r <= 0.0:
            return -math.inf
        s += (m * math.log(r) if m else 0.0) - r
    return s


def _total(row):
    s = 0.0
    for x in row:
        s += x
    return s


def summarise(prep, expo, min_fraction=0.05):
    """The figures of the tables from the exposures ``expo`` ([B + 1, K]: row 0 the spectrum's, rows 1..B the
    replicates'), as a dict: recon, cosine, loglik, and per signature exposure, fraction, exposure_genome and, with B > 0,
    lo, median, hi (numpy.percentile 2.5 / 50 / 97.5 over the replicates) and presence (the share of replicates whose
    fraction >= ``min_fraction``)."""
    expo = np.asarray(expo, np.float64)
    e = [float(x) for x in expo[0]]
    total = _total(e)
    recon = reconstruct(prep.sig, e)
    if prep.weighted:
        genome = [x / d for x, d in zip(e, prep.scale)]
        g = _total(genome)
        genome = [0.0 if g == 0.0 else x * (float(prep.N) / g) for x in genome]
    else:
        genome = list(e)
    out = {"exposure": e, "fraction": [0.0 if total == 0.0 else x / total for x in e], "exposure_genome": genome,
           "recon": recon, "cosine": cosine(prep.counts, recon), "loglik": loglik(prep.counts, recon), "boot": None}
    if expo.shape[0] > 1:
        reps = expo[1:]
        pct = np.percentile(reps, [2.5, 50.0, 97.5], axis=0)
        present = [0] * len(e)
        for row in reps.tolist():
            t = _total(row)
            for k, x in enumerate(row):
                if (0.0 if t == 0.0 else x / t) >= min_fraction:
                    present[k] += 1
        out["boot"] = {"lo": [float(x) for x in pct[0]], "median": [float(x) for x in pct[1]], "hi": [float(x) for x in pct[2]],
                       "presence": [n / float(reps.shape[0]) for n in present]}
    return out


def write_exposures(prep, res, out_file):
    """exposures.tsv: the `#` lines (N, fitted N, unexplained, cosine, log-likelihood), then a row per signature; floats
    as repr() writes them."""
    with open(out_file, "w") as o:
        o.write("# N\t{}\n".format(sum(prep.all_counts)))
        o.write("# fitted_N\t{}\n".format(prep.N))
        o.write("# unexplained\t{}\n".format(prep.unexplained))
        o.write("# cosine\t{!r}\n".format(res["cosine"]))
        o.write("# loglik\t{!r}\n".format(res["loglik"]))
        cols = ["exposure", "fraction", "exposure_genome"]
        boot = res["boot"]
        o.write("\t".join(["signature"] + cols + (["lo", "median", "hi", "presence"] if boot else [])) + "\n")
        for k, name in enumerate(prep.names):
            row = [res[c][k] for c in cols] + ([boot[c][k] for c in ("lo", "median", "hi", "presence")] if boot else [])
            o.write("\t".join([name] + [repr(x) for x in row]) + "\n")


def write_recon(prep, res, out_file):
    """--recon: label, counts and reconstructed for every channel of the spectrum, in its order; a channel set aside is
    reconstructed as 0.0."""
    r = dict(zip(prep.labels, res["recon"]))
    with open(out_file, "w") as o:
        o.write("label\tcounts\treconstructed\n")
        for k, n in zip(prep.all_labels, prep.all_counts):
            o.write("{}\t{}\t{!r}\n".format(k, n, r.get(k, 0.0)))


def write_boot(prep, expo, out_file):
    """--boot: the replicate x signature matrix of exposures, replicate 0 (the spectrum itself) first."""
    with open(out_file, "w") as o:
        o.write("\t".join(["replicate"] + prep.names) + "\n")
        for b, row in enumerate(np.asarray(expo, np.float64).tolist()):
            o.write("\t".join([str(b)] + [repr(x) for x in row]) + "\n")


def write_log(prep, n_boot, iters, log_file):
    cells = (len(prep.labels), len(prep.aside), len(prep.names), prep.N, n_boot + 1, iters)
    with open(log_file, "w") as o:
        for name, x in zip(LOG_ROWS, cells):
            o.write("{:30}{}\n".format(name, x))


def load_inputs(spectrum_file, signatures_file, select=None, opp=None):
    """The command's files as a Prepared.  ``select``: a comma separated string or None; ``opp``: a file, the word
    ``normcounts`` or None."""
    spec = read_spectrum(spectrum_file)
    names = [s for s in select.split(",") if s] if select else None
    sig_labels, names, rows = read_signatures(signatures_file, names)
    weights = None
    if opp == "normcounts":
        weights = normcounts_weights(spec, spectrum_file)
    elif opp is not None:
        weights = read_opportunities(opp)
    return prepare(spec.labels, spec.counts, sig_labels, names, rows, weights)


def check_limits(n_boot, iters, N):
    if not 0 <= n_boot <= MAX_BOOT:
        raise FitError("--bootstrap must lie in 0..{}".format(MAX_BOOT))
    if not 1 <= iters <= MAX_ITERS:
        raise FitError("--iters must lie in 1..{}".format(MAX_ITERS))
    if N >= 2 ** 31:
        raise FitError("the spectrum holds 2^31 mutations or more")


def dump_exposures(spectrum_file, signatures_file, out_file, select=None, opp=None, n_boot=1000, seed=1, iters=1000,
                   min_fraction=0.05, recon_file=None, boot_file=None, device=0, log_file="himut_fit.log"):
    """Driver of `himut fit`: the files prepared on the host, the spectrum and its ``n_boot`` replicates fitted on the
    device, the tables and the counters written."""
    from . import _ffi, caller
    _ffi.lib()                                   # no CPU implementation: raises here without the HIP library
    prep = load_inputs(spectrum_file, signatures_file, select, opp)
    check_limits(n_boot, iters, prep.N)
    ctx = caller._worker_for(device).ctx
    expo, _res = ctx.fit_exposures(prep.sig, prep.counts, n_boot=n_boot, seed=seed, iters=iters, want_resampled=False)
    res = summarise(prep, expo, min_fraction)
    write_exposures(prep, res, out_file)
    if recon_file:
        write_recon(prep, res, recon_file)
    if boot_file:
        write_boot(prep, expo, boot_file)
    write_log(prep, n_boot, iters, log_file)
    return expo
