"""Hand-built cases of `himut fit` with the answer written down: matrices and counts whose exposures follow from the
definition without running it, and a spectrum file of each accepted layout with a signature file and the files the
command must write around the figures."""

# ---- numeric cases: name -> dict(sig = C rows of K floats, counts, iters, and what must hold)


def identity(n):
    return [[1.0 if c == k else 0.0 for k in range(n)] for c in range(n)]


# K = C with the identity matrix: r[c] = e[c], so e[c] becomes e[c] * (m[c] / e[c]); from the second iteration on e[c]
# is within an ulp of m[c] and the product rounds to m[c].  The exposures equal the counts.
IDENTITY_COUNTS = [7, 0, 1, 1000, 3, 250000, 12, 1, 0, 99]

# Two signatures with disjoint support: A on the first four channels, B on the last three.  g_A = sum over A's channels
# of S[c][A] * m[c] / (S[c][A] * e[A]) ~ (sum of A's counts) / e[A]: each exposure equals the sum of its channels' counts
# to 1e-12 relative.
DISJOINT_SIG = [[0.4, 0.0], [0.3, 0.0], [0.2, 0.0], [0.1, 0.0], [0.0, 0.5], [0.0, 0.25], [0.0, 0.25]]
DISJOINT_COUNTS = [11, 0, 29, 3, 40, 17, 100]
DISJOINT_EXPECT = [43.0, 157.0]

# Counts all on channel 0; A is a delta on channel 0, B has 0.001 there and the rest on channel 1.  B's exposure shrinks by
# about 0.001 an iteration, passes through the subnormals and is exactly 0.0 well before iteration 120; channel 1 has
# m == 0 throughout and r == 0.0 from then on.
SUBNORMAL_SIG = [[1.0, 0.001], [0.0, 0.999]]
SUBNORMAL_COUNTS = [1000, 0]
SUBNORMAL_ITERS = 120

# N = 0 and N = 1 under a dense matrix
SMALL_SIG = [[0.5, 0.2, 0.1], [0.25, 0.3, 0.1], [0.125, 0.4, 0.3], [0.125, 0.1, 0.5]]
ZERO_COUNTS = [0, 0, 0, 0]
ONE_COUNTS = [0, 0, 1, 0]

# zero channels at the start, between non-zero channels and at the end: no replicate ever holds a count there
GAPS_SIG = [[0.1, 0.2], [0.1, 0.1], [0.2, 0.1], [0.1, 0.1], [0.1, 0.2], [0.2, 0.1], [0.1, 0.1], [0.1, 0.1]]
GAPS_COUNTS = [0, 0, 9, 0, 0, 14, 2, 0]
GAPS_ZERO = [0, 1, 3, 4, 7]

# ---- files.  Six channels, N = 100; the same spectrum in each layout this package writes.
LABELS = ["A[C>A]A", "A[C>A]C", "A[C>G]A", "A[C>T]G", "T[T>C]A", "T[T>G]T"]
COUNTS = [30, 0, 12, 45, 8, 5]

SPECTRUM_SIMPLE = "sbs384\tcounts\n" + "".join("{}\t{}\n".format(k, n) for k, n in zip(LABELS, COUNTS))
SPECTRUM_SBS96 = "sub\ttri\tsbs96\tcounts\n" + "".join(
    "{}\t{}\t{}\t{}\n".format(k[2:5], k[0] + k[2] + k[6], k, n) for k, n in zip(LABELS, COUNTS))
SPECTRUM_SBS1536 = "sub\ttri\tpenta\tsbs1536\tcounts\tproportion\n" + "".join(
    "{}\t{}\tA---T\t{}\t{}\t0.5\n".format(k[2:5], k[0] + k[2] + k[6], k, n) for k, n in zip(LABELS, COUNTS))
# the normcounts table: its command line first, the two ratios per trinucleotide (TTT has no callable base)
_RATIOS = {"ACA": ("0.5", "0.25"), "ACC": ("0.4", "0.5"), "ACG": ("0.8", "0.5"), "TTA": ("1.0", "0.5"), "TTT": ("0", "0")}
SPECTRUM_NORMCOUNTS = (
    "##himut_command=himut normcounts -i x.bam --ref r.fa --sbs s.vcf counts\n"
    "sub\ttri\tsbs96\tcounts\tnormcounts\tref_tri_ratio\tref_ccs_tri_ratio\tref_tri_count\tref_callable_tri_count\tccs_callable_tri_count\n" +
    "".join("{}\t{}\t{}\t{}\t1.5\t{}\t{}\t100\t50\t200\n".format(k[2:5], k[0] + k[2] + k[6], k, n, *_RATIOS[k[0] + k[2] + k[6]])
            for k, n in zip(LABELS, COUNTS)))
SPECTRA = {"simple": SPECTRUM_SIMPLE, "sbs96": SPECTRUM_SBS96, "sbs1536": SPECTRUM_SBS1536, "normcounts": SPECTRUM_NORMCOUNTS}
# 1 / (ref_tri_ratio * ref_ccs_tri_ratio), worked by hand: 1 / 0.125, 1 / 0.2, 1 / 0.125, 1 / 0.4, 1 / 0.5, and 0 for TTT
NORMCOUNTS_WEIGHTS = {"A[C>A]A": 8.0, "A[C>A]C": 5.0, "A[C>G]A": 8.0, "A[C>T]G": 2.5, "T[T>C]A": 2.0, "T[T>G]T": 0.0}

# the signature matrix, rows in another order than the spectrum's; SigC lives on T[T>G]T alone, which no other column touches
SIGNATURES = ("Type\tSigA\tSigB\tSigC\n"
              "T[T>G]T\t0\t0\t2.0\n"
              "A[C>A]A\t0.5\t0.1\t0\n"
              "A[C>T]G\t0.1\t0.6\t0\n"
              "A[C>A]C\t0.2\t0.0\t0\n"
              "T[T>C]A\t0.1\t0.2\t0\n"
              "A[C>G]A\t0.1\t0.1\t0\n")
SIG_LABELS = ["T[T>G]T", "A[C>A]A", "A[C>T]G", "A[C>A]C", "T[T>C]A", "A[C>G]A"]
SIG_ROWS = [[0.0, 0.0, 2.0], [0.5, 0.1, 0.0], [0.1, 0.6, 0.0], [0.2, 0.0, 0.0], [0.1, 0.2, 0.0], [0.1, 0.1, 0.0]]
# with SigA and SigB selected T[T>G]T is set aside: five channels, 95 mutations fitted, 5 unexplained
SELECT_AB_LABELS = LABELS[:5]
SELECT_AB_COUNTS = COUNTS[:5]
# prepared, in the spectrum's order, columns already summing to 1 (SigC: 2.0 / 2.0)
PREPARED_ALL = [[0.5, 0.1, 0.0], [0.2, 0.0, 0.0], [0.1, 0.1, 0.0], [0.1, 0.6, 0.0], [0.1, 0.2, 0.0], [0.0, 0.0, 1.0]]

OPPORTUNITIES = ("label\tweight\n"
                 "A[C>A]A\t2\n"
                 "A[C>A]C\t1\n"
                 "A[C>G]A\t0.5\n"
                 "A[C>T]G\t1\n"
                 "T[T>C]A\t4\n"
                 "T[T>G]T\t1\n")
OPP_WEIGHTS = {"A[C>A]A": 2.0, "A[C>A]C": 1.0, "A[C>G]A": 0.5, "A[C>T]G": 1.0, "T[T>C]A": 4.0, "T[T>G]T": 1.0}

SIG_MISSING_ROW = "\n".join(ln for ln in SIGNATURES.split("\n") if not ln.startswith("A[C>T]G"))
SIG_EXTRA_ROW = SIGNATURES + "G[T>A]G\t0.1\t0.1\t0\n"
SIG_ZERO_COLUMN = "Type\tSigA\tSigZ\n" + "".join("{}\t{}\t0\n".format(k, x) for k, x in zip(LABELS, (0.5, 0.1, 0.1, 0.1, 0.1, 0.1)))
SIG_NEGATIVE = SIGNATURES.replace("0.6", "-0.6")
SIG_TEXT = SIGNATURES.replace("0.6", "n/a")


def log_text(channels, aside, signatures, n, replicates, iterations):
    """himut_fit.log as the command must write it."""
    rows = (("channels", channels), ("channels_set_aside", aside), ("signatures", signatures), ("N", n),
            ("replicates", replicates), ("iterations", iterations))
    return "".join("{:30}{}\n".format(k, v) for k, v in rows)
