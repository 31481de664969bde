"""The spectra's contract (himut_id83_classify, himut_dbs78_counts) in plain Python: nothing of
the device side or of himut_amd.spectra.  The ID83 rule is written in its literal form -- shift the allele left as far as it
goes, rotating an insertion's bases, then scan right -- where the kernel scans both sides of the allele as it is placed.
The label lists and the DBS78 table are written a second time here, independently of the product's."""

ID83_LABELS = """
1:Del:C:0 1:Del:C:1 1:Del:C:2 1:Del:C:3 1:Del:C:4 1:Del:C:5 1:Del:T:0 1:Del:T:1 1:Del:T:2 1:Del:T:3 1:Del:T:4 1:Del:T:5
1:Ins:C:0 1:Ins:C:1 1:Ins:C:2 1:Ins:C:3 1:Ins:C:4 1:Ins:C:5 1:Ins:T:0 1:Ins:T:1 1:Ins:T:2 1:Ins:T:3 1:Ins:T:4 1:Ins:T:5
2:Del:R:0 2:Del:R:1 2:Del:R:2 2:Del:R:3 2:Del:R:4 2:Del:R:5 3:Del:R:0 3:Del:R:1 3:Del:R:2 3:Del:R:3 3:Del:R:4 3:Del:R:5
4:Del:R:0 4:Del:R:1 4:Del:R:2 4:Del:R:3 4:Del:R:4 4:Del:R:5 5:Del:R:0 5:Del:R:1 5:Del:R:2 5:Del:R:3 5:Del:R:4 5:Del:R:5
2:Ins:R:0 2:Ins:R:1 2:Ins:R:2 2:Ins:R:3 2:Ins:R:4 2:Ins:R:5 3:Ins:R:0 3:Ins:R:1 3:Ins:R:2 3:Ins:R:3 3:Ins:R:4 3:Ins:R:5
4:Ins:R:0 4:Ins:R:1 4:Ins:R:2 4:Ins:R:3 4:Ins:R:4 4:Ins:R:5 5:Ins:R:0 5:Ins:R:1 5:Ins:R:2 5:Ins:R:3 5:Ins:R:4 5:Ins:R:5
2:Del:M:1 3:Del:M:1 3:Del:M:2 4:Del:M:1 4:Del:M:2 4:Del:M:3 5:Del:M:1 5:Del:M:2 5:Del:M:3 5:Del:M:4 5:Del:M:5
""".split()
assert len(ID83_LABELS) == 83 and len(set(ID83_LABELS)) == 83

DBS78_LABELS = """
AC>CA AC>CG AC>CT AC>GA AC>GG AC>GT AC>TA AC>TG AC>TT AT>CA AT>CC AT>CG AT>GA AT>GC AT>TA
CC>AA CC>AG CC>AT CC>GA CC>GG CC>GT CC>TA CC>TG CC>TT CG>AT CG>GC CG>GT CG>TA CG>TC CG>TT
CT>AA CT>AC CT>AG CT>GA CT>GC CT>GG CT>TA CT>TC CT>TG GC>AA GC>AG GC>AT GC>CA GC>CG GC>TA
TA>AT TA>CG TA>CT TA>GC TA>GG TA>GT TC>AA TC>AG TC>AT TC>CA TC>CG TC>CT TC>GA TC>GG TC>GT
TG>AA TG>AC TG>AT TG>CA TG>CC TG>CT TG>GA TG>GC TG>GT TT>AA TT>AC TT>AG TT>CA TT>CC TT>CG TT>GA TT>GC TT>GG
""".split()
assert len(DBS78_LABELS) == 78 and len(set(DBS78_LABELS)) == 78

NBASE, RANGE = "nbase", "range"                 # the two ID83 counters an allele can fall into instead of a class
NLETTER, UNCHANGED = "nletter", "unchanged"     # the two DBS78 counters
LETTERS = "ACGT"


def same(x, y):
    """Two letters match: equal without case, and both of ACGT (N matches nothing, itself included)."""
    return x.upper() == y.upper() and x.upper() in LETTERS


def id83_label(seq, a, kind, L, ins=""):
    """The label of the allele (anchor ``a`` 0-based, ``kind`` "del" or "ins", length ``L``, inserted bases ``ins``) on the
    string ``seq``, or NBASE / RANGE."""
    n = len(seq)
    if kind == "del":
        if a < 0 or a + L >= n:
            return RANGE
        if any(ch.upper() not in LETTERS for ch in seq[a + 1:a + 1 + L]):
            return NBASE
        # as far left as it goes: the base that leaves the stretch on the right equals the one that enters on the left
        while a >= 0 and same(seq[a], seq[a + L]):
            a -= 1
        unit = seq[a + 1:a + 1 + L]
        m = 0
        while a + 1 + L + m < n and same(seq[a + 1 + L + m], seq[a + 1 + m]):
            m += 1
    else:
        if a < 0 or a >= n:
            return RANGE
        if any(ch.upper() not in LETTERS for ch in ins):
            return NBASE
        unit = ins
        while a >= 0 and same(seq[a], unit[-1]):
            unit = unit[-1] + unit[:-1]
            a -= 1
        m = 0
        while a + 1 + m < n and same(seq[a + 1 + m], unit[m % L]):
            m += 1
    word = "Del" if kind == "del" else "Ins"
    if L == 1:
        return "1:{}:{}:{}".format(word, "C" if unit.upper() in "CG" else "T", min(m, 5))
    if kind == "del" and 0 < m < L:
        return "{}:Del:M:{}".format(min(L, 5), min(m, 5))
    return "{}:{}:R:{}".format(min(L, 5), word, min(m // L, 5))


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(s))


def dbs78_label(ref, alt):
    """The label of the doublet, or NLETTER / UNCHANGED."""
    ref, alt = ref.upper(), alt.upper()
    if any(c not in LETTERS for c in ref + alt):
        return NLETTER
    if ref[0] == alt[0] or ref[1] == alt[1]:
        return UNCHANGED
    for r, a in ((ref, alt), (revcomp(ref), revcomp(alt)), (ref, revcomp(alt))):
        if "{}>{}".format(r, a) in DBS78_LABELS:
            return "{}>{}".format(r, a)
    raise AssertionError((ref, alt))


def id83_bins(seq, alleles):
    """(labels, the 88 bins) of a list of (a, kind, L, ins)."""
    labels = [id83_label(seq, *al) for al in alleles]
    bins = [0] * 88
    for k in labels:
        bins[83 if k == NBASE else 84 if k == RANGE else ID83_LABELS.index(k)] += 1
    return labels, bins
