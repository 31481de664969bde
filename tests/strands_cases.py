"""Hand-built strings, genes and substitutions for the transcription-strand spectrum, with what each must give written
down from the construction (not computed): used by tests/test_strands_cpu.py, tests/test_gpu_strands.py and
tests/test_gpu_strands_cli.py.  The seeded strings and segment lists of the GPU tests are built here too."""
import random

TILE = 4096                                  # positions per workgroup tile of the reference pass

# ---- chr1: ACGT ten times, position p holds "ACGT"[p % 4] -------------------------------------------------------------
CHR1 = "ACGT" * 10
# overlapping (4-12 and 8-20), nested on the same strand (26-28 inside 24-30), one that reaches past the contig's end
CHR1_GENES = [(4, 12, "+"), (8, 20, "-"), (24, 30, "-"), (26, 28, "-"), (36, 100, "+")]
CHR1_SEG_START = [0, 4, 8, 12, 20, 24, 30, 36]
CHR1_SEG_MASK = [0, 1, 3, 2, 0, 2, 0, 1]
CHR1_BASES_PER_MASK = [4 + 4 + 6, 4 + 4, 8 + 6, 4]
# (1-based VCF position, REF, ALT, category, label or the flag it raises)
CHR1_SUBS = [
    (1, "A", "C", "N", "N:G[T>G]A"),         # position 0: the upstream letter is the string's last one (T); no gene
    (2, "C", "T", "N", "N:A[C>T]G"),         # no gene, pyrimidine
    (3, "G", "T", "N", "N:A[C>A]G"),         # no gene, purine
    (4, "T", "C", "N", "N:G[T>C]A"),         # the last position in front of the + gene
    (5, "A", "G", "T", "T:G[T>C]A"),         # the + gene's first position, purine: T
    (6, "C", "T", "U", "U:A[C>T]G"),         # + gene, pyrimidine: U
    (7, "G", "A", "T", "T:A[C>T]G"),         # + gene, purine: T
    (10, "C", "G", "B", "B:A[C>G]G"),        # both strands
    (11, "G", "C", "B", "B:A[C>G]G"),
    (14, "C", "A", "T", "T:A[C>A]G"),        # a - gene with a + strand C: T
    (15, "G", "T", "U", "U:A[C>A]G"),        # - gene, purine: U
    (20, "T", "A", "T", "T:G[T>A]A"),        # the - gene's last position
    (21, "A", "T", "N", "N:G[T>A]A"),        # the first position behind it
    (38, "C", "G", "U", "U:A[C>G]G"),        # the gene that reaches past the end
    (39, "G", "G", None, "outside"),         # ALT equals REF: a class outside the 96
    (40, "T", "C", None, "range"),           # the last position: position + 1 is behind the string
]
# the reference's trinucleotides per category, counted by hand (positions 1 .. 38)
CHR1_OPP = {("T", "ACG"): 6, ("T", "GTA"): 5, ("U", "ACG"): 5, ("U", "GTA"): 5, ("B", "ACG"): 2, ("B", "GTA"): 2,
            ("N", "ACG"): 7, ("N", "GTA"): 6}

# ---- chr2: an N and a lower-case letter; one gene on - ----------------------------------------------------------------
CHR2 = "TTCAGNACgTGA"
CHR2_GENES = [(2, 9, "-")]
CHR2_SEG_START = [0, 2, 9]
CHR2_SEG_MASK = [0, 2, 0]
CHR2_SUBS = [
    (3, "C", "T", "T", "T:T[C>T]A"),
    (4, "A", "C", "U", "U:C[T>G]G"),
    (5, "G", "A", None, "n"),                # the N is its neighbour
    (8, "C", "A", None, "outside"),          # a lower-case neighbour of a pyrimidine
    (11, "G", "T", "N", "N:T[C>A]A"),
    (12, "A", "G", None, "range"),
]
CHR2_OPP = {("N", "TTC"): 1, ("T", "TCA"): 1, ("U", "CTG"): 1, ("N", "TCA"): 1}

FLAG_ROW = {"n": "num_n_class", "outside": "num_outside_class", "range": "num_range"}


def fasta_text():
    return ">chr1 first\n" + "\n".join(CHR1[i:i + 16] for i in range(0, len(CHR1), 16)) + "\n>chr2\n" + CHR2 + "\n"


def vcf_text(extra_contig=False):
    """The substitutions above as PASS lines, with a filtered line, a two-allele line and an indel that `sbs96` does not
    select; ``extra_contig``: a contig chr3 with one substitution that the FASTA lacks."""
    head = ["##fileformat=VCFv4.2", "##contig=<ID=chr1,length={}>".format(len(CHR1)), "##contig=<ID=chr2,length={}>".format(len(CHR2))]
    if extra_contig:
        head.append("##contig=<ID=chr3,length=50>")
    head.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1")
    body = []
    for chrom, subs in (("chr1", CHR1_SUBS), ("chr2", CHR2_SUBS)):
        for pos, ref, alt, _cat, _label in subs:
            body.append("{}\t{}\t.\t{}\t{}\t50\tPASS\t.\tGT\t0/1".format(chrom, pos, ref, alt))
    body.append("chr1\t6\t.\tC\tA\t50\tLowBQ\t.\tGT\t0/1")
    body.append("chr1\t7\t.\tG\tA,T\t50\tPASS\t.\tGT\t1/2")
    body.append("chr1\t9\t.\tAC\tA\t50\tPASS\t.\tGT\t0/1")
    if extra_contig:
        body.append("chr3\t10\t.\tC\tT\t50\tPASS\t.\tGT\t0/1")
    return "\n".join(head + body) + "\n"


def bed_text():
    """The genes as BED: a comment, a gene without a strand, one on a contig that is not there."""
    lines = ["# genes", "track name=genes"]
    for chrom, genes in (("chr1", CHR1_GENES), ("chr2", CHR2_GENES)):
        for k, (s, e, strand) in enumerate(genes):
            lines.append("{}\t{}\t{}\tg{}\t0\t{}".format(chrom, s, e, k, strand))
    lines.append("chr1\t0\t40\tnostrand\t0\t.")
    lines.append("chr9\t5\t50\telsewhere\t0\t+")
    return "\n".join(lines) + "\n"


def gff_text():
    """The same genes as GFF3 (1-based, inclusive), with exon records that a `gene` filter must skip."""
    lines = ["##gff-version 3"]
    for chrom, genes in (("chr1", CHR1_GENES), ("chr2", CHR2_GENES)):
        for k, (s, e, strand) in enumerate(genes):
            lines.append("{}\tsrc\tgene\t{}\t{}\t.\t{}\t.\tID=g{}".format(chrom, s + 1, e, strand, k))
            lines.append("{}\tsrc\texon\t{}\t{}\t.\t{}\t.\tParent=g{}".format(chrom, 1, 3, "+" if strand == "-" else "-", k))
    lines.append("chr1\tsrc\tgene\t1\t40\t.\t.\t.\tID=nostrand")
    lines.append("chr9\tsrc\tgene\t6\t50\t.\t+\t.\tID=elsewhere")
    return "\n".join(lines) + "\n"


def expected_counts():
    """label -> count over both contigs, and flag -> count."""
    counts, flags = {}, {}
    for subs in (CHR1_SUBS, CHR2_SUBS):
        for _pos, _ref, _alt, cat, label in subs:
            if cat is None:
                flags[label] = flags.get(label, 0) + 1
            else:
                counts[label] = counts.get(label, 0) + 1
    return counts, flags


def expected_opp():
    out = dict(CHR1_OPP)
    for k, v in CHR2_OPP.items():
        out[k] = out.get(k, 0) + v
    return out


# ---- seeded strings and segment lists of the GPU tests --------------------------------------------------------------
LENGTHS = (1, 2, 3, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)


def random_string(length, seed=0):
    rs = random.Random(1000 + 31 * length + seed)
    return "".join(rs.choice("ACGTACGTACGTacgtN") for _ in range(length))


def _listed(starts, length, seed):
    """(seg_start, seg_mask) from the starts inside (0, length), masks seeded with all four values and equal neighbours."""
    rs = random.Random(seed)
    starts = [0] + sorted({s for s in starts if 0 < s < length})
    masks = [rs.randrange(4) for _ in starts]
    for k in range(1, len(masks), 5):
        masks[k] = masks[k - 1]                # equal neighbouring masks
    return starts, masks


def segment_lists(length):
    """name -> (seg_start, seg_mask) for a string of ``length``: one segment; boundaries at 1 and at length - 1; at every
    multiple of 16, +- 1; at the tile size, +- 1; 300 one-base segments in a row inside one tile; a segment over three
    tiles.  Lists that a short string cannot hold fall back to what fits."""
    out = {"one": ([0], [2])}
    out["ends"] = _listed([1, length - 1], length, 1)
    out["sixteens"] = _listed([m + d for m in range(16, length + 16, 16) for d in (-1, 0, 1)], length, 2)
    out["tiles"] = _listed([m + d for m in range(TILE, length + TILE, TILE) for d in (-1, 0, 1)], length, 3)
    out["one_base"] = _listed(range(700, 1000), length, 4)
    starts, masks = _listed([TILE - 100, 4 * TILE - 50], length, 5)
    out["long"] = (starts, [1, 3, 2][:len(starts)])
    return out


def substitutions(seq, seg_start, seed=0):
    """(pos0, ref, alt) lists: at each segment's first and last position and just outside it, at position 0, len - 1, -1
    and len; REF is the string's letter upper-cased (N and lower-case neighbours come with the string), ALT seeded."""
    n = len(seq)
    rs = random.Random(seed)
    at = {0, n - 1, -1, n}
    for s in list(seg_start) + [n]:
        at.update((s - 2, s - 1, s, s + 1))
    pos = sorted(at)
    rs.shuffle(pos)
    ref, alt = [], []
    for p in pos:
        r = seq[p].upper() if 0 <= p < n else "C"
        if r not in "ACGT":
            r = rs.choice("AG")
        ref.append(r)
        alt.append(rs.choice([b for b in "ACGTN" if b != r]))
    return pos, ref, alt
