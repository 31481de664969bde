"""`himut sbs384`: the transcription-strand spectrum of a `himut call` VCF and its opportunity counts (no counterpart in
the reference; its authors' scripts/gff2sigprofiler_transcripts.py and scripts/draw_sbs192_barplot.py).

SBS384 is the 96 classes of `sbs96` split by where the substitution lies relative to the genes of an annotation; its T
and U blocks alone are SBS192.  A strand split is read next to its denominators, so the same run counts how much of
each trinucleotide the reference holds per category (``--opp``), and `himut intervals --genes --strands` counts how
much of each the caller could call.  The annotation is parsed on the host into a segment list per contig; the
classification and all three tallies run on the device (himut_sbs384_counts, himut_strand_tricounts,
himut_strand_callable over the contig's resident string and the callable run's map).  There is no CPU implementation:
without the HIP library the commands raise.

The definitions are THIS PACKAGE'S (include/himut_hip.h):

* A gene is a stranded interval on a contig.  Per contig the genes become segments: ``seg_start`` ascending from 0,
  segment k covering [seg_start[k], seg_start[k + 1]), the last one running to the contig's end; ``seg_mask[k]`` has
  bit 0 set when a gene on + covers the segment and bit 1 when a gene on - does.  A contig without genes is one
  segment of mask 0.
* The category of a position depends on its segment's mask and on whether the letter at the position -- the VCF's REF
  for a substitution, the centre letter for a trinucleotide -- is a purine, that is, is read on the other strand by
  `sbs96` / `tricount`:
      mask 0 (no gene)      N either way
      mask 1 (+ gene)       pyrimidine here: U     purine here: T
      mask 2 (- gene)       pyrimidine here: T     purine here: U
      mask 3 (both)         B either way
  T means the pyrimidine of the pair lies on the transcribed (template) strand, SigProfiler's convention.  The
  categories are ordered T, U, B, N.
* The class of a substitution is category * 96 + the bin himut_sbs96_counts gives it, labelled ``T:A[C>A]A``; what
  `sbs96` raises for (a class with an N, a class outside the 96, a position at the end of the string) is counted in
  himut_sbs384.log and has no category.
* The trinucleotide class of a position is `intervals`' (first * 8 + (centre == T) * 4 + last after the fold); it exists
  only when all three letters are upper-case ACGT, and a position at either end of the contig has none.
"""
import numpy as np

from ._ffi import INTERVAL_TRI_NAMES
from .normcounts import SBS96_LST, SUB_LST

CATEGORIES = ("T", "U", "B", "N")
NO_CLASS = 0xFFFF
TRI_NAMES = INTERVAL_TRI_NAMES[:32]
# the file's order: a block per category, the 96 in `sbs96`'s order inside it
SBS384_LST = ["{}:{}".format(c, k) for c in CATEGORIES for k in SBS96_LST]
SBS192_LST = SBS384_LST[:192]
# the device's order: label of bin category * 96 + sub * 16 + up * 4 + down
SBS384_BIN_LST = ["{}:{}[{}]{}".format(c, "ACGT"[u], sub, "ACGT"[d]) for c in CATEGORIES for sub in SUB_LST
                  for u in range(4) for d in range(4)]
STRANDS_LOG_ROWS = ("num_genes", "num_unstranded_genes", "num_genes_absent_contig", "num_segments", "num_bases_no_gene",
                    "num_bases_plus_gene", "num_bases_minus_gene", "num_bases_both", "num_sbs", "num_sbs_T", "num_sbs_U",
                    "num_sbs_B", "num_sbs_N", "num_n_class", "num_outside_class", "num_range")
_GFF_SUFFIXES = (".gff", ".gff3", ".gtf")


def read_genes(path, feature="gene"):
    """({contig: [(start, end, strand)]}, {contig: records without a strand}) of an annotation, 0-based half-open, file
    order.  A name that ends in .gff, .gff3 or .gtf is read as GFF3 / GTF: nine tab-separated columns, the records whose
    third column is ``feature``, 1-based inclusive coordinates.  Every other file is BED with at least six columns.  Lines
    that begin with #, track or browser and empty lines are skipped; a strand other than + or - is counted and the record
    skipped."""
    gff = path.lower().endswith(_GFF_SUFFIXES)
    genes, unstranded = {}, {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            arr = line.split("\t")
            if gff:
                if len(arr) != 9:
                    raise ValueError("{}:{}: a GFF3 / GTF line has nine tab-separated columns".format(path, n))
                if arr[2] != feature:
                    continue
                chrom, start, end, strand = arr[0], int(arr[3]) - 1, int(arr[4]), arr[6]
            else:
                if len(arr) < 6:
                    raise ValueError("{}:{}: a BED line of genes has at least six tab-separated columns "
                                     "(chrom, start, end, name, score, strand)".format(path, n))
                chrom, start, end, strand = arr[0], int(arr[1]), int(arr[2]), arr[5]
            if strand not in ("+", "-"):
                unstranded[chrom] = unstranded.get(chrom, 0) + 1
                continue
            genes.setdefault(chrom, []).append((start, end, strand))
    return genes, unstranded


def segments(genes, length):
    """(seg_start int32, seg_mask uint8) of one contig of ``length`` letters from its [(start, end, strand)]: the genes are
    clipped to [0, length), empty ones dropped, and neighbouring stretches with equal masks joined."""
    if length < 1:
        raise ValueError("segments: a contig has at least one letter")
    bounds = {0}
    clipped = {"+": ([], []), "-": ([], [])}
    for start, end, strand in genes:
        s, e = max(int(start), 0), min(int(end), length)
        if s >= e:
            continue
        clipped[strand][0].append(s)
        clipped[strand][1].append(e)
        bounds.add(s)
        if e < length:
            bounds.add(e)
    at = np.array(sorted(bounds), np.int64)
    mask = np.zeros(at.shape[0], np.uint8)
    for bit, strand in ((1, "+"), (2, "-")):
        s, e = (np.sort(np.array(v, np.int64)) for v in clipped[strand])
        depth = np.searchsorted(s, at, side="right") - np.searchsorted(e, at, side="right")
        mask |= np.where(depth > 0, bit, 0).astype(np.uint8)
    keep = np.ones(at.shape[0], bool)
    keep[1:] = mask[1:] != mask[:-1]
    return at[keep].astype(np.int32), mask[keep]


def category_of(mask, purine):
    """The category index (T 0, U 1, B 2, N 3) of a letter in a segment of ``mask``."""
    if mask == 0:
        return 3
    if mask == 3:
        return 2
    return 0 if (mask == 1) == bool(purine) else 1


def bases_per_mask(seg_start, seg_mask, length):
    """[letters of the contig in segments of mask 0, 1, 2, 3]."""
    ends = np.append(np.asarray(seg_start, np.int64)[1:], length)
    out = np.bincount(np.asarray(seg_mask, np.int64), weights=ends - np.asarray(seg_start, np.int64), minlength=4)
    return [int(x) for x in out]


def sbs_categories(seg_start, seg_mask, pos0, ref):
    """The category index per substitution (0-based positions inside the contig, REF letters) on the host."""
    pos0 = np.asarray(pos0, np.int64)
    k = np.searchsorted(np.asarray(seg_start, np.int64), pos0, side="right") - 1
    return np.array([category_of(int(seg_mask[i]), r in "AG") for i, r in zip(k.tolist(), ref)], np.int64)


def write_counts(name, labels, counts, out_file):
    """A spectrum's table: ``name``, counts; ``counts`` maps label -> count."""
    with open(out_file, "w") as o:
        o.write("{}\tcounts\n".format(name))
        for k in labels:
            o.write("{}\t{}\n".format(k, int(counts[k])))


def write_opportunity(tri, out_file):
    """The --opp table: category, trinucleotide, reference count (``tri``: int64[4, 32])."""
    with open(out_file, "w") as o:
        o.write("category\ttri\tref_count\n")
        for c, cat in enumerate(CATEGORIES):
            for t, name in enumerate(TRI_NAMES):
                o.write("{}\t{}\t{}\n".format(cat, name, int(tri[c][t])))


def strand_lines(chrom, pos, bases, sbs=None):
    """The lines of one contig of `intervals --strands`: chrom, category, tri, callable_pos, callable_bases and, with
    ``sbs`` (int64[4, 32]), the substitutions."""
    out = []
    for c, cat in enumerate(CATEGORIES):
        for t, name in enumerate(TRI_NAMES):
            cells = [chrom, cat, name, str(int(pos[c][t])), str(int(bases[c][t]))]
            if sbs is not None:
                cells.append(str(int(sbs[c][t])))
            out.append("\t".join(cells) + "\n")
    return out


def contig_callable(ctx, chrom, genes, length, seq=None, snvs=None):
    """The `intervals --strands` lines of the contig whose callable run ``ctx`` has just completed: the contig's segment
    list goes to the device and the map pass runs once (himut_strand_callable).  ``snvs`` ((pos0, ref, alt) of the contig's
    substitutions, with ``seq``): the sbs column, on the host from intervals.sbs_classes and the segments."""
    seg_start, seg_mask = segments(genes, length)
    ctx.set_strands(seg_start, seg_mask)
    pos, bases = ctx.strand_callable()
    sbs = None
    if snvs is not None:
        from .intervals import OTHER, sbs_classes
        pos0, ref, _alt = snvs
        order = np.argsort(np.asarray(pos0, np.int64), kind="stable")
        sorted_pos, cls = sbs_classes(chrom, seq, pos0, ref)
        cat = sbs_categories(seg_start, seg_mask, sorted_pos, [ref[i] for i in order.tolist()])
        sbs = np.zeros((4, 32), np.int64)
        has = cls < OTHER
        np.add.at(sbs, (cat[has], cls[has]), 1)
    return strand_lines(chrom, pos, bases, sbs)


def dump_sbs384_counts(vcf_file, ref_file, genes_file, region, region_list, out_file, feature="gene", sbs192_file=None,
                       opp_file=None, classes_file=None, device=0, log_file="himut_sbs384.log"):
    """Driver of `himut sbs384`: the substitutions `sbs96` selects (PASS, bi-allelic, single base, the contigs of
    util.load_loci over the VCF's header) classified on the device against the genes of ``genes_file``; the 384 counts,
    with ``sbs192_file`` the T and U blocks, with ``opp_file`` the reference's trinucleotides per category summed over the
    contigs, with ``classes_file`` one line per classified substitution, and the counters.  A selected contig the FASTA
    lacks is reported and skipped.  Returns the counts by label."""
    import contextlib
    from . import _ffi, caller, mutlib, util, vcflib
    from .normcounts import tri_classes
    from .reflib import WHITESPACE, MappedFasta
    _ffi.lib()                                   # no CPU implementation: raises here without the HIP library
    _sample, tname2tsize = mutlib.get_sample(vcf_file)
    chrom_lst, _ = util.load_loci(region, region_list, tname2tsize)
    per_chrom = mutlib._snvs(vcf_file)
    genes, unstranded = read_genes(genes_file, feature)
    bins = np.zeros(387, np.int64)
    tri = np.zeros((4, 32), np.int64)
    chrom2log = {}
    fa = MappedFasta(ref_file)
    try:
        with contextlib.ExitStack() as files:
            cfh = files.enter_context(open(classes_file, "w")) if classes_file else None
            if cfh:
                cfh.write("chrom\tpos\tref\talt\tsbs384\n")
            for chrom in chrom_lst:
                log = chrom2log[chrom] = [0] * len(STRANDS_LOG_ROWS)
                mine = genes.get(chrom, [])
                log[0], log[1] = len(mine), unstranded.get(chrom, 0)
                pos0, ref, alt = per_chrom[chrom]       # KeyError for a contig the header does not list, as `sbs96`
                if chrom not in fa.index:
                    print("himut sbs384: contig {} of {} is not in {}: its {} substitutions and {} genes are skipped".format(
                        chrom, vcf_file, ref_file, len(pos0), len(mine)))
                    log[2] = len(mine)
                    continue
                seq = fa.body(chrom).tobytes().translate(None, WHITESPACE).decode("latin-1")
                ctx = caller._worker_for(device).ctx
                chars, cls = tri_classes(seq)
                ctx.set_reference(seq, cls, len(chars))
                seg_start, seg_mask = segments(mine, len(seq))
                ctx.set_strands(seg_start, seg_mask)
                log[3] = int(seg_start.shape[0])
                log[4:8] = bases_per_mask(seg_start, seg_mask, len(seq))
                if opp_file:
                    tri += ctx.strand_tricounts()
                k, h = ctx.sbs384_counts(pos0, [ord(x) for x in ref], [ord(x) for x in alt], want_classes=cfh is not None)
                bins += h
                log[8] = len(pos0)
                log[9:13] = [int(h[c * 96:(c + 1) * 96].sum()) for c in range(4)]
                log[13:16] = [int(x) for x in h[384:387]]
                if cfh:
                    for p, r, a, b in zip(pos0, ref, alt, k.tolist()):
                        if b != NO_CLASS:
                            cfh.write("{}\t{}\t{}\t{}\t{}\n".format(chrom, p + 1, r, a, SBS384_BIN_LST[b]))
    finally:
        fa.close()
    counts = {SBS384_BIN_LST[b]: int(bins[b]) for b in range(384)}
    write_counts("sbs384", SBS384_LST, counts, out_file)
    if sbs192_file:
        write_counts("sbs192", SBS192_LST, counts, sbs192_file)
    if opp_file:
        write_opportunity(tri, opp_file)
    vcflib.dump_counter_log(STRANDS_LOG_ROWS, chrom_lst, chrom2log, log_file)
    return counts
