"""`himut id83` and `himut dbs78`: the indel and doublet spectra of a VCF (no counterpart in the reference).

`indels` and `sindels` write indel VCFs and `dbs` writes a doublet VCF; these two commands turn such a file into the
spectrum indel and doublet signatures are defined on: the 83 ID classes and the 78 DBS classes of COSMIC, labelled in
SigProfiler's form so the TSV feeds signature tools as it is.  The VCF is parsed on the host; the classification and the
counting run on the device (himut_id83_classify over the contig's resident string, himut_dbs78_counts).  There is no CPU
implementation: without the HIP library the commands raise.

The classification is THIS PACKAGE'S DEFINITION of the COSMIC scheme (include/himut_hip.h):

* An indel allele is (anchor a, deletion or insertion, length L, inserted bases I).  A deletion removes seq[a+1 .. a+L], an
  insertion puts I between seq[a] and seq[a+1].  Letters compare without case, a byte outside ACGTacgt matches nothing
  (itself included), nothing beyond either end of the string is read.
* Its periodic extent is m = l + r: for a deletion r counts how far seq[a+1+L+j] == seq[a+1+j] holds and l how far
  seq[a-j] == seq[a+L-j] holds; for an insertion r counts seq[a+1+j] == I[j mod L] and l counts
  seq[a-j] == I[(L-1-j) mod L].  The scan ends at m >= 5L.  m is what shifting the allele left as far as it goes (rotating
  an insertion's bases) and then scanning right finds, so the class does not depend on where in its repeat the VCF's
  writer placed the allele.
* L = 1: `1:Del:C|T:n` / `1:Ins:C|T:n`, the deleted or inserted letter with G read as C and A as T, n = min(m, 5): the
  length of the homopolymer run minus one for a deletion, the run's length for an insertion, 5 meaning more.
* L >= 2, deletion with 0 < m < L: microhomology, `s:Del:M:n`, s = min(L, 5), n = min(m, 5).
* L >= 2 otherwise: `s:Del:R:n` / `s:Ins:R:n`, s = min(L, 5), n = min(m // L, 5): the copies of the unit left behind
  (deletion) or present before (insertion).  Insertions have no microhomology class.

DBS78 is a table: a doublet whose reference pair is not one of AC AT CC CG CT GC TA TC TG TT is reverse-complemented, and
for the four self-complementary references (AT CG GC TA) an alternative the table does not list is replaced by its
reverse complement -- COSMIC's representatives.
"""
import numpy as np

ID83_LST = (["1:Del:{}:{}".format(b, n) for b in "CT" for n in range(6)] +
            ["1:Ins:{}:{}".format(b, n) for b in "CT" for n in range(6)] +
            ["{}:Del:R:{}".format(s, n) for s in range(2, 6) for n in range(6)] +
            ["{}:Ins:R:{}".format(s, n) for s in range(2, 6) for n in range(6)] +
            ["{}:Del:M:{}".format(s, n) for s in range(2, 6) for n in range(1, s if s < 5 else 6)])
assert len(ID83_LST) == 83

_DBS78 = (("AC", "CA CG CT GA GG GT TA TG TT"), ("AT", "CA CC CG GA GC TA"), ("CC", "AA AG AT GA GG GT TA TG TT"),
          ("CG", "AT GC GT TA TC TT"), ("CT", "AA AC AG GA GC GG TA TC TG"), ("GC", "AA AG AT CA CG TA"),
          ("TA", "AT CG CT GC GG GT"), ("TC", "AA AG AT CA CG CT GA GG GT"), ("TG", "AA AC AT CA CC CT GA GC GT"),
          ("TT", "AA AC AG CA CC CG GA GC GG"))
DBS78_LST = ["{}>{}".format(r, a) for r, alts in _DBS78 for a in alts.split()]
assert len(DBS78_LST) == 78

MAX_LEN = 64                                 # the longest indel the package's records hold
NO_CLASS = 255
ID83_LOG_ROWS = ("num_alleles", "num_snv_or_mnv", "num_complex", "num_long", "num_ref_mismatch", "num_nbase", "num_range",
                 "num_classified")
DBS78_LOG_ROWS = ("num_doublets", "num_non_acgt", "num_unchanged", "num_classified")
_CODE = {"A": 0, "T": 1, "G": 2, "C": 3}     # the indel record's 2-bit codes (vcflib._INDEL_CODES)


def pack_bases(ins):
    """An insertion's bases (upper-case ACGT, at most 64) as the 16 bytes of the indel record: base j in bits
    2 * (j & 3) of byte j >> 2."""
    row = np.zeros(16, np.uint8)
    for j, ch in enumerate(ins):
        row[j >> 2] |= _CODE[ch] << (2 * (j & 3))
    return row


def vcf_contigs(vcf_file):
    """{contig: length} of a VCF, plain or .bgz: the ##contig lines, then every contig a data line names that the header
    does not (length 0)."""
    from .normcounts import _open_sbs
    sizes = {}
    with _open_sbs(vcf_file) as fh:
        for line in fh:
            if line.startswith("##contig=<ID="):
                arr = line.strip()[len("##contig=<ID="):].rstrip(">").split(",")
                length = [x for x in arr[1:] if x.startswith("length=")]
                sizes[arr[0]] = int(length[0][7:]) if length else 0
            elif not line.startswith("#") and line.strip():
                sizes.setdefault(line.split(None, 1)[0], 0)
    return sizes


def _lines(vcf_file, all_filters):
    """(chrom, pos, ref, [alt]) of the data lines taken: the PASS lines, or every line with ``all_filters``."""
    from .normcounts import _open_sbs
    with _open_sbs(vcf_file) as fh:
        for line in fh:
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 8:
                f = line.split()
            if all_filters or f[6] == "PASS":
                yield f[0], int(f[1]), f[3], f[4].split(",")


class IndelAlleles:
    """The indel alleles of one contig as the arrays of himut_id83_classify, with the VCF's own (pos, ref, alt) per allele;
    ``log``: the host's counters in the order of ID83_LOG_ROWS (the device's three are added by the caller)."""

    def __init__(self):
        self.anchor, self.type, self.len, self.bases, self.text = [], [], [], [], []
        self.log = [0] * len(ID83_LOG_ROWS)

    def arrays(self):
        n = len(self.anchor)
        bases = np.stack(self.bases) if n else np.zeros((0, 16), np.uint8)
        return np.array(self.anchor, np.int32), np.array(self.type, np.uint8), np.array(self.len, np.int32), bases


def sort_allele(out, pos, ref, alt, seq):
    """One ALT allele of a line into ``out`` (an IndelAlleles) or one of its counters.  ``seq``: the contig's string
    (bytes, as the FASTA holds it).  Equal lengths: num_snv_or_mnv.  First bases that differ, or neither allele of length
    1: num_complex.  Longer than 64: num_long.  A deletion whose REF is not the upper-cased string at its place:
    num_ref_mismatch.  An insertion with a base outside ACGT: num_nbase."""
    log = out.log
    log[0] += 1
    if len(ref) == len(alt):
        log[1] += 1
        return
    if ref[:1] != alt[:1] or (len(ref) != 1 and len(alt) != 1) or not ref or not alt:
        log[2] += 1
        return
    L = abs(len(ref) - len(alt))
    if L > MAX_LEN:
        log[3] += 1
        return
    a = pos - 1
    if len(ref) > 1:
        if a < 0 or seq[a:a + 1 + L].upper() != ref.encode("latin-1"):
            log[4] += 1
            return
        out.type.append(0)
        out.bases.append(np.zeros(16, np.uint8))
    else:
        ins = alt[1:].upper()
        if any(ch not in _CODE for ch in ins):
            log[5] += 1
            return
        out.type.append(1)
        out.bases.append(pack_bases(ins))
    out.anchor.append(a)
    out.len.append(L)
    out.text.append((pos, ref, alt))


def load_indel_alleles(vcf_file, chrom_lst, seq_of, all_filters=False):
    """({contig: IndelAlleles} for the contigs of ``chrom_lst`` that ``seq_of(chrom)`` has a string for, {contig: alleles}
    for the others).  Every ALT allele of a line is taken on its own."""
    per_chrom, absent, seqs = {}, {}, {}
    want = set(chrom_lst)
    for chrom, pos, ref, alts in _lines(vcf_file, all_filters):
        if chrom not in want:
            continue
        if chrom not in seqs:
            seqs = {chrom: seq_of(chrom)}            # one contig's string at a time (the lines come contig by contig)
        seq = seqs[chrom]
        if seq is None:
            absent[chrom] = absent.get(chrom, 0) + len(alts)
            continue
        out = per_chrom.setdefault(chrom, IndelAlleles())
        for alt in alts:
            sort_allele(out, pos, ref, alt, seq)
    return per_chrom, absent


def classify_indels(ctx, alleles):
    """(cls, the 83 counts, the eight counters of ID83_LOG_ROWS) of one contig's IndelAlleles on ``ctx``, whose reference
    is that contig's string."""
    cls, h = ctx.id83_classify(*alleles.arrays())
    log = list(alleles.log)
    log[5] += int(h[83])
    log[6] += int(h[84])
    log[7] = int(h[:83].sum())
    return cls, [int(x) for x in h[:83]], log


def write_counts(name, labels, counts, out_file):
    """The spectrum's table: ``name``, counts in bin order."""
    with open(out_file, "w") as o:
        o.write("{}\tcounts\n".format(name))
        for k, c in zip(labels, counts):
            o.write("{}\t{}\n".format(k, int(c)))


def write_classes(fh, chrom, alleles, cls):
    """The --classes lines of one contig: chrom, pos, ref, alt as the VCF has them, and the allele's class."""
    for (pos, ref, alt), k in zip(alleles.text, cls):
        if int(k) != NO_CLASS:
            fh.write("{}\t{}\t{}\t{}\t{}\n".format(chrom, pos, ref, alt, ID83_LST[int(k)]))


def _selected(vcf_file, region, region_list):
    from .util import load_loci
    chrom_lst, _ = load_loci(region, region_list, vcf_contigs(vcf_file))
    return chrom_lst


def dump_id83_counts(vcf_file, ref_file, region, region_list, out_file, all_filters=False, classes_file=None, device=0,
                     log_file="himut_id83.log"):
    """Driver of `himut id83`: the indel alleles of the selected contigs (util.load_loci over the VCF's contigs, as
    `sbs96`), each contig's string made resident through mutlib._device_refs and its alleles classified on the device;
    the 83 counts, with ``classes_file`` one line per classified allele, and the counters."""
    import contextlib
    from . import _ffi, mutlib, util, vcflib
    from .reflib import WHITESPACE
    _ffi.lib()                                   # no CPU implementation: raises here without the HIP library
    chrom_lst = _selected(vcf_file, region, region_list)
    fa, ctx_for = mutlib._device_refs(ref_file, device)

    def seq_of(chrom):
        if chrom not in fa.index:
            return None
        return fa.body(chrom).tobytes().translate(None, WHITESPACE)

    counts = [0] * 83
    chrom2log = {}
    try:
        per_chrom, absent = load_indel_alleles(vcf_file, chrom_lst, seq_of, all_filters)
        for chrom in util.natsorted(absent):
            print("himut id83: contig {} of {} is not in {}: its {} alleles are skipped".format(
                chrom, vcf_file, ref_file, absent[chrom]))
        chrom_lst = [c for c in chrom_lst if c not in absent]
        with contextlib.ExitStack() as files:
            cfh = files.enter_context(open(classes_file, "w")) if classes_file else None
            if cfh:
                cfh.write("chrom\tpos\tref\talt\tid83\n")
            for chrom in chrom_lst:
                alleles = per_chrom.get(chrom)
                if alleles is None:
                    chrom2log[chrom] = [0] * len(ID83_LOG_ROWS)
                    continue
                cls, h, chrom2log[chrom] = classify_indels(ctx_for(chrom), alleles)
                counts = [x + y for x, y in zip(counts, h)]
                if cfh:
                    write_classes(cfh, chrom, alleles, cls)
    finally:
        fa.close()
    write_counts("id83", ID83_LST, counts, out_file)
    vcflib.dump_counter_log(ID83_LOG_ROWS, chrom_lst, chrom2log, log_file)
    return counts


def load_doublets(vcf_file, chrom_lst, all_filters=False):
    """{contig: ([ref], [alt])} of the lines with a two-letter REF and a two-letter ALT without a comma."""
    want = set(chrom_lst)
    per_chrom = {}
    for chrom, _pos, ref, alts in _lines(vcf_file, all_filters):
        if chrom in want and len(alts) == 1 and len(ref) == 2 and len(alts[0]) == 2:
            r, a = per_chrom.setdefault(chrom, ([], []))
            r.append(ref); a.append(alts[0])
    return per_chrom


def dump_dbs78_counts(vcf_file, region, region_list, out_file, all_filters=False, device=0, log_file="himut_dbs78.log"):
    """Driver of `himut dbs78`: the doublets of the selected contigs classified and counted on the device; the 78 counts
    and the counters.  No FASTA is needed."""
    from . import _ffi, caller, vcflib
    _ffi.lib()
    chrom_lst = _selected(vcf_file, region, region_list)
    per_chrom = load_doublets(vcf_file, chrom_lst, all_filters)
    ctx = caller._worker_for(device).ctx
    counts = [0] * 78
    chrom2log = {}
    for chrom in chrom_lst:
        r, a = per_chrom.get(chrom, ([], []))
        ref2 = np.frombuffer("".join(r).encode("latin-1", "replace"), np.uint8).reshape(-1, 2)
        alt2 = np.frombuffer("".join(a).encode("latin-1", "replace"), np.uint8).reshape(-1, 2)
        _cls, h = ctx.dbs78_counts(ref2, alt2, want_classes=False)
        counts = [x + int(y) for x, y in zip(counts, h[:78])]
        chrom2log[chrom] = [len(r), int(h[78]), int(h[79]), int(h[:78].sum())]
    write_counts("dbs78", DBS78_LST, counts, out_file)
    vcflib.dump_counter_log(DBS78_LOG_ROWS, chrom_lst, chrom2log, log_file)
    return counts
