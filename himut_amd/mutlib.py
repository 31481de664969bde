"""`himut sbs96`, `himut sbs1536` and `himut burden` (reference: src/himut/mutlib.py:1998-2230, 2542-2602): the
substitution spectra of a `himut call` VCF and the mutation burden per cell of a `himut normcounts` table.  The
classification and counting run on the device (himut_sbs96_counts / himut_sbs1536_counts over the contig's resident
string); the reference trinucleotide counts of `burden --ref` come from himut_fasta_tricounts.  Only the TSV files
are written: the PDF plots need plotnine."""
import sys

from .normcounts import PUR2PYR, PURINE, SBS96_LST, SUB_LST, TRI_LST

# sorted by (substitution, uu, u, d, dd): uu u [ref>alt] d dd
SBS1536_LST = ["{}{}[{}]{}{}".format(uu, u, sub, d, dd)
               for sub in SUB_LST for uu in "ACGT" for u in "ACGT" for d in "ACGT" for dd in "ACGT"]


def get_sample(vcf_file):
    """vcflib.get_sample (vcflib.py:55-68) for a plain .vcf: the last token of #CHROM and {contig: length} from the
    ##contig lines."""
    tname2tsize = {}
    sample = None
    for line in open(vcf_file).readlines():
        if line.startswith("##"):
            if line.startswith("##contig"):
                arr = line.strip().replace("##contig=<ID=", "").split(",")
                tname2tsize[arr[0]] = int(arr[1].replace("length=", "").replace(">", ""))
        elif line.startswith("#CHROM"):
            sample = line.strip().split()[-1]
            break
    return sample, tname2tsize


def _snvs(vcf_file):
    """{contig: ([pos0], [ref], [alt])} of the PASS bi-allelic SNVs, one entry per ##contig line (KeyError for a record on
    a contig the header does not list, as the reference)."""
    from .normcounts import _open_sbs
    from .vcflib import VcfRecord
    per_chrom = None
    contigs = []
    for line in _open_sbs(vcf_file):
        if line.startswith("##"):
            if line.startswith("##contig"):
                contigs.append(line.strip().replace("##contig=<ID=", "").split(",")[0])
            continue
        if line.startswith("#CHROM"):
            per_chrom = {t: ([], [], []) for t in contigs}
            continue
        v = VcfRecord(line)
        if v.is_snp and v.is_pass:
            p, r, a = per_chrom[v.chrom]
            p.append(v.pos - 1); r.append(v.ref); a.append(v.alt)
    return per_chrom


def get_sbs1536(chrom, pos, ref, alt, refseq):
    """mutlib.get_sbs1536 (pos 0-based): purine references are reported on the other strand."""
    seq = refseq[chrom]
    if ref in PURINE:
        return "{}{}[{}>{}]{}{}".format(*[PUR2PYR.get(c, "N") for c in
                                          (seq[pos + 2], seq[pos + 1], ref, alt, seq[pos - 1], seq[pos - 2])])
    return "{}{}[{}>{}]{}{}".format(seq[pos - 2], seq[pos - 1], ref, alt, seq[pos + 1], seq[pos + 2])


def load_sbs1536_counts(vcf_file, refseq, chrom_lst):
    """Host mirror of mutlib.load_sbs1536_counts (the reference for the device path in the tests): classes that contain
    an N are dropped, KeyError for a class outside the 1536, IndexError for a position at the end of the string."""
    per_chrom = _snvs(vcf_file)
    counts = {k: 0 for k in SBS1536_LST}
    labels = {}
    for chrom in per_chrom:
        d = labels.setdefault(chrom, {})
        for p, r, a in zip(*per_chrom[chrom]):
            k = get_sbs1536(chrom, p, r, a, refseq)
            d[k] = d.get(k, 0) + 1
    for chrom in chrom_lst:
        for k, c in labels[chrom].items():
            if k.count("N") == 0:
                counts[k] += c
    return counts


def load_sbs1536_counts_device(ctx_for, vcf_file, chrom_lst):
    """load_sbs1536_counts with the classification and the counting on the device (himut_sbs1536_counts, k_sbs<2>).
    ``ctx_for(chrom)`` returns a context whose reference is that contig's string."""
    per_chrom = _snvs(vcf_file)
    counts = {k: 0 for k in SBS1536_LST}
    for chrom in chrom_lst:
        p, r, a = per_chrom[chrom]
        if not p:
            continue
        h = ctx_for(chrom).sbs1536_counts(p, [ord(x) for x in r], [ord(x) for x in a])
        if h[1538]:
            raise IndexError("string index out of range")
        if h[1537]:
            raise KeyError("SBS1536 class outside the 1536 (a neighbour or alternative allele that is not A/C/G/T/N)")
        for i, k in enumerate(SBS1536_LST):
            counts[k] += int(h[i])
    return counts


def _device_refs(ref_file, device):
    """ctx_for(chrom) over the mapped FASTA: the contig's string is made resident on the device's worker context."""
    from . import caller
    from .normcounts import tri_classes
    from .reflib import WHITESPACE, MappedFasta
    fa = MappedFasta(ref_file)

    def ctx_for(chrom):
        seq = fa.body(chrom).tobytes().translate(None, WHITESPACE).decode("latin-1")
        ctx = caller._worker_for(device).ctx
        chars, cls = tri_classes(seq)
        ctx.set_reference(seq, cls, len(chars))
        return ctx
    return fa, ctx_for


def dump_sbs96_counts(vcf_file, ref_file, region, region_list, tname2tsize, out_file, device=0):
    """mutlib.dump_sbs96_counts (mutlib.py:2177-2194)."""
    from .normcounts import load_sbs96_counts_device
    from .util import load_loci
    chrom_lst, _ = load_loci(region, region_list, tname2tsize)
    fa, ctx_for = _device_refs(ref_file, device)
    try:
        counts = load_sbs96_counts_device(ctx_for, vcf_file, None, chrom_lst)
    finally:
        fa.close()
    write_sbs96_counts(counts, out_file)


def write_sbs96_counts(counts, out_file):
    """The table of mutlib.dump_sbs96_counts: sub, tri, label, count in sbs96_lst order."""
    o = open(out_file, "w")
    o.write("{}\t{}\t{}\t{}\n".format("sub", "tri", "sbs96", "counts"))
    for k in SBS96_LST:
        o.write("{}\t{}\t{}\t{}\n".format(k[2:5], k[0] + k[2] + k[6], k, counts[k]))
    o.close()


def write_sbs1536_counts(counts, out_file):
    """The table of mutlib.dump_sbs1536_counts (mutlib.py:2197-2230), in its loop order: an empty (tri, sub) group raises
    ZeroDivisionError with the rows before it written, as the reference."""
    group = {}
    for k in SBS1536_LST:
        uu, u, _, ref, _, alt, _, d, dd = list(k)
        key = "{},{}".format(u + ref + d, "{}>{}".format(ref, alt))
        group[key] = group.get(key, 0) + counts[k]
    o = open(out_file, "w")
    try:
        o.write("{}\t{}\t{}\t{}\t{}\t{}\n".format("sub", "tri", "penta", "sbs1536", "counts", "proportion"))
        for k in SBS1536_LST:
            uu, u, _, ref, _, alt, _, d, dd = list(k)
            sub = "{}>{}".format(ref, alt)
            tri = "{}{}{}".format(u, ref, d)
            count = counts[k]
            proportion = count / float(group["{},{}".format(tri, sub)])
            o.write("{}\t{}\t{}\t{}\t{}\t{}\n".format(sub, tri, "{}---{}".format(uu, dd), k, count, proportion))
    finally:
        o.close()


def dump_sbs1536_counts(vcf_file, ref_file, region, region_list, tname2tsize, out_file, device=0):
    """mutlib.dump_sbs1536_counts (mutlib.py:2197-2230)."""
    from .util import load_loci
    chrom_lst, _ = load_loci(region, region_list, tname2tsize)
    fa, ctx_for = _device_refs(ref_file, device)
    try:
        counts = load_sbs1536_counts_device(ctx_for, vcf_file, chrom_lst)
    finally:
        fa.close()
    write_sbs1536_counts(counts, out_file)


def load_ref_tricount(ref_file, tri_file, region_list, tricounts=None):
    """mutlib.load_ref_tricount (mutlib.py:2542-2566): --tri wins over --ref; with neither, the message and exit 0.
    region_list is opened in every case (TypeError when it is None, as the reference).  ``tricounts(path, chrom_lst)``
    counts the FASTA (the device path by default)."""
    chrom_lst = [line.strip() for line in open(region_list).readlines()]
    if tri_file is not None:
        tri2count = dict(line.strip().split() for line in open(tri_file).readlines())
    elif ref_file is not None:
        if tricounts is None:
            from .reflib import get_genome_tricounts_device as tricounts
        tri2count = tricounts(ref_file, chrom_lst)
    else:
        print("Please provide either --ref or --tri file")
        print("exiting himut")
        sys.exit(0)
    return {tri: int(count) for tri, count in tri2count.items()}


def get_burden_per_cell(infile, ref_file, tri_file, region_list, threads, outfile, tricounts=None):
    """mutlib.get_burden_per_cell (mutlib.py:2569-2602).  The reference loads the trinucleotide counts twice, once
    before and once after the table; they are loaded once here, where the first of the two loads is (same result)."""
    tri2mut_rate = {}
    ref_tri2count = load_ref_tricount(ref_file, tri_file, region_list, tricounts)
    for line in open(infile).readlines():
        if line.startswith("#") or line.startswith("sub"):
            continue
        (_sub, tri, _sbs, _count, normcounts, _ref_tri_ratio, _ref_ccs_tri_ratio, _ref_tri_count,
         _ref_callable_tri_count, ccs_callable_tri_count) = line.strip().split()
        tri2mut_rate[tri] = tri2mut_rate.get(tri, 0) + float(normcounts) / int(ccs_callable_tri_count)
    total_mut_count = sum([tri2mut_rate.get(tri, 0) * ref_tri2count[tri] for tri in TRI_LST])
    o = open(outfile, "w")
    o.write("{}\n".format(total_mut_count * 2))
    o.close()
