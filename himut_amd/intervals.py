"""`himut intervals`: callable counts and mutation burden per BED interval.

`himut callable` leaves the normcounts verdict of every swept position in HBM: a state and the callable read bases per
position.  This run asks that map what lies inside each interval of a BED file (exons, a capture panel, replication
timing bins) or of a fixed-width binning: the entries and bases per state and three histograms over the trinucleotide
class of the position (himut_run_intervals), tallied on the device while the contig is still resident.  The run in front
of it is the callable run, so every flag of `callable` means here what it means there.  The contract is DESIGN.md section
8 (Row 14) and include/himut_hip.h.  There is no CPU implementation: without the HIP library the call raises.

With ``--sbs`` the substitutions `sbs96` counts (PASS, bi-allelic, single base) are placed into every interval that holds
them, by the same trinucleotide class, and four columns are derived per interval -- definitions chosen here:
    sbs             the substitutions in the interval, all 33 classes
    sbs_uncallable  those of class ``other`` or of a class without a callable base in the interval (ccs_tri == 0)
    rate            (sbs - sbs_uncallable) / sum(ccs_tri[:32])
    burden          2 * sum over the classes c < 32 with ccs_tri[c] > 0 of sbs_tri[c] / ccs_tri[c] * all_tri[c]
both printed with repr, NA without a denominator.

With ``--genes`` and ``--strands`` the contig's CALLABLE entries are also tallied by transcription-strand category and
trinucleotide class (himut_strand_callable, once per contig behind the intervals run; the definitions are `himut sbs384`'s,
strands.py): one line per contig, category and class.
"""
import numpy as np

from ._ffi import CALLABLE_STATES, INTERVAL_TRI_NAMES

CALLABLE = 13
OTHER = 32
HEADER = ["chrom", "start", "end", "name", "length", "entries", "callable_pos", "callable_bases", "sbs", "sbs_uncallable",
          "rate", "burden"]
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def read_bed(path):
    """[(chrom, start, end, name)] of a tab-separated BED file in file order; lines that begin with #, track or browser
    and empty lines are skipped; a line without a fourth column has the name "."."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            arr = line.split("\t")
            if len(arr) < 3:
                raise ValueError("{}:{}: a BED line has chrom, start and end, tab-separated".format(path, n))
            out.append((arr[0], int(arr[1]), int(arr[2]), arr[3] if len(arr) > 3 and arr[3] != "" else "."))
    return out


def bin_intervals(chrom, length, bin_size):
    """[(chrom, k * N, min((k + 1) * N, length), name)] over one contig."""
    if bin_size <= 0:
        raise ValueError("--bin_size must be positive")
    return [(chrom, a, min(a + bin_size, length), "{}:{}-{}".format(chrom, a, min(a + bin_size, length)))
            for a in range(0, length, bin_size)]


def tri_class(seq, pos):
    """The class of position ``pos`` (0-based) of ``seq``: the key normcounts' get_tri_context gives -- case-sensitive, an
    upper-case purine centre read on the other strand, NNN at the string's ends -- as first * 8 + (centre == T) * 4 + last
    with A0 C1 G2 T3 for the 32 pyrimidine-centred ACGT keys, 32 for every other key."""
    if pos - 1 < 0 or pos + 2 > len(seq):
        return OTHER
    a, m, b = (_CODE.get(ch, -1) for ch in seq[pos - 1:pos + 2])
    if a < 0 or m < 0 or b < 0:
        return OTHER
    if m & 1:
        return a * 8 + (4 if m == 3 else 0) + b
    return (3 - b) * 8 + (4 if m == 0 else 0) + (3 - a)


def sbs_classes(chrom, seq, pos0, ref):
    """(positions ascending, their classes) of a contig's substitutions; a REF that is not the string's letter raises."""
    pos0 = np.asarray(pos0, np.int64)
    order = np.argsort(pos0, kind="stable")
    cls = np.zeros(pos0.shape[0], np.int64)
    for k, p in enumerate(pos0.tolist()):
        if not 0 <= p < len(seq) or seq[p].upper() != ref[k]:
            raise ValueError("{}:{}: REF {} of --sbs is not the reference's letter {}".format(
                chrom, p + 1, ref[k], seq[p] if 0 <= p < len(seq) else "(outside the contig)"))
        cls[k] = tri_class(seq, p)
    return pos0[order], cls[order]


def sbs_per_interval(start, end, pos_sorted, cls_sorted):
    """int64[n, 33]: per interval the substitutions with start <= pos < end, by class."""
    out = np.zeros((len(start), 33), np.int64)
    lo = np.searchsorted(pos_sorted, np.asarray(start, np.int64), side="left")
    hi = np.searchsorted(pos_sorted, np.asarray(end, np.int64), side="left")
    for i in np.flatnonzero(hi > lo).tolist():
        out[i] = np.bincount(cls_sorted[lo[i]:hi[i]], minlength=33)
    return out


def derived(all_tri, ccs_tri, sbs_tri):
    """(sbs, sbs_uncallable, rate, burden) of one interval; rate / burden None without a denominator."""
    all_tri, ccs_tri, sbs_tri = ([int(x) for x in v] for v in (all_tri, ccs_tri, sbs_tri))
    sbs = sum(sbs_tri)
    uncallable = sbs_tri[OTHER] + sum(sbs_tri[c] for c in range(32) if ccs_tri[c] == 0)
    denom = sum(ccs_tri[:32])
    if denom == 0:
        return sbs, uncallable, None, None
    burden = 0.0
    for c in range(32):
        if ccs_tri[c] > 0:
            burden += sbs_tri[c] / ccs_tri[c] * all_tri[c]
    return sbs, uncallable, (sbs - uncallable) / denom, 2 * burden


def _na(x):
    return "NA" if x is None else repr(x)


def main_lines(intervals, rows, sbs_tri):
    """The main TSV: header, then one line per (chrom, start, end, name) with its row; ``sbs_tri`` None: no --sbs."""
    out = ["\t".join(HEADER) + "\n"]
    for k, ((chrom, s, e, name), r) in enumerate(zip(intervals, rows)):
        if sbs_tri is None:
            tail = ["NA"] * 4
        else:
            sbs, unc, rate, burden = derived(r["all_tri"], r["ccs_tri"], sbs_tri[k])
            tail = [str(sbs), str(unc), _na(rate), _na(burden)]
        out.append("\t".join([chrom, str(s), str(e), name, str(max(e - s, 0)), str(int(r["entries"])),
                              str(int(r["positions"][CALLABLE])), str(int(r["bases"][CALLABLE]))] + tail) + "\n")
    return out


def tri_lines(intervals, rows, sbs_tri):
    out = ["chrom\tstart\tend\tname\ttri\tall_tri\tref_tri\tccs_tri\tsbs\n"]
    for k, ((chrom, s, e, name), r) in enumerate(zip(intervals, rows)):
        for c, tri in enumerate(INTERVAL_TRI_NAMES):
            out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
                chrom, s, e, name, tri, int(r["all_tri"][c]), int(r["ref_tri"][c]), int(r["ccs_tri"][c]),
                "NA" if sbs_tri is None else int(sbs_tri[k][c])))
    return out


def state_lines(intervals, rows):
    out = ["chrom\tstart\tend\tname\tstate\tpositions\tbases\n"]
    for (chrom, s, e, name), r in zip(intervals, rows):
        for code, state in CALLABLE_STATES.items():
            if r["positions"][code]:
                out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(chrom, s, e, name, state, int(r["positions"][code]),
                                                                 int(r["bases"][code])))
    return out


def contig_rows(ctx, intervals):
    """The rows of [(chrom, start, end, name)] on the contig whose callable run ``ctx`` has just completed."""
    ctx.run_intervals(np.array([iv[1] for iv in intervals], np.int32), np.array([iv[2] for iv in intervals], np.int32))
    return ctx.intervals()


def dump_intervals(bam_file, ref_file, bed_file, bin_size, sbs_file, vcf_file, phased_vcf_file, common_snps, panel_of_normals,
                   region, region_list, min_qv, min_mapq, min_sequence_identity, min_gq, min_bq, min_trim, mismatch_window,
                   max_mismatch_count, min_ref_count, min_alt_count, min_hap_count, somatic_snv_prior, germline_snv_prior,
                   germline_indel_prior, threads, phase, non_human_sample, reference_sample, out_file, tri_file=None,
                   states_file=None, devices=(0,), log_path="intervals.log", cs_from_ref=False, genes_file=None, feature="gene",
                   strands_file=None):
    """Driver of `himut intervals`: callable.dump_callable with a step behind each contig's run that tallies the contig's
    intervals while its map is resident; then the TSV files.  A single process: under torch.distributed.run it raises.
    ``genes_file`` and ``strands_file`` (both or neither): the strand tally of every swept contig goes to ``strands_file``.
    Returns (intervals in output order, their rows, their substitutions by class or None)."""
    from . import dist
    from .callable import dump_callable
    dist.require_single_process("intervals", dist.DEVICES_HINT)
    if (bed_file is None) == (bin_size is None):
        raise ValueError("himut intervals takes exactly one of --bed and --bin_size")
    bed = read_bed(bed_file) if bed_file is not None else None
    int32 = np.iinfo(np.int32)
    if bed is not None and any(not (int32.min <= v <= int32.max) for iv in bed for v in iv[1:3]):
        raise ValueError("{}: a start or end outside 32 bits".format(bed_file))
    snvs = None
    if sbs_file is not None:
        from .mutlib import _snvs
        snvs = _snvs(sbs_file)
    if (genes_file is None) != (strands_file is None):
        raise ValueError("himut intervals takes --genes and --strands together")
    genes, strand_lines = None, {}
    if genes_file is not None:
        from . import strands
        genes, _unstranded = strands.read_genes(genes_file, feature)
    per_contig = {}                      # contig -> (indices into the output order or None, intervals, rows, sbs by class)

    def tally(chrom, worker, seq, length):
        if bed is None:
            idx, ivs = None, bin_intervals(chrom, length, bin_size)
        else:
            idx = [k for k, iv in enumerate(bed) if iv[0] == chrom]
            ivs = [bed[k] for k in idx]
        rows = contig_rows(worker.ctx, ivs)
        sbs_tri = None
        if snvs is not None:
            pos0, ref, _alt = snvs.get(chrom, ([], [], []))
            pos, cls = sbs_classes(chrom, seq, pos0, ref)
            sbs_tri = sbs_per_interval([iv[1] for iv in ivs], [iv[2] for iv in ivs], pos, cls)
        per_contig[chrom] = (idx, ivs, rows, sbs_tri)
        if genes is not None:
            strand_lines[chrom] = strands.contig_callable(worker.ctx, chrom, genes.get(chrom, []), length, seq,
                                                          None if snvs is None else snvs.get(chrom, ([], [], [])))

    runs, _log = dump_callable(
        bam_file, ref_file, sbs_file, vcf_file, phased_vcf_file, common_snps, panel_of_normals, region, region_list, min_qv,
        min_mapq, min_sequence_identity, min_gq, min_bq, min_trim, mismatch_window, max_mismatch_count, min_ref_count,
        min_alt_count, min_hap_count, somatic_snv_prior, germline_snv_prior, germline_indel_prior, threads, phase,
        non_human_sample, reference_sample, None, devices=devices, log_path=log_path, cs_from_ref=cs_from_ref,
        contig_hook=tally)
    chrom_lst = list(runs)               # the swept contigs in contig order
    if bed is None:
        order = [(chrom, k) for chrom in chrom_lst for k in range(len(per_contig[chrom][1]))]
    else:
        where = {}
        for chrom in chrom_lst:
            for k, i in enumerate(per_contig[chrom][0]):
                where[i] = (chrom, k)
        order = [where[i] for i in range(len(bed)) if i in where]
        print("himut intervals: {} of {} BED lines lie on contigs that are not swept and give no row".format(
            len(bed) - len(order), len(bed)))
    intervals = [per_contig[c][1][k] for c, k in order]
    rows = np.array([per_contig[c][2][k] for c, k in order], dtype=per_contig[order[0][0]][2].dtype) if order else []
    sbs_tri = None if snvs is None else [per_contig[c][3][k] for c, k in order]
    with open(out_file, "w") as o:
        o.writelines(main_lines(intervals, rows, sbs_tri))
    if tri_file is not None:
        with open(tri_file, "w") as o:
            o.writelines(tri_lines(intervals, rows, sbs_tri))
    if states_file is not None:
        with open(states_file, "w") as o:
            o.writelines(state_lines(intervals, rows))
    if strands_file is not None:
        with open(strands_file, "w") as o:
            o.write("chrom\tcategory\ttri\tcallable_pos\tcallable_bases{}\n".format("" if snvs is None else "\tsbs"))
            for chrom in chrom_lst:
                o.writelines(strand_lines[chrom])
    return intervals, rows, sbs_tri
