"""`himut indelcal`: the empirical indel error of the reads per homopolymer run of the reference.

`himut indels` genotypes every allele with one per-read error, ``--indel_error``; HiFi indel error is small outside
repeats and grows by orders of magnitude with the length of a homopolymer run.  This run measures it on the BAM at hand,
as `bqcal` measures what a reported base quality is worth: for every run of one letter in the regions -- a single base
between two others is a run of one -- the pile reads that span it and the insertions and deletions they show in it, per
class of run (letter, length; lengths 32 to 64 share a bin) and kind of event (a deletion or an insertion of the run's own
letter by length 1, 2, 3 and more; anything else).  Runs at anchors that look like germline variants are set aside and
counted (``excluded``).  `himut indels --error_table` reads the table back.  The contract -- runs, variant anchors,
spans, the four event rules, counters -- is DESIGN.md section 8 (Row 13) and include/himut_hip.h (himut_run_indelcal).
There is no CPU implementation: without the HIP library the call raises.
"""
import math

import numpy as np

from ._ffi import INDEL_ERROR_CELLS, INDELCAL_CLASSES, INDELCAL_COLUMNS, INDELCAL_EVENT_COLUMNS, INDELCAL_LOG_NAMES
from .caller import reads_for

BASES = "ATGC"                                   # the code order of the classes
HEADER = "base\trun\t" + "\t".join(INDELCAL_COLUMNS) + "\tdel_rate\tins_rate\n"
LOG_ROWS = ["num_" + k if not k.startswith("num_") else k for k in INDELCAL_LOG_NAMES]
MAX_ERROR = 0.25                                 # an estimate above this is capped: a het allele is seen in half of the reads


def vaf_permille(germline_vaf):
    """--germline_vaf as the integer the device compares with: n_alt * 1000 >= vaf_permille * DP."""
    v = int(round(float(germline_vaf) * 1000))
    if not 0 <= v <= 1000:
        raise ValueError("germline_vaf must lie in [0, 1]")
    return v


def get_indel_counts(chrom, bam_file, chrom_seq, chunkloci_lst, min_mapq, min_alt_count, germline_vaf, max_indel_len,
                     chrom2table, chrom2log, device=0, read_batch=None, resident_worker=None):
    """One contig (the shape of bqcal.get_bq_counts): its reads from ``read_batch``, from ``bam_file`` with the package's
    BAM reader, or already in HBM under ``resident_worker``.  ``chrom_seq``: the contig's string as the FASTA spells it,
    or None when the worker's context holds it already.  chrom2table[chrom]: int64[128, 10]; chrom2log[chrom]: the
    fourteen counters."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    if chrom_seq is not None:
        from .bamio import set_contig_reference
        set_contig_reference(w.ctx, chrom_seq)
    w.ctx.set_chunks([(int(s), int(e)) for (_c, s, e) in chunkloci_lst])
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.run_indelcal(min_mapq=min_mapq, max_len=max_indel_len, min_alt_count=min_alt_count,
                       vaf_permille=vaf_permille(germline_vaf))
    chrom2table[chrom], chrom2log[chrom] = w.ctx.indelcal()


def table_lines(table):
    """The TSV: the header, then the 128 classes in class order -- base, run length (``32+`` for the last bin), the ten
    integers, and del_rate and ins_rate: the deletions and the insertions of the run's letter per spanning read, printed
    with repr, NA without spans."""
    out = [HEADER]
    for c in range(INDELCAL_CLASSES):
        row = [int(x) for x in table[c]]
        n = c % 32 + 1
        spans = row[2]
        rates = [repr(sum(row[k:k + 3]) / spans) if spans else "NA" for k in (3, 6)]
        out.append("\t".join([BASES[c // 32], "32+" if n == 32 else str(n)] + [str(x) for x in row] + rates) + "\n")
    return out


def load_table(path):
    """The integer columns of an indelcal TSV as int64[128, 10]; the rates are not read."""
    table = np.zeros((INDELCAL_CLASSES, len(INDELCAL_COLUMNS)), np.int64)
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or lines[0] + "\n" != HEADER or len(lines) != 1 + INDELCAL_CLASSES:
        raise ValueError("{}: not an indelcal table (a header and {} rows)".format(path, INDELCAL_CLASSES))
    for c, line in enumerate(lines[1:]):
        cells = line.split("\t")
        n = c % 32 + 1
        if len(cells) != 14 or cells[0] != BASES[c // 32] or cells[1] != ("32+" if n == 32 else str(n)):
            raise ValueError("{}: row {} is not class {}".format(path, c + 2, c))
        table[c] = [int(x) for x in cells[2:12]]
    if (table < 0).any():
        raise ValueError("{}: negative count".format(path))
    return table


def error_logs(table, indel_error, min_spans=1000):
    """(l_hit[896], l_err[896]) for Context.set_indel_error_table: per class and event column e = min((count + 1) /
    (spans + 2), 0.25), ``indel_error`` for a class with fewer than ``min_spans`` spans; log10(1 - e) and log10(e) with
    math.log10 (the GtLut precedent)."""
    l_hit, l_err = np.zeros(INDEL_ERROR_CELLS, np.float64), np.zeros(INDEL_ERROR_CELLS, np.float64)
    for c in range(INDELCAL_CLASSES):
        spans = int(table[c][2])
        for k in range(INDELCAL_EVENT_COLUMNS):
            e = float(indel_error)
            if spans >= min_spans:
                e = min((int(table[c][3 + k]) + 1) / (spans + 2), MAX_ERROR)
            l_hit[c * INDELCAL_EVENT_COLUMNS + k] = math.log10(1 - e)
            l_err[c * INDELCAL_EVENT_COLUMNS + k] = math.log10(e)
    return l_hit, l_err


def dump_indel_error(bam_file, ref_file, region, region_list, min_mapq, min_alt_count, germline_vaf, max_indel_len,
                     threads, out_file, devices=(0,), cs_from_ref=False, log_path="himut_indelcal.log"):
    """Driver of `himut indelcal`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``), the contig's string, the run; the tables summed over the contigs, the TSV and
    himut_indelcal.log.  ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from CIGAR, SEQ and
    ``ref_file``.  A single process: under torch.distributed.run it raises.  Returns (table[128, 10], contig -> counters)."""
    from . import vcflib
    from .feed import SampledRun
    run = SampledRun("indelcal")
    vaf_permille(germline_vaf)
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2table, chrom2log = {}, {}

    def per_contig(chrom, dev, worker, thresholds, chrom_seq):
        get_indel_counts(chrom, bam_file, chrom_seq, feed.chrom2chunkloci_lst[chrom], min_mapq, min_alt_count, germline_vaf,
                         max_indel_len, chrom2table, chrom2log, device=dev, resident_worker=worker)

    run.each(per_contig, ref_file, cs_from_ref, contig_strings=True)
    table = np.zeros((INDELCAL_CLASSES, len(INDELCAL_COLUMNS)), np.int64)
    for chrom in feed.chrom_lst:
        table += chrom2table[chrom]
    with open(out_file, "w") as o:
        o.writelines(table_lines(table))
    vcflib.dump_counter_log(LOG_ROWS, feed.chrom_lst, chrom2log, log_path)
    run.done("himut indelcal")
    return table, chrom2log
