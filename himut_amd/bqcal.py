"""`himut bqcal`: the empirical base quality of every reported base quality.

himut rests on a CCS base of high reported quality being nearly always right (--min_bq 93, the genotyper's
10^(-BQ/10)); whether that holds depends on the instrument and the basecaller.  The reference's authors checked it with a
script outside the package (scripts/ccs2bq_calculation.py): every position genotyped, and at the confidently genotyped
ones the pile's bases counted per reported quality, as matches where they agree with the genotype and as mismatches where
they do not.  This run makes that table from the reads, the reference string and the genotyper the package holds
anyway.  The contract -- pile, positions swept, the five steps, counters -- is DESIGN.md section 8 (Row 8) and
include/himut_hip.h (himut_run_bqcal).  There is no CPU implementation: without the HIP library the call raises.
"""
import math

import numpy as np

from .caller import reads_for

HEADER = "bq\tmismatch\tmatch\tpq\n"


def get_bq_counts(chrom, bam_file, chrom_seq, chunkloci_lst, min_mapq, min_gq, md_threshold, germline_snv_prior,
                  chrom2match, chrom2mismatch, chrom2log, device=0, read_batch=None, resident_worker=None):
    """One contig (the shape of germline.get_germline_snvs): its reads from ``read_batch``, from ``bam_file`` with the
    package's BAM reader, or already in HBM under ``resident_worker``.  ``chrom_seq``: the contig's string as the FASTA
    spells it, or None when the worker's context holds it already.  chrom2match[chrom], chrom2mismatch[chrom]: 256
    counts indexed by BQ; chrom2log[chrom]: the twelve counters."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    w.set_prior(germline_snv_prior)
    if chrom_seq is not None:
        from .bamio import set_contig_reference
        set_contig_reference(w.ctx, chrom_seq)
    w.ctx.set_chunks([(int(s), int(e)) for (_c, s, e) in chunkloci_lst])
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.run_bqcal(min_mapq=min_mapq, min_gq=min_gq, md_threshold=md_threshold)
    chrom2match[chrom], chrom2mismatch[chrom], chrom2log[chrom] = w.ctx.bqcal()


def table_lines(match, mismatch):
    """The script's table: the header, the rows of BQ 1 .. 93 whatever they count, then a row for every BQ above 93 that
    counts anything (the script would have died on such a value).  pq as the script divides and formats it, NA when
    either count is 0."""
    out = [HEADER]
    for bq in range(1, 256):
        match_count, mismatch_count = int(match[bq]), int(mismatch[bq])
        if bq > 93 and match_count == 0 and mismatch_count == 0:
            continue
        if match_count != 0 and mismatch_count != 0:
            pq = -10 * math.log10(mismatch_count / float(match_count))
            out.append("{}\t{}\t{}\t{}\n".format(bq, mismatch_count, match_count, pq))
        else:
            out.append("{}\t{}\t{}\t{}\n".format(bq, mismatch_count, match_count, "NA"))
    return out


def dump_empirical_bq(bam_file, ref_file, region, region_list, min_mapq, min_gq, germline_snv_prior, threads, out_file,
                      devices=(0,), cs_from_ref=False):
    """Driver of `himut bqcal`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``), the depth threshold from the same samples `call` takes it from (the script takes
    its own from bamlib.get_thresholds), the contig's string, the sweep; the counts summed over the contigs and the
    table.  ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from CIGAR, SEQ and ``ref_file``.  A
    single process: under torch.distributed.run it raises.  Returns (match[256], mismatch[256], contig -> counters)."""
    from .feed import SampledRun
    run = SampledRun("bqcal")
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2match, chrom2mismatch, chrom2log = {}, {}, {}

    def per_contig(chrom, dev, worker, thresholds, chrom_seq):
        get_bq_counts(chrom, bam_file, chrom_seq, feed.chrom2chunkloci_lst[chrom], min_mapq, min_gq, thresholds[2],
                      germline_snv_prior, chrom2match, chrom2mismatch, chrom2log, device=dev, resident_worker=worker)

    run.each(per_contig, ref_file, cs_from_ref, contig_strings=True)
    match, mismatch = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for chrom in feed.chrom_lst:
        match += chrom2match[chrom]
        mismatch += chrom2mismatch[chrom]
    with open(out_file, "w") as o:
        o.writelines(table_lines(match, mismatch))
    run.done("himut bqcal")
    return match, mismatch, chrom2log
