"""`himut germline`: the sample's germline SNVs from the call path's pile.

The reference has no such command: `phase --vcf`, `call --phase` (through phase's output) and `call
--non_human_sample` (vcflib.get_germline_priors) take a germline VCF that an external caller made from the same BAM.
The call path already builds the pile the reference genotypes (caller.py:299-305) and its genotyper is
gtlib.get_germ_gt bit for bit; this run keeps the columns `call` throws away as germline.  The contract -- pile,
candidate positions, FILTER cascade, counters -- is DESIGN.md section 8 and include/himut_hip.h (himut_run_germline).
There is no CPU implementation: without the HIP library the call raises.
"""
from .caller import reads_for


def get_germline_snvs(chrom, bam_file, chunkloci_lst, min_mapq, min_gq, min_bq, min_ref_count, min_alt_count, md_threshold,
                      germline_snv_prior, chrom2records, chrom2log, device=0, read_batch=None, resident_worker=None):
    """One contig (the shape of caller.get_somatic_substitutions): its reads from ``read_batch``, from ``bam_file``
    with the package's BAM reader, or already in HBM under ``resident_worker``.  chrom2records[chrom]: the integer
    records (vcflib.germline_lines prints them), chrom2log[chrom]: the twelve counters."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    w.set_prior(germline_snv_prior)
    w.ctx.set_chunks([(int(s), int(e)) for (_c, s, e) in chunkloci_lst])
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.run_germline(min_mapq=min_mapq, min_gq=min_gq, min_bq=min_bq, min_ref_count=min_ref_count,
                       min_alt_count=min_alt_count, md_threshold=md_threshold)
    chrom2records[chrom], chrom2log[chrom] = w.ctx.germline()


def call_germline_snvs(bam_file, region, region_list, min_mapq, min_gq, min_bq, min_ref_count, min_alt_count,
                       germline_snv_prior, threads, version, out_file, devices=(0,), ref_file=None, cs_from_ref=False,
                       log_path="himut_germline.log"):
    """Driver of `himut germline`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``), the depth threshold from the same samples `call` takes it from, the VCF and
    himut_germline.log.  ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from CIGAR, SEQ and
    ``ref_file``.  A single process: under torch.distributed.run it raises."""
    from . import vcflib
    from .feed import SampledRun
    run = SampledRun("germline")
    if not out_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2records, chrom2log = {}, {}

    def per_contig(chrom, dev, worker, thresholds, _seq):
        get_germline_snvs(chrom, bam_file, feed.chrom2chunkloci_lst[chrom], min_mapq, min_gq, min_bq, min_ref_count,
                          min_alt_count, thresholds[2], germline_snv_prior, chrom2records, chrom2log, device=dev,
                          resident_worker=worker)

    _lo, _hi, md_threshold = run.each(per_contig, ref_file, cs_from_ref)
    header = vcflib.get_germline_vcf_header(bam_file, region, region_list, feed.tname2tsize, min_mapq, min_gq, min_bq,
                                            min_ref_count, min_alt_count, md_threshold, germline_snv_prior, threads,
                                            version, out_file, feed.bam.sample(), ref_file=ref_file,
                                            cs_from_ref=cs_from_ref)
    vcflib.dump_vcf(out_file, header, feed.chrom_lst, lambda chrom: vcflib.germline_lines(chrom, chrom2records[chrom]))
    vcflib.dump_counter_log(vcflib.GERMLINE_LOG_ROWS, feed.chrom_lst, chrom2log, log_path)
    run.done("himut germline SNV detection")
    return chrom2records, chrom2log
