"""`himut sindels`: somatic insertion and deletion candidates carried by single reads.

The reference has no such command.  `call` gives single-base substitutions and `dbs` doublets; this run lists the third
COSMIC class (ID) from the same reads under `call`'s read filters: an allele that a proposing read shows away from its
trimmed ends, with no other mismatch in the window and every base of its footprint at ``--min_bq``, in a pile that
genotypes hom-ref.  The contract -- proposing reads, the per-event rules, candidates, the verdict cascade, the twenty
counters -- is DESIGN.md section 8 (Row 16) and include/himut_hip.h (himut_run_sindels).

The records are *candidates under stated rules*, not calls: HiFi indel error outside repeats is orders of magnitude above
a somatic indel rate, and inside homopolymers it is higher still.  himut_sindels.log keeps the counters a user needs to
subtract an expected error load (`himut indelcal` gives the rate).  ``--max_run`` (2), ``--indel_error`` (0.01) and the
footprint rule are definitions chosen here; repeats of units longer than one base are not recognised.
There is no CPU implementation: without the HIP library the call raises.
"""
from .caller import reads_for


def get_somatic_indels(chrom, bam_file, chrom_seq, chunkloci_lst, min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit,
                       min_sequence_identity, min_gq, min_bq, min_trim, mismatch_window_size, max_mismatch_count,
                       md_threshold, min_ref_count, min_alt_count, germline_indel_prior, indel_error, max_indel_len,
                       max_run, chrom2records, chrom2log, device=0, read_batch=None, resident_worker=None, error_logs=None):
    """One contig (the shape of indels.get_germline_indels).  chrom2records[chrom]: the integer records
    (vcflib.sindel_lines prints them), chrom2log[chrom]: the twenty counters.  ``error_logs``: (l_hit, l_err) of
    indelcal.error_logs, the table the genotype reads in place of ``indel_error`` (None: the context's table is cleared)."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    if chrom_seq is not None:
        from .bamio import set_contig_reference
        set_contig_reference(w.ctx, chrom_seq)
    w.ctx.set_chunks([(int(s), int(e)) for (_c, s, e) in chunkloci_lst])
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.set_indel_error_table(*(error_logs or ()))
    w.ctx.run_sindels(min_mapq=min_mapq, min_gq=min_gq, min_ref_count=min_ref_count, min_alt_count=min_alt_count,
                      md_threshold=md_threshold, max_len=max_indel_len, max_run=max_run, min_qv=min_qv,
                      indel_error=indel_error, germline_indel_prior=germline_indel_prior,
                      qlen_lower_limit=qlen_lower_limit, qlen_upper_limit=qlen_upper_limit, min_bq=min_bq,
                      mismatch_window_size=mismatch_window_size, max_mismatch_count=max_mismatch_count,
                      min_sequence_identity=min_sequence_identity, min_trim=min_trim)
    chrom2records[chrom], chrom2log[chrom] = w.ctx.sindels()


def call_somatic_indels(bam_file, ref_file, region, region_list, min_qv, min_mapq, min_sequence_identity, min_gq, min_bq,
                        min_trim, mismatch_window_size, max_mismatch_count, min_ref_count, min_alt_count,
                        germline_indel_prior, indel_error, max_indel_len, max_run, threads, version, out_file,
                        devices=(0,), cs_from_ref=False, log_path="himut_sindels.log", error_table=None, min_spans=1000):
    """Driver of `himut sindels`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``), the query-length limits and the depth threshold from the same samples `call` takes
    them from, the contig's string, the run; the VCF and himut_sindels.log.  ``cs_from_ref`` and ``error_table`` as in
    `himut indels`.  A single process: under torch.distributed.run it raises."""
    from . import vcflib
    from .feed import SampledRun
    run = SampledRun("sindels")
    if not out_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    error_logs = None
    if error_table is not None:
        from . import indelcal
        error_logs = indelcal.error_logs(indelcal.load_table(error_table), indel_error, min_spans)
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2records, chrom2log = {}, {}

    def per_contig(chrom, dev, worker, thresholds, chrom_seq):
        get_somatic_indels(chrom, bam_file, chrom_seq, feed.chrom2chunkloci_lst[chrom], min_qv, min_mapq, thresholds[0],
                           thresholds[1], min_sequence_identity, min_gq, min_bq, min_trim, mismatch_window_size,
                           max_mismatch_count, thresholds[2], min_ref_count, min_alt_count, germline_indel_prior,
                           indel_error, max_indel_len, max_run, chrom2records, chrom2log, device=dev,
                           resident_worker=worker, error_logs=error_logs)

    qlen_lower_limit, qlen_upper_limit, md_threshold = run.each(per_contig, ref_file, cs_from_ref, contig_strings=True)
    header = vcflib.get_sindels_vcf_header(bam_file, region, region_list, feed.tname2tsize, min_qv, min_mapq,
                                           qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq,
                                           min_trim, max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count,
                                           min_alt_count, germline_indel_prior, indel_error, max_indel_len, max_run,
                                           threads, version, out_file, feed.bam.sample(), ref_file=ref_file,
                                           cs_from_ref=cs_from_ref, error_table=error_table, min_spans=min_spans)
    vcflib.dump_vcf(out_file, header, feed.chrom_lst,
                    lambda chrom: vcflib.sindel_lines(chrom, chrom2records[chrom], run.refseq[chrom]))
    vcflib.dump_counter_log(vcflib.SINDEL_LOG_ROWS, feed.chrom_lst, chrom2log, log_path)
    run.done("himut somatic indel candidate detection")
    return chrom2records, chrom2log
