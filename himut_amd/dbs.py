"""`himut dbs`: somatic doublet base substitutions (CC>TT and the like) from the call path's pile.

`himut call` cannot report one: a read that carries a doublet proposes two single-base candidates, each inside the
other's mismatch window, and with the default ``max_mismatch_count 0`` bamlib.is_mismatch_conflict removes both.  The
reference has a half-written ``tdbs_lst`` branch (cslib.cs2mut) that `call` never reaches, and its panel of normals is
named ``...sbs.dbs.vcf.bgz``.  This run proposes doublets from the reads' mismatch lists, evaluates both columns with
`call`'s cascade and joins the verdicts.  The contract -- proposals, halves, joint counts, verdict, counters -- is
DESIGN.md section 8 (row 10) and include/himut_hip.h (himut_run_dbs).  There is no CPU implementation: without the HIP
library the call raises.
"""
from .caller import reads_for, site_sets


def get_doublet_substitutions(chrom, bam_file, common_snps, panel_of_normals, chunkloci_lst, min_qv, min_mapq,
                              qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                              max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count, min_alt_count,
                              germline_snv_prior, chrom2records, chrom2log, device=0, read_batch=None, resident_worker=None):
    """One contig (the shape of caller.get_somatic_substitutions): its reads from ``read_batch``, from ``bam_file``
    with the package's BAM reader, or already in HBM under ``resident_worker``.  chrom2records[chrom]: the integer
    records (vcflib.dbs_lines prints them), chrom2log[chrom]: the twenty counters."""
    pon_keys, com_keys = site_sets(chrom, common_snps, panel_of_normals)
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    w.configure(min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count, min_alt_count, 0,
                germline_snv_prior, False)
    w.load([(int(s), int(e)) for (_c, s, e) in chunkloci_lst], pon_keys, com_keys, None, read_batch)
    w.ctx.run_dbs()
    chrom2records[chrom], chrom2log[chrom] = w.ctx.dbs()


def call_doublet_substitutions(bam_file, common_snps, panel_of_normals, region, region_list, min_qv, min_mapq,
                               min_sequence_identity, min_gq, min_bq, min_trim, max_mismatch_count, mismatch_window_size,
                               min_ref_count, min_alt_count, germline_snv_prior, threads, version, out_file, devices=(0,),
                               ref_file=None, cs_from_ref=False, log_path="himut_dbs.log"):
    """Driver of `himut dbs`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``), the query-length limits and the depth threshold from the same samples `call` takes
    them from, the VCF and himut_dbs.log.  ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from
    CIGAR, SEQ and ``ref_file``.  A single process: under torch.distributed.run it raises."""
    from . import vcflib
    from .feed import SampledRun
    run = SampledRun("dbs")
    if not out_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2records, chrom2log = {}, {}

    def per_contig(chrom, dev, worker, thresholds, _seq):
        get_doublet_substitutions(chrom, bam_file, common_snps, panel_of_normals, feed.chrom2chunkloci_lst[chrom], min_qv,
                                  min_mapq, thresholds[0], thresholds[1], min_sequence_identity, min_gq, min_bq, min_trim,
                                  max_mismatch_count, mismatch_window_size, thresholds[2], min_ref_count, min_alt_count,
                                  germline_snv_prior, chrom2records, chrom2log, device=dev, resident_worker=worker)

    qlen_lower_limit, qlen_upper_limit, md_threshold = run.each(per_contig, ref_file, cs_from_ref)
    header = vcflib.get_dbs_vcf_header(bam_file, region, region_list, feed.tname2tsize, common_snps, panel_of_normals, min_qv,
                                       min_mapq, qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq,
                                       min_trim, max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count,
                                       min_alt_count, germline_snv_prior, threads, version, out_file, feed.bam.sample(),
                                       ref_file=ref_file, cs_from_ref=cs_from_ref)
    vcflib.dump_vcf(out_file, header, feed.chrom_lst, lambda chrom: vcflib.dbs_lines(chrom, chrom2records[chrom]))
    vcflib.dump_counter_log(vcflib.DBS_LOG_ROWS, feed.chrom_lst, chrom2log, log_path)
    run.done("himut doublet base substitution detection")
    return chrom2records, chrom2log
