"""`himut indels`: the sample's germline short insertions and deletions from the decoded reads.

The reference has no such command: in `call` an indel only vetoes a site (IndelSite), the pile keeps no length or
sequence of one, and ``--germline_indel_prior`` is parsed and never read.  Everything an indel caller needs is in HBM
behind the cs decode -- the reads' segments, SEQ, the reference string -- so this run is the decode plus three small
kernels: no capture, no column store.  The contract -- pile reads, events, the left shift, alleles, the three-state
genotype, FILTER cascade, counters -- is DESIGN.md section 8 (Row 12) and include/himut_hip.h (himut_run_indels).
``--indel_error`` (0.01) is one constant, a definition chosen here; HiFi indel error grows by orders of magnitude with the
length of a homopolymer run, and `himut indelcal` (indelcal.py, Row 13) measures it on the BAM at hand: under
``--error_table`` an allele in a run is genotyped with the error of its row of that table, the constant elsewhere.
There is no CPU implementation: without the HIP library the call raises.
"""
from .caller import reads_for


def get_germline_indels(chrom, bam_file, chrom_seq, chunkloci_lst, min_mapq, min_gq, min_ref_count, min_alt_count,
                        md_threshold, germline_indel_prior, indel_error, max_indel_len, chrom2records, chrom2log, device=0,
                        read_batch=None, resident_worker=None, error_logs=None):
    """One contig (the shape of germline.get_germline_snvs): its reads from ``read_batch``, from ``bam_file`` with the
    package's BAM reader, or already in HBM under ``resident_worker``.  ``chrom_seq``: the contig's string as the FASTA
    spells it, or None when the worker's context holds it already.  chrom2records[chrom]: the integer records
    (vcflib.indel_lines prints them), chrom2log[chrom]: the thirteen counters.  ``error_logs``: (l_hit, l_err) of
    indelcal.error_logs, the table the run reads in place of ``indel_error`` (None: the context's table is cleared)."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    if chrom_seq is not None:
        from .bamio import set_contig_reference
        set_contig_reference(w.ctx, chrom_seq)
    w.ctx.set_chunks([(int(s), int(e)) for (_c, s, e) in chunkloci_lst])
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.set_indel_error_table(*(error_logs or ()))
    w.ctx.run_indels(min_mapq=min_mapq, min_gq=min_gq, min_ref_count=min_ref_count, min_alt_count=min_alt_count,
                     md_threshold=md_threshold, max_len=max_indel_len, indel_error=indel_error,
                     germline_indel_prior=germline_indel_prior)
    chrom2records[chrom], chrom2log[chrom] = w.ctx.indels()


def call_germline_indels(bam_file, ref_file, region, region_list, min_mapq, min_gq, min_ref_count, min_alt_count,
                         germline_indel_prior, indel_error, max_indel_len, threads, version, out_file, devices=(0,),
                         cs_from_ref=False, log_path="himut_indels.log", error_table=None, min_spans=1000):
    """Driver of `himut indels`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``), the depth threshold from the same samples `call` takes it from, the contig's string,
    the run; the VCF and himut_indels.log.  ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from
    CIGAR, SEQ and ``ref_file``.  ``error_table``: the TSV of `himut indelcal` the genotype takes its per-read error
    from, rows with fewer than ``min_spans`` spanning reads aside.  A single process: under torch.distributed.run it
    raises."""
    from . import vcflib
    from .feed import SampledRun
    run = SampledRun("indels")
    if not out_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    error_logs = None
    if error_table is not None:
        from . import indelcal
        error_logs = indelcal.error_logs(indelcal.load_table(error_table), indel_error, min_spans)
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2records, chrom2log = {}, {}

    def per_contig(chrom, dev, worker, thresholds, chrom_seq):
        get_germline_indels(chrom, bam_file, chrom_seq, feed.chrom2chunkloci_lst[chrom], min_mapq, min_gq, min_ref_count,
                            min_alt_count, thresholds[2], germline_indel_prior, indel_error, max_indel_len, chrom2records,
                            chrom2log, device=dev, resident_worker=worker, error_logs=error_logs)

    _lo, _hi, md_threshold = run.each(per_contig, ref_file, cs_from_ref, contig_strings=True)
    header = vcflib.get_indels_vcf_header(bam_file, region, region_list, feed.tname2tsize, min_mapq, min_gq, min_ref_count,
                                          min_alt_count, md_threshold, germline_indel_prior, indel_error, max_indel_len,
                                          threads, version, out_file, feed.bam.sample(), ref_file=ref_file,
                                          cs_from_ref=cs_from_ref, error_table=error_table, min_spans=min_spans)
    vcflib.dump_vcf(out_file, header, feed.chrom_lst,
                    lambda chrom: vcflib.indel_lines(chrom, chrom2records[chrom], run.refseq[chrom]))
    vcflib.dump_counter_log(vcflib.INDEL_LOG_ROWS, feed.chrom_lst, chrom2log, log_path)
    run.done("himut germline indel detection")
    return chrom2records, chrom2log
