"""`himut germline`: the sample's germline SNVs from the call path's pile.

The reference has no such command: `phase --vcf`, `call --phase` (through phase's output) and `call
--non_human_sample` (vcflib.get_germline_priors) take a germline VCF that an external caller made from the same BAM.
The call path already builds the pile the reference genotypes (caller.py:299-305) and its genotyper is
gtlib.get_germ_gt bit for bit; this run keeps the columns `call` throws away as germline.  The contract -- pile,
candidate positions, FILTER cascade, counters -- is DESIGN.md section 8 and include/himut_hip.h (himut_run_germline).
There is no CPU implementation: without the HIP library the call raises.
"""
import os

from . import gtlib
from .caller import Worker


def get_germline_snvs(chrom, bam_file, chunkloci_lst, min_mapq, min_gq, min_bq, min_ref_count, min_alt_count, md_threshold,
                      germline_snv_prior, chrom2records, chrom2log, device=0, read_batch=None, resident_worker=None):
    """One contig (the shape of caller.get_somatic_substitutions): its reads from ``read_batch``, from ``bam_file``
    with the package's BAM reader, or already in HBM under ``resident_worker``.  chrom2records[chrom]: the integer
    records (vcflib.germline_lines prints them), chrom2log[chrom]: the twelve counters."""
    w = resident_worker
    if w is None:
        from .caller import _worker_for
        w = _worker_for(device)
        if read_batch is None:
            from . import bamio
            read_batch = bamio.read_contig(bam_file, chrom)
    if w._lut_prior != germline_snv_prior:
        w.ctx.set_gt_lut(*gtlib.build_tables(germline_snv_prior))
        w._lut_prior = germline_snv_prior
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
    import time
    from . import bamio, bamlib, dist, util, vcflib
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("himut germline runs as a single process: start it without torch.distributed.run "
                           "(WORLD_SIZE={}); --devices spreads the contigs over GPUs".format(os.environ["WORLD_SIZE"]))
    if not out_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    t0 = time.time()
    bam = bamio.BamStream(bam_file, threads if threads and threads > 1 else 0)
    tname2tsize = bam.tname2tsize
    chrom_lst, chrom2chunkloci_lst = util.load_loci(region, region_list, tname2tsize)
    sizes = {c: tname2tsize[c] for c in chrom_lst}
    devices = list(devices) or [0]
    share = [(c, d) for d, contigs in zip(devices, dist.lpt_assign(sizes, len(devices))) for c in contigs]
    starts = bamlib.sample_starts(chrom_lst, tname2tsize)
    refseq = bamio.reference_for_cs(ref_file, chrom_lst, tname2tsize, bam_file) if cs_from_ref else None
    resident, samples = {}, {}
    try:
        for chrom, dev in share:
            w = Worker(dev)
            resident[chrom] = w
            if cs_from_ref:
                bamio.set_contig_reference(w.ctx, refseq[chrom])
            res = bam.ingest_contig(w.ctx, chrom, derive_cs=cs_from_ref)
            ts, te, ql_, mq_, tp_ = w.ctx.ingest_read_meta(res["n_reads"])
            samples[chrom] = bamlib.sample_qlens(ts, te, ql_, mq_, tp_, starts[chrom])
        _lo, _hi, md_threshold = bamlib.thresholds_from_samples(samples, chrom_lst)
        chrom2records, chrom2log = {}, {}
        for chrom, dev in share:
            get_germline_snvs(chrom, bam_file, chrom2chunkloci_lst[chrom], min_mapq, min_gq, min_bq, min_ref_count,
                              min_alt_count, md_threshold, germline_snv_prior, chrom2records, chrom2log, device=dev,
                              resident_worker=resident[chrom])
            resident.pop(chrom).close()        # the contig's reads leave HBM
    finally:
        for w in resident.values():
            w.close()
    header = vcflib.get_germline_vcf_header(bam_file, region, region_list, tname2tsize, min_mapq, min_gq, min_bq,
                                            min_ref_count, min_alt_count, md_threshold, germline_snv_prior, threads,
                                            version, out_file, bam.sample(), ref_file=ref_file, cs_from_ref=cs_from_ref)
    vcflib.dump_germline_records(out_file, header, chrom_lst, chrom2records)
    vcflib.dump_germline_log(chrom_lst, chrom2log, path=log_path)
    print("himut germline SNV detection took {} minutes".format((time.time() - t0) / 60))
    return chrom2records, chrom2log
