"""`himut duplex`: substitutions that both strands of one molecule show.

`ccs --by-strand` writes two reads per molecule, ``<movie>/<zmw>/ccs/fwd`` and ``<movie>/<zmw>/ccs/rev``, one per DNA
strand.  A mutation sits on both; polymerase error, deamination and 8-oxoG damage sit on one.  `himut call` takes every
alignment as a molecule of its own: on such a BAM it counts the two strands as two supporting reads and neither asks
them to agree nor sees them disagree.  This run pairs the two reads of a molecule on the host (mate_index) and asks on
the device, for every substitution a read shows under call's read and event rules, what its mate shows at the same
reference position; the substitutions both show are genotyped on the pile with call's cascade, the ones only one shows
are tallied by the change on that strand, and the positions both strands cover well enough to have shown a mutation
are counted.  The contract -- pairs in play, a read's own rules, the mate's state, double-strand events, candidates, the
record, the spectrum, the denominator, the forty counters -- is DESIGN.md section 8 (row 19) and include/himut_hip.h
(himut_run_duplex).  There is no CPU implementation: without the HIP library the call raises.

Pairing is per contig: a molecule whose strands align to different contigs is two lone reads.  Indels on both strands,
the trinucleotide context of the denominator and a burden are not part of this run.
"""
import numpy as np

from .caller import reads_for, site_sets

SUFFIXES = ("/fwd", "/rev")
HOST_LOG_ROWS = ["num_reads_paired", "num_reads_unsuffixed", "num_reads_not_primary", "num_reads_single", "num_reads_ambiguous"]
LOG_ROWS = HOST_LOG_ROWS + ["num_reads", "num_pile_reads", "num_proposing_reads", "num_pairs", "num_pairs_in_play",
                            "num_pairs_notpile", "num_pairs_identity", "num_pairs_lowqv", "num_pairs_qlen", "num_events",
                            "num_trim", "num_window", "num_lowbq", "num_mate_nocover", "num_mate_del", "num_mate_lowbq",
                            "num_mate_trim", "num_concordant", "num_single", "num_mate_other", "num_mate_window",
                            "num_ds_events", "num_ds_events_in_chunk", "num_ss_events_in_chunk", "num_ds_bases",
                            "num_ds_pairs_overlap", "num_candidates", "num_Germline", "num_HetSite", "num_HetAltSite",
                            "num_HomAltSite", "num_IndelSite", "num_LowGQ", "num_LowBQ", "num_PanelOfNormal", "num_ComSnp",
                            "num_LowDepth", "num_HighDepth", "num_PASS", "reserved"]


def pair_reads(names, flag):
    """(mate, counts): ``mate[i]`` the partner of read i in this contig's batch or -1, and how the reads fared in the
    order of HOST_LOG_ROWS.  A name ending in /fwd or /rev has the stem in front of that suffix; only primary
    alignments take part (flags 0x100 and 0x800 clear); a stem pairs iff the batch holds exactly one primary /fwd and
    exactly one primary /rev alignment of it.  Every other read gets -1 and is counted once: no suffix (whatever its
    flags), not primary, more than one primary of a strand under its stem (ambiguous), or the other strand absent
    (single)."""
    n = len(names)
    mate = np.full(n, -1, np.int32)
    counts = dict.fromkeys(HOST_LOG_ROWS, 0)
    stems = {}
    for i, q in enumerate(names):
        if not q.endswith(SUFFIXES):
            counts["num_reads_unsuffixed"] += 1
        elif int(flag[i]) & 0x900:
            counts["num_reads_not_primary"] += 1
        else:
            stems.setdefault(q[:-4], ([], []))[q.endswith("/rev")].append(i)
    for fwd, rev in stems.values():
        if len(fwd) > 1 or len(rev) > 1:
            counts["num_reads_ambiguous"] += len(fwd) + len(rev)
        elif not fwd or not rev:
            counts["num_reads_single"] += 1
        else:
            mate[fwd[0]], mate[rev[0]] = rev[0], fwd[0]
            counts["num_reads_paired"] += 2
    return mate, [counts[k] for k in HOST_LOG_ROWS]


def mate_index(names, flag, mapq=None):
    """int32[n]: pair_reads' mate array.  ``mapq`` is not read: a mapping quality does not unpair a molecule here, the
    device's pile rule weighs it and counts the pair under pairs_notpile."""
    return pair_reads(names, flag)[0]


def ss_lines(ss, log):
    """The lines of the --ss table for the summed spectrum and counters: a header, the twelve classes in the order
    A>C .. T>G (the change on the read's own strand), then ds_bases and ds_pairs_overlap."""
    from ._ffi import DUPLEX_LOG_NAMES, DUPLEX_SS_CLASSES
    out = ["class\tcount\n"] + ["{}\t{}\n".format(c, int(x)) for c, x in zip(DUPLEX_SS_CLASSES, ss)]
    return out + ["{}\t{}\n".format(k, int(log[DUPLEX_LOG_NAMES.index(k)])) for k in ("ds_bases", "ds_pairs_overlap")]


def get_duplex_substitutions(chrom, bam_file, mate, common_snps, panel_of_normals, chunkloci_lst, min_qv, min_mapq,
                             qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                             max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count, min_alt_count,
                             germline_snv_prior, chrom2records, chrom2ss, chrom2log, device=0, read_batch=None,
                             resident_worker=None):
    """One contig (the shape of dbs.get_doublet_substitutions): its reads from ``read_batch``, from ``bam_file`` with the
    package's BAM reader, or already in HBM under ``resident_worker``; ``mate``: mate_index of the contig's reads (None:
    from ``read_batch``'s names).  chrom2records[chrom]: the integer records (vcflib.duplex_lines prints them),
    chrom2ss[chrom]: the twelve classes, chrom2log[chrom]: the forty counters."""
    pon_keys, com_keys = site_sets(chrom, common_snps, panel_of_normals)
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    if mate is None:
        mate = mate_index([read_batch.query_name(i) for i in range(read_batch.n)], read_batch.flag, read_batch.mapq)
    w.configure(min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count, min_alt_count, 0,
                germline_snv_prior, False)
    w.load([(int(s), int(e)) for (_c, s, e) in chunkloci_lst], pon_keys, com_keys, None, read_batch)
    w.ctx.run_duplex(mate)
    chrom2records[chrom], chrom2ss[chrom], chrom2log[chrom] = w.ctx.duplex()


def call_duplex_substitutions(bam_file, common_snps, panel_of_normals, region, region_list, min_qv, min_mapq,
                              min_sequence_identity, min_gq, min_bq, min_trim, max_mismatch_count, mismatch_window_size,
                              min_ref_count, min_alt_count, germline_snv_prior, threads, version, out_file, ss_file=None,
                              devices=(0,), ref_file=None, cs_from_ref=False, log_path="himut_duplex.log"):
    """Driver of `himut duplex`: every target contig through the device-side ingest (one resident context per contig,
    contigs spread over ``devices``) with the reads' names kept long enough to pair them, the query-length limits and
    the depth threshold from the same samples `call` takes them from, the run; the VCF, with ``ss_file`` the spectrum of
    the single-strand events and the denominator, and himut_duplex.log with the host's and the device's counters.
    ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from CIGAR, SEQ and ``ref_file``.  A single
    process: under torch.distributed.run it raises."""
    from . import vcflib
    from .feed import SampledRun
    run = SampledRun("duplex")
    if not out_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    feed = run.open(bam_file, region, region_list, threads, devices)
    chrom2mate, chrom2host = {}, {}
    chrom2records, chrom2ss, chrom2log = {}, {}, {}

    def pair(chrom, worker, res):
        n = int(res["n_reads"])
        flag = worker.ctx.read_info(n)[2]
        chrom2mate[chrom], chrom2host[chrom] = pair_reads([feed.bam.read_name(i) for i in range(n)], flag)

    def per_contig(chrom, dev, worker, thresholds, _seq):
        get_duplex_substitutions(chrom, bam_file, chrom2mate[chrom], common_snps, panel_of_normals,
                                 feed.chrom2chunkloci_lst[chrom], min_qv, min_mapq, thresholds[0], thresholds[1],
                                 min_sequence_identity, min_gq, min_bq, min_trim, max_mismatch_count, mismatch_window_size,
                                 thresholds[2], min_ref_count, min_alt_count, germline_snv_prior, chrom2records, chrom2ss,
                                 chrom2log, device=dev, resident_worker=worker)

    qlen_lower_limit, qlen_upper_limit, md_threshold = run.each(per_contig, ref_file, cs_from_ref, on_ingest=pair)
    header = vcflib.get_duplex_vcf_header(bam_file, region, region_list, feed.tname2tsize, common_snps, panel_of_normals,
                                          min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq,
                                          min_bq, min_trim, max_mismatch_count, mismatch_window_size, md_threshold,
                                          min_ref_count, min_alt_count, germline_snv_prior, threads, version, out_file,
                                          feed.bam.sample(), ss_file=ss_file, ref_file=ref_file, cs_from_ref=cs_from_ref)
    vcflib.dump_vcf(out_file, header, feed.chrom_lst, lambda chrom: vcflib.duplex_lines(chrom, chrom2records[chrom]))
    if ss_file is not None:
        with open(ss_file, "w") as fh:
            fh.writelines(ss_lines(np.sum([chrom2ss[c] for c in feed.chrom_lst], axis=0) if feed.chrom_lst else [0] * 12,
                                   np.sum([chrom2log[c] for c in feed.chrom_lst], axis=0) if feed.chrom_lst else [0] * 40))
    vcflib.dump_counter_log(LOG_ROWS, feed.chrom_lst, {c: list(chrom2host[c]) + list(chrom2log[c]) for c in feed.chrom_lst},
                            log_path)
    run.done("himut double-strand substitution detection")
    return chrom2records, chrom2ss, chrom2log
