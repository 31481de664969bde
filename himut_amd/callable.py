"""`himut callable`: where the caller could have called.

`himut normcounts` decides for every reference position of its chunks which row of norm.log the position adds its bases
to -- unphased, het, indel in the pile, depth, allele balance, low GQ, panel of normals, common SNP, callable -- and
keeps the sums.  This run keeps the verdict: a state per position, turned into runs of equal state on the device
(himut_run_callable), written as BED.  The contract -- inputs, states, runs, counters -- is DESIGN.md section 8 (Row 9) and
include/himut_hip.h.  There is no CPU implementation: without the HIP library the call raises.
"""
import numpy as np

from ._ffi import CALLABLE_STATES
from .caller import reads_for, site_sets
from .normcounts import alt_order_table, tri_classes

CALLABLE = 13


def callable_contig(worker, batch, chunks, refseq, pon_keys=None, common_keys=None, non_human_sample=False,
                    alt_order=None, phase_sets=None):
    """The callable run on one contig through a configured caller.Worker (the arguments of normcounts.norm_contig);
    returns (runs as _ffi.CALLABLE_RUN_DTYPE, log[14]).  ``refseq`` None: the context holds the contig's string already.
    The per-position map stays in the context (worker.ctx.callable_map)."""
    ctx = worker.ctx
    if refseq is not None:
        chars, cls = tri_classes(refseq)
        ctx.set_reference(refseq, cls, len(chars))
    worker.load(chunks, pon_keys, common_keys, phase_sets, batch)
    ctx.run_callable(alt_order_table(alt_order), non_human_sample)
    return ctx.callable()


def merge_runs(runs):
    """The writer's lines of one contig: (start, end, state, bases) arrays.  Runs of equal state that abut across a chunk
    boundary become one line, their bases added; chunks that overlap or leave gaps give their runs as they come."""
    n = runs.shape[0]
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    joins = np.zeros(n, bool)
    joins[1:] = ((runs["chunk"][1:] != runs["chunk"][:-1]) & (runs["start"][1:] == runs["end"][:-1]) &
                 (runs["state"][1:] == runs["state"][:-1]))
    first = np.flatnonzero(~joins)
    last = np.concatenate([first[1:], [n]]) - 1
    return (runs["start"][first].astype(np.int64), runs["end"][last].astype(np.int64), runs["state"][first].astype(np.int64),
            np.add.reduceat(runs["bases"].astype(np.int64), first))


def bed_lines(chrom, runs, callable_only=False):
    start, end, state, bases = merge_runs(runs)
    if callable_only:
        keep = state == CALLABLE
        start, end, state, bases = start[keep], end[keep], state[keep], bases[keep]
    return ["{}\t{}\t{}\t{}\t{}\n".format(chrom, s, e, CALLABLE_STATES[st], b)
            for s, e, st, b in zip(start.tolist(), end.tolist(), state.tolist(), bases.tolist())]


def summary_lines(chrom_lst, chrom2runs):
    """chrom, STATE, positions, bases: one line per contig and state that has a position."""
    out = ["chrom\tstate\tpositions\tbases\n"]
    for chrom in chrom_lst:
        r = chrom2runs[chrom]
        for code, name in CALLABLE_STATES.items():
            m = r["state"] == code
            if m.any():
                out.append("{}\t{}\t{}\t{}\n".format(chrom, name, int((r["end"][m].astype(np.int64) - r["start"][m]).sum()),
                                                     int(r["bases"][m].sum())))
    return out


def get_callable_runs(
    chrom, seq, bam_file, common_snps, panel_of_normals, chunkloci_lst, phase_set2hbit_lst, phase_set2hpos_lst,
    phase_set2hetsnp_lst, min_qv, min_mapq, min_trim, qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq,
    min_bq, mismatch_window, max_mismatch_count, min_ref_count, min_alt_count, min_hap_count, md_threshold,
    germline_snv_prior, phase, non_human_sample, chrom2runs, chrom2log, device=0, read_batch=None, resident_worker=None,
):
    """One contig (the shape of normcounts.get_callable_tricounts): chrom2runs[chrom] = the runs, chrom2log[chrom] = the
    fourteen counters of norm.log."""
    pon_keys, com_keys = site_sets(chrom, common_snps, panel_of_normals)
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    w.configure(min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                max_mismatch_count, mismatch_window, md_threshold, min_ref_count, min_alt_count, min_hap_count,
                germline_snv_prior, phase)
    chunks = [(int(s), int(e)) for (_c, s, e) in chunkloci_lst]
    phase_sets = (phase_set2hbit_lst, phase_set2hpos_lst, phase_set2hetsnp_lst) if phase else None
    chrom2runs[chrom], chrom2log[chrom] = callable_contig(w, read_batch, chunks, seq, pon_keys, com_keys, non_human_sample,
                                                           phase_sets=phase_sets)


def dump_callable(bam_file, ref_file, sbs_file, vcf_file, phased_vcf_file, common_snps, panel_of_normals, region,
                  region_list, min_qv, min_mapq, min_sequence_identity, min_gq, min_bq, min_trim, mismatch_window,
                  max_mismatch_count, min_ref_count, min_alt_count, min_hap_count, somatic_snv_prior, germline_snv_prior,
                  germline_indel_prior, threads, phase, non_human_sample, reference_sample, out_file, callable_only=False,
                  summary_file=None, devices=(0,), log_path="callable.log", cs_from_ref=False, contig_hook=None):
    """Driver of `himut callable`: the arguments of normcounts.get_normcounts, ``sbs_file`` optional.  With it the depth
    threshold and the read length limits come from its header, as in `normcounts`; without it they are computed from the
    BAM as `himut call` computes them.  Contigs are spread over ``devices`` (under torch.distributed.run: over the ranks,
    rank 0 writes).  ``contig_hook(chrom, worker, seq, length)``, where given, is called behind each contig's run while the
    worker's context still holds the contig's reads, string and map (`himut intervals` tallies its intervals there);
    ``out_file`` None: no BED is written.  Returns (contig -> runs, contig -> counters), or (None, None) on the other
    ranks."""
    import time
    from . import bamlib, dist, vcflib
    from .feed import ContigFeed
    from .normcounts import dump_norm_log, get_thresholds, read_fasta
    t0 = time.time()
    group = dist.join_group(devices)       # (rank, world, device) under torch.distributed.run, else None
    feed = ContigFeed(bam_file, region, region_list, threads, devices, group)
    tname2tsize, chrom_lst, chrom2chunkloci_lst = feed.tname2tsize, feed.chrom_lst, feed.chrom2chunkloci_lst
    ps2hbit, ps2hpos, ps2hetsnp = {}, {}, {}
    if phase:
        ps2hbit, ps2hpos, ps2hetsnp, chrom2chunkloci_lst = vcflib.load_phased_hetsnps(phased_vcf_file, chrom_lst,
                                                                                      tname2tsize)
    if non_human_sample:
        germline_snv_prior, germline_indel_prior = vcflib.get_germline_priors(chrom_lst, ref_file, vcf_file, reference_sample)
    refseq = feed.derive_cs_from(ref_file) if cs_from_ref else read_fasta(ref_file)
    for chrom in chrom_lst:
        if chrom not in refseq:
            raise ValueError("{}: contig {} of {} is not in the FASTA".format(ref_file, chrom, bam_file))
    share = feed.share()
    runs, log = {}, {}

    def on_every_rank(step):
        """What ``step`` returns for this rank's share, from every rank (a list, rank order); a rank that fails still joins
        the collective and every rank leaves with the same error."""
        if group is None:
            return [step()]
        out = err = None
        try:
            out = step()
        except Exception as e:              # noqa: BLE001 -- handed to every rank, re-raised there
            err = e
        return dist.share_or_raise(out, err)

    def sweep_share(limits):
        for chrom, dev in share:
            w = feed.resident[chrom] if limits is None else feed.ingest(chrom, dev)[0]
            lo, hi, md = thresholds if limits is None else limits
            get_callable_runs(
                chrom, refseq[chrom], bam_file, common_snps, panel_of_normals, chrom2chunkloci_lst[chrom],
                ps2hbit.get(chrom, {}), ps2hpos.get(chrom, {}), ps2hetsnp.get(chrom, {}), min_qv, min_mapq, min_trim, lo, hi,
                min_sequence_identity, min_gq, min_bq, mismatch_window, max_mismatch_count, min_ref_count, min_alt_count,
                min_hap_count, md, germline_snv_prior, phase, non_human_sample, runs, log, device=dev, resident_worker=w)
            if contig_hook is not None:
                contig_hook(chrom, w, refseq[chrom], tname2tsize[chrom])
            feed.release(chrom)             # the contig's reads leave HBM
        return runs, log

    with feed:                              # a failed ingest or sweep leaves nothing resident
        if sbs_file is not None:
            parts = on_every_rank(lambda: sweep_share(get_thresholds(sbs_file)))
        else:
            # as `himut call`: every contig of the share resident, the thresholds from all of their samples
            samples = {c: s for part in on_every_rank(lambda: feed.ingest_sampled(share)) for c, s in part.items()}
            thresholds = bamlib.thresholds_from_samples(samples, chrom_lst)
            parts = on_every_rank(lambda: sweep_share(None))
    if group is not None:
        dist.leave_group()
        if group[0] != 0:
            return None, None
        runs, log = {}, {}
        for r_, l_ in parts:
            runs.update(r_); log.update(l_)
    runs = {chrom: runs[chrom] for chrom in chrom_lst}      # (contig order, whichever device took which contig)
    if out_file is not None:
        with open(out_file, "w") as o:
            for chrom in chrom_lst:
                o.writelines(bed_lines(chrom, runs[chrom], callable_only))
    if summary_file is not None:
        with open(summary_file, "w") as o:
            o.writelines(summary_lines(chrom_lst, runs))
    dump_norm_log(chrom_lst, log, log_path)
    print("himut callable took {} minutes".format((time.time() - t0) / 60))
    return runs, log
