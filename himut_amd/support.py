"""`himut support`: the reads that carry each called substitution.

A `himut call` line says ``AD 11,1``; this command says which molecule carried the 1, where in that read the
substitution sits, what its base quality was, how good the read was and what else mismatched nearby -- the tables the
reference's authors made with one-off pysam scripts outside the package (scripts/sbs2ccs.py,
scripts/sbs_qpos_distribution.py), from which min_trim, min_qv and the mismatch window were chosen.  The decoded reads
are resident in HBM already; one kernel turns a site list into (site, read) rows.  The contract -- reads in play,
cover / support, the row fields, the window count -- is DESIGN.md section 8 and include/himut_hip.h
(himut_run_support).  There is no CPU implementation: without the HIP library the call raises.
"""
import numpy as np

from .caller import reads_for

COLUMNS = ("chrom", "pos", "ref", "alt", "filter", "alt_reads", "cover", "qname", "strand", "mapq", "qlen", "qpos", "bq",
           "qv", "n_sub", "n_indel", "window_mismatches")
READ_COLUMNS = len(COLUMNS) - 7          # the columns that describe a read: "." on the line of a site without rows
BASES = "ATGC"


def load_sites(sbs_file, all_filters=False):
    """The sites of a himut VCF (plain .vcf or .vcf.bgz): a data line whose REF is one of ATGC, with each of its
    single-base ALT alleles from ATGC (a HetAltSite line ``A,C`` gives two sites); PASS lines only unless
    ``all_filters``.  Returns (chrom -> [(pos, ref, alt, filter)] de-duplicated and sorted, number of lines skipped
    because they hold no such site)."""
    from .normcounts import _open_sbs
    seen, skipped = {}, 0
    with _open_sbs(sbs_file) as fh:
        for line in fh:
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\n").split("\t")
            if len(f) < 7:
                f = line.split()
            if not all_filters and f[6] != "PASS":
                continue
            ref = f[3]
            alts = [a for a in f[4].split(",") if len(a) == 1 and a in BASES and a != ref]
            if len(ref) != 1 or ref not in BASES or not alts:
                skipped += 1
                continue
            for a in alts:
                seen.setdefault(f[0], {}).setdefault((int(f[1]), ref, a), f[6])
    return {c: [k + (flt,) for k, flt in sorted(d.items())] for c, d in seen.items()}, skipped


def site_arrays(sites):
    """(pos1, ref, alt) of a site list [(pos, ref, alt, ...)] as the arrays Context.run_support and run_sites take."""
    return (np.array([s[0] for s in sites], np.int32),
            np.frombuffer("".join(s[1] for s in sites).encode("ascii"), np.uint8),
            np.frombuffer("".join(s[2] for s in sites).encode("ascii"), np.uint8))


def format_rows(chrom, sites, rows, site_counts, name_of):
    """The TSV lines (no header) of one contig: ``sites`` as load_sites lists them, ``rows`` / ``site_counts`` as
    Context.support returns them, ``name_of(read ordinal, qid)`` the read's name.  A site without rows is one line with
    "." in every read column."""
    out = []
    first = np.searchsorted(rows["site"], np.arange(len(sites) + 1)) if len(sites) else np.zeros(1, np.int64)
    for k, (pos, ref, alt, flt) in enumerate(sites):
        head = "{}\t{}\t{}\t{}\t{}\t{}\t{}".format(chrom, pos, ref, alt, flt, int(site_counts[k][1]), int(site_counts[k][0]))
        if first[k] == first[k + 1]:
            out.append(head + "\t." * READ_COLUMNS)
        for r in rows[first[k]:first[k + 1]]:
            out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{:.2f}\t{}\t{}\t{}".format(
                head, name_of(int(r["read"]), int(r["qid"])), "-" if int(r["flag"]) & 0x10 else "+", int(r["mapq"]),
                int(r["qlen"]), int(r["qpos"]), int(r["bq"]), int(r["bq_sum"]) / int(r["qlen"]), int(r["n_sub"]),
                int(r["n_indel"]), int(r["window_mismatches"])))
    return out


def get_support_rows(chrom, bam_file, sites, min_mapq, mismatch_window_size, chrom2rows, chrom2counts, device=0,
                     read_batch=None, resident_worker=None):
    """One contig (the shape of germline.get_germline_snvs): its reads from ``read_batch``, from ``bam_file`` with the
    package's BAM reader, or already in HBM under ``resident_worker``.  ``sites``: [(pos, ref, alt, ...)] sorted by
    position.  chrom2rows[chrom]: the rows, chrom2counts[chrom]: per site (cover, alt_reads)."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.run_support(*site_arrays(sites), min_mapq=min_mapq, mismatch_window_size=mismatch_window_size)
    chrom2rows[chrom], chrom2counts[chrom] = w.ctx.support()


def dump_support(bam_file, sbs_file, region, region_list, min_mapq, mismatch_window_size, all_filters, threads, out_file,
                 devices=(0,), ref_file=None, cs_from_ref=False):
    """Driver of `himut support`: the VCF's sites, every target contig the VCF names through the device-side ingest (one
    resident context per contig, contigs spread over ``devices``, the reads' names kept on the host), the TSV.
    ``cs_from_ref``: the BAM needs no cs tags, the ingest derives the text from CIGAR, SEQ and ``ref_file``.  A single
    process: under torch.distributed.run it raises."""
    import time
    from . import _ffi, dist, util
    from .feed import ContigFeed
    dist.require_single_process("support", dist.DEVICES_HINT)
    _ffi.lib()                                  # no CPU implementation: raises here without the HIP library
    t0 = time.time()
    chrom2sites, skipped = load_sites(sbs_file, all_filters)
    feed = ContigFeed(bam_file, region, region_list, threads, devices)
    for chrom in util.natsorted(chrom2sites):
        if chrom not in feed.tname2tsize:
            print("himut support: contig {} of {} is not in {}: its {} sites are skipped".format(
                chrom, sbs_file, bam_file, len(chrom2sites[chrom])))
    chrom_lst = [c for c in feed.chrom_lst if c in chrom2sites]
    if skipped:
        print("himut support: {} lines of {} hold no single-base substitution and are skipped".format(skipped, sbs_file))
    if cs_from_ref:
        feed.derive_cs_from(ref_file, chrom_lst)
    lines = {}
    with feed:
        for chrom, dev in feed.share(chrom_lst):
            w, _res = feed.ingest(chrom, dev, keep_names=True)
            chrom2rows, chrom2counts = {}, {}
            get_support_rows(chrom, bam_file, chrom2sites[chrom], min_mapq, mismatch_window_size, chrom2rows, chrom2counts,
                             device=dev, resident_worker=w)
            lines[chrom] = format_rows(chrom, chrom2sites[chrom], chrom2rows[chrom], chrom2counts[chrom],
                                       lambda i, _qid: feed.bam.read_name(i))
            feed.release(chrom)                 # the contig's reads leave HBM
    with open(out_file, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for chrom in chrom_lst:
            for line in lines[chrom]:
                fh.write(line + "\n")
    print("himut support took {} minutes".format((time.time() - t0) / 60))
    return chrom_lst
