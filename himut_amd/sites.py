"""`himut sites`: the substitutions of a himut VCF genotyped in another BAM.

`himut call` finds single-molecule substitutions in one tissue; the next question is what the matched normal, or
another tissue of the same donor, shows at each of those positions: seen there, germline there, covered at all?  That is
matched-normal subtraction, a panel of normals built from real normals, and every shared-mutation analysis.  `call`
itself only evaluates positions one of *this* BAM's reads proposes, and `support` lists alt reads without depth,
genotype or verdict; the reference's authors re-fetched every read around every site with pysam scripts.  The pile, the
genotyper and `call`'s cascade are resident during a run already: this run takes its column positions from the site
list.  The contract -- the pile of a site, the record, the statuses, the counters -- is DESIGN.md section 8 (row 11) and
include/himut_hip.h (himut_run_sites).  There is no CPU implementation: without the HIP library the call raises.
"""
import numpy as np

from .caller import reads_for, site_sets
from .support import load_sites, site_arrays

COLUMNS = ("chrom", "pos", "ref", "alt", "input_filter", "status", "gt", "gq", "dp", "ref_count", "alt_count", "A", "T", "G",
           "C", "ins", "del", "alt_bq", "alt_hi", "alt_mq", "vaf")
BASES = "ATGC"
LOG_ROWS = ["num_sites", "num_NoCoverage", "num_Germline", "num_HetSite", "num_HetAltSite", "num_HomAltSite", "num_IndelSite",
            "num_LowGQ", "num_LowBQ", "num_PanelOfNormal", "num_ComSnp", "num_LowDepth", "num_HighDepth", "num_PASS",
            "num_alt_seen", "num_positions", "reserved0", "reserved1", "reserved2", "reserved3"]


def depth_of(r):
    c = r["counts"]
    return int(c[0]) + int(c[1]) + int(c[2]) + int(c[3]) + int(c[5])            # bamlib.py:213-219


def format_rows(chrom, sites, recs):
    """The TSV lines (no header) of one contig: ``sites`` as load_sites lists them, ``recs`` as Context.sites returns
    them (record k answers site k).  Python divides the integers, as caller.records_to_tuples does."""
    from ._ffi import SITE_STATUS_NAMES
    out = []
    for (pos, ref, alt, flt), r in zip(sites, recs):
        c = [int(x) for x in r["counts"]]
        dp, n_ref, n_alt = depth_of(r), c[BASES.index(ref)], c[BASES.index(alt)]
        status = SITE_STATUS_NAMES[int(r["status"])]
        gt = "." if status == "NoCoverage" else chr(r["gt"][0]) + chr(r["gt"][1])
        alt_bq = "{:0.1f}".format(int(r["alt_bqsum"]) / float(n_alt)) if n_alt else "."
        vaf = "{:.2f}".format(n_alt / float(dp)) if dp else "."
        out.append("\t".join(str(x) for x in (chrom, pos, ref, alt, flt, status, gt, int(r["gq"]), dp, n_ref, n_alt, c[0], c[1],
                                              c[2], c[3], c[4], c[5], alt_bq, int(r["alt_hi"]), int(r["alt_mq"]), vaf)))
    return out


def unseen_sites(sites, recs, min_depth):
    """The (pos, ref, alt) of one contig this BAM does not show: no alt read and depth >= min_depth."""
    return {(pos, ref, alt) for (pos, ref, alt, _flt), r in zip(sites, recs)
            if int(r["counts"][BASES.index(alt)]) == 0 and depth_of(r) >= min_depth}


def select_unseen(sbs_file, all_filters, chrom2unseen, contigs, command):
    """(lines of the --unseen VCF, data lines dropped because their contig is not in ``contigs``): the header of
    ``sbs_file`` with one ``##himut_sites_command=`` line in front of its #CHROM line, then every data line that
    load_sites loaded (PASS only unless ``all_filters``; a REF of ATGC with at least one single-base ALT of ATGC) and all
    of whose sites are in chrom2unseen[contig]."""
    from .normcounts import _open_sbs
    out, missing, stamped = [], 0, False
    with _open_sbs(sbs_file) as fh:
        for line in fh:
            if line.startswith("#"):
                if line.startswith("#CHROM") and not stamped:
                    out.append("##himut_sites_command={}\n".format(command))
                    stamped = True
                out.append(line if line.endswith("\n") else line + "\n")
                continue
            if not line.strip():
                continue
            f = line.rstrip("\n").split("\t")
            if len(f) < 7:
                f = line.split()
            if not all_filters and f[6] != "PASS":
                continue
            ref = f[3]
            alts = [a for a in f[4].split(",") if len(a) == 1 and a in BASES and a != ref]
            if len(ref) != 1 or ref not in BASES or not alts:
                continue
            if f[0] not in contigs:
                missing += 1
                continue
            seen = chrom2unseen.get(f[0], ())
            if all((int(f[1]), ref, a) in seen for a in alts):
                out.append(line if line.endswith("\n") else line + "\n")
    if not stamped:
        out.insert(0, "##himut_sites_command={}\n".format(command))
    return out, missing


def get_site_genotypes(chrom, bam_file, sites, common_snps, panel_of_normals, min_mapq, min_gq, min_bq, md_threshold,
                       min_ref_count, min_alt_count, germline_snv_prior, chrom2records, chrom2log, device=0, read_batch=None,
                       resident_worker=None):
    """One contig (the shape of dbs.get_doublet_substitutions): its reads from ``read_batch``, from ``bam_file`` with
    the package's BAM reader, or already in HBM under ``resident_worker``.  ``sites``: [(pos, ref, alt, ...)] sorted by
    position.  chrom2records[chrom]: the integer records (format_rows prints them), chrom2log[chrom]: the twenty
    counters.  The read-filter fields of the parameter block are not read by the run."""
    pon_keys, com_keys = site_sets(chrom, common_snps, panel_of_normals)
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    w.configure(0, min_mapq, 0, 1 << 30, 0.0, min_gq, min_bq, 0.0, 0, 0, md_threshold, min_ref_count, min_alt_count, 0,
                germline_snv_prior, False)
    ctx = w.ctx
    ctx.set_site_set(0, pon_keys if pon_keys is not None else np.zeros(0, np.uint64))
    ctx.set_site_set(1, com_keys if com_keys is not None else np.zeros(0, np.uint64))
    if read_batch is not None:
        ctx.push_reads(read_batch)
    ctx.run_sites(*site_arrays(sites))
    chrom2records[chrom], chrom2log[chrom] = ctx.sites()


def dump_sites_log(chrom_lst, chrom2log, path="himut_sites.log"):
    """The counters per contig and their totals, one row per counter (the layout of himut_dbs.log)."""
    with open(path, "w") as fh:
        fh.write("{:30}{}\n".format("", "".join("{:16}".format(c) for c in chrom_lst + ["total"])))
        for k, name in enumerate(LOG_ROWS):
            vals = [int(chrom2log[c][k]) for c in chrom_lst]
            fh.write("{:30}{}\n".format(name, "".join("{:16}".format(v) for v in vals + [sum(vals)])))


def dump_sites(bam_file, sbs_file, common_snps, panel_of_normals, region, region_list, min_mapq, min_gq, min_bq, min_ref_count,
               min_alt_count, germline_snv_prior, all_filters, threads, out_file, devices=(0,), ref_file=None, cs_from_ref=False,
               unseen_file=None, min_depth=10, command=None, log_path="himut_sites.log"):
    """Driver of `himut sites`: the VCF's sites, every target contig through the device-side ingest (one resident context
    per contig, contigs spread over ``devices``), the depth threshold from the same samples `call` takes it from, the TSV,
    himut_sites.log and, with ``unseen_file``, the matched-normal subtraction.  ``cs_from_ref``: the BAM needs no cs tags,
    the ingest derives the text from CIGAR, SEQ and ``ref_file``.  A single process: under torch.distributed.run it
    raises."""
    from . import _ffi, util
    from .feed import SampledRun
    run = SampledRun("sites")
    _ffi.lib()                                  # no CPU implementation: raises here without the HIP library
    chrom2sites, skipped = load_sites(sbs_file, all_filters)
    feed = run.open(bam_file, region, region_list, threads, devices)
    for chrom in util.natsorted(chrom2sites):
        if chrom not in feed.tname2tsize:
            print("himut sites: contig {} of {} is not in {}: its {} sites are skipped".format(
                chrom, sbs_file, bam_file, len(chrom2sites[chrom])))
    if skipped:
        print("himut sites: {} lines of {} hold no single-base substitution and are skipped".format(skipped, sbs_file))
    chrom_lst = [c for c in feed.chrom_lst if c in chrom2sites]
    chrom2records, chrom2log = {}, {}

    def per_contig(chrom, dev, worker, thresholds, _seq):
        get_site_genotypes(chrom, bam_file, chrom2sites[chrom], common_snps, panel_of_normals, min_mapq, min_gq, min_bq,
                           thresholds[2], min_ref_count, min_alt_count, germline_snv_prior, chrom2records, chrom2log,
                           device=dev, resident_worker=worker)

    # (every target contig is sampled for the thresholds; the run takes those the VCF names)
    run.each(per_contig, ref_file, cs_from_ref, contigs=chrom2sites)
    with open(out_file, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for chrom in chrom_lst:
            for line in format_rows(chrom, chrom2sites[chrom], chrom2records[chrom]):
                fh.write(line + "\n")
    dump_sites_log(chrom_lst, chrom2log, path=log_path)
    if unseen_file is not None:
        chrom2unseen = {c: unseen_sites(chrom2sites[c], chrom2records[c], min_depth) for c in chrom_lst}
        lines, missing = select_unseen(sbs_file, all_filters, chrom2unseen, set(feed.tname2tsize),
                                       command or "himut sites -i {} --sbs {} --unseen {}".format(bam_file, sbs_file, unseen_file))
        with open(unseen_file, "w") as fh:
            fh.writelines(lines)
        if missing:
            print("himut sites: {} lines of {} lie on contigs {} lacks and are dropped from {}".format(
                missing, sbs_file, bam_file, unseen_file))
    run.done("himut sites")
    return chrom_lst, chrom2records, chrom2log
