"""The contig feed of the run-shaped drivers (`call`, `germline`, `support`, `normcounts`, `phase --cs_from_ref`): the
BAM opened for the device-side ingest, the target contigs and their chunks, which contig goes to which device, and the
step that brings one contig into HBM under a worker of its own.  The drivers keep their own order -- `call` ingests
everything, takes the global thresholds, then runs and releases contig by contig; `normcounts` and `support` ingest,
run and release one contig at a time -- and leave through ``with feed:``, which closes whatever is still resident.
The single-process drivers that follow `call`'s order (`germline`, `dbs`, `indels`, `bqcal`, `sites`) are one skeleton,
SampledRun, around a per-contig callback."""
import time

from . import bamio, bamlib, dist, util
from .caller import Worker


def contig_share(sizes, devices, group=None):
    """[(contig, device)] of this process for the contigs of ``sizes`` (name -> length): its rank's LPT share on the
    rank's device under a process group (``group`` as dist.join_group returns it), else every contig, LPT-packed over
    ``devices``.  No contigs, no share."""
    if group is not None:
        rank, world, dev = group
        return [(c, dev) for c in dist.lpt_assign(sizes, world)[rank]]
    return [(c, d) for d, contigs in zip(devices, dist.lpt_assign(sizes, len(devices))) for c in contigs]


class ContigFeed:
    def __init__(self, bam_file, region, region_list, threads, devices=(0,), group=None):
        self.bam = bamio.BamStream(bam_file, threads if threads and threads > 1 else 0)
        self.bam_file = bam_file
        self.tname2tsize = self.bam.tname2tsize
        self.chrom_lst, self.chrom2chunkloci_lst = util.load_loci(region, region_list, self.tname2tsize)
        self.devices, self.group = list(devices) or [0], group
        self.refseq = None              # contig -> string once the ingest derives the cs text (derive_cs_from)
        self.resident = {}              # contig -> the Worker that holds its reads

    def share(self, contigs=None):
        """contig_share of the target contigs, or of the ``contigs`` among them a driver narrows itself to."""
        return contig_share({c: self.tname2tsize[c] for c in (self.chrom_lst if contigs is None else contigs)},
                            self.devices, self.group)

    def derive_cs_from(self, ref_file, contigs=None):
        """From here on the ingest derives the cs text from CIGAR, SEQ and the strings of ``ref_file``, which are
        checked against the BAM's header first (bamio.reference_for_cs) and returned."""
        self.refseq = bamio.reference_for_cs(ref_file, self.chrom_lst if contigs is None else contigs, self.tname2tsize,
                                             self.bam_file)
        return self.refseq

    def ingest(self, chrom, device=None, keep_names=False, worker=None):
        """Brings ``chrom`` into HBM under a new Worker on ``device``, resident until ``release`` -- or under ``worker``
        (a device's shared one), which stays the caller's.  Returns (worker, ingest result)."""
        w = worker
        if w is None:
            w = self.resident[chrom] = Worker(device)
        if self.refseq is not None:
            bamio.set_contig_reference(w.ctx, self.refseq[chrom])
        return w, self.bam.ingest_contig(w.ctx, chrom, derive_cs=self.refseq is not None, keep_names=keep_names)

    def ingest_sampled(self, share, on_ingest=None):
        """Every contig of ``share`` into HBM; returns contig -> the query lengths over its sampled windows, a few
        thousand integers each: the thresholds are global (bamlib.py:137-178), bamlib.thresholds_from_samples takes
        them from every contig's.  With ``on_ingest`` the reads' names are kept during each contig's ingest and
        ``on_ingest(chrom, worker, ingest result)`` is called behind it, while ``self.bam.read_name`` still serves them
        (the next contig's ingest drops them)."""
        starts = bamlib.sample_starts(self.chrom_lst, self.tname2tsize)
        samples = {}
        for chrom, dev in share:
            w, res = self.ingest(chrom, dev, keep_names=on_ingest is not None)
            samples[chrom] = bamlib.sample_qlens(*w.ctx.ingest_read_meta(res["n_reads"]), starts[chrom])
            if on_ingest is not None:
                on_ingest(chrom, w, res)
        return samples

    def release(self, chrom):
        """The contig's reads leave HBM."""
        self.resident.pop(chrom).close()

    def close(self):
        for w in self.resident.values():
            w.close()
        self.resident.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SampledRun:
    """The skeleton of a single-process driver under global thresholds, in the order its steps have side effects:

        run = SampledRun("germline")        # refuses to run under torch.distributed.run; the clock starts
        feed = run.open(bam_file, ...)      # the BAM, the target contigs, the devices
        thresholds = run.each(per_contig)   # reference, ingest, thresholds, the contigs one by one
        run.done("himut germline ...")      # the elapsed-time line, once the driver has written its files

    What a driver checks, loads or prints in between is its own."""

    def __init__(self, command):
        dist.require_single_process(command, dist.DEVICES_HINT)
        self.t0 = time.time()
        self.feed = self.refseq = None

    def open(self, bam_file, region, region_list, threads, devices):
        self.feed = ContigFeed(bam_file, region, region_list, threads, devices)
        return self.feed

    def each(self, per_contig, ref_file=None, cs_from_ref=False, contig_strings=False, contigs=None, on_ingest=None):
        """Every target contig into HBM, (qlen_lower_limit, qlen_upper_limit, md_threshold) from all of their samples,
        then ``per_contig(chrom, device, resident_worker, thresholds, chrom_seq)`` and the contig's release, contig by
        contig -- for the ``contigs`` among them only (None: all; the others are ingested, sampled and released all the
        same).  The reference: none; with ``cs_from_ref`` the ingest derives the cs text from ``ref_file``; with
        ``contig_strings`` the run needs the contigs' strings (``self.refseq``) from the FASTA, every target contig must
        be in it, and chrom_seq is the contig's string -- or None when ``cs_from_ref`` has put it into the context
        already.  ``on_ingest``: ContigFeed.ingest_sampled's, for a run that needs the reads' names.  Returns the
        thresholds."""
        feed = self.feed
        share = feed.share()
        if contig_strings:
            from .normcounts import read_fasta
            self.refseq = feed.derive_cs_from(ref_file) if cs_from_ref else read_fasta(ref_file)
            for chrom in feed.chrom_lst:
                if chrom not in self.refseq:
                    raise ValueError("{}: contig {} of {} is not in the FASTA".format(ref_file, chrom, feed.bam_file))
        elif cs_from_ref:
            feed.derive_cs_from(ref_file)
        with feed:
            samples = feed.ingest_sampled(share, on_ingest)
            thresholds = bamlib.thresholds_from_samples(samples, feed.chrom_lst)
            for chrom, dev in share:
                if contigs is None or chrom in contigs:
                    per_contig(chrom, dev, feed.resident[chrom], thresholds,
                               self.refseq[chrom] if contig_strings and not cs_from_ref else None)
                feed.release(chrom)             # the contig's reads leave HBM
        return thresholds

    def done(self, what):
        print("{} took {} minutes".format(what, (time.time() - self.t0) / 60))
