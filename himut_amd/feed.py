"""The contig feed of the run-shaped drivers (`call`, `germline`, `support`, `normcounts`, `phase --cs_from_ref`): the
BAM opened for the device-side ingest, the target contigs and their chunks, which contig goes to which device, and the
step that brings one contig into HBM under a worker of its own.  The drivers keep their own order -- `call` and
`germline` ingest everything, take the global thresholds, then run and release contig by contig; `normcounts` and
`support` ingest, run and release one contig at a time -- and leave through ``with feed:``, which closes whatever is
still resident."""
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

    def ingest_sampled(self, share):
        """Every contig of ``share`` into HBM; returns contig -> the query lengths over its sampled windows, a few
        thousand integers each: the thresholds are global (bamlib.py:137-178), bamlib.thresholds_from_samples takes
        them from every contig's."""
        starts = bamlib.sample_starts(self.chrom_lst, self.tname2tsize)
        samples = {}
        for chrom, dev in share:
            w, res = self.ingest(chrom, dev)
            samples[chrom] = bamlib.sample_qlens(*w.ctx.ingest_read_meta(res["n_reads"]), starts[chrom])
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
