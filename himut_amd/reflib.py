"""`himut tricount` (reference: src/himut/reflib.py:11-93): the 32 pyrimidine-centred trinucleotide counts of the
selected contigs of a FASTA file, counted on the device from the file's bytes (himut_fasta_tricounts,
k_fasta_tricounts).  The file is mapped, not read: the record index below holds offsets into the mapping, and each
selected record's sequence lines go to the library as they lie in the page cache."""
import mmap
import sys

WHITESPACE = b"\n\r\t "              # the bytes read_fasta deletes from a record's sequence lines


def index_fasta(buf):
    """name -> (start, end) of the record's sequence lines in ``buf`` (bytes or an mmap), line ends included.  A record
    starts at a '>' at the start of a line, its name is the first whitespace-separated token of the header, a header
    without tokens is skipped, a later record of the same name replaces an earlier one and text before the first
    record is ignored (read_fasta's rules)."""
    recs = {}
    if buf[:1] == b">":
        pos = 0
    else:
        i = buf.find(b"\n>")
        pos = i + 1 if i >= 0 else -1
    n = len(buf)
    while pos >= 0:
        nxt = buf.find(b"\n>", pos + 1)
        end = nxt if nxt >= 0 else n
        hl = buf.find(b"\n", pos + 1, end)
        head_end, body = (hl, hl + 1) if hl >= 0 else (end, end)
        fields = buf[pos + 1:head_end].split()
        if fields:
            recs[fields[0].decode()] = (body, end)
        pos = nxt + 1 if nxt >= 0 else -1
    return recs


class MappedFasta:
    """A FASTA file mapped read-only, with its record index."""

    def __init__(self, path):
        with open(path, "rb") as fh:
            self._mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if _size(fh) else None
        self.index = index_fasta(self._mm) if self._mm is not None else {}

    def body(self, name):
        """The record's sequence lines as a zero-copy view (KeyError for a name the file does not hold)."""
        s, e = self.index[name]
        return memoryview(self._mm)[s:e]

    def close(self):
        if self._mm is not None:
            self._mm.close()
            self._mm = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _size(fh):
    fh.seek(0, 2)
    n = fh.tell()
    fh.seek(0)
    return n


def tricount_dict(h):
    """64 device bins -> {tri: count} over the 32 keys of TRI_LST."""
    from .normcounts import TRI_LST
    return {t: int(h["ACGT".index(t[0]) * 16 + "ACGT".index(t[1]) * 4 + "ACGT".index(t[2])]) for t in TRI_LST}


def get_genome_tricounts_device(path, chrom_lst, device=0):
    """reflib.get_genome_tricounts (reflib.py:36-61) on the device: the records of ``chrom_lst`` counted from the
    file's bytes and summed.  KeyError for a name the file does not hold, as the reference."""
    from . import caller
    from .normcounts import TRI_LST
    tot = {t: 0 for t in TRI_LST}
    with MappedFasta(path) as fa:
        for chrom in chrom_lst:
            view = fa.body(chrom)
            try:
                h = caller._worker_for(device).ctx.fasta_tricounts(view)
            finally:
                view.release()
            for t, c in tricount_dict(h).items():
                tot[t] += c
    return tot


def get_genome_tricounts_host(path, chrom_lst):
    """The same counts on the host (read_fasta + normcounts.get_chrom_tricount): the CPU baseline and the tests'
    mirror of the device path."""
    from .normcounts import TRI_LST, get_chrom_tricount, read_fasta
    refseq = read_fasta(path)
    tot = {t: 0 for t in TRI_LST}
    for chrom in chrom_lst:
        for t, c in get_chrom_tricount(refseq[chrom]).items():
            tot[t] += c
    return tot


def get_ref_tricount(ref_file, region, region_list, threads, out_file, device=0, tricounts=None):
    """reflib.get_ref_tricount (reflib.py:64-93): --region_list (even with --region) names the contigs, else --region;
    with neither, the message and exit 0.  Rows "{tri}\t{count}" in sorted order.  ``tricounts(path, chrom_lst)``
    counts the FASTA (the device path by default)."""
    chrom_lst = []
    if region_list is not None:
        for line in open(region_list).readlines():
            chrom_lst.append(line.strip())
    elif region is not None:
        chrom_lst.append(region)
    else:
        print("Please provide --region or --region_list")
        print("exiting himut")
        sys.exit(0)
    if tricounts is None:
        def tricounts(path, chroms):
            return get_genome_tricounts_device(path, chroms, device)
    o = open(out_file, "w")
    tri2count = tricounts(ref_file, chrom_lst)
    for tri in sorted(tri2count):
        o.write("{}\t{}\n".format(tri, tri2count[tri]))
    o.close()
