"""BAM in / out for the hot path (ctypes front-end of libhimut_host.so: csrc/bam_load.cpp, bam_stream.cpp,
bam_write.cpp and vcf_format.cpp).

``read_bam`` stands where the reference opens ``pysam.AlignmentFile`` and wraps every record
in ``bamlib.BAM`` (caller.py:267,299-300; bamlib.py:14-32, 89-129): it returns the header
facts the driver needs (contig sizes, sample name) and one ReadBatch per contig, reads in
file order.  ``write_bam`` turns read batches (e.g. synthetic ones) into a BAM file."""
import ctypes
import os

import numpy as np

from . import build
from .readbatch import ReadBatch, read_arrays

_lib = None


class _WriteContig(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("length", ctypes.c_int64), ("n", ctypes.c_int64)] + [
        (k, ctypes.c_void_p) for k in ("tstart", "qstart", "qlen", "mapq", "flag", "qid", "qoff", "cs_off", "seq",
                                       "bq", "cs", "tp", "names", "name_off")]


# the host library's C ABI: name -> (restype, argtypes)
_I, _I32, _I64, _P, _S = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p
_ABI = {
    "bam_load_threads": (_P, [_S, _I]),
    "bam_error": (_S, [_P]),
    "bam_header_text": (_S, [_P]),
    "bam_n_ref": (_I64, [_P]),
    "bam_ref_name": (_S, [_P, _I64]),
    "bam_ref_len": (_I64, [_P, _I64]),
    "bam_ref_nreads": (_I64, [_P, _I64]),
    "bam_ref_bases_padded": (_I64, [_P, _I64]),
    "bam_ref_cs_bytes": (_I64, [_P, _I64]),
    "bam_count": (_I64, [_P, _I]),
    "bam_ref_copy": (None, [_P, _I64] + [_P] * 10),
    "bam_ref_bytes": (_P, [_P, _I64, _I]),
    "bam_free": (None, [_P]),
    "bam_stream_open": (_P, [_S, _I]),
    "bam_stream_error": (_S, [_P]),
    "bam_stream_header_text": (_S, [_P]),
    "bam_stream_n_ref": (_I64, [_P]),
    "bam_stream_ref_name": (_S, [_P, _I64]),
    "bam_stream_ref_len": (_I64, [_P, _I64]),
    "bam_stream_indexed": (_I, [_P]),
    "bam_stream_unique_names": (_I, [_P]),
    "bam_stream_scan_parts": (_I64, [_P]),
    "bam_stream_inflated_bytes": (_I64, [_P]),
    "bam_stream_head": (_I64, []),
    "bam_stream_close": (None, [_P]),
    "bam_stream_select": (_I, [_P, _I32, ctypes.POINTER(_I64)]),
    "bam_stream_sum_cigar": (None, [_P, _I]),
    "bam_stream_keep_names": (None, [_P, _I]),
    "bam_stream_read_name": (_S, [_P, _I64]),
    "bam_stream_pump": (_I, [_P] * 6 + [_I64, _I64]),
    "bam_write": (_I, [_S, _S, ctypes.POINTER(_WriteContig), _I64]),
    "vcf_format_records": (_I64, [_P, _I64, _S, _I, _I, _P, _I64]),
}


def _load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build.build_host())
        for name, (restype, argtypes) in _ABI.items():
            f = getattr(L, name)               # a name the library does not export is an error here
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class BamFile:
    """All contigs of one BAM, loaded once."""

    def __init__(self, path, threads=0):
        """threads: BGZF inflate threads (0 = HIMUT_INGEST_THREADS or one per hardware thread, at most 16)."""
        L = _load()
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        h = L.bam_load_threads(path.encode(), int(threads))
        self._h = h            # the big arrays of the batches are views into the library's memory
        self._L = L
        err = L.bam_error(h).decode()
        if err:
            raise ValueError("{}: {}".format(path, err))
        if L.bam_count(h, 0):
            # the reference does line.get_tag("cs") on every record (bamlib.py:32)
            raise KeyError("tag 'cs' not present in {} records of {}".format(L.bam_count(h, 0), path))
        if L.bam_count(h, 2):
            raise ValueError("{} is not coordinate sorted".format(path))
        self.header_text = L.bam_header_text(h).decode("utf-8", "replace")
        self.tname2tsize = {}
        self.batches = {}

        def view(i, which, n):
            if n == 0:
                return np.zeros(0, np.uint8)
            buf = (ctypes.c_uint8 * n).from_address(L.bam_ref_bytes(h, i, which))
            a = np.frombuffer(buf, dtype=np.uint8)
            a.flags.writeable = True
            return a

        for i in range(L.bam_n_ref(h)):
            name = L.bam_ref_name(h, i).decode()
            length = L.bam_ref_len(h, i)
            self.tname2tsize[name] = length
            n = L.bam_ref_nreads(h, i)
            tot = L.bam_ref_bases_padded(h, i)
            csb = L.bam_ref_cs_bytes(h, i)
            a = read_arrays(n)                     # the per-read arrays, in the order bam_ref_copy takes them
            a["tp"] = np.zeros(n, np.uint8)
            L.bam_ref_copy(h, i, *[_p(x) for x in a.values()])
            a["seq"] = view(i, 0, tot // 2)
            a["bq"] = view(i, 1, tot)
            a["cs"] = view(i, 2, csb)
            b = ReadBatch(name=name, length=length, **a)
            b._owner = self        # keeps the library's memory alive as long as the batch is
            self.batches[name] = b

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.bam_free(self._h)
                self._h = None
        except Exception:
            pass

    def sample(self):
        """SM of the first @RG line (bamlib.get_sample, bamlib.py:89-106)."""
        for line in self.header_text.strip().split("\n"):
            if line.startswith("@RG"):
                for f in line.split():
                    if f.startswith("SM"):
                        return f.split(":")[1]
        raise ValueError("SM field is missing; provide a BAM file with an @RG group")


def stream_rec_cap(window_bytes):
    """Records a window of the device-side ingest can hold at the most: its bytes and the head room in front of them,
    cut into the shortest legal records (a length field and the 32 fixed bytes).  The stream carries what it
    cannot list over to the next window, so a smaller list lets the carry outgrow the head room."""
    return (int(window_bytes) + int(_load().bam_stream_head())) // 36 + 16


class BamStream:
    """One BAM opened for the device-side ingest: the header here, the records of one contig at a time to the GPU
    (``ingest_contig``).  With an index beside the file (x.bam.bai) only the contig's own BGZF blocks are inflated."""

    def __init__(self, path, threads=0):
        L = _load()
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self._L = L
        self._h = L.bam_stream_open(path.encode(), int(threads))
        err = L.bam_stream_error(self._h).decode()
        if err:
            raise ValueError("{}: {}".format(path, err))
        self.path = path
        self.header_text = L.bam_stream_header_text(self._h).decode("utf-8", "replace")
        self.names = [L.bam_stream_ref_name(self._h, i).decode() for i in range(L.bam_stream_n_ref(self._h))]
        self.tname2tsize = {n: L.bam_stream_ref_len(self._h, i) for i, n in enumerate(self.names)}
        self.indexed = bool(L.bam_stream_indexed(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.bam_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    sample = BamFile.sample

    def inflated_bytes(self):
        """Inflated bytes this stream has produced since it was opened (the header's blocks not counted)."""
        return int(self._L.bam_stream_inflated_bytes(self._h))

    def read_name(self, i):
        """Name of read ``i`` (ordinal in the batch) of the contig last ingested with ``keep_names=True``."""
        s = self._L.bam_stream_read_name(self._h, int(i))
        if s is None:
            raise LookupError("no name for read {}: the last ingest_contig kept no names (keep_names=True) or the contig "
                              "has fewer reads".format(i))
        return s.decode("utf-8", "replace")

    def ingest_contig(self, ctx, chrom, window_bytes=None, derive_cs=False, keep_names=False):
        """Streams the records of ``chrom`` into the context ``ctx`` (an _ffi.Context), parsed on the device.  Two
        pinned windows: while the GPU copies and parses one, the host's pool inflates the next.  Leaves the context as
        ``push_reads`` would and returns the ingest result (n_reads, bases_padded, cs_bytes, read_bases).
        ``derive_cs``: the cs text of every record is derived from its CIGAR and the contig's reference string, which
        the context has from ``set_reference``; cs tags are neither needed nor read.  ``keep_names``: the reads' names stay
        on the host by ordinal (``read_name``) until the next ingest."""
        L, h = self._L, self._h
        L.bam_stream_keep_names(h, 1 if keep_names else 0)
        ctx.ingest_derive_cs(1 if derive_cs else 0)
        L.bam_stream_sum_cigar(h, 1 if derive_cs else 0)
        if window_bytes is None:
            window_bytes = int(os.environ.get("HIMUT_INGEST_WINDOW_KB", str(64 << 10))) << 10
        bound = ctypes.c_int64()
        if L.bam_stream_select(h, self.names.index(chrom), ctypes.byref(bound)):
            raise ValueError(L.bam_stream_error(h).decode())
        cap = window_bytes + L.bam_stream_head()       # head room for the record a window boundary cuts
        bufs = ctx.ingest_begin(bound.value, cap)
        rec_cap = stream_rec_cap(window_bytes)
        # the loop -- wait for window k's inflate, start window k + 1's, hop over k's records, hand k to the GPU -- is one
        # call into the host library, which calls the device library's himut_ingest_wait / himut_ingest_window itself
        rc = L.bam_stream_pump(h, ctx.handle, ctx.fn_address("himut_ingest_wait"), ctx.fn_address("himut_ingest_window"),
                               bufs[0], bufs[1], cap, rec_cap)
        if rc:
            # the two pinned windows belong to the process: a failed pump gives them back (himut_ingest_end, whatever it
            # answers) before it raises, or no context could ingest or count a FASTA until this one is destroyed
            try:
                if rc == -2:
                    raise ValueError("{}: {}".format(self.path, L.bam_stream_error(h).decode()))
                ctx.raise_for(rc)
            finally:
                try:
                    ctx.ingest_end(False)
                except RuntimeError:
                    pass
        res = ctx.ingest_end(bool(L.bam_stream_unique_names(h)))
        if derive_cs:
            bad = ctx.ingest_derive_result()["n_underivable"]
            if bad:
                raise ValueError("{}: cs cannot be derived for {} records of {} (no CIGAR, an N or P op, CIGAR and SEQ "
                                 "lengths that disagree, or an alignment that leaves the reference)".format(self.path, bad, chrom))
        if res["n_missing_cs"]:
            # the reference does line.get_tag("cs") on every record (bamlib.py:32)
            raise KeyError("tag 'cs' not present in {} records of {}".format(res["n_missing_cs"], self.path))
        if res["n_unsorted"]:
            raise ValueError("{} is not coordinate sorted".format(self.path))
        return res


def reference_for_cs(ref_file, chrom_lst, tname2tsize, bam_path):
    """The contig strings an ingest that derives the cs text reads (``normcounts.read_fasta`` of ``ref_file``), checked
    before the first ingest: every target contig is in the FASTA, as long as the BAM's @SQ line says."""
    from .normcounts import read_fasta
    if ref_file is None:
        raise ValueError("deriving the cs text needs the reference FASTA file")
    refseq = read_fasta(ref_file)
    for chrom in chrom_lst:
        if chrom not in refseq:
            raise ValueError("{}: contig {} of {} is not in the FASTA".format(ref_file, chrom, bam_path))
        if len(refseq[chrom]) != tname2tsize[chrom]:
            raise ValueError("{}: contig {} is {} bases long, @SQ LN of {} says {}".format(
                ref_file, chrom, len(refseq[chrom]), bam_path, tname2tsize[chrom]))
    return refseq


def set_contig_reference(ctx, seq):
    """The contig's string into the context, in front of an ingest that derives the cs text from it."""
    from .normcounts import tri_classes
    chars, cls = tri_classes(seq)
    ctx.set_reference(seq, cls, len(chars))


_cache = {}


def read_bam(path, threads=0):
    key = (os.path.abspath(path), os.path.getmtime(path))
    if key not in _cache:
        _cache.clear()
        _cache[key] = BamFile(path, threads)
    return _cache[key]


def read_contig(path, chrom):
    return read_bam(path).batches[chrom]


def write_bam(path, batches, sample="syn", names=False):
    """batches: list of ReadBatch in @SQ order.  CIGARs are derived from the cs tags.  A read is named ccs/<qid>; with
    ``names`` a batch that carries names (ReadBatch.qnames, 1 to 254 bytes each) gives its reads those."""
    L = _load()
    arr = (_WriteContig * len(batches))()
    keep = []
    for k, b in enumerate(batches):
        cols = [np.ascontiguousarray(x) for x in (b.tstart, b.qstart, b.qlen, b.mapq, b.flag, b.qid, b.qoff, b.cs_off,
                                                  b.seq, b.bq, b.cs, b.tp)]
        keep.append(cols)
        nm = b.name.encode()
        keep.append(nm)
        own = [None, None]
        if names and b.qnames is not None:
            raw = [q.encode() for q in b.qnames]
            own = [np.frombuffer(b"".join(raw) or b"\0", np.uint8), np.cumsum([0] + [len(q) for q in raw]).astype(np.int64)]
            keep.append(own)
        arr[k] = _WriteContig(nm, int(b.length), int(b.n), *[_p(x) for x in cols], *[None if x is None else _p(x) for x in own])
    rc = L.bam_write(path.encode(), sample.encode(), arr, len(batches))
    if rc:
        raise IOError("bam_write failed ({})".format(rc))


def format_records(recs, chrom, phased=False, single_molecule_file=False):
    """VCF body lines (bytes) of a records array, printed by the host library exactly as
    caller.records_to_tuples + vcflib._body_line would."""
    L = _load()
    recs = np.ascontiguousarray(recs)
    cap = int(recs.shape[0]) * 256 + 1024
    out = np.empty(cap, np.uint8)
    n = L.vcf_format_records(_p(recs), int(recs.shape[0]), chrom.encode(), 1 if phased else 0,
                             1 if single_molecule_file else 0, _p(out), cap)
    if n < 0:
        raise RuntimeError("vcf_format_records: buffer too small")
    return out[:n].tobytes()
