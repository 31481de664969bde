"""The intervals run's contract (Row 14; himut_run_intervals) in plain Python and numpy, over what
tests/callmap_model.py gives: the map of a callable run (a state and the callable bases per entry, the chunks' positions
one behind the other), the chunk list and the reference string.

A map entry of chunk k at position rpos belongs to interval (start, end) iff start <= rpos < end; a position two chunks
hold has two entries.  A row: the entries, entries and bases per state, and three histograms over the trinucleotide class
of the entry's position -- the key callmap_model.get_tri_context (normcounts.get_tri_context) gives, one of the 32
pyrimidine-centred ACGT keys in the order first * 8 + (centre == 'T') * 4 + last with A0 C1 G2 T3, or slot 32 for every
other key.  Nothing of the library or of the device side."""
import numpy as np

from tests import callmap_model as M

ROW_DTYPE = np.dtype([("entries", "<i8"), ("positions", "<i8", (14,)), ("bases", "<i8", (14,)), ("all_tri", "<i8", (33,)),
                      ("ref_tri", "<i8", (33,)), ("ccs_tri", "<i8", (33,))])
FIELDS = ROW_DTYPE.names
TRI_KEYS = [a + m + b for a in "ACGT" for m in "CT" for b in "ACGT"]        # class order: NormTally::ccs
TRI_NAMES = TRI_KEYS + ["other"]
CLASS_OF = {k: i for i, k in enumerate(TRI_KEYS)}
OTHER = 32


def tri_class(seq, pos):
    return CLASS_OF.get(M.get_tri_context(seq, pos), OTHER)


class Map:
    """A callable run's map with the class of every entry's position, computed once."""

    def __init__(self, chunks, state, bases, refseq):
        seq = refseq.decode("latin-1") if isinstance(refseq, (bytes, bytearray)) else refseq
        self.chunks = [(int(s), int(e)) for s, e in chunks]
        self.state = np.asarray(state, np.int64)
        self.bases = np.asarray(bases, np.int64)
        self.mapoff = np.concatenate([[0], np.cumsum([max(e - s, 0) for s, e in self.chunks])]).astype(np.int64)
        assert self.state.shape[0] == self.bases.shape[0] == int(self.mapoff[-1])
        self.cls = np.zeros(self.state.shape[0], np.int64)
        for k, (s, e) in enumerate(self.chunks):
            off = int(self.mapoff[k])
            for rpos in range(s, e):
                self.cls[off + rpos - s] = tri_class(seq, rpos)

    @classmethod
    def of(cls, res, refseq):
        """Of a callmap_model.Result (or anything with chunks, state and bases)."""
        return cls(res.chunks, res.state, res.bases, refseq)

    def row(self, start, end):
        r = np.zeros((), ROW_DTYPE)
        for k, (s, e) in enumerate(self.chunks):
            a, b = max(int(start), s), min(int(end), e)
            if a >= b:
                continue
            sl = slice(int(self.mapoff[k]) + a - s, int(self.mapoff[k]) + b - s)
            st, bs, cl = self.state[sl], self.bases[sl], self.cls[sl]
            r["entries"] += b - a
            r["positions"] += np.bincount(st, minlength=14)
            r["bases"] += np.bincount(st, weights=bs, minlength=14).astype(np.int64)
            r["all_tri"] += np.bincount(cl, minlength=33)
            call = st == M.CALLABLE
            r["ref_tri"] += np.bincount(cl[call], minlength=33)
            r["ccs_tri"] += np.bincount(cl[call], weights=bs[call], minlength=33).astype(np.int64)
        return r

    def rows(self, intervals):
        out = np.zeros(len(intervals), ROW_DTYPE)
        for i, (s, e) in enumerate(intervals):
            out[i] = self.row(s, e)
        return out


def total(rows):
    """The field-by-field sum of rows, as one row."""
    r = np.zeros((), ROW_DTYPE)
    for f in FIELDS:
        r[f] = rows[f].sum(axis=0)
    return r


def same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


def fold_tri(tri2count):
    """A {key: count} histogram of the reference (ref_tri2count, ccs_tri2count) as the 33 slots of a row."""
    out = np.zeros(33, np.int64)
    for key, n in tri2count.items():
        out[CLASS_OF.get(key, OTHER)] += int(n)
    return out
