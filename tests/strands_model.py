"""The definitions of the transcription-strand spectrum in plain Python / numpy, written
from the definitions and not from the package's code: the category of a letter in a segment, the SBS96 bin of a
substitution as himut_sbs96_counts gives it, the trinucleotide class of a position, the three tallies, and the labels a
second time."""
import bisect

import numpy as np

CATS = "TUBN"
NO_CLASS = 0xFFFF
CALLABLE = 13
_SUBS = ("C>A", "C>G", "C>T", "T>A", "T>C", "T>G")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def bin_labels():
    """Label of every bin category * 96 + sub * 16 + up * 4 + down."""
    out = []
    for cat in CATS:
        for sub in _SUBS:
            for up in "ACGT":
                for down in "ACGT":
                    out.append(cat + ":" + up + "[" + sub + "]" + down)
    return out


def file_labels():
    """The labels in the order `sbs384` writes them: per category, `sbs96`'s order (first letter, substitution, last)."""
    out = []
    for cat in CATS:
        for up in "ACGT":
            for sub in _SUBS:
                for down in "ACGT":
                    out.append(cat + ":" + up + "[" + sub + "]" + down)
    return out


def tri_names():
    return [a + m + b for a in "ACGT" for m in "CT" for b in "ACGT"]


def category(mask, letter):
    """T 0, U 1, B 2, N 3 for ``letter`` (upper-case ACGT) in a segment of ``mask``."""
    purine = letter in "AG"
    if mask == 0:
        return 3
    if mask == 3:
        return 2
    if mask == 1:                       # a gene on +: the + strand is the coding one, the - strand is transcribed
        return 0 if purine else 1       # (a purine here has its pyrimidine partner on the - strand: T)
    return 1 if purine else 0           # a gene on -: the + strand is transcribed


def segment_of(seg_start, pos):
    """The segment that holds ``pos``: the last k with seg_start[k] <= pos."""
    return bisect.bisect_right(list(seg_start), pos) - 1


def _code(c):
    return "ACGT".index(c) if c in "ACGT" else 4 if c == "N" else 5


def _comp(c):
    return 3 - _code(c) if _code(c) < 4 else 4


def sbs96_bin(seq, pos, ref, alt):
    """0..95 (sub * 16 + up * 4 + down), or 96 (a class with an N), 97 (a class outside the 96 without an N), 98 (the
    position below 0 or position + 1 behind the string).  Position 0 reads its upstream letter at the string's end."""
    if pos < 0 or pos + 1 >= len(seq):
        return 98
    before, after = seq[pos - 1], seq[pos + 1]
    if ref in "AG":
        up, down, r, a = _comp(after), _comp(before), _comp(ref), _comp(alt)
    else:
        up, down, r, a = _code(before), _code(after), _code(ref), _code(alt)
    if 4 in (up, down, r, a):
        return 96
    if up > 3 or down > 3 or a > 3 or r not in (1, 3) or a == r:
        return 97
    return _SUBS.index("ACGT"[r] + ">" + "ACGT"[a]) * 16 + up * 4 + down


def sbs384(seq, seg_start, seg_mask, pos0, ref, alt):
    """(cls uint16, out int64[387]) of himut_sbs384_counts."""
    cls = np.full(len(pos0), NO_CLASS, np.uint16)
    out = np.zeros(387, np.int64)
    for i, (p, r, a) in enumerate(zip(pos0, ref, alt)):
        b = sbs96_bin(seq, p, r, a)
        if b >= 96:
            out[384 + b - 96] += 1
            continue
        k = category(seg_mask[segment_of(seg_start, p)], r) * 96 + b
        cls[i] = k
        out[k] += 1
    return cls, out


def tri_class(seq, pos):
    """first * 8 + (centre == T) * 4 + last of the trinucleotide around ``pos`` with a purine centre read on the other
    strand; None unless the three letters exist and are upper-case ACGT."""
    if pos < 1 or pos + 1 >= len(seq):
        return None
    t = seq[pos - 1:pos + 2]
    if any(c not in "ACGT" for c in t):
        return None
    if t[1] in "AG":
        t = _COMP[t[2]] + _COMP[t[1]] + _COMP[t[0]]
    return "ACGT".index(t[0]) * 8 + (4 if t[1] == "T" else 0) + "ACGT".index(t[2])


def _position_bins(seq, seg_start, seg_mask):
    """Per position the bin category * 32 + class, -1 without a class."""
    n = len(seq)
    bins = np.full(n, -1, np.int64)
    mask_at = np.asarray(seg_mask)[np.searchsorted(np.asarray(seg_start), np.arange(n), side="right") - 1]
    for p in range(n):
        c = tri_class(seq, p)
        if c is not None:
            bins[p] = category(int(mask_at[p]), seq[p]) * 32 + c
    return bins


def strand_tricounts(seq, seg_start, seg_mask):
    """int64[4, 32] of himut_strand_tricounts."""
    b = _position_bins(seq, seg_start, seg_mask)
    return np.bincount(b[b >= 0], minlength=128).reshape(4, 32)


def strand_callable(state, bases, chunks, seq, seg_start, seg_mask):
    """(positions, bases), int64[4, 32] each, of himut_strand_callable: ``state`` / ``bases`` are the callable run's map,
    the entries of ``chunks`` one behind the other."""
    at = np.concatenate([np.arange(s, e, dtype=np.int64) for s, e in chunks] + [np.zeros(0, np.int64)])
    assert at.shape[0] == state.shape[0] == bases.shape[0]
    b = _position_bins(seq, seg_start, seg_mask)[at]
    take = (b >= 0) & (np.asarray(state) == CALLABLE)
    pos = np.bincount(b[take], minlength=128)
    nb = np.bincount(b[take], weights=np.asarray(bases, np.float64)[take], minlength=128)
    return pos.reshape(4, 32).astype(np.int64), np.rint(nb).astype(np.int64).reshape(4, 32)
