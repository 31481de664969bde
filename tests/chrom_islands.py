"""Islands: small inputs the plain-Python models handle, planted at chosen offsets in one long contig.

The models of the added runs (tests/indels_model.py, indelcal_model.py, germline_model.py, dbs_model.py, sites_model.py)
cannot run on a chromosome: they walk strings and reads in Python.  Their results compose, though.  An island is
(batch, regions, contig string or None); between the islands the reference is N and no read lies there.  The records of
the composite are each island's records with the position field moved by the island's offset, behind one another in
offset order, and the counters and tables are the element-wise sums -- provided each island is modelled alone inside the
N padding it has in the composite (isolated), so that "no position in front", "the run reaches the end of the string" and
the stops of the left shift mean the same in both.  tests/test_chrom_islands_cpu.py holds the models to that; then
tests/test_gpu_chrom_coords.py compares the device, on a contig of chr1's length, with the translated sums.

Plain numpy; nothing of the device side."""
import numpy as np

from himut_amd.readbatch import ReadBatch

CHR1 = 248_956_422
PAD = 300                    # N on each side of an island; at least 81 (the span sweep of indelcal looks 80 ahead)
GAP = 1_013                  # between the padded spans of one place (odd: the block phases differ)

# The four places of the chr1-length composites: (kind, boundary, origin mod 256).  The origin is the padded one.
#   start     the first island's padding begins at position 0
#   straddle  the middle island of the group lies across the boundary, its padded origin at the given phase of a block
#   end       the last island ends at the contig's last position (no padding behind it)
SITES_CHR1 = (("start", 0, 0), ("straddle", 1 << 24, 77), ("straddle", 1 << 27, 255), ("end", CHR1, None))

_PER_READ = ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "tp")


def island_length(island):
    return int(island[0].length)


def place(groups, sites=SITES_CHR1, pad=PAD, gap=GAP):
    """The offsets (of each island's first letter) of len(sites) groups of island lengths, flat and in group order."""
    assert len(groups) == len(sites)
    out = []
    for lengths, (kind, at, phase) in zip(groups, sites):
        lengths = [int(n) for n in lengths]
        offs = [0] * len(lengths)
        if kind == "start":
            k, offs[0] = 0, at + pad
        elif kind == "straddle":
            k = len(lengths) // 2
            n = lengths[k]
            assert n // 2 > 256 and n - n // 2 > 256, n
            s = at - n // 2
            s -= ((s - pad) - phase) % 256
            assert s < at < s + n and (s - pad) % 256 == phase
            offs[k] = s
        else:
            assert kind == "end"
            k = len(lengths) - 1
            offs[k] = at - lengths[k]
        for i in range(k + 1, len(lengths)):                     # to the right of the fixed island
            offs[i] = offs[i - 1] + lengths[i - 1] + 2 * pad + gap
        for i in range(k - 1, -1, -1):                           # to its left
            offs[i] = offs[i + 1] - 2 * pad - gap - lengths[i]
        out += offs
    return out


def _moved(item, o):
    """A region (start, end) or a site (pos1, ref, alt, ...) of an island at offset o."""
    if len(item) == 2:
        return (int(item[0]) + o, int(item[1]) + o)
    return (int(item[0]) + o,) + tuple(item[1:])


def compose(islands, offsets, length, pad=PAD, name="chrC"):
    """(ReadBatch, regions, reference as uint8 array or None) of the islands planted at the offsets in a contig of the
    given length.  An island's second member is its list of regions (start, end) or, for the sites run, of sites
    (pos1, ref, alt, ...): the positions move.  The last island may end at the contig's last position; every other padded span
    lies inside the contig and no two of them touch."""
    assert len(islands) == len(offsets) > 0
    offsets = [int(o) for o in offsets]
    spans = [(o, o + island_length(isl)) for isl, o in zip(islands, offsets)]
    for k, (s, e) in enumerate(spans):
        assert s - pad >= 0, (k, s)
        if k + 1 < len(spans):
            assert e + pad < spans[k + 1][0] - pad, (k, e, spans[k + 1][0])     # neither the islands nor their padding touch
        else:
            assert e + pad <= length or e == length, (k, e, length)
    with_ref = [isl[2] is not None for isl in islands]
    assert all(with_ref) or not any(with_ref)
    ref = np.full(length, ord("N"), np.uint8) if all(with_ref) else None
    arrays = {k: [] for k in _PER_READ + ("qid", "qoff", "cs_off", "seq", "bq", "cs")}
    regions = []
    n_reads = n_bases = n_cs = 0
    for (b, regs, letters), o in zip(islands, offsets):
        b.validate()
        total = (b.bq.shape[0] + 31) & ~31                       # the next island's qoff stays a multiple of 32
        assert b.seq.shape[0] * 2 <= total
        for k in _PER_READ:
            a = getattr(b, k)
            arrays[k].append(a + np.int32(o) if k in ("tstart", "tend") else a)
        arrays["qid"].append(b.qid + np.int32(n_reads))
        arrays["qoff"].append(b.qoff + np.int64(n_bases))
        arrays["cs_off"].append(b.cs_off[:-1] + np.int64(n_cs))
        arrays["seq"] += [b.seq, np.zeros(total // 2 - b.seq.shape[0], np.uint8)]
        arrays["bq"] += [b.bq, np.zeros(total - b.bq.shape[0], np.uint8)]
        arrays["cs"].append(b.cs)
        assert int(b.cs_off[-1]) == b.cs.shape[0]
        n_reads, n_bases, n_cs = n_reads + b.n, n_bases + total, n_cs + b.cs.shape[0]
        regions += [_moved(r, o) for r in regs]
        if ref is not None:
            raw = np.frombuffer(letters.encode("ascii") if isinstance(letters, str) else bytes(letters), np.uint8)
            assert raw.shape[0] == b.length
            ref[o:o + b.length] = raw
    arrays["cs_off"].append(np.array([n_cs], np.int64))
    cat = {k: np.ascontiguousarray(np.concatenate(v)).astype(getattr(islands[0][0], k).dtype, copy=False) for k, v in arrays.items()}
    out = ReadBatch(name=name, length=int(length), qnames=None, **cat)
    out.validate()
    assert out.n == n_reads and int(out.tend.max(initial=0)) <= length
    return out, regions, ref


def isolated(island, left=PAD, right=PAD):
    """The island alone inside its padding: `left` N in front of it, `right` behind it (0 for a composite's last island,
    whose end is the contig's)."""
    assert left > 0 and (right == 0 or right > 0)
    return compose([island], [left], left + island_length(island) + right, pad=min(left, right) if right else left)


def letters(ref):
    """The reference of a small composite as the str the models take."""
    return None if ref is None else ref.tobytes().decode("ascii")


def expected(parts, field, index=None):
    """What the composite must give.  parts: (records or table, log, shift) per island, the shift being what its `field`
    ("anchor" or "tpos") moves by.  Records: each island's with the field moved, in shift order behind one another; index
    names a field that numbers the input items (the site of a site record), which moves by the records in front.  Tables
    (plain arrays, field None) and the counters are summed."""
    parts = sorted(parts, key=lambda p: p[2])
    log = [int(sum(int(x) for x in col)) for col in zip(*(p[1] for p in parts))]
    if field is None:
        return sum(np.asarray(p[0], np.int64) for p in parts), log
    out, done = [], 0
    for recs, _log, shift in parts:
        r = recs.copy()
        r[field] += shift
        if index is not None:
            r[index] += done
        done += len(r)
        out.append(r)
    return np.concatenate(out), log
