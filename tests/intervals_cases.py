"""Scenes and interval lists for the intervals run (himut_run_intervals): builders only, used by
tests/test_intervals_cpu.py, tests/test_gpu_intervals.py and tests/test_gpu_intervals_cli.py.  Every scene's map and
model are computed once per process and left unchanged."""
import functools
import random
from collections import namedtuple

from himut_amd.readbatch import batch_from_records
from tests import callmap_cases as C
from tests import callmap_model as M
from tests import intervals_model as IM
from tests.germline_model import make_read

TILE, BLOCK = 256, 2048                     # HIMUT_CALLMAP_TILE, HIMUT_CALLMAP_BLOCK (a slice of the tally)
Case = namedtuple("Case", "scene res map")
UNORDERED_CHUNKS = [(1500, 2000), (900, 1700), (0, 50)]


def _case(sc, chunks=None):
    sc = sc if chunks is None else sc._replace(chunks=chunks)
    res = M.run(sc.batch, sc.ref, sc.chunks, sc.params)
    return Case(sc, res, IM.Map.of(res, sc.ref))


@functools.lru_cache(maxsize=None)
def boundary():
    return _case(C.boundary_scene(TILE, BLOCK))


@functools.lru_cache(maxsize=None)
def hetalt():
    return _case(C.hetalt_scene())


@functools.lru_cache(maxsize=None)
def hetalt_unordered():
    """The hetalt contig under chunks that are neither ascending nor disjoint: 1500..1699 lie in two of them."""
    return _case(C.hetalt_scene(), UNORDERED_CHUNKS)


@functools.lru_cache(maxsize=None)
def string_ends():
    """One chunk (0, length) with reads over both ends of the string."""
    length = 700
    ref = C.random_ref(77, length)
    recs = C.stack(ref, 0, 400, 6, "L") + C.stack(ref, 300, 400, 6, "R")
    recs.sort(key=lambda r: r["tstart"])
    sc = C.Scene(ref, batch_from_records(C.CONTIG, length, recs), [(0, length)], C.params(), {})
    return _case(sc)


def span_of(chunks):
    return min(s for s, _e in chunks), max(e for _s, e in chunks)


def partition(lo, hi, seed, pieces):
    """[lo, hi) cut at ``pieces - 1`` seeded places (places may coincide: empty intervals), in ascending order."""
    rs = random.Random(seed)
    cuts = sorted([lo, hi] + [rs.randint(lo, hi) for _ in range(pieces - 1)])
    return list(zip(cuts[:-1], cuts[1:]))


def steps(lo, hi, width):
    return [(a, min(a + width, hi)) for a in range(lo, hi, width)]


def boundary_intervals():
    """The interval list of the GPU test on boundary_scene, in the order the issue of Row 14 lists it (the test shuffles
    it): where a span, a slice or a vector load of the tally can go wrong."""
    sc = boundary().scene
    c0 = sc.chunks[0][0]
    out = []
    for off in range(16):                                    # every start alignment x every short length: 656
        for n in range(41):
            out.append((c0 + 2 * TILE + off, c0 + 2 * TILE + off + n))
    for first in (c0, c0 + 5):                               # chunk 0's first entry (entry 0) and an odd entry
        for S in (64, 256, 2048, 4096):
            for n in (S - 1, S, S + 1):
                out.append((first, first + n))
    c2 = sc.chunks[2][0]
    out.append((c2 - 7, c2 + 150))                           # across chunks 2, 3 and 4
    _c, a, _b = sc.notes["no_base"]
    out.append((a - 3, sc.chunks[5][1] + 11))                # the long NO_BASE stretch and the island behind it
    _c, a, b = sc.notes["non_acgt"]
    out.append((a, b))
    lo, hi = span_of(sc.chunks)
    out.append((lo, hi))                                     # all chunks
    out.append((sc.chunks[0][1] + 10, sc.chunks[1][0] - 10))   # between chunks
    out.append((5000, 4000))                                 # start > end
    out.append((-1000, len(sc.ref) + 1000))                  # below 0 and beyond the contig
    out += [(c0 + 100, c0 + 3000)] * 3                       # three times the same
    out += [(c0 + 50, c0 + 9000), (c0 + 60, c0 + 5000), (c0 + 70, c0 + 71)]   # nested
    return out
