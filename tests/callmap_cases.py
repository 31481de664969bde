"""Hand-built contigs for the callable run (himut_run_callable): builders only, used by tests/test_callmap_cpu.py and
tests/test_gpu_callmap.py.  Nothing is drawn at run time but the contig's letters, and those are seeded.

``boundary_scene`` places reads so that the states change where the kernels can go wrong: at a tile boundary of the map
sweep, at a block boundary of the run compaction, at every position of more than a whole compaction block, across
several blocks without a change, and over more than 100,000 positions without a base."""
import random
from collections import namedtuple

from himut_amd.readbatch import batch_from_records
from tests.callable_cases import BASE
from tests.germline_model import make_read

Scene = namedtuple("Scene", "ref batch chunks params notes")
CONTIG = "chrM1"


def random_ref(seed, length):
    rs = random.Random(seed)
    return "".join(rs.choice("ACGT") for _ in range(length))


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


def params(**kw):
    p = dict(BASE, min_bq=30)
    p.update(kw)
    return p


def stack(ref, start, length, depth, name, **kw):
    return [make_read(ref, start, length, qname="{}/{}".format(name, k), **kw) for k in range(depth)]


def boundary_scene(tile=256, block=2048):
    """Chunks and reads around the sweep's tile (``tile`` positions of a chunk) and the compaction's block (``block``
    entries of the map).  notes: name -> (chunk index, first position, last position + 1) of what a test looks at."""
    length = 150_000
    ref = random_ref(20260, length)
    recs, notes = [], {}
    # ---- chunk 0: start 37, length 5 blocks + 300: neither a multiple of 256.  Its first map entry is entry 0, so entry i
    #      is position 37 + i.
    c0 = 37
    len0 = 5 * block + 300
    #   island A: from a tile boundary of the chunk (entry 2 * tile) to a block boundary of the map (entry block)
    recs += stack(ref, c0 + 2 * tile, block - 2 * tile, 10, "A")
    notes["tile_edge"] = (0, c0 + 2 * tile - 1, c0 + 2 * tile + 1)
    notes["block_edge"] = (0, c0 + block - 1, c0 + block + 1)
    #   island B: one state over more than three blocks, four bases a position (the scan's int64 carry)
    b_start, b_len = c0 + block + 52, 3 * block + 404
    recs += stack(ref, b_start, b_len, 4, "B")
    notes["long_run"] = (0, b_start, b_start + b_len)
    # ---- chunk 1: every other base of its reads has a quality under min_bq: CALLABLE, NO_BASE, CALLABLE ... over more than
    #      two blocks of the map, so that a whole block holds nothing but runs of one position
    c1 = 20_011
    len1 = 2 * block + 517
    low = {p: 20 for p in range(c1 + 1, c1 + len1, 2)}
    recs += stack(ref, c1, len1, 4, "ALT", bq_at=low)
    notes["alternating"] = (1, c1, c1 + len1)
    # ---- chunks 2, 3, 4: shorter than a tile; one position; both under one stack of reads (equal state at the seams)
    c2 = 30_000
    recs += stack(ref, c2 - 10, 400, 5, "S")
    notes["seam"] = (2, c2, c2 + 102)
    # ---- chunk 5: a deep pile (more rows than one LDS batch of the sweep) beside a shallow one, with a het, a hetalt, a
    #      homalt, an insertion and a deletion in it; then 103,000 positions without a read; then another island
    c5 = 40_000
    deep = []
    for k in range(120):
        subs = {}
        if k % 2 == 0:
            subs[c5 + 100] = other(ref[c5 + 100])                        # het
        subs[c5 + 200] = other(ref[c5 + 200], 1 + (k % 2))               # hetalt
        subs[c5 + 300] = other(ref[c5 + 300], 2)                         # homalt
        deep.append(make_read(ref, c5, 600, subs=subs, ins={c5 + 400: "AC"} if k == 7 else None,
                              dels={c5 + 500: 3} if k == 9 else None, qname="D/{}".format(k)))
    recs += deep
    recs += stack(ref, c5 + 600, 400, 3, "shallow")
    recs += stack(ref, c5 + 104_000, 1000, 6, "far", subs={c5 + 104_500: other(ref[c5 + 104_500])})
    notes["deep"] = (5, c5, c5 + 600)
    notes["no_base"] = (5, c5 + 1000, c5 + 104_000)
    chunks = [(c0, c0 + len0), (c1, c1 + len1), (c2, c2 + 100), (c2 + 100, c2 + 101), (c2 + 101, c2 + 102),
              (c5, c5 + 105_000)]
    recs.sort(key=lambda r: r["tstart"])
    # the reference string with an N and a lower-case stretch inside island A (the reads keep their letters): NON_ACGT
    # between covered positions
    masked = ref[:1000] + "N" + ref[1001:1010] + ref[1010:1014].lower() + ref[1014:]
    notes["non_acgt"] = (0, 1000, 1014)
    return Scene(masked, batch_from_records(CONTIG, length, recs), chunks, params(), notes)


def hetalt_scene():
    """A small contig whose piles reach HETALT (no golden normcounts case does) beside HET, HOMALT and CALLABLE."""
    length = 3000
    ref = random_ref(4, length)
    recs = []
    for k in range(12):
        subs = {1200: other(ref[1200], 1 + (k % 2)), 1300: other(ref[1300])}
        if k % 2:
            subs[1400] = other(ref[1400], 3)
        recs.append(make_read(ref, 1000, 900, subs=subs, qname="H/{}".format(k)))
    return Scene(ref, batch_from_records(CONTIG, length, recs), [(900, 2000)], params(), {"hetalt": 1200, "homalt": 1300, "het": 1400})
