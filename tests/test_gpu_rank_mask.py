"""The call run's mask by column rank (chunks in coordinate order): the cell of (chunk k, position p) is the position's
number among the marked positions + k, a thread of k_mask_emit takes a 256-position block, a workgroup's blocks are one
tile.  Records and the 15 counters against oracle.call, bit for bit, where that layout can go wrong: positions that
chunks share, chunk edges inside and on the edges of blocks and tiles, a block with every position marked, more than
2^18 blocks (two blocks a thread), what a context keeps between runs (the zeroed mask and tile counts, the kept
capacities), and the switch to the mask by chunk cell for any other chunk list."""
import numpy as np
import pytest

from tests import chrom_islands as CI
from tests import util

pytestmark = pytest.mark.gpu

READ_LEN, STEP = 3000, 300
FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum")
P = dict(util.CALL_DEFAULTS, qlen_lower_limit=1000, qlen_upper_limit=10000, md_threshold=400)
P_DENSE = dict(P, max_mismatch_count=100)          # admits a read's substitutions that are neighbours


def _read(ref, start, end, subs):
    """A read over ref[start:end] with a substitution at each of subs (reference positions, 0-based)."""
    seq, cs, p = [], [], start
    for pos in sorted(subs):
        if pos > p:
            seq.append(ref[p:pos])
            cs.append(":{}".format(pos - p))
        alt = "ACGT"[("ACGT".index(ref[pos]) + 1) % 4]
        seq.append(alt)
        cs.append("*{}{}".format(ref[pos].lower(), alt.lower()))
        p = pos + 1
    if end > p:
        seq.append(ref[p:end])
        cs.append(":{}".format(end - p))
    s = "".join(seq)
    return dict(tstart=start, tend=end, qstart=0, seq=s, bq=[93] * len(s), cs="".join(cs))


def pile(length, subs, seed, lo=0, hi=None, name="chrM"):
    """A batch of reads of 3 kb every 300 bp over [lo, hi) of a random contig: ten deep.  Each substitution of subs
    (0-based positions) is carried by one read, the reads over it taking turns, so that it looks somatic and a read's
    own substitutions lie far apart unless the positions are neighbours."""
    from himut_amd.readbatch import batch_from_records
    rs = np.random.RandomState(seed)
    ref = "".join("ACGT"[k] for k in rs.randint(0, 4, length))
    hi = length if hi is None else hi
    spans = [(s, s + READ_LEN) for s in range(lo, hi - READ_LEN + 1, STEP)]
    carried = [[] for _ in spans]
    for i, p in enumerate(sorted(set(subs))):
        first = max(0, (p - lo - READ_LEN + 100) // STEP + 1)
        over = [k for k in range(first, min(len(spans), (p - lo) // STEP + 1)) if spans[k][0] + 100 <= p < spans[k][1] - 100]
        if over:
            carried[over[i % len(over)]].append(p)
    return batch_from_records(name, length, [_read(ref, s, e, c) for (s, e), c in zip(spans, carried)])


def in_order(chunks):
    return all(chunks[k][0] >= chunks[k - 1][1] for k in range(1, len(chunks)))


def configure(worker, p, phase=False):
    worker.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"],
                     p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"],
                     p["md_threshold"], p["min_ref_count"], p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"], phase)


def hip(worker, batch, chunks, p=P, phase_sets=None):
    configure(worker, p, phase_sets is not None)
    return worker.call_contig(batch, chunks, None, None, phase_sets)


def oracle(batch, chunks, p=P, phase_sets=None):
    from oracle import oracle as O
    return O.call(batch, chunks, p, p["germline_snv_prior"], None, None, phase_sets)


def assert_same(got, want):
    (grecs, glog), (wrecs, wlog) = got, want
    assert glog == wlog
    assert len(grecs) == len(wrecs)
    for name in FIELDS:
        assert np.array_equal(grecs[name], wrecs[name]), name


def fresh(batch, chunks, p=P):
    """The records of a context that has run nothing else."""
    from himut_amd.caller import Worker
    w = Worker(0)
    try:
        recs, log = hip(w, batch, chunks, p)
        return recs.copy(), log
    finally:
        w.close()


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


# ---- one pile of 100 kb for the cases that only differ in their chunks
N1 = 100_000
EDGE_CHUNKS = [(0, 30_000), (30_000, 60_000), (60_000, 60_000), (60_000, 90_000), (90_000, N1 - 1)]
OTHER_CHUNKS = [(1, 20_000), (20_000, 45_000), (50_000, 50_500), (50_500, N1 - 1)]
UNORDERED_CHUNKS = [(50_000, 90_000), (1000, 60_000), (59_990, 60_010), (95_000, N1 - 1)]


@pytest.fixture(scope="module")
def pile1():
    # substitutions at tpos 30,000 and 60,000 (tpos = position + 1) and next to them, and some everywhere
    subs = list(range(500, N1 - 500, 997)) + [29_998, 29_999, 30_000, 59_998, 59_999, 60_000]
    return pile(N1, subs, seed=21)


def test_shared_edge(worker, pile1):
    """Two chunks share tpos 30,000; three chunks, a one-position chunk between two others, hold tpos 60,000: the cells
    of one position are neighbours, one per chunk.  The reads over either position are fetched by all of its chunks.  The
    first chunk starts at 0."""
    assert in_order(EDGE_CHUNKS) and EDGE_CHUNKS[0][0] == 0
    want = oracle(pile1, EDGE_CHUNKS)
    assert {30_000, 60_000} <= set(int(t) for t in want[0]["tpos"]) and want[1][1] > 100
    assert_same(hip(worker, pile1, EDGE_CHUNKS), want)


@pytest.fixture(scope="module")
def block_case():
    """140 kb; chunk edges on a block edge (tpos 65,280), on a tile edge (65,536) and, chunks of 40 to 100 bp, several inside one
    block; a substitution every 37 bp around them and one at each of those edges."""
    n = 140_000
    chunks = [(1, 64_000), (64_000, 65_280), (65_280, 65_536), (65_536, 65_600)]
    rs = np.random.RandomState(5)
    while chunks[-1][1] < 67_000:
        chunks.append((chunks[-1][1], chunks[-1][1] + int(rs.randint(40, 101))))
    chunks.append((chunks[-1][1], n - 1))
    subs = list(range(63_000, 68_000, 37)) + [63_999, 65_279, 65_535, 65_599] + list(range(1000, n - 1000, 2003))
    return pile(n, subs, seed=22), chunks


def test_chunk_edges_in_blocks(worker, block_case):
    b, chunks = block_case
    assert in_order(chunks)
    inside = [k for k, (s, e) in enumerate(chunks) if s >> 8 == e >> 8]
    assert len(inside) > 10 and max(np.bincount([chunks[k][0] >> 8 for k in inside])) >= 3      # several chunks inside one block
    want = oracle(b, chunks)
    assert {64_000, 65_280, 65_536, 65_600} <= set(int(t) for t in want[0]["tpos"])
    assert_same(hip(worker, b, chunks), want)


def test_phase_block_chunks(worker):
    """--phase: the chunks are the phase blocks, two hetSNPs each at a hetSNP per 100 bp: about 100 bp wide with gaps
    between them, across the tile edge at 65,536."""
    import os
    import tempfile
    from himut_amd import synth, vcflib
    cfg = synth.SynthConfig(seed=14, contig_len=120_000, read_len_mean=5000, read_len_sd=900, read_len_min=2000, read_len_max=9000,
                            snp_rate=1e-2, het_frac=1.0, som_rate=1e-3, name="chrP")
    s = synth.generate(cfg)
    b = s.batch
    with tempfile.TemporaryDirectory() as d:
        pv = os.path.join(d, "p.vcf")
        synth.write_phased_vcf(pv, s, block=2)
        hb, hp, hs, c2c = vcflib.load_phased_hetsnps(pv, [b.name], {b.name: b.length})
    phase_sets = (dict(hb[b.name]), dict(hp[b.name]), dict(hs[b.name]))
    chunks = [(c[1], c[2]) for c in c2c[b.name]]
    widths = np.array([e - s for s, e in chunks])
    assert in_order(chunks) and len(chunks) > 300 and 30 < np.median(widths) < 150
    p = dict(P, qlen_lower_limit=2000, qlen_upper_limit=9000, md_threshold=52)
    want = oracle(b, chunks, p, phase_sets)
    assert want[1][1] > 20                                      # candidates there are
    assert_same(hip(worker, b, chunks, p, phase_sets), want)


def test_crowded_block(worker):
    """Every position of one block marked (block 40: positions 10,240 to 10,495), none in its neighbours, a few far away."""
    n = 30_000
    subs = list(range(40 * 256, 41 * 256)) + [2000, 5000, 20_000, 25_000]
    b = pile(n, subs, seed=23)
    chunks = [(1, 10_300), (10_300, n - 1)]
    want = oracle(b, chunks, P_DENSE)
    tp = set(int(t) for t in want[0]["tpos"])
    assert want[1][1] >= 256 and len(tp & set(range(40 * 256 + 1, 41 * 256 + 1))) > 200
    assert_same(hip(worker, b, chunks, P_DENSE), want)


def test_two_blocks_a_thread(worker):
    """A contig of 70 Mb has more than 2^18 blocks: a thread of the column index and of the emit takes two, a tile is 512
    blocks.  Islands of reads at the start, across a tile edge, across the edge between a thread's two blocks and at
    the end; each island's two chunks share the position in its middle, which is where the edge lies."""
    length, n = 70_000_000, 6000
    tile_edge = 300 * 512 * 256
    pair_edge = (2 * 100_000 + 1) * 256                         # between blocks 200,000 and 200,001: one thread's
    offsets = [CI.PAD, tile_edge - n // 2, pair_edge - n // 2, length - n - CI.PAD]
    subs = list(range(200, n - 200, 41)) + [n // 2 - 2, n // 2 - 1, n // 2, n // 2 + 1]
    islands = [(pile(n, subs, seed=30 + k, name="chrC"), [(100, n // 2), (n // 2, n - 100)], None) for k in range(len(offsets))]
    b, chunks, _ref = CI.compose(islands, offsets, length)
    assert ((max(int(b.tend.max()), max(e for _s, e in chunks)) >> 8) + 2) > (1 << 18) and in_order(chunks)
    want = oracle(b, chunks)
    assert {tile_edge, tile_edge + 1, pair_edge, pair_edge + 1} <= set(int(t) for t in want[0]["tpos"])
    assert_same(hip(worker, b, chunks), want)


def test_clean_state(pile1, block_case):
    """What a run leaves for the next one: the same reads three times; a shorter contig behind a longer one; other chunks
    on the same reads."""
    from himut_amd.caller import Worker
    long_b, long_chunks = block_case
    w = Worker(0)
    try:
        first = hip(w, pile1, EDGE_CHUNKS)
        first = (first[0].copy(), first[1])
        for _ in range(2):
            w.ctx.run()
            assert_same((w.ctx.records(), w.ctx.log()), first)
        assert_same(first, oracle(pile1, EDGE_CHUNKS))
        # a shorter contig behind a longer one
        hip(w, long_b, long_chunks)
        hip(w, pile1, EDGE_CHUNKS)
        assert_same(hip(w, pile1, EDGE_CHUNKS), fresh(pile1, EDGE_CHUNKS))
        # other chunks on the same reads
        hip(w, pile1, OTHER_CHUNKS)
        assert_same(hip(w, pile1, OTHER_CHUNKS), fresh(pile1, OTHER_CHUNKS))
    finally:
        w.close()


def test_kept_capacities(pile1):
    """A run on the capacities an earlier one left, with more marked positions than they hold: the run is made again with
    exact sizes, gives a fresh context's records, and the run behind it is clean."""
    from himut_amd.caller import Worker
    small = pile(20_000, [5000, 9000], seed=24)
    many = pile(N1, range(500, N1 - 500, 17), seed=25)           # some 5,800 marked positions, ten reads deep
    w = Worker(0)
    try:
        hip(w, small, [(1, 19_999)])
        hip(w, small, [(1, 19_999)])
        assert w.ctx.stats()["reran"] == 0                       # on kept capacities
        got = hip(w, many, EDGE_CHUNKS)
        assert w.ctx.stats()["reran"] == 1
        want = fresh(many, EDGE_CHUNKS)
        assert want[1][1] > 4000
        assert_same(got, want)
        assert_same(got, oracle(many, EDGE_CHUNKS))
        assert_same(hip(w, pile1, EDGE_CHUNKS), oracle(pile1, EDGE_CHUNKS))
        assert w.ctx.stats()["reran"] == 0
    finally:
        w.close()


def test_fall_back_per_run(pile1):
    """Overlapping and out-of-order chunks take the mask by chunk cell and the sort; which of the two a run takes is decided
    by its own chunks: in order, not in order, in order again on one context."""
    from himut_amd.caller import Worker
    assert not in_order(UNORDERED_CHUNKS)
    w = Worker(0)
    try:
        for chunks in (EDGE_CHUNKS, UNORDERED_CHUNKS, OTHER_CHUNKS, UNORDERED_CHUNKS, EDGE_CHUNKS):
            assert_same(hip(w, pile1, chunks), oracle(pile1, chunks))
    finally:
        w.close()
