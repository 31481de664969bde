"""Chunk geometry the uniform phase blocks of the other tests never build: a heavy-tailed phase-set layout (one long block,
hundreds of one-to-three-hetSNP blocks, interleaved pairs), chunks at the edges of the 256-position tiles and 1024-position
workgroup tiles, zero-length and overlapping chunks, chunks that touch the contig's first and last positions (the NNN
trinucleotide key), the list overflow and pool paths on such chunks, reuse of one context across shapes, the 65,535-chunk
limit, and a chromosome-sized contig whose longest phase block is megabases.  normcounts and the call run against the CPU
oracle, bit for bit; the sweep's device scratch against a bound by the positions the chunks hold."""
import os
import tempfile

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

ORDER = {"A": ["T", "G", "C"], "T": ["C", "A", "G"], "G": ["A", "C", "T"], "C": ["G", "T", "A"]}
HIMUT_ERR_ARG = 1                  # include/himut_hip.h
CALL_FIELDS = ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum")


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _fresh():
    from himut_amd.caller import Worker
    return Worker(0)


def _configure(worker, p, phase):
    worker.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"],
                     p["min_sequence_identity"], p["min_gq"], p["min_bq"], p["min_trim"], p["max_mismatch_count"],
                     p["mismatch_window_size"], p["md_threshold"], p["min_ref_count"], p["min_alt_count"],
                     p["min_hap_count"], p["germline_snv_prior"], phase)


def scratch_bound(chunks):
    """What the sweep may hold on the device: 64 B per position the chunks hold, 4 KB per chunk, 32 MB."""
    return 64 * sum(max(e - s, 0) for s, e in chunks) + 4096 * len(chunks) + (32 << 20)


def _phased(s, ids):
    from himut_amd import synth, vcflib
    b = s.batch
    with tempfile.TemporaryDirectory() as d:
        pv = os.path.join(d, "p.vcf")
        synth.write_phased_vcf(pv, s, block_ids=ids)
        hb, hp, hs, c2c = vcflib.load_phased_hetsnps(pv, [b.name], {b.name: b.length})
    phase_sets = (dict(hb[b.name]), dict(hp[b.name]), dict(hs[b.name]))
    return [(c[1], c[2]) for c in c2c[b.name]], phase_sets


def _n_het(s):
    return int(((s.snp_gt == 1) | (s.snp_gt == 2)).sum())


class Case:
    pass


@pytest.fixture(scope="module")
def skewed():
    """About 1.2 Mb at 25x with the heavy-tailed phase layout of synth.skewed_blocks; the oracle's answers computed once."""
    from oracle import oracle as O
    from himut_amd import synth, util as hutil
    c = Case()
    c.s = synth.generate(synth.SynthConfig(seed=61, contig_len=1_200_000, depth=25.0, name="chrK"), want_ref=True)
    c.b = c.s.batch
    c.refseq = bytes(c.s.ref)
    c.chunks, c.phase_sets = _phased(c.s, synth.skewed_blocks(_n_het(c.s), 61))
    c.uniform = [(x[1], x[2]) for x in hutil.chunkloci((c.b.name, 0, c.b.length))]
    c.p = dict(util.CALL_DEFAULTS)
    c.p.update(qlen_lower_limit=9000, qlen_upper_limit=22500, md_threshold=52)
    span = sorted(e - s for s, e in c.chunks)
    assert len(c.chunks) > 150 and span[-1] > 500_000 and span[len(span) // 2] < 5_000 and span[0] == 0
    assert any(a[0] < b[0] < a[1] for a in c.chunks for b in c.chunks if a != b), "no interleaved blocks"
    het_last = int(c.s.snp_pos[(c.s.snp_gt == 1) | (c.s.snp_gt == 2)].max())
    assert max(e for _, e in c.chunks) == het_last + 1          # (VCF positions: one-based)
    c.o_norm = {}
    for key, chunks, ph in (("phase", c.chunks, c.phase_sets), ("nophase", c.chunks, None), ("uniform", c.uniform, None)):
        c.o_norm[key] = O.normcounts(c.b, chunks, c.p, c.refseq, c.p["germline_snv_prior"], alt_order=ORDER, phase=ph)
    assert c.o_norm["phase"][2][2] > 0 and c.o_norm["phase"][2][13] > 0
    return c


def _norm(w, c, key, **dbg):
    """normcounts of one of the skewed case's chunk lists on `w`, against the oracle; returns the run's stats."""
    from himut_amd import normcounts
    chunks, ph = {"phase": (c.chunks, c.phase_sets), "nophase": (c.chunks, None), "uniform": (c.uniform, None)}[key]
    _configure(w, c.p, ph is not None)
    if dbg:
        w.ctx.debug_normcounts(**dbg)
    try:
        got = normcounts.norm_contig(w, c.b, chunks, c.refseq, alt_order=ORDER, phase_sets=ph)
        st = w.ctx.stats()
    finally:
        w.ctx.debug_normcounts()
    o_ccs, o_ref, o_log = c.o_norm[key]
    assert got[2] == o_log
    assert got[0] == o_ccs and got[1] == o_ref
    return st


def _call_parity(w, b, chunks, p, phase_sets, oracle_result=None):
    from oracle import oracle as O
    orecs, olog = oracle_result or O.call(b, chunks, p, p["germline_snv_prior"], None, None, phase_sets)
    _configure(w, p, phase_sets is not None)
    recs, log = w.call_contig(b, chunks, None, None, phase_sets)
    assert log == olog
    assert len(recs) == len(orecs)
    for name in CALL_FIELDS:
        if name in recs.dtype.names and name in orecs.dtype.names:
            assert np.array_equal(recs[name], orecs[name]), name
    return recs


# ---- 1. skewed phase blocks on a small contig

def test_skewed_blocks_normcounts_and_scratch_bound(skewed):
    """The sweep's plan, left-over list and tile list are laid out by each chunk's own tiles: the scratch follows the
    positions, not (chunks x longest chunk), which for this layout was about 250 times the bound."""
    w = _fresh()
    try:
        _norm(w, skewed, "phase")
        sc = w.ctx.norm_scratch()
        assert sc[3] == sc[0] + sc[1] + sc[2] and min(sc[:3]) > 0
        assert sc[3] <= scratch_bound(skewed.chunks), sc
        _norm(w, skewed, "nophase")
        assert w.ctx.norm_scratch()[3] <= scratch_bound(skewed.chunks)
    finally:
        w.close()


def test_skewed_blocks_call_phase(worker, skewed):
    """The same chunks through the call run: k_read_hap's grid takes (most reads under a chunk) x chunks."""
    recs = _call_parity(worker, skewed.b, skewed.chunks, skewed.p, skewed.phase_sets)
    assert len(recs) > 100


# ---- 3. the overflow and pool paths on skewed chunks

def test_skewed_blocks_left_over_list_overflows(skewed):
    """A left-over list of one entry per part: the sweep is repeated once and is exact; the next run on the context is
    exact and the scratch bound still holds (a part that overflowed only under the test's cap raises no room)."""
    w = _fresh()
    try:
        st = _norm(w, skewed, "phase", dirty_cap=1)
        assert st["reran"] == 1
        st = _norm(w, skewed, "phase")
        assert st["reran"] == 0
        assert w.ctx.norm_scratch()[3] <= scratch_bound(skewed.chunks)
    finally:
        w.close()


def test_skewed_blocks_pool_runs_out(worker, skewed):
    """One pool slot per wave: the tiles go to k_norm_tile through the tile list, no repeat of the contig."""
    st = _norm(worker, skewed, "phase", pool_slots=1)
    assert st["reran"] == 0 and st["column_slots"] > 0


# ---- 4. one context across shapes

def test_one_context_across_chunk_shapes(skewed):
    """uniform -> skewed -> uniform -> skewed with phase on one context: what one run leaves in the plan and the lists
    does not reach the next."""
    w = _fresh()
    try:
        for key in ("uniform", "nophase", "uniform", "phase"):
            _norm(w, skewed, key)
    finally:
        w.close()


# ---- 2. tile and window edges

def _edge_batch(seed, L):
    """Reads of test_gpu_edge_reads' kinds over an L-position contig, and perfect reads that start at 0 or end at L."""
    from himut_amd.readbatch import batch_from_records
    from tests.test_gpu_edge_reads import BASES, _make_read
    rs = np.random.RandomState(seed)
    ref = "".join(BASES[i] for i in rs.randint(0, 4, L))
    recs = []
    while len(recs) < 560:
        kind = ["plain", "short", "clip", "trailins"][int(rs.randint(0, 4))]
        target = int(rs.randint(400, 1900)) if kind == "short" else int(rs.randint(3000, 16000))
        r = _make_read(rs, ref, int(rs.randint(0, L - 500)), target, kind)
        if r is not None:
            recs.append(r)
    for k in range(8):
        n = 4000 + 700 * k
        for a in (0, L - n):
            recs.append(dict(tstart=a, tend=a + n, qstart=0, seq=ref[a:a + n], bq=np.full(n, 60, np.uint8),
                             cs=":{}".format(n), mapq=60))
    recs.sort(key=lambda r: r["tstart"])
    for i, r in enumerate(recs):
        r["qname"] = "m/{}/ccs".format(i)
    return batch_from_records("chrG", L, recs), ref.encode("ascii")


def _edge_chunks(L):
    lengths = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385]
    chunks, pos = [(0, 700)], 2000
    for i, n in enumerate(lengths):
        s = (pos // 256 + 1) * 256 + (1, 128, 255)[i % 3]
        chunks.append((s, s + n))
        pos = s + n + 300
    chunks += [(pos, pos + 777), (pos + 777, pos + 2001)]                            # touching
    chunks += [(pos + 3000, pos + 9000), (pos + 5000, pos + 7000), (pos + 8000, pos + 12_100)]   # overlapping
    chunks.append((L - 900, L))
    assert pos + 12_100 < L - 900
    return chunks


@pytest.fixture(scope="module")
def edges():
    from oracle import oracle as O
    from tests.test_gpu_edge_reads import _params
    c = Case()
    c.L = 300_000
    c.b, c.refseq = _edge_batch(71, c.L)
    c.chunks = _edge_chunks(c.L)
    c.p = _params(min_trim=0.0, min_bq=30, min_gq=5, min_ref_count=2, md_threshold=60)
    c.o = O.normcounts(c.b, c.chunks, c.p, c.refseq, c.p["germline_snv_prior"], alt_order=ORDER)
    assert c.o[0].get("NNN", 0) > 0 and c.o[1].get("NNN", 0) == 2
    return c


@pytest.mark.parametrize("sweep", [0, 1])
def test_tile_edges_normcounts(worker, edges, sweep):
    """Chunk lengths 0 .. 16,385 around the tile sizes, starts at 1, 128 and 255 modulo 256, touching and overlapping
    chunks, [0, x) and [y, L): the quad sweep and k_norm_tile both equal the oracle, the NNN key of the contig's ends
    included."""
    from himut_amd import normcounts
    _configure(worker, edges.p, False)
    worker.ctx.debug_normcounts(sweep=sweep)
    try:
        ccs, rf, log = normcounts.norm_contig(worker, edges.b, edges.chunks, edges.refseq, alt_order=ORDER)
    finally:
        worker.ctx.debug_normcounts()
    o_ccs, o_ref, o_log = edges.o
    assert "NNN" in ccs and "NNN" in rf and ccs["NNN"] == o_ccs["NNN"] and rf["NNN"] == o_ref["NNN"]
    assert log == o_log
    assert ccs == o_ccs and rf == o_ref


def test_tile_edges_call(worker, edges):
    """The same chunks through the call run."""
    _call_parity(worker, edges.b, edges.chunks, edges.p, None)


# ---- 5. the chunk-count limit

@pytest.fixture(scope="module")
def many():
    """A 1 Mb contig of short reads at 3x with a hetSNP every ~12 positions: one phase set per hetSNP (zero-length
    chunks)."""
    from himut_amd import synth
    c = Case()
    c.s = synth.generate(synth.SynthConfig(seed=81, contig_len=1_000_000, depth=3.0, snp_rate=0.12, read_len_mean=3000.0,
                                           read_len_sd=500.0, read_len_min=2000, read_len_max=4000, name="chrM"),
                         want_ref=True)
    c.b = c.s.batch
    c.refseq = bytes(c.s.ref)
    n = _n_het(c.s)
    assert n > 65_536
    c.chunks, c.phase_sets = _phased(c.s, np.where(np.arange(n) < 65_535, np.arange(n), -1))
    c.over, c.over_sets = _phased(c.s, np.where(np.arange(n) < 65_536, np.arange(n), -1))
    assert len(c.chunks) == 65_535 and len(c.over) == 65_536
    c.p = dict(util.CALL_DEFAULTS)        # (reads with a hetSNP every ~12 bases pass only loose filters)
    c.p.update(qlen_lower_limit=1000, qlen_upper_limit=40000, md_threshold=52, min_sequence_identity=0.5,
               max_mismatch_count=1000, min_gq=0, min_ref_count=1, min_hap_count=1)
    return c


def test_chunk_limit_normcounts(worker, many):
    """65,535 chunks of zero or one position equal the oracle; 65,536 are refused with the message, and the context still
    runs a valid contig afterwards."""
    from oracle import oracle as O
    from himut_amd import _ffi, normcounts
    b, p = many.b, many.p
    one = [(s, s + (k & 1)) for k, (s, _) in enumerate(many.chunks)]
    o_one = O.normcounts(b, one, p, many.refseq, p["germline_snv_prior"], alt_order=ORDER)
    o_ph = O.normcounts(b, many.chunks, p, many.refseq, p["germline_snv_prior"], alt_order=ORDER, phase=many.phase_sets)
    assert o_one[2][13] > 0
    for chunks, ph, o in ((one, None, o_one), (many.chunks, many.phase_sets, o_ph)):
        _configure(worker, p, ph is not None)
        got = normcounts.norm_contig(worker, b, chunks, many.refseq, alt_order=ORDER, phase_sets=ph)
        assert got[2] == o[2] and got[0] == o[0] and got[1] == o[1]
    _configure(worker, p, False)
    with pytest.raises(_ffi.HimutError) as e:
        normcounts.norm_contig(worker, b, [(s, s + 1) for s, _ in many.over], many.refseq, alt_order=ORDER)
    assert e.value.code == HIMUT_ERR_ARG and "65,535 chunks" in e.value.message
    got = normcounts.norm_contig(worker, b, one, many.refseq, alt_order=ORDER)
    assert got[2] == o_one[2] and got[0] == o_one[0] and got[1] == o_one[1]


def test_chunk_limit_call_phase(worker, many):
    """--phase call on 65,535 one-hetSNP phase sets equals the oracle; 65,536 are refused; the context goes on."""
    from oracle import oracle as O
    from himut_amd import _ffi
    b, p = many.b, many.p
    o = O.call(b, many.chunks, p, p["germline_snv_prior"], None, None, many.phase_sets)
    _call_parity(worker, b, many.chunks, p, many.phase_sets, o)
    _configure(worker, p, True)
    with pytest.raises(_ffi.HimutError) as e:
        worker.call_contig(b, many.over, None, None, many.over_sets)
    assert e.value.code == HIMUT_ERR_ARG and "65,535 chunks" in e.value.message
    _call_parity(worker, b, many.chunks, p, many.phase_sets, o)


# ---- 6. chromosome-like, full size

def test_chromosome_skewed_phase_full_size():
    """A chr20-sized contig at 30x whose phase sets are one block of about 5 Mb and thousands of short or interleaved
    blocks: normcounts --phase on the whole contig (before the sweep was laid out by each chunk's tiles it asked for
    more device memory than the card has), the counters add up, the scratch bound holds, and a window of chunks around
    the long block equals the oracle on the reads under it."""
    from oracle import oracle as O
    from himut_amd import bamlib, normcounts, synth
    from tests.test_gpu_fullsize import _reads_for, _sub_batch
    L = 64_444_167
    s = synth.generate(synth.SynthConfig(seed=2, contig_len=L, name="chr20"), want_ref=True)
    b = s.batch
    refseq = bytes(s.ref)
    het = (s.snp_gt == 1) | (s.snp_gt == 2)
    hpos = s.snp_pos[het]
    inside = hpos < 16_000_000
    ids = np.full(hpos.shape[0], -1, np.int64)
    ids[inside] = synth.skewed_blocks(int(inside.sum()), 5, big=5_000_000 / 16_000_000)
    chunks, phase_sets = _phased(s, ids)
    span = [e - st for st, e in chunks]
    long_k = int(np.argmax(span))
    assert span[long_k] > 4_000_000 and len(chunks) > 1_000
    ql, qu, md = bamlib.get_thresholds({b.name: b}, [b.name], {b.name: b.length})
    p = dict(util.CALL_DEFAULTS)
    p.update(qlen_lower_limit=ql, qlen_upper_limit=qu, md_threshold=md)
    w = _fresh()
    try:
        _configure(w, p, True)
        ccs, rf, log = normcounts.norm_contig(w, b, chunks, refseq, alt_order=ORDER, phase_sets=phase_sets)
        assert log[1] == log[2] + log[3] + log[4] + log[5] + log[6]
        assert log[6] == sum(log[7:14])
        assert sum(ccs.values()) == log[13] and log[13] > 100_000_000 and log[2] > 0
        assert w.ctx.norm_scratch()[3] <= scratch_bound(chunks)
        # the long block and the short blocks around it (the ten chunks that start before it, the ten after)
        order = sorted(range(len(chunks)), key=lambda k: chunks[k][0])
        at = order.index(long_k)
        win = [chunks[k] for k in sorted(order[max(at - 10, 0):at + 11])]
        lo, hi = min(c[0] for c in win), max(c[1] for c in win)
        win = [c for c in chunks if c[0] >= lo and c[1] <= hi]
        sub = _sub_batch(b, _reads_for(b, win))
        o_ccs, o_ref, o_log = O.normcounts(sub, win, p, refseq, p["germline_snv_prior"], alt_order=ORDER, phase=phase_sets)
        h_ccs, h_ref, h_log = normcounts.norm_contig(w, sub, win, refseq, alt_order=ORDER, phase_sets=phase_sets)
        assert h_log == o_log and h_ccs == o_ccs and h_ref == o_ref
    finally:
        w.close()
