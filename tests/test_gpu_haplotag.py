"""The haplotag run (himut_run_haplotag / himut_get_haplotag) through the C ABI against the plain-Python model of its
contract (tests/haplotag_model.py): every row, hetSNP row and counter equal, down to the bytes.  The hand-built cases
(tests/haplotag_cases.py) name the places where the kernels can go wrong; a case at chr1-scale coordinates, two synthetic
samples with phase blocks, and sequences on one context -- what a haplotag run and the other runs leave each other, buffer
growth, bad arguments -- cover the run as a whole."""
import numpy as np
import pytest

from tests import chrom_islands as CI
from tests import haplotag_cases as C
from tests import haplotag_model as M
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _arrays(snps):
    return (np.array([s[0] for s in snps], np.int32), "".join(s[1] for s in snps).encode(), "".join(s[2] for s in snps).encode(),
            np.array([s[3] for s in snps], np.uint8), np.array([s[4] for s in snps], np.int32))


def _run(c, snps, batch=None, n_sets=None, **kw):
    if batch is not None:
        c.push_reads(batch)
    c.run_haplotag(*_arrays(snps), n_sets=n_sets, **kw)
    return c.haplotag()


def _both(c, batch, snps, push=True, **kw):
    """The run and the model on the same input: equal, and what holds of every result; returns the device's."""
    got = _run(c, snps, batch if push else None, **kw)
    want = M.haplotag(batch, snps, **kw)
    M.assert_same(got, want)
    M.check_identities(snps, *got)
    assert np.array_equal(M.depth(got[1]), M.depth(want[1]))
    return got


# ---- 1. the hand-built cases

@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_case(ctx, case):
    rows, snp_rows, _log = _both(ctx, case.batch, case.snps, **case.kw)
    C.check_expectations(case, rows, snp_rows)
    st = ctx.stats()
    assert st["n_reads"] == case.batch.n and st["n_records"] == case.batch.n and st["positions"] == len(case.snps)


def test_every_size_of_the_list(ctx):
    """The search of the sorted positions for a read's range: lists of every size from none to forty and a few hundred,
    with reads in front of, inside and behind the list (keys below, between and above every position).  The first list is
    the lanes case's own; the second packs a hetSNP into every fifth position, in slices of many sizes and places."""
    case = C.BY_NAME["lanes"]
    ctx.push_reads(case.batch)
    for n in range(len(case.snps) + 1):
        M.assert_same(_run(ctx, case.snps[:n]), M.haplotag(case.batch, case.snps[:n]))
    dense = [C.snp(950 + 5 * k, k & 1, k // 40) for k in range(320)]
    for lo, n in [(0, n) for n in (41, 255, 288, 289, 290, 306, 320)] + [(13, 17), (20, 33), (20, 34), (100, 35), (300, 20)]:
        part = dense[lo:lo + n]
        M.assert_same(_run(ctx, part), M.haplotag(case.batch, part))


def test_a_set_voted_only_by_a_read_outside_the_pile(ctx):
    case = C.BY_NAME["sets"]
    rows, snp_rows, log = _both(ctx, case.batch, case.snps)
    assert int(rows[6]["status"]) == M.NOT_IN_PILE and not np.any(rows["set"] == 4)
    assert M.depth(snp_rows)[9:].tolist() == [0, 0] and log[8] == 6      # multi_set


def test_only_assigned_reads_of_the_snps_own_set_move_agree(ctx):
    case = C.BY_NAME["agree"]
    rows, snp_rows, _ = _both(ctx, case.batch, case.snps)
    assert [int(r["set"]) for r in rows] == [0, 0, 1] and case.snps[3][4] == 1
    assert int(snp_rows[3]["n_ref"] + snp_rows[3]["n_alt"]) == 3 and int(snp_rows[3]["agree"] + snp_rows[3]["disagree"]) == 1
    # without an Assigned read nothing agrees or disagrees: at a permille of 1000 read 1 (1:5) is a Conflict
    rows, snp_rows, _ = _both(ctx, case.batch, case.snps, push=False, min_agree_permille=1000)
    assert int(rows[1]["status"]) == M.CONFLICT and int(snp_rows[0]["disagree"]) == 0 and int(snp_rows[0]["agree"]) == 1


def test_a_context_without_reads(ctx):
    """An empty batch is a valid run with zero rows; a context nothing was ever pushed to is refused, as by every run."""
    from himut_amd._ffi import Context, HimutError
    case = C.BY_NAME["no_reads"]
    rows, snp_rows, log = _both(ctx, case.batch, case.snps)
    assert rows.shape == (0,) and snp_rows.shape == (4,) and log == [0] * 13
    rows, snp_rows, log = _both(ctx, case.batch, [], push=False)
    assert rows.shape == (0,) and snp_rows.shape == (0,)
    with Context(0) as fresh, pytest.raises(HimutError) as e:
        _run(fresh, case.snps)
    assert e.value.code == 1 and "himut_push_reads" in e.value.message


# ---- 2. bad arguments

def test_bad_arguments_leave_the_context_usable(ctx):
    from himut_amd._ffi import HimutError
    case = C.BY_NAME["pile"]
    good = case.snps
    want = _both(ctx, case.batch, good, **case.kw)
    s0, s1 = good[0], good[1]
    bad_lists = [("ascending", [s1, s0]), ("ascending", [s0, s0]), ("differ", [s0[:2] + (s0[1],) + s0[3:]]),
                 ("ACGT", [(s0[0], s0[1].lower(), s0[2], 0, 0)]), ("ACGT", [(s0[0], "N", s0[2], 0, 0)]),
                 ("set", [s0[:4] + (-1,)]), ("bit", [s0[:3] + (2, 0)]), ("1-based", [(0,) + s0[1:]])]
    for word, bad in bad_lists:
        with pytest.raises(HimutError) as e:
            _run(ctx, bad, n_sets=1)
        assert e.value.code == 1 and word in e.value.message, (word, e.value.message)
        M.assert_same(ctx.haplotag(), want)                               # the last good run is still served
        M.assert_same(_run(ctx, good, **case.kw), want)                   # ... and a good run right after gives the model's bytes
    with pytest.raises(HimutError) as e:
        _run(ctx, good, n_sets=0)                                         # set >= n_sets
    assert e.value.code == 1 and "set" in e.value.message
    for word, kw in (("min_snps", dict(min_snps=0)), ("min_agree_permille", dict(min_agree_permille=500)),
                     ("min_agree_permille", dict(min_agree_permille=1001))):
        with pytest.raises(HimutError) as e:
            _run(ctx, good, **kw)
        assert e.value.code == 1 and word in e.value.message
        M.assert_same(_run(ctx, good, **case.kw), want)


# ---- 3. chr1-scale coordinates

def test_a_case_beyond_2_to_the_27(ctx):
    """The lanes case in front of 2^27, the sets case across it and the segments case at the end of a contig of chr1's
    length: the device on the composite against the model on the composite (the model walks reads, not positions)."""
    islands = [(C.BY_NAME[n].batch, C.BY_NAME[n].snps, None) for n in ("lanes", "sets", "segments")]
    o1 = (1 << 27) - C.N // 2
    offsets = [o1 - C.N - 2 * CI.PAD - CI.GAP, o1, CI.CHR1 - C.N]
    batch, moved, _ref = CI.compose(islands, offsets, CI.CHR1)
    snps, base = [], 0
    for _b, isl, _r in islands:                                          # an island's sets are numbered behind the last one's
        part = moved[len(snps):len(snps) + len(isl)]
        snps += [s[:4] + (s[4] + base,) for s in part]
        base += 1 + max(s[4] for s in isl)
    assert snps[0][0] < (1 << 27) < snps[-1][0] and snps[-1][0] > 248_000_000
    rows, snp_rows, log = _both(ctx, batch, snps)
    alone = [M.haplotag(b, s) for b, s, _ in islands]
    assert log == [sum(col) for col in zip(*(a[2] for a in alone))]
    assert rows["status"].tolist() == [int(x) for a in alone for x in a[0]["status"]]


# ---- 4. synthetic samples with phase blocks

@pytest.fixture(scope="module")
def sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=23, contig_len=60_000, depth=30.0, snp_rate=4e-3, frac_softclip=0.3,
                                            softclip_max=100))


def _phased(sample, tmp_path, **kw):
    from himut_amd import haplotag, synth
    path = str(tmp_path / "phased.vcf")
    synth.write_phased_vcf(path, sample, **kw)
    b = sample.batch
    return haplotag.load_phased(path, [b.name], {b.name: b.length})[0][b.name]


@pytest.mark.parametrize("layout", ["blocks", "skewed"])
def test_synthetic_sample(ctx, sample, tmp_path, layout):
    from himut_amd import synth
    n_het = int(np.sum((sample.snp_gt == 1) | (sample.snp_gt == 2)))
    s = _phased(sample, tmp_path, **(dict(block=25) if layout == "blocks" else dict(block_ids=synth.skewed_blocks(n_het, 7))))
    assert len(s) == n_het > 100 and len(s.names) > 3
    rows, snp_rows, log = _both(ctx, sample.batch, s.tuples())
    assert log[2] + log[3] > 0 and log[2] > 0 and log[3] > 0              # both haplotypes occur
    assert int(rows["n_sets"].max()) >= 2 and log[8] > 0
    assert int(np.max(rows["n0"] + rows["n1"])) > 16                      # reads that vote in more than one turn
    hi = _both(ctx, sample.batch, s.tuples(), push=False, min_mapq=60, min_bq=93, min_snps=3, min_agree_permille=950)
    assert 0 < hi[2][1] < log[1] and hi[2][12] > log[12]


# ---- 5. independence and reuse

def _call(c, batch, chunks, push=True):
    from himut_amd import gtlib
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=0, qlen_upper_limit=1 << 30, md_threshold=1 << 30, phase=0)
    c.set_params(**{k: v for k, v in p.items() if not k.endswith("_prior")})
    c.set_gt_lut(*gtlib.build_tables(p["germline_snv_prior"]))
    c.set_site_set(0, np.zeros(0, np.uint64)); c.set_site_set(1, np.zeros(0, np.uint64))
    c.set_chunks(chunks)
    if push:
        c.push_reads(batch)
    c.run()
    return c.records(), c.log()


def test_call_haplotag_call(ctx, sample, tmp_path):
    b = sample.batch
    snps = _phased(sample, tmp_path, block=25).tuples()
    recs, log = _call(ctx, b, [(0, b.length)])
    assert len(recs) > 0
    got = _run(ctx, snps)
    assert ctx.records().tobytes() == recs.tobytes() and ctx.log() == log      # the call run's results are still served
    again, log2 = _call(ctx, b, [(0, b.length)], push=False)
    assert again.tobytes() == recs.tobytes() and log2 == log
    M.assert_same(ctx.haplotag(), got)                                         # ... and the haplotag run's behind a call run
    M.assert_same(_run(ctx, snps), got)
    M.assert_same(got, M.haplotag(b, snps))


def test_two_runs_give_the_same_bytes_and_buffers_grow(ctx, sample, tmp_path):
    b = sample.batch
    snps = _phased(sample, tmp_path, block=25).tuples()
    small = snps[:9]
    first = _both(ctx, b, small)
    large = _both(ctx, b, snps, push=False)
    again = _run(ctx, snps)
    assert again[0].tobytes() == large[0].tobytes() and again[1].tobytes() == large[1].tobytes() and again[2] == large[2]
    M.assert_same(_run(ctx, small), first)
    # a smaller batch after a larger one, and its stats
    case = C.BY_NAME["pile"]
    _both(ctx, case.batch, case.snps, **case.kw)
    st = ctx.stats()
    assert st["n_reads"] == 5 and st["n_records"] == 5 and st["positions"] == 4 and st["read_bases"] == 1000 and st["ms_total"] > 0
