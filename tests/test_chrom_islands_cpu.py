"""The premise of tests/test_gpu_chrom_coords.py, without a GPU: the plain-Python models of the indels, indelcal,
germline, dbs and sites runs compose (tests/chrom_islands.py).  For the islands the GPU tests plant in a contig of chr1's
length, composed here at small offsets of different block phases: model(composite) is the translated sum of
model(island alone in its padding) -- record bytes, counters, table -- with the islands' own regions and, for the two
indel runs, under the one region (0, length) and with the regions of the first islands left out; all islands with padding
behind the last, and the last place's islands with the last one ending at the contig's last position.  (The composites of
the indel runs stay under 90 kb; the twelve 20 kb samples of the other three make one of 250 kb, which their models walk
read by read in a few seconds.)  Then the conditions on the inputs the GPU tests rely on, on the very records they expect at
chr1's coordinates: every place contributes.

The islands, the parameter sets and the per-island model results (computed once, left unchanged) are shared with the GPU
tests from here."""
import functools
import random

import numpy as np
import pytest

from tests import chrom_islands as I
from tests import dbs_model as D
from tests import germline_model as G
from tests import indelcal_model as K
from tests import indels_model as M
from tests import sites_model as S

RUNS = ("indels", "indelcal", "germline", "dbs", "sites")
PER_PLACE = dict(indels=6, indelcal=6, germline=3, dbs=3, sites=3)
FIELD = dict(indels="anchor", indelcal=None, germline="tpos", dbs="tpos", sites="tpos")
INDELS_KW = dict(min_alt_count=1, report_homref=True, min_gq=0, max_len=50)           # the rounds' own are not used
INDELCAL_KW = dict(min_mapq=0, max_len=50, min_alt_count=2, vaf_permille=250)
INDEL_SEEDS = tuple(range(3000, 3024))
SNV_SEEDS = tuple(range(9100, 9111)) + (9112,)       # the last: a dbs record within 3,000 of its end
PHASES = (0, 77, 255, 130, 1, 201)           # of the padded origins in the small composites


def _snv_sample(seed):
    from tests.test_gpu_germline import _sample
    return _sample(seed, 20_000, depth=8.0, sub_rate=5e-3).batch


def _site_list(b, seed):
    """The substitutions the reads carry plus as many triples they do not, every position inside the span of the reads, as
    (pos1, ref, alt, set): every seventh site is in the first site set (1), every seventh in the second (2)."""
    from tests.test_sites_cpu import read_substitutions
    real = read_substitutions(b)
    lo, hi = int(b.tstart.min()) + 1, int(b.tend.max())
    rs, decoys = random.Random(seed), set()
    while len(decoys) < len(real):
        p, r, a = rs.randrange(lo, hi + 1), rs.choice("ATGC"), rs.choice("ATGC")
        if r != a and (p, r, a) not in real:
            decoys.add((p, r, a))
    return [s + ({0: 1, 3: 2}.get(k % 7, 0),) for k, s in enumerate(sorted(real | decoys))]


@functools.lru_cache(maxsize=None)
def islands(run):
    """The islands of a run, in the order they are planted: (batch, regions or sites, contig string or None)."""
    if run == "indels":
        from tests.test_indels_cpu import random_round
        return tuple(random_round(seed)[:3] for seed in INDEL_SEEDS)
    if run == "indelcal":
        from tests.test_indelcal_cpu import SEEDS, random_round
        return tuple(random_round(seed)[:3] for seed in SEEDS[:24])
    if run == "sites":
        return tuple((b, _site_list(b, 40 + k), None) for k, (b, _r, _n) in enumerate(islands("germline")))
    if run == "dbs":
        return islands("germline")
    assert run == "germline"
    return tuple((b, [(1, b.length)], None) for b in map(_snv_sample, SNV_SEEDS))


def site_keys(sites):
    """The keys of the two site sets of a site list (pos1, ref, alt, set): pos << 4 | ref << 2 | alt."""
    key = lambda s: (s[0] << 4) | (S.BASES.index(s[1]) << 2) | S.BASES.index(s[2])           # noqa: E731
    return sorted(key(s) for s in sites if s[3] == 1), sorted(key(s) for s in sites if s[3] == 2)


def model(run, batch, regions, ref):
    """(records or table, log) of a run's model under the parameters every island and composite is run with."""
    if run == "indels":
        return M.run(batch, regions, ref, **INDELS_KW)
    if run == "indelcal":
        return K.run(batch, regions, ref, **INDELCAL_KW)
    if run == "germline":
        return G.run(batch, regions)
    if run == "dbs":
        from tests.test_dbs_cpu import SAMPLE_KW
        return D.run(batch, regions, **SAMPLE_KW)
    from tests.test_sites_cpu import SAMPLE_KW
    pon, com = site_keys(regions)
    return S.run(batch, [s[:3] for s in regions], pon_keys=pon, com_keys=com, **SAMPLE_KW)


@functools.lru_cache(maxsize=None)
def island_part(run, k, right, mode):
    """The model on island k alone inside its padding (right: the N behind it, 0 for a last island at the contig's end)
    under its own regions, under the one region (0, padded length) ("whole"), or under none ("none": what its reads add
    to the counters when no region holds them)."""
    b, regions, ref = I.isolated(islands(run)[k], I.PAD, right)
    return model(run, b, {"own": regions, "whole": [(0, b.length)], "none": []}[mode], I.letters(ref))


def want(run, offsets, last_at_end, whole=False, ks=None, without=()):
    """What a composite of the run's islands (ks: of these of them) at these offsets must give; without: the islands whose
    regions are left out."""
    ks = list(range(len(islands(run)))) if ks is None else list(ks)
    assert len(ks) == len(offsets)
    mode = lambda k: "none" if k in without else "whole" if whole else "own"           # noqa: E731
    parts = [island_part(run, k, 0 if last_at_end and k == ks[-1] else I.PAD, mode(k)) + (int(o) - I.PAD,) for k, o in zip(ks, offsets)]
    return I.expected(parts, FIELD[run], "site" if run == "sites" else None)


SITE_KINDS = {"PASS", "LowBQ", "Germline", "PanelOfNormal", "ComSnp"}      # the site sets are looked up and decide


def site_kinds(recs):
    return {S.STATUS[int(s)] for s in recs["status"]}


def assert_same(run, got, got_log, wanted, wanted_log):
    {"indels": M, "indelcal": K, "germline": G, "dbs": D, "sites": S}[run].assert_same(got, got_log, wanted, wanted_log)


def small_layout(run, ks, last_at_end):
    """(offsets, length) of islands ks: the padded origins one behind the other, each at its own phase of a 256-position
    block."""
    offsets, end = [], 0
    for k in ks:
        isl = islands(run)[k]
        origin = ((end + 256) & ~255) + PHASES[k % len(PHASES)]
        offsets.append(origin + I.PAD)
        end = offsets[-1] + I.island_length(isl) + I.PAD
    return offsets, end - I.PAD if last_at_end else end


def later_regions(run, ks, offsets, without):
    """The regions of a composite of islands ks without those of the islands in `without`."""
    return [(s + o, e + o) for k, o in zip(ks, offsets) if k not in without for s, e in islands(run)[k][1]]


def chr1_offsets(run):
    lengths = [I.island_length(isl) for isl in islands(run)]
    n = PER_PLACE[run]
    return I.place([lengths[k * n:(k + 1) * n] for k in range(len(I.SITES_CHR1))])


def check_places(run, recs, offsets):
    """Conditions on the inputs: records of every place -- in the first group, on both sides of 2^24 and of 2^27 inside
    the island that lies across it, and within 3,000 of the contig's end."""
    pos = np.asarray(recs[FIELD[run]], np.int64)
    n = PER_PLACE[run]
    lengths = [I.island_length(isl) for isl in islands(run)]
    assert np.count_nonzero(pos < offsets[n - 1] + lengths[n - 1] + I.PAD) > 0
    for g, at in ((1, 1 << 24), (2, 1 << 27)):
        k = g * n + n // 2
        assert offsets[k] < at < offsets[k] + lengths[k]
        assert np.count_nonzero((pos >= offsets[k] - 1) & (pos < at)) > 0 and np.count_nonzero((pos > at) & (pos <= offsets[k] + lengths[k])) > 0, (run, at)
    assert np.count_nonzero(pos > 1 << 24) > 0 and np.count_nonzero(pos > 1 << 27) > 0 and np.count_nonzero(pos > I.CHR1 - 3000) > 0
    assert int(pos.max()) <= I.CHR1 and np.all(np.diff(pos) >= 0)


# ---- the helper

def test_place_puts_the_groups_where_it_says():
    for run in RUNS:
        offs = chr1_offsets(run)
        n = PER_PLACE[run]
        lengths = [I.island_length(isl) for isl in islands(run)]
        assert len(offs) == 4 * n == len(lengths) and offs == sorted(offs)
        assert offs[0] == I.PAD                                                     # the first padding starts at 0
        for g, at, phase in ((1, 1 << 24, 77), (2, 1 << 27, 255)):
            k = g * n + n // 2
            assert offs[k] < at < offs[k] + lengths[k] and (offs[k] - I.PAD) % 256 == phase
        assert offs[-1] + lengths[-1] == I.CHR1
        assert all(offs[k] + lengths[k] + I.PAD < offs[k + 1] - I.PAD for k in range(len(offs) - 1))
        assert len({(o - I.PAD) % 256 for o in offs}) > n                           # many block phases


def test_compose_moves_what_it_must():
    isl = islands("indels")[:3]
    offs = [I.PAD + 77, 9_000, 20_001]
    b, regions, ref = I.compose(isl, offs, 30_000)
    assert b.n == sum(x[0].n for x in isl) and b.length == 30_000 and ref.shape == (30_000,) and ref.dtype == np.uint8
    r0 = 0
    for (x, regs, letters), o in zip(isl, offs):
        for i in (0, x.n - 1):
            j = r0 + i
            assert (int(b.tstart[j]), int(b.tend[j])) == (int(x.tstart[i]) + o, int(x.tend[i]) + o)
            assert b.query_sequence(j) == x.query_sequence(i) and b.cs_tag(j) == x.cs_tag(i) and int(b.qid[j]) == int(x.qid[i]) + r0
            assert np.array_equal(b.query_qualities(j), x.query_qualities(i)) and int(b.qoff[j]) % 32 == 0
        assert ref[o:o + x.length].tobytes().decode() == letters and chr(ref[o - 1]) == "N" == chr(ref[o + x.length])
        r0 += x.n
    assert regions == [(s + o, e + o) for (x, regs, _l), o in zip(isl, offs) for s, e in regs]
    assert int(np.count_nonzero(ref != ord("N"))) == sum(len(x[2]) - x[2].upper().count("N") for x in isl)
    for bad in ([I.PAD - 1, 9_000, 20_001], [I.PAD, 9_000, 9_000 + isl[1][0].length + 2 * I.PAD], [I.PAD, 9_000, 30_000 - isl[2][0].length - 1]):
        with pytest.raises(AssertionError):
            I.compose(isl, bad, 30_000)
    I.compose(isl, [I.PAD, 9_000, 30_000 - isl[2][0].length], 30_000)                # the last island may end at the end


def test_expected_moves_and_sums():
    a = np.zeros(2, S.SITE_RECORD_DTYPE)
    a["tpos"], a["site"] = [5, 9], [0, 1]
    recs, log = I.expected([(a, [1, 2], 1000), (a, [10, 20], 100)], "tpos", "site")
    assert list(recs["tpos"]) == [105, 109, 1005, 1009] and list(recs["site"]) == [0, 1, 2, 3] and log == [11, 22]
    assert list(a["tpos"]) == [5, 9]
    t, log = I.expected([(np.ones((2, 2), np.int64), [1], 0), (np.ones((2, 2), np.int64), [2], 7)], None)
    assert t.tolist() == [[2, 2], [2, 2]] and log == [3]


# ---- the premise

@pytest.mark.parametrize("last_at_end", (False, True), ids=("padded_end", "last_at_end"))
@pytest.mark.parametrize("run", RUNS)
def test_models_compose(run, last_at_end):
    """Every island with padding behind the last; the last place's islands with the last one ending at the contig's end."""
    n = len(islands(run))
    ks = list(range(n - PER_PLACE[run], n) if last_at_end else range(n))
    offsets, length = small_layout(run, ks, last_at_end)
    b, regions, ref = I.compose([islands(run)[k] for k in ks], offsets, length)
    assert len({(o - I.PAD) % 256 for o in offsets}) == min(len(ks), len(PHASES))
    assert (offsets[-1] + I.island_length(islands(run)[ks[-1]]) == length) == last_at_end
    assert_same(run, *model(run, b, regions, I.letters(ref)), *want(run, offsets, last_at_end, ks=ks))
    if run in ("indels", "indelcal"):
        assert_same(run, *model(run, b, [(0, length)], I.letters(ref)), *want(run, offsets, last_at_end, whole=True, ks=ks))
        first = set(ks[:2])                                      # the regions begin behind the first islands
        assert_same(run, *model(run, b, later_regions(run, ks, offsets, first), I.letters(ref)),
                    *want(run, offsets, last_at_end, ks=ks, without=first))


# ---- the inputs of the GPU tests

@pytest.mark.parametrize("run", RUNS)
def test_every_place_contributes(run):
    offsets = chr1_offsets(run)
    n = PER_PLACE[run]
    if run == "indelcal":                                        # no records: every place counts runs, spans and events
        for whole in (False, True):
            for g in range(4):
                t, log = I.expected([island_part(run, k, 0 if k == 4 * n - 1 else I.PAD, "whole" if whole else "own") + (0,) for k in range(g * n, (g + 1) * n)], None)
                d = K.check_invariants(t, log)
                assert d["runs"] > 100 and d["spans"] > 100 and d["events_counted"] > 10, (g, d)
        assert int(want(run, offsets, True)[0].sum()) > 10_000
        return
    for whole in ((False, True) if run == "indels" else (False,)):
        recs, log = want(run, offsets, True, whole)
        check_places(run, recs, offsets)
        if run == "indels":
            assert log[0] >= 1000 and len(recs) >= 1000, (log, len(recs))
        if run == "sites":
            assert len(recs) > 10_000 and SITE_KINDS <= site_kinds(recs), site_kinds(recs)
            for g in range(4):                                   # ... in every place
                lo, hi = offsets[g * n] - I.PAD, offsets[g * n + n - 1] + 20_000 + I.PAD
                assert {"PanelOfNormal", "ComSnp"} <= site_kinds(recs[(recs["tpos"] >= lo) & (recs["tpos"] < hi)]), g
    print(run, len(recs), log)
