"""The dense pile (himut_pile_counts, k_pile_dense) against the oracle's, cell for cell, on one hand-built contig whose
reads take every path of the pile-tile staging (himut_amd/csrc/himut_piletile.h): a row with more pieces than the piece
list holds (the segment-list fall-back), insertions at a tile's first position, a deletion across a tile border, a
trailing insertion at a tile's first position, odd packed-base offsets, more rows than one LDS batch (PD_RB = 56) and
more reads in a tile's window than one round of the row listing takes (PD_NT = 256), and a tile whose row list is
exactly one wave of kept threads (64 reads, the other three waves list nothing).

pile_counts(p0, p1) puts its tile borders at p0 - 1 + 512 k: from 101 they are at 100, 612 and 1124."""
import random

import numpy as np
import pytest

from tests import germline_model as GM
from tests import util

pytestmark = pytest.mark.gpu

LENGTH = 4000
RANGES = ((101, 2300), (613, 700), (1, 4000), (1400, 1785))


def _batch():
    from himut_amd.readbatch import batch_from_records
    rnd = random.Random(44)
    ref = "".join(rnd.choice("ACGT") for _ in range(LENGTH))
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    recs = [GM.make_read(ref, 90 + 3 * i, 300) for i in range(8)]
    # more than four pieces in the tile from 100; insertions at 612, a tile's (and a lane's) first position
    recs.append(GM.make_read(ref, 260, 500, dels={300: 2, 320: 1, 340: 3, 360: 2}, ins={380: "A", 400: "GT", 612: "C"},
                             subs={330: other[ref[330]]}, bq=33))
    recs.append(GM.make_read(ref, 500, 250, dels={610: 4}, bq=27))           # a deletion across the border at 612
    recs.append(GM.make_read(ref, 400, 212, ins={612: "AC"}, bq=31))         # ends at 612, trailing insertion there
    recs.append(GM.make_read(ref, 700, 201, softclip=("ACG", "T"), bq=29))   # odd offsets into the packed bases
    recs += [GM.make_read(ref, 1200, 106, bq=q) for q in range(1, 61)]       # 60 rows in one tile: two batches of PD_RB
    recs += [GM.make_read(ref, 1700 + (400 * i) // 300, 40, bq=20 + i % 50) for i in range(300)]   # two rounds of PD_NT
    recs.sort(key=lambda r: r["tstart"])
    return batch_from_records("tiles", LENGTH, recs)


@pytest.fixture(scope="module")
def batch():
    return _batch()


@pytest.fixture(scope="module")
def want(batch):
    from oracle import oracle as O
    return {rng: O.pile_counts(batch, *rng) for rng in RANGES}


@pytest.fixture(scope="module")
def worker(batch):
    from himut_amd.caller import Worker
    from tests.test_gpu_parity import _configure
    w = Worker(0)
    _configure(w, dict(util.CALL_DEFAULTS, qlen_lower_limit=10, qlen_upper_limit=10000, md_threshold=1000), False)
    w.ctx.push_reads(batch)
    yield w
    w.close()


def test_fixture_reaches_every_staging_path(want, batch):
    """What the oracle says about the fixture: a change to it cannot silently drop a path."""
    # (1400, 1785) is one tile; its window is the first 64 reads of the group from 1700, and the fetch rule keeps them all
    ts, te = batch.tstart, batch.tend
    window = np.flatnonzero((ts < 1785) & (te >= 1399))
    assert len(window) == 64 and np.all(te[window] > 1400) and window[-1] - window[0] == 63
    assert int(np.maximum.accumulate(te)[window[0] - 1]) < 1399
    counts, _ = want[(101, 2300)]
    ins = counts[:, 4]
    assert int(ins.sum()) == 4 and int(ins[612 - 101]) == 2
    assert [int(x) for x in counts[610 - 101:614 - 101, 5]] == [1, 1, 1, 1]
    assert int((counts[:, :4].sum(1) + counts[:, 5]).max()) == 60


@pytest.mark.parametrize("rng", RANGES)
def test_pile_tiles_match_oracle(worker, want, rng):
    hc, hb = worker.ctx.pile_counts(*rng)
    oc, ob = want[rng]
    assert np.array_equal(hc, oc)
    assert np.array_equal(hb, ob)
