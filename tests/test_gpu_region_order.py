"""A region list out of start order, with two overlapping regions and one nested in another, through the three runs that
build the regions-by-start table (sorted_regions, himut_ctx.hip): the germline run (through the chunk tables), the bqcal
run and the indels run.  Germline and indel records are a matter of which positions the list holds, so the list in any
order gives the records of the sorted list; bqcal counts a position once per region that holds it, a sum that no order
changes.  Each result equals the plain-Python model of the run on the same list."""
import numpy as np
import pytest

from tests import bqcal_model as BM
from tests import germline_model as GM
from tests import indels_model as IM

pytestmark = pytest.mark.gpu

N = 4000
# out of start order; (600, 1400) and (1200, 1900) overlap, (700, 900) lies inside (600, 1400)
REGIONS = [(2500, 3200), (600, 1400), (1200, 1900), (700, 900), (3900, 3950), (100, 300)]
SUBS = (150, 800, 1300, 2000, 2600, 3000)       # one in the nested region, one in the overlap, one outside every region
INS, DEL = (1250, "TA"), (2700, 3)
PRIOR = 1 / (10 ** 3)


def _read(ref, start, end, carrier):
    """A read over ref[start:end]; a carrier holds every event of its span."""
    events = {}
    if carrier:
        events.update({p: "sub" for p in SUBS if start + 5 <= p < end - 5})
        events.update({p: kind for p, kind in ((INS[0], "ins"), (DEL[0], "del")) if start + 5 <= p < end - 5})
    seq, cs, p = [], [], start
    for pos in sorted(events):
        if pos > p:
            seq.append(ref[p:pos])
            cs.append(":{}".format(pos - p))
            p = pos
        if events[pos] == "sub":
            alt = "ACGT"[("ACGT".index(ref[pos]) + 1) % 4]
            seq.append(alt)
            cs.append("*{}{}".format(ref[pos].lower(), alt.lower()))
            p = pos + 1
        elif events[pos] == "ins":
            seq.append(INS[1])
            cs.append("+" + INS[1].lower())
        else:
            cs.append("-" + ref[pos:pos + DEL[1]].lower())
            p = pos + DEL[1]
    seq.append(ref[p:end])
    cs.append(":{}".format(end - p))
    s = "".join(seq)
    return dict(tstart=start, tend=end, qstart=0, seq=s, bq=[93] * len(s), cs="".join(cs))


@pytest.fixture(scope="module")
def pile():
    """(batch, contig string): fourteen reads in four stacks over a 4 kb contig, every other read a carrier."""
    from himut_amd.readbatch import batch_from_records
    rs = np.random.RandomState(11)
    ref = "".join("ACGT"[k] for k in rs.randint(0, 4, N))
    # the insertion and the deletion where they cannot shift: no repeat of their bases beside them
    ref = ref[:INS[0] - 3] + "CAGCAG" + ref[INS[0] + 3:]
    ref = ref[:DEL[0] - 3] + "CAGTTCA" + ref[DEL[0] + 4:]
    assert len(ref) == N
    spans = [(0, 1600)] * 4 + [(1000, 2600)] * 4 + [(2200, 3900)] * 4 + [(3000, 4000)] * 2
    recs = [_read(ref, s, e, k % 2 == 0) for k, (s, e) in enumerate(spans)]
    return batch_from_records("chrR", N, sorted(recs, key=lambda r: r["tstart"])), ref


@pytest.fixture(scope="module")
def ctx(pile):
    from himut_amd import _ffi, bamio, gtlib
    b, ref = pile
    c = _ffi.Context(0)
    c.set_gt_lut(*gtlib.build_tables(PRIOR))
    bamio.set_contig_reference(c, ref)
    c.push_reads(b)
    yield c
    c.close()


def test_germline(ctx, pile):
    b, _ref = pile
    kw = dict(min_gq=0, min_bq=1, min_ref_count=0, min_alt_count=0)
    out = []
    for regions in (REGIONS, sorted(REGIONS)):
        ctx.set_chunks(regions)
        ctx.run_germline(**kw)
        got, glog = ctx.germline()
        want, wlog = GM.run(b, regions, PRIOR, **kw)
        GM.assert_same(got, glog, want, wlog)
        out.append((got.tobytes(), glog))
    assert out[0] == out[1]
    # the substitutions inside the list, each once (the one at 2000 lies in no region), in position order
    assert [int(t) for t in got["tpos"]] == [p + 1 for p in SUBS if p != 2000]


def test_bqcal(ctx, pile):
    b, ref = pile
    out = []
    for regions in (REGIONS, sorted(REGIONS)):
        ctx.set_chunks(regions)
        ctx.run_bqcal(min_gq=0)
        match, mismatch, log = ctx.bqcal()
        wmatch, wmismatch, wlog = BM.run(b, ref, regions, PRIOR, min_gq=0)
        assert log == [int(x) for x in wlog]
        assert np.array_equal(match, wmatch) and np.array_equal(mismatch, wmismatch)
        out.append((match.tobytes(), mismatch.tobytes(), log))
    assert out[0] == out[1]
    assert log[0] == sum(e - s for s, e in REGIONS) and match.sum() > 10_000


def test_indels(ctx, pile):
    b, ref = pile
    kw = dict(min_alt_count=1, report_homref=True)
    out = []
    for regions in (REGIONS, sorted(REGIONS)):
        ctx.set_chunks(regions)
        ctx.run_indels(**kw)
        got, glog = ctx.indels()
        want, wlog = IM.run(b, regions, ref, **kw)
        IM.assert_same(got, glog, want, wlog)
        out.append((got.tobytes(), glog))
        assert ctx.stats()["positions"] == sum(e - s + 1 for s, e in REGIONS)
    assert out[0] == out[1]
    assert [(int(r["anchor"]), int(r["type"]), int(r["len"])) for r in got] == [(INS[0] - 1, 1, 2), (DEL[0] - 1, 0, 3)]
