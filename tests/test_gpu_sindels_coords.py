"""The sindels run at chromosome-scale coordinates: the indels run's islands (tests/chrom_islands.py, twenty-four random
rounds, six a place) at the four places of SITES_CHR1 on a contig of chr1's length, under this run's parameters.  The
device runs once on the whole contig per region list; what it must give is each island's model records with the anchor
moved by the island's offset, in offset order, and the sums of the counters (tests/test_sindels_cpu.py holds the model to
that).  tests/test_gpu_chrom_coords.py is the pattern."""
import pytest

from tests import chrom_islands as I
from tests import sindels_model as S
from tests import test_chrom_islands_cpu as T
from tests import test_sindels_cpu as SC
from tests.test_gpu_chrom_coords import _composite, _set_reference

pytestmark = pytest.mark.gpu


def test_sindels():
    from himut_amd import _ffi
    b, regions, raw, offsets = _composite("indels")
    with _ffi.Context(0) as c:
        _set_reference(c, "indels", raw)
        c.push_reads(b)
        for whole in (False, True):
            want, wlog = SC.want(offsets, True, whole)
            c.set_chunks([(0, I.CHR1)] if whole else regions)
            c.run_sindels(**SC.ISLAND_KW)
            got, glog = c.sindels()
            print("sindels, one region" if whole else "sindels, own regions", len(got), S.logd(glog))
            S.assert_same(got, glog, want, wlog)
            T.check_places("indels", got, offsets)
            d = S.logd(glog)
            assert d["candidates"] >= 500 and len(got) >= 500 and d["num_germ_het"] > 0
            assert set(int(x) for x in got["status"]) >= {S.ST_PASS, S.ST_INDEL, S.ST_REPEAT}
