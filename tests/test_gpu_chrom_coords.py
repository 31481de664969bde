"""The added runs at chromosome-scale coordinates: indels, indelcal, germline, dbs and sites on a contig of chr1's length
(248,956,422) against their plain-Python models, by composition (tests/chrom_islands.py).  Small inputs the models handle
-- islands -- are planted at four places: from position 0, across 2^24 at block phase 77, across 2^27 at block phase 255,
and up to the contig's last position; everything between them is N and holds no read.  The device runs once on the whole
contig; what it must give is each island's model records with the position moved by the island's offset, in offset order,
and the sums of the counters and tables (tests/test_chrom_islands_cpu.py holds the models to that and checks that every
place contributes records).  Anchors and tpos need up to 28 bits here, the indel events' sort 35.

One test per run, one composite per test; every test prints its wall times."""
import time

import numpy as np
import pytest

from tests import chrom_islands as I
from tests import test_chrom_islands_cpu as T

pytestmark = pytest.mark.gpu

PARAM_NAMES = ("min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq", "min_bq", "max_mismatch_count",
               "mismatch_window_size", "md_threshold", "min_ref_count", "min_alt_count", "min_hap_count", "min_sequence_identity",
               "min_trim")


class _Clock:
    def __init__(self, name):
        self.name, self.t, self.laps = name, time.perf_counter(), []

    def lap(self, what):
        now = time.perf_counter()
        self.laps.append("{} {:.2f}s".format(what, now - self.t))
        self.t = now

    def show(self):
        print(self.name + ": " + ", ".join(self.laps))


def _composite(run):
    """(batch, regions or sites, the reference as bytes or None, offsets) of the run's islands at chr1's four places."""
    offsets = T.chr1_offsets(run)
    b, regions, ref = I.compose(T.islands(run), offsets, I.CHR1, name="chr1")
    return b, regions, None if ref is None else ref.tobytes(), offsets


def _set_reference(c, run, raw):
    """The 249 Mb string as bytes; its classes from the islands' letters (everything else is N)."""
    from himut_amd.normcounts import tri_classes
    chars, cls = tri_classes("".join(isl[2] for isl in T.islands(run)) + "N")
    assert len(raw) == I.CHR1
    c.set_reference(raw, cls, len(chars))


def _configure(c, kw, pon=(), com=()):
    """The call parameters, the genotype tables and the two site sets, as the dbs and sites tests set them."""
    from himut_amd import gtlib
    from tests import dbs_model as D
    p = dict(D.DEFAULTS, **kw)
    c.set_params(**{k: p[k] for k in PARAM_NAMES})
    c.set_gt_lut(*gtlib.build_tables(1 / (10 ** 3)))
    c.set_site_set(0, np.array(sorted(pon), np.uint64))
    c.set_site_set(1, np.array(sorted(com), np.uint64))


def test_indels():
    """Twenty-four random rounds, six a place, under one parameter set: the islands' own regions (48 of them), then the
    one region (0, chr1) on the same pushed reads.  Equal record bytes and counters."""
    from himut_amd import _ffi
    clock = _Clock("indels")
    b, regions, raw, offsets = _composite("indels")
    clock.lap("compose")
    with _ffi.Context(0) as c:
        _set_reference(c, "indels", raw)
        c.push_reads(b)
        clock.lap("upload")
        for whole in (False, True):
            want, wlog = T.want("indels", offsets, True, whole)
            clock.lap("model")
            c.set_chunks([(0, I.CHR1)] if whole else regions)
            c.run_indels(**T.INDELS_KW)
            got, glog = c.indels()
            clock.lap("run")
            print("indels, one region" if whole else "indels, own regions", len(got), glog)
            T.assert_same("indels", got, glog, want, wlog)
            T.check_places("indels", got, offsets)
            assert glog[0] >= 1000 and len(got) >= 1000
    clock.show()


def test_indelcal():
    """Twenty-four random rounds, six a place: with the islands' regions most of the 972,486 blocks of the span sweep are
    dead; with (0, chr1) every block is live, the sweep walks the whole chromosome and the N between the islands must not
    count as runs; with the regions of the first place left out the sweep's first block is the 65,000th or so, and the first
    place's reads add to the counters in front of the regions alone.  Equal tables and counters, and the table's
    invariants."""
    from himut_amd import _ffi
    from tests import indelcal_model as K
    clock = _Clock("indelcal")
    b, regions, raw, offsets = _composite("indelcal")
    clock.lap("compose")
    with _ffi.Context(0) as c:
        _set_reference(c, "indelcal", raw)
        c.push_reads(b)
        clock.lap("upload")
        first = set(range(T.PER_PLACE["indelcal"]))
        later = T.later_regions("indelcal", range(len(offsets)), offsets, first)
        assert min(s for s, _e in later) > 1 << 23 and len(later) < len(regions)
        for name, chunks, kw in (("own regions", regions, {}), ("one region", [(0, I.CHR1)], dict(whole=True)),
                                 ("regions behind the first place", later, dict(without=first))):
            want, wlog = T.want("indelcal", offsets, True, **kw)
            clock.lap("model")
            c.set_chunks(chunks)
            c.run_indelcal(**T.INDELCAL_KW)
            got, glog = c.indelcal()
            clock.lap("run")
            print("indelcal,", name, int(got.sum()), glog)
            T.assert_same("indelcal", got, glog, want, wlog)
            d = K.check_invariants(got, glog)
            assert d["runs"] > 1000 and d["spans"] > 1000 and d["events_counted"] > 100
    clock.show()


def test_germline():
    """Twelve 20 kb samples, three a place, under the run's defaults: tpos through the shared record back end."""
    from himut_amd import _ffi, gtlib
    clock = _Clock("germline")
    b, regions, _raw, offsets = _composite("germline")
    want, wlog = T.want("germline", offsets, True)
    clock.lap("compose and model")
    with _ffi.Context(0) as c:
        c.set_gt_lut(*gtlib.build_tables(1 / (10 ** 3)))
        c.set_chunks(regions)
        c.push_reads(b)
        c.run_germline()
        got, glog = c.germline()
    clock.lap("run")
    print("germline", len(got), glog)
    T.assert_same("germline", got, glog, want, wlog)
    T.check_places("germline", got, offsets)
    clock.show()


def test_dbs():
    """The same samples under the parameters of the dbs sample, empty site sets: the proposal keys tpos << 8 | ..."""
    from himut_amd import _ffi
    from tests.test_dbs_cpu import SAMPLE_KW
    clock = _Clock("dbs")
    b, regions, _raw, offsets = _composite("dbs")
    want, wlog = T.want("dbs", offsets, True)
    clock.lap("compose and model")
    with _ffi.Context(0) as c:
        _configure(c, SAMPLE_KW)
        c.set_chunks(regions)
        c.push_reads(b)
        c.run_dbs()
        got, glog = c.dbs()
    clock.lap("run")
    print("dbs", len(got), glog)
    T.assert_same("dbs", got, glog, want, wlog)
    T.check_places("dbs", got, offsets)
    clock.show()


def test_sites():
    """The same samples; every island's sites are the substitutions its reads carry and as many decoys, all inside the
    span of its reads, every seventh in the first site set and every seventh in the second: the keys pos << 4 | ref << 2
    | alt of sites and sets at 28-bit positions."""
    from himut_amd import _ffi
    from tests.test_sites_cpu import SAMPLE_KW
    clock = _Clock("sites")
    b, sites, _raw, offsets = _composite("sites")
    want, wlog = T.want("sites", offsets, True)
    clock.lap("compose and model")
    pon, com = T.site_keys(sites)
    assert len(sites) == len(want) > 10_000 and len(pon) > 1000 and len(com) > 1000
    with _ffi.Context(0) as c:
        _configure(c, SAMPLE_KW, pon, com)
        c.push_reads(b)
        c.run_sites(np.array([s[0] for s in sites], np.int32), "".join(s[1] for s in sites).encode(), "".join(s[2] for s in sites).encode())
        got, glog = c.sites()
    clock.lap("run")
    print("sites", len(got), glog)
    T.assert_same("sites", got, glog, want, wlog)
    T.check_places("sites", got, offsets)
    assert T.SITE_KINDS <= T.site_kinds(got)
    clock.show()
