"""The device-side BAM ingest (k_bam_decode, k_bam_scatter, k_bam_advance behind bamio.BamStream.ingest_contig) against
a parser written from the SAM/BAM specification (tests/bam_spec.py), on records our own writer never emits
(tests/bam_zoo.py), and on files that must be refused: the device path raises what the host parser raises, and the
context ingests on afterwards."""
import numpy as np
import pytest

from tests import bam_spec as S
from tests import bam_zoo as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def zoo_dir(tmp_path_factory):
    d = tmp_path_factory.getbasetemp() / "bam_zoo"
    d.mkdir(exist_ok=True)
    return str(d)


def _ingest_equals(worker, st, want, window):
    ctx = worker.ctx
    res = st.ingest_contig(ctx, want.name, window_bytes=window)
    assert (res["n_reads"], res["bases_padded"], res["cs_bytes"]) == (want.n, want.bq.shape[0], want.cs.shape[0])
    assert res["read_bases"] == want.read_bases()
    assert res["n_missing_cs"] == res["n_unsorted"] == res["n_malformed"] == 0
    Z.same_batch(ctx.download_reads(res, want.name, want.length), want)
    ts, te, qlen, mapq, tp = ctx.ingest_read_meta(res["n_reads"])
    for got, k in ((ts, "tstart"), (te, "tend"), (qlen, "qlen"), (mapq, "mapq"), (tp, "tp")):
        assert np.array_equal(got, getattr(want, k)), k


@pytest.mark.parametrize("window", Z.WINDOWS)
def test_zoo_device_parse_equals_spec_parser(worker, zoo_dir, window):
    """Every contig, in any order, one twice; before them a larger contig of all-N bases, all-255 qualities and '~' cs
    text through the same context, so that padding and masked bytes the kernels fail to write are not zero by luck."""
    from himut_amd import bamio
    path, parsed, _ = Z.cached("zoo", zoo_dir)
    stale_path, stale, _ = Z.cached("stale", zoo_dir)
    st0 = bamio.BamStream(stale_path, threads=3)
    _ingest_equals(worker, st0, stale.batches["stale"], 1 << 20)
    st0.close()
    st = bamio.BamStream(path, threads=3)
    assert not st.indexed and st.sample() == parsed.sample() and st.tname2tsize == parsed.tname2tsize
    for name in ("zooC", "zooA", "zooEmpty", "zooA"):
        _ingest_equals(worker, st, parsed.batches[name], window)
    st.close()


def test_windows_of_very_short_records_on_the_device(worker, zoo_dir):
    """The file of tests/test_bam_records_cpu.py::test_stream_takes_windows_of_very_short_records: far more records in a
    1 MB window than window_bytes / 64."""
    from himut_amd import bamio
    path, _, (pos, flag) = Z.cached("short", zoo_dir)
    want = S.parse(path).batches["short"]
    assert want.n == pos.shape[0] and np.array_equal(want.tstart, pos) and np.array_equal(want.flag, flag)
    st = bamio.BamStream(path, threads=8)
    _ingest_equals(worker, st, want, 1 << 20)
    st.close()


def _good_again(worker, zoo_dir):
    """After a refused file the same context ingests a good contig byte for byte and counts a FASTA."""
    from himut_amd import bamio
    path, parsed, _ = Z.cached("zoo", zoo_dir)
    st = bamio.BamStream(path, threads=3)
    _ingest_equals(worker, st, parsed.batches["zooC"], 64 << 10)
    st.close()
    assert int(worker.ctx.fasta_tricounts(b"ACGT\n").sum()) == 2


@pytest.mark.parametrize("case", sorted(Z.ERROR_CASES))
def test_device_path_refuses_what_the_spec_parser_refuses(worker, zoo_dir, tmp_path, case):
    from himut_amd import bamio
    from himut_amd._ffi import HimutError
    kind, make = Z.ERROR_CASES[case]
    path = str(tmp_path / (case + ".bam"))
    make(path)
    st = bamio.BamStream(path, threads=3)
    want = Z.expected_error(case, device=True)
    if kind is None:
        _ingest_equals(worker, st, S.parse(path).batches["errc"], 64 << 10)
    else:
        with pytest.raises(want[0]) as e:
            st.ingest_contig(worker.ctx, "errc", window_bytes=64 << 10)
        assert want[1] in str(e.value)
        assert not isinstance(e.value, HimutError) or e.value.code == 1          # HIMUT_ERR_ARG
        # the refused ingest is closed: the process's pinned windows are free for this context's FASTA count and for
        # another context's ingest at once, before any other ingest here and with the refused stream still open
        assert int(worker.ctx.fasta_tricounts(b"ACGT\n").sum()) == 2
        from himut_amd.caller import Worker
        other = Worker(0)
        try:
            other.ctx.ingest_begin(0, 1 << 16)
            other.ctx.ingest_end(True)
        finally:
            other.close()
        with pytest.raises(Z.expected_error(case, device=False)[0]):              # the host parser: the same class, or its
            bamio.BamFile(path)                                                   # ValueError for the device's HIMUT_ERR_ARG
    st.close()
    _good_again(worker, zoo_dir)


@pytest.mark.parametrize("case", sorted(Z.STRAY_CASES))
def test_stray_bytes_behind_the_last_tag_device_agrees_with_host(worker, zoo_dir, tmp_path, case):
    from himut_amd import bamio
    path = str(tmp_path / (case + ".bam"))
    Z.STRAY_CASES[case](path)
    host = bamio.BamFile(path).batches["errc"]
    assert host.n == Z.ERR_N
    st = bamio.BamStream(path, threads=3)
    res = st.ingest_contig(worker.ctx, "errc", window_bytes=64 << 10)
    Z.same_batch(worker.ctx.download_reads(res, "errc", host.length), host)
    st.close()
