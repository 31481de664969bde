"""The host BAM parser (bam_load_threads) and the host half of the device ingest (bam_stream_*) against a parser written
from the SAM/BAM specification (tests/bam_spec.py), on records our own writer never emits (tests/bam_zoo.py), and on
files that must be refused.  The spec parser itself is pinned on hand-written records first."""
import struct

import numpy as np
import pytest

from himut_amd import bamio
from tests import bam_spec as S
from tests import bam_zoo as Z
from tests.test_bamio import _stream_records, check_hand_packed, hand_packed_bam


@pytest.fixture(scope="module")
def zoo_dir(tmp_path_factory):
    d = tmp_path_factory.getbasetemp() / "bam_zoo"
    d.mkdir(exist_ok=True)
    return str(d)


# ---- the spec parser on records whose fields are written out here -------------------------------------------------

class _AsReadBatch:
    """query_sequence / query_qualities / cs_tag over a bam_spec.Batch, for check_hand_packed."""

    def __init__(self, b):
        self.__dict__.update(b.__dict__)

    def query_sequence(self, i):
        o, n = int(self.qoff[i]), int(self.qlen[i])
        by = self.seq[o // 2:o // 2 + (n + 1) // 2]
        nib = np.stack([by >> 4, by & 15], 1).reshape(-1)[:n]
        return "".join(S.NIBBLES[v] for v in nib)

    def query_qualities(self, i):
        return self.bq[int(self.qoff[i]):int(self.qoff[i]) + int(self.qlen[i])]

    def cs_tag(self, i):
        return self.cs[int(self.cs_off[i]):int(self.cs_off[i + 1])].tobytes().decode()


def test_spec_parser_on_the_hand_packed_record(tmp_path):
    path = str(tmp_path / "hand.bam")
    seq, qual = hand_packed_bam(path)
    p = S.parse(path)
    assert p.tname2tsize == {"ctg": 1000}
    check_hand_packed(_AsReadBatch(p.batches["ctg"]), p.sample(), seq, qual)


def test_spec_parser_on_literal_records(tmp_path):
    T = S.tag
    recs = [
        S.record(0, 100, "r1", 7, 0x10, "5H2S3M1I2D4N3=2X1P2S3H", "NNACGTACGTAGG", bytes(range(13)),
                 [T("NM", "C", 1), T("cs", "Z", b":3+a"), T("tp", "A", "P")], low_nibble=9),
        S.record(0, 100, "r2", 60, 0, "2S3I5M", "ACGTACGTAC", bytes([255] * 10), [T("tp", "A", "S"), T("cs", "Z", b"")]),
        S.record(0, 150, "r1", 0, 0x800, "4M3S", "TTTTAAA", bytes(7), [T("cs", "i", 5), T("cs", "Z", b":4"), T("tp", "Z", b"P")]),
        S.record(0, 150, "r4", 60, 0x4, "4M", "ACGT", bytes(4), [T("cs", "Z", b":4")]),
        S.record(0, 200, "r5", 1, 0x100, "2H3M", "ACG", b"\x01\x02\xff",
                 [T("xx", "Bs", [1, -2, 3]), T("cs", "Z", b"=ACG"), T("yy", "H", b"1F"), T("zz", "Bf", [])], low_nibble=15),
        S.record(1, 0, "r1", 255, 0x400, "5=3X2=", "=ACMGRSVTW", bytes(range(10, 20)), [T("cs", "Z", b":5*ag*ag*ag:2"), T("tp", "A", "I")]),
        S.record(1, 0, "r7", 3, 0x210, "1M", "N", b"\x00", [T("tp", "c", 80), T("xz", "Z", b"csZ:9"), T("cs", "Z", b":1")]),
        S.record(-1, -1, "r8", 0, 0x4, "", "A", b"\x00", b""),
    ]
    path = str(tmp_path / "lit.bam")
    S.write_bgzf(path, S.header([("c0", 5000), ("c1", 700)], "lit") + b"".join(recs), [3, 0, 70, 1, 0, 0, 200])
    p = S.parse(path)
    assert p.contigs == [("c0", 5000), ("c1", 700)] and p.sample() == "lit"
    a, b = p.batches["c0"], p.batches["c1"]
    assert a.n == 4 and b.n == 2
    assert a.tstart.tolist() == [100, 100, 150, 200] and a.tend.tolist() == [114, 105, 154, 203]
    assert a.qstart.tolist() == [2, 2, 0, 0] and a.qlen.tolist() == [13, 10, 7, 3]
    assert a.mapq.tolist() == [7, 60, 0, 1] and a.flag.tolist() == [16, 0, 0x800, 0x100]
    assert a.qid.tolist() == [0, 1, 0, 3] and a.tp.tolist() == [ord("P"), ord("S"), 0, 0]
    assert a.qoff.tolist() == [0, 32, 64, 96] and a.cs_off.tolist() == [0, 4, 4, 6, 10]
    assert a.cs.tobytes() == b":3+a" + b"" + b":4" + b"=ACG"
    assert a.seq.tobytes() == bytes.fromhex("ff124812481440") + bytes(9) + bytes.fromhex("1248124812") + bytes(11) + \
        bytes.fromhex("88881110") + bytes(12) + bytes.fromhex("1240") + bytes(14)
    assert a.bq.tobytes() == bytes(range(13)) + bytes(19) + bytes([255] * 10) + bytes(22) + bytes(32) + b"\x01\x02\xff" + bytes(29)
    assert b.tstart.tolist() == [0, 0] and b.tend.tolist() == [10, 1] and b.qstart.tolist() == [0, 0]
    assert b.qlen.tolist() == [10, 1] and b.mapq.tolist() == [255, 3] and b.flag.tolist() == [0x400, 0x210]
    assert b.qid.tolist() == [0, 1] and b.tp.tolist() == [ord("I"), 0] and b.cs.tobytes() == b":5*ag*ag*ag:2:1"
    assert b.seq.tobytes() == bytes.fromhex("0123456789") + bytes(11) + b"\xf0" + bytes(15)
    assert b.bq.tobytes() == bytes(range(10, 20)) + bytes(22) + bytes(32)
    for k in S.FIELDS:
        assert getattr(a, k).dtype == getattr(bamio.BamFile(path).batches["c0"], k).dtype, k
    Z.same_batch(bamio.BamFile(path).batches["c0"], a)
    Z.same_batch(bamio.BamFile(path).batches["c1"], b)


# ---- the zoo ------------------------------------------------------------------------------------------------------

def test_zoo_covers_what_it_claims(zoo_dir):
    path, parsed, (raw, cuts) = Z.cached("zoo", zoo_dir)
    assert len(raw) < 10 << 20 and [c for c, _ in parsed.contigs] == [c for c, _ in Z.ZOO_CONTIGS]
    a, e, c = (parsed.batches[n] for n, _ in Z.ZOO_CONTIGS)
    assert a.n > 2000 and e.n == 0 and c.n > 100
    spans = S.field_spans(raw)
    cut = np.array(sorted(set(cuts)))
    for kind in ("len", "fixed", "name", "cigar", "seq", "qual", "aux"):       # a block ends strictly inside such a part
        assert any(np.searchsorted(cut, s0, "right") < np.searchsorted(cut, s1, "left") for k, s0, s1 in spans if k == kind), kind
    assert len(cuts) != len(set(cuts))                                          # empty blocks in the middle
    ops, n_ops, name_len = set(), set(), set()
    for k, s0, s1 in spans:
        if k == "cigar":
            v = np.frombuffer(raw[s0:s1], "<u4")
            ops.update((v & 15).tolist())
            n_ops.add(len(v))
        if k == "name":
            name_len.add(s1 - s0 - 1)
    assert ops == set(range(9)) and 1 in n_ops and 300 in n_ops and name_len >= set(range(1, 255))
    assert set(Z.L_SEQS) <= set(a.qlen.tolist())
    assert set(a.bq.tolist()) == set(range(256)) and set((a.seq >> 4).tolist()) == set(range(16))
    recs = [spans[i:i + 7] for i in range(0, len(spans), 7)]                    # len fixed name cigar seq qual aux
    low = [raw[g[4][2] - 1] & 15 for g in recs if (g[5][2] - g[5][1]) & 1]
    assert sum(1 for v in low if v) > 500                                       # odd lengths: a stray low nibble in the file
    assert set(a.tp.tolist()) >= {0, ord("P"), ord("S")} and (np.diff(a.cs_off) == 0).any() and (a.cs == ord("=")).any()
    assert a.tstart[0] == 0 and a.tstart[-1] > 1 << 29 and (np.diff(a.tstart) == 0).sum() > 8
    assert (a.qid != np.arange(a.n)).sum() == 3 and (c.qid == np.arange(c.n)).all()      # a triple and a pair; no link across contigs
    for fl in (0x100, 0x800, 0x400, 0x200, 0x10):
        assert (a.flag & fl).any()
    assert not (a.flag & 4).any()


def test_host_parser_equals_spec_parser_on_the_zoo(zoo_dir, monkeypatch):
    path, parsed, _ = Z.cached("zoo", zoo_dir)
    for kb, threads in ((None, 1), (96, 3), (64, 8)):
        if kb:
            monkeypatch.setenv("HIMUT_INGEST_WINDOW_KB", str(kb))
        f = bamio.BamFile(path, threads=threads)
        assert f.tname2tsize == parsed.tname2tsize and f.sample() == parsed.sample()
        for name, _ in Z.ZOO_CONTIGS:
            Z.same_batch(f.batches[name], parsed.batches[name])


@pytest.mark.parametrize("window", Z.WINDOWS)
def test_stream_lists_the_zoo(zoo_dir, window):
    """The host half of the device ingest: every kept record once, in order, whatever a block or window end cuts."""
    path, parsed, _ = Z.cached("zoo", zoo_dir)
    for name in ("zooC", "zooA", "zooEmpty", "zooA"):
        b = parsed.batches[name]
        recs, qids, uniq, _ = _stream_records(path, name, window)
        assert [r[0] for r in recs] == b.tstart.tolist() and [r[1] for r in recs] == b.qlen.tolist()
        assert [r[2] for r in recs] == b.flag.tolist() and qids == b.qid.tolist()
        assert uniq == bool((b.qid == np.arange(b.n)).all())


def test_host_parser_on_the_stale_contig(zoo_dir):
    path, parsed, _ = Z.cached("stale", zoo_dir)
    zoo = Z.cached("zoo", zoo_dir)[1].batches["zooA"]
    st = parsed.batches["stale"]
    assert st.n > zoo.n and st.bq.shape[0] > zoo.bq.shape[0] and st.cs.shape[0] > zoo.cs.shape[0]
    assert (st.bq == 255).all() and (st.seq == 255).all() and (st.cs == ord("~")).all()
    Z.same_batch(bamio.BamFile(path).batches["stale"], st)


# ---- files that must be refused -----------------------------------------------------------------------------------

def test_refused_files_put_their_record_where_their_name_says(tmp_path):
    """The geometry the cases 'first / middle / last of a window' rely on: at 64 KB every ingest window of these files is
    ERR_PER_BLOCK whole records, so record F opens the second window (nothing carried over: it sits right behind its
    length field) and record L closes it."""
    path = str(tmp_path / "good.bam")
    Z._err_file(path, lambda recs: None)
    wins = []
    recs, _, _, _ = _stream_records(path, "errc", 64 << 10, per_window=wins)
    assert len(recs) == Z.ERR_N and wins == [(Z.ERR_PER_BLOCK, 4)] * (Z.ERR_N // Z.ERR_PER_BLOCK)
    assert (Z.F, Z.L) == (Z.ERR_PER_BLOCK, 2 * Z.ERR_PER_BLOCK - 1) and Z.F < Z.M < Z.L


@pytest.mark.parametrize("case", sorted(Z.ERROR_CASES))
def test_host_parser_refuses_what_the_spec_parser_refuses(tmp_path, case):
    kind, make = Z.ERROR_CASES[case]
    path = str(tmp_path / (case + ".bam"))
    make(path)
    want = Z.expected_error(case, device=False)
    if kind is None:
        Z.same_batch(bamio.BamFile(path).batches["errc"], S.parse(path).batches["errc"])
        return
    with pytest.raises(S.SpecError) as e:
        S.parse(path)
    assert e.value.kind == kind
    if kind == "no_cs":
        assert "{} records".format(e.value.count) == want[1]
    with pytest.raises(want[0]) as e:
        bamio.BamFile(path)
    assert want[1] in str(e.value)


@pytest.mark.parametrize("case", sorted(Z.STRAY_CASES))
def test_stray_bytes_behind_the_last_tag_are_accepted(tmp_path, case):
    """One or two bytes that cannot be an auxiliary field: the host parser takes the record (the device parser too,
    tests/test_gpu_bam_records.py); the strict reading of the specification refuses it.  Parity with htslib unpinned."""
    path = str(tmp_path / (case + ".bam"))
    Z.STRAY_CASES[case](path)
    with pytest.raises(S.SpecError) as e:
        S.parse(path)
    assert e.value.kind == "malformed"
    b = bamio.BamFile(path).batches["errc"]
    assert b.n == Z.ERR_N and int(b.tp[Z.M]) == ord("S") and b.cs_tag(Z.M) == ":700"


# ---- more records in a window than window_bytes / 64 ----------------------------------------------------------------

@pytest.mark.parametrize("window", [1 << 20, 96 << 10])
def test_stream_takes_windows_of_very_short_records(zoo_dir, window):
    """54-byte records, enough of them to fill head / (0.15 * window) + 8 windows of 1 MB: a stream that lists at most
    window_bytes / 64 records per window carries the rest forward until the head room overflows."""
    path, _, (pos, flag) = Z.cached("short", zoo_dir)
    head = bamio._load().bam_stream_head()
    assert pos.shape[0] * Z.SHORT_REC_BYTES >= (head / (0.15 * (1 << 20)) + 8) * (1 << 20)
    recs, qids, uniq, _ = _stream_records(path, "short", window)
    got = np.array(recs, np.int64).reshape(-1, 3)
    assert got.shape[0] == pos.shape[0]
    assert np.array_equal(got[:, 0], pos) and (got[:, 1] == 1).all() and np.array_equal(got[:, 2], flag)
    assert np.array_equal(np.array(qids), np.arange(pos.shape[0])) and uniq


# ---- broken headers, stale indexes: what both entry points do with them -------------------------------------------

PIN_CONTIGS = [("hA", 50_000), ("hB", 70_000)]
PIN_L_SEQ = 30_000              # seven records of 45 KB: several BGZF blocks, so an index has block starts to hint at


def _pin_records():
    rng = np.random.default_rng(5)
    out = []
    for ref_id, n, flag in ((0, 4, 0), (1, 3, 16)):
        for k in range(n):
            out.append(S.record(ref_id, 10 * k, "pin{}/{}".format(ref_id, k), 60, flag, "%dM" % PIN_L_SEQ,
                                rng.integers(0, 16, PIN_L_SEQ, dtype=np.uint8), rng.integers(0, 94, PIN_L_SEQ, dtype=np.uint8).tobytes(),
                                [S.tag("cs", "Z", b":%d" % PIN_L_SEQ), S.tag("tp", "A", "P")]))
    return b"".join(out)


def _broken_header(case):
    """The inflated bytes of a file whose header is broken as ``case`` says."""
    hdr = S.header(PIN_CONTIGS, "pin")
    n_ref_at = 8 + struct.unpack_from("<i", hdr, 4)[0]
    if case == "bad_magic":
        return b"BAX\1" + hdr[4:] + _pin_records()
    if case == "l_text_longer_than_file":
        return hdr[:4] + struct.pack("<i", 1 << 30) + hdr[8:] + _pin_records()
    if case == "n_ref_larger_than_file":
        return hdr[:n_ref_at] + struct.pack("<i", 1 << 28) + hdr[n_ref_at + 4:] + _pin_records()
    if case == "cut_inside_contig_name":
        return hdr[:n_ref_at + 4 + 4 + 1]                       # n_ref, l_name and one byte of the first name
    assert case == "l_name_zero"
    return hdr[:n_ref_at] + struct.pack("<iii", 2, 0, 50_000) + struct.pack("<i", 3) + b"hB\0" + struct.pack("<i", 70_000) + \
        _pin_records()


# case -> message of (BamFile, BamStream); both raise ValueError.  None: the file is read.
BROKEN_HEADERS = {
    "bad_magic": ("not a BAM file", "not a BAM file"),
    "l_text_longer_than_file": ("BAM header text longer than the file", "BAM header text longer than the file"),
    "n_ref_larger_than_file": ("BAM header lists more contigs than the file can hold",
                               "BAM header lists more contigs than the file can hold"),
    "cut_inside_contig_name": ("unexpected end of BAM", "truncated BAM header"),     # the entry points word it differently
    "l_name_zero": (None, None),
}


@pytest.mark.parametrize("case", sorted(BROKEN_HEADERS))
def test_broken_headers_per_entry_point(tmp_path, case):
    path = str(tmp_path / (case + ".bam"))
    S.write_bgzf(path, _broken_header(case))
    for cls, want in zip((bamio.BamFile, bamio.BamStream), BROKEN_HEADERS[case]):
        if want is None:                                        # a contig without a name: taken, under the name ""
            f = cls(path)
            assert f.tname2tsize == {"": 50_000, "hB": 70_000} and f.sample() == "pin"
            if cls is bamio.BamFile:
                assert {k: b.n for k, b in f.batches.items()} == {"": 4, "hB": 3}
            else:
                assert f.names == ["", "hB"]
            continue
        with pytest.raises(ValueError) as e:
            cls(path)
        assert str(e.value) == "{}: {}".format(path, want)


def _stale_index(case, bai):
    if case == "truncated":
        return bai[:3 * len(bai) // 4]                          # inside the second contig's part
    assert case == "other_n_ref"                                # the same index with a third, empty contig
    return bai[:4] + struct.pack("<i", 3) + bai[8:] + struct.pack("<ii", 0, 0)


@pytest.mark.parametrize("case", ["truncated", "other_n_ref"])
def test_stale_index_costs_the_seek_only(tmp_path, monkeypatch, case):
    """An index that cannot be walked to its end, or lists another number of contigs: no seek (``indexed`` is false, the
    contig is found by hopping), the records listed are the host loader's, and the block starts the index gave before
    it broke off still split the block scan."""
    plain = str(tmp_path / "plain.bam")
    S.write_bgzf(plain, S.header(PIN_CONTIGS, "pin") + _pin_records())
    path = str(tmp_path / "x.bam")
    bamio.write_bam(path, [bamio.BamFile(plain).batches[n] for n, _ in PIN_CONTIGS], sample="pin")
    host = bamio.BamFile(path)
    with open(path + ".bai", "rb") as f:
        bai = f.read()

    def open_facts():
        monkeypatch.setenv("HIMUT_INGEST_SCAN_MIN_KB", "1")
        st = bamio.BamStream(path, 3)
        facts = (st.indexed, int(st._L.bam_stream_scan_parts(st._h)))
        st.close()
        monkeypatch.delenv("HIMUT_INGEST_SCAN_MIN_KB")
        return facts

    assert open_facts() == (True, 2)
    with open(path + ".bai", "wb") as f:
        f.write(_stale_index(case, bai))
    assert open_facts() == (False, 2)
    for name, _ in reversed(PIN_CONTIGS):
        hb = host.batches[name]
        recs, qids, uniq, _ = _stream_records(path, name, 64 << 10)
        assert [r[0] for r in recs] == hb.tstart.tolist() and [r[1] for r in recs] == hb.qlen.tolist()
        assert [r[2] for r in recs] == hb.flag.tolist() and qids == hb.qid.tolist() and uniq
