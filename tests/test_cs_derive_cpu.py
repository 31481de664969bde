"""Deriving the cs text from CIGAR and the reference, the parts that need no GPU: the command line, the C
ABI's declarations, and the Python restatement of the rule (tests/cs_from_cigar.py) against texts written by hand and
against the synthetic generator's own cs tags -- the restatement is what the GPU tests hold the device's text to."""
import re

import pytest

from tests import bam_spec
from tests import cs_from_cigar as C


@pytest.mark.parametrize("sub,rest", [
    ("call", ["-i", "x.bam", "-o", "o.vcf"]),
    ("normcounts", ["-i", "x.bam", "--sbs", "s.vcf", "-o", "o.tsv"]),
    ("phase", ["-i", "x.bam", "--vcf", "g.vcf", "-o", "o.vcf"]),
])
def test_parser_takes_cs_from_ref_only_with_ref(sub, rest, capsys):
    from himut_amd.parse_args import parse_args
    _, o = parse_args("t", [sub] + rest + ["--ref", "g.fa", "--cs_from_ref"])
    assert o.cs_from_ref is True and o.ref == "g.fa"
    if sub != "normcounts":                       # normcounts requires --ref anyway
        _, o = parse_args("t", [sub] + rest)
        assert o.cs_from_ref is False and o.ref is None
    with pytest.raises(SystemExit) as e:
        parse_args("t", [sub] + rest + ["--cs_from_ref"])
    assert e.value.code == 2
    assert "--ref" in capsys.readouterr().err


def test_header_declares_and_ffi_exports_the_two_entry_points():
    import os
    from himut_amd import _ffi
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "himut_hip.h")).read()
    for name in ("himut_ingest_derive_cs", "himut_ingest_derive_result"):
        assert "int {}(himut_ctx* ctx".format(name) in text
        assert name in _ffi.EXPORTS
    assert "#define HIMUT_ABI_VERSION 2" in text


def test_checker_reproduces_texts_written_by_hand():
    refs = (C.hand_reference(), C.long_reference())
    n = 0
    for contig, pos, cigar, seq, literal, _tags in C.hand_cases():
        got = C.derive_cs(cigar, pos, [bam_spec.NIBBLES.index(ch) for ch in seq], refs[contig])
        assert got is not None, (pos, cigar)
        assert re.search(r":0", got) is None, got           # no empty run, no leading zero
        if literal is not None:
            assert got == literal, (pos, cigar)
            n += 1
    assert n >= 12


def test_checker_literals_on_a_small_reference():
    ref = "ACGTNacgtRACGT"
    assert C.derive_cs("5M5=", 0, [1, 2, 4, 8, 1, 1, 2, 4, 8, 1], "ACGTAACGTA") == ":10"
    assert C.derive_cs("4M", 0, [1, 2, 4, 8], ref) == ":4"
    assert C.derive_cs("5M", 0, [1, 2, 4, 8, 1], ref) == ":4*na"
    assert C.derive_cs("4M", 5, [1, 2, 4, 8], ref) == ":4"                       # lower-case reference: matches
    assert C.derive_cs("4M", 5, [1, 2, 2, 8], ref) == ":2*gc:1"
    assert C.derive_cs("2M", 9, [4, 1], ref) == "*ng:1"                           # R
    assert C.derive_cs("3X", 10, [1, 15, 4], ref) == ":1*cn:1"                   # query N; X over matching bases
    assert C.derive_cs("1S2M2I2M2D2M1S", 0, [8, 1, 2, 15, 8, 4, 8, 2, 4, 1], ref) == ":2+nt:2-na:2"
    assert C.derive_cs("2H2M2H", 0, [1, 2], ref) == ":2"
    assert C.derive_cs("1I1D", 4, [0], ref) == "+n-n"
    # what cannot be derived
    assert C.derive_cs([], 0, [], ref) is None
    assert C.derive_cs("2M3N2M", 0, [1, 2, 1, 2], ref) is None
    assert C.derive_cs("2M1P2M", 0, [1, 2, 4, 8], ref) is None
    assert C.derive_cs("4M", 0, [1, 2, 4], ref) is None
    assert C.derive_cs("4M", 11, [2, 4, 8, 1], ref) is None
    assert C.derive_cs("3M", 11, [2, 4, 8], ref) == ":3"


def test_cigar_forms_from_a_cs_text():
    cs = ":3*ac*gt:2+ac-g:4"
    assert C.cs_to_cigar(cs, 2, 16, "M") == [(2, C.S), (7, C.M), (2, C.I), (1, C.D), (4, C.M), (1, C.S)]
    assert C.cs_to_cigar(cs, 0, 13, "EQX") == [(3, C.EQ), (1, C.X), (1, C.X), (2, C.EQ), (2, C.I), (1, C.D), (4, C.EQ)]


@pytest.mark.parametrize("rates", C.SYNTH_RATES)
@pytest.mark.parametrize("seed", C.SYNTH_SEEDS)
def test_checker_reproduces_the_generators_cs(seed, rates):
    """Every read of the GPU tests' samples: the CIGAR from the generator's cs tag (both forms), SEQ and the generator's
    reference give the tag back byte for byte."""
    s = C.synth_sample(seed, rates)
    b, ref = s.batch, bytes(s.ref)
    assert b.n > 100
    for i in range(b.n):
        want = C.read_cs(b, i)
        for form in ("M", "EQX"):
            cig = C.cs_to_cigar(want, int(b.qstart[i]), int(b.qlen[i]), form)
            assert C.derive_cs(cig, int(b.tstart[i]), C.read_codes(b, i), ref) == want, (i, form)


def _pump_sums(path, chrom, window_bytes, sum_cigar):
    """bam_stream_pump with host buffers and a Python callback in place of himut_ingest_window: per window (records,
    padded bases, tag bytes) as the device library would be told."""
    import ctypes

    import numpy as np
    from himut_amd import bamio
    st = bamio.BamStream(path, 2)
    L, h = st._L, st._h
    bound = ctypes.c_int64()
    assert L.bam_stream_select(h, st.names.index(chrom), ctypes.byref(bound)) == 0
    L.bam_stream_sum_cigar(h, 1 if sum_cigar else 0)
    cap = window_bytes + L.bam_stream_head()
    bufs = [np.zeros(cap, np.uint8) for _ in (0, 1)]
    seen = []

    @ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int)
    def wait(_ctx, _slot):
        return 0

    @ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64)
    def window(_ctx, _slot, _start, _nbytes, _rec_off, _qid, n, padded, tag_bytes):
        seen.append((int(n), int(padded), int(tag_bytes)))
        return 0

    rc = L.bam_stream_pump(h, None, ctypes.cast(wait, ctypes.c_void_p), ctypes.cast(window, ctypes.c_void_p),
                           bufs[0].ctypes.data_as(ctypes.c_void_p), bufs[1].ctypes.data_as(ctypes.c_void_p), cap,
                           bamio.stream_rec_cap(window_bytes))
    assert rc == 0, L.bam_stream_error(h)
    st.close()
    return seen


def test_host_announces_the_cigar_bytes_of_every_window(tmp_path):
    """Records whose CIGAR is larger than their auxiliary fields and their SEQ: what the host hands over as the bound
    of the window's text bytes is, for a deriving ingest, exactly 4 * n_cigar summed -- and the auxiliary bytes, as
    before, otherwise."""
    cigar = [(20, C.EQ)] + [(1, C.EQ)] * 20
    recs = [bam_spec.record(0, 10 * k, "s{}".format(k), 60, 0, cigar, [1] * 40, bytes([50] * 40),
                            [bam_spec.tag("tp", "A", b"P")] if k % 2 else b"") for k in range(3000)]
    path = str(tmp_path / "short.bam")
    bam_spec.write_bgzf(path, bam_spec.header([("chrS", 40_000)], "syn") + b"".join(recs))
    derive, tags = _pump_sums(path, "chrS", 96 << 10, True), _pump_sums(path, "chrS", 96 << 10, False)
    assert len(derive) > 3 and [w[:2] for w in derive] == [w[:2] for w in tags]
    assert sum(w[0] for w in derive) == 3000
    assert all(w[2] == 84 * w[0] for w in derive)
    assert sum(w[2] for w in tags) == 1500 * 4 and all(w[2] < 84 * w[0] for w in tags)
