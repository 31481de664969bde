"""Inputs for the BAM ingest tests, packed with tests/bam_spec.py: the record zoo (every CIGAR op, every auxiliary type,
sequence lengths around the lane and wave edges of k_bam_scatter, names of every length, BGZF blocks that cut every part
of a record), a contig of stale bytes, a file of very many very short records, and the malformed / refused files."""
import functools
import os
import struct

import numpy as np

from tests import bam_spec as S

L_SEQS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
FIXED_CIGARS = ("5H2S3M1I2D4N3=2X1P2S3H", "2S3I5M", "4M3S", "3H4M", "4M3H", "2H3S10M4S1H", "5=3X2=", "7M", "3M2N1P4M",
                "1H1M", "6X", "3S1M1I1M1D1M1N1M1P1M1=1X2S")
ZOO_CONTIGS = (("zooA", 600_000_000), ("zooEmpty", 5000), ("zooC", 100_000))
WINDOWS = (64 << 10, 96 << 10, 1 << 20)
_QUERY_OPS = "MIS=X"


def _qlen(cigar):
    return sum(ln for ln, op in S.cigar_ops(cigar) if S.CIGAR_OPS[op] in _QUERY_OPS)


def _rand_cigar(rng, l_seq):
    """A CIGAR over all nine ops that consumes l_seq query bases: H and S outside, the rest in between."""
    if l_seq == 1:
        return rng.choice(["1M", "1=", "1X", "2H1M", "1M3H"])
    lead = int(rng.integers(0, min(4, l_seq - 1) + 1))
    trail = int(rng.integers(0, min(4, l_seq - 1 - lead) + 1))
    left = l_seq - lead - trail
    ops = []
    while left:
        ln = int(min(left, rng.integers(1, max(2, l_seq // 6))))
        ops.append("{}{}".format(ln, "M=XI"[int(rng.integers(0, 4))] if ops else "M=X"[int(rng.integers(0, 3))]))
        left -= ln
        if left and rng.random() < 0.5:
            ops.append("{}{}".format(int(rng.integers(1, 9)), "DNP"[int(rng.integers(0, 3))]))
    out = ("{}H".format(int(rng.integers(1, 9))) if rng.random() < 0.3 else "") + ("{}S".format(lead) if lead else "")
    out += "".join(ops) + ("{}S".format(trail) if trail else "")
    return out + ("{}H".format(int(rng.integers(1, 9))) if rng.random() < 0.3 else "")


# every kind of auxiliary field that is neither cs nor tp, as (type, value maker)
def _fillers(rng):
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))
    kinds = [("A", lambda: chr(r(33, 126))), ("c", lambda: r(-128, 127)), ("C", lambda: r(0, 255)), ("s", lambda: r(-32768, 32767)),
             ("S", lambda: r(0, 65535)), ("i", lambda: r(-2 ** 31, 2 ** 31 - 1)), ("I", lambda: r(0, 2 ** 32 - 1)),
             ("f", lambda: float(rng.random())), ("Z", lambda: bytes(rng.integers(33, 127, r(0, 40), dtype=np.uint8))),
             ("H", lambda: b"".join(b"%02X" % r(0, 255) for _ in range(r(0, 12))))]
    for sub, lo, hi in (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", -2 ** 31, 2 ** 31 - 1),
                        ("I", 0, 2 ** 32 - 1)):
        kinds.append(("B" + sub, lambda lo=lo, hi=hi: [r(lo, hi) for _ in range(r(1, 9))]))
        kinds.append(("B" + sub, lambda: []))
    kinds.append(("Bf", lambda: [float(rng.random()) for _ in range(r(1, 9))]))
    kinds.append(("Bf", lambda: []))
    return kinds


_DECOYS = (lambda: S.tag("cs", "i", 7), lambda: S.tag("cs", "A", "Z"), lambda: S.tag("tp", "Z", b"S"), lambda: S.tag("tp", "c", 83),
           lambda: S.tag("xz", "Z", b"..csZ:99"), lambda: S.tag("tp", "Z", b"tpAX"),
           lambda: S.tag("xb", "BC", list(b"csZ:5\0tpAX\0")), lambda: S.tag("cs", "H", b"1F"), lambda: S.tag("CS", "Z", b":3"),
           lambda: S.tag("tp", "C", 80))


def _rand_cs(rng, l_seq, k):
    if k % 97 == 5:
        return b""
    if k % 7 == 3:                                      # long form
        return b"=" + bytes(rng.choice(list(b"ACGT"), min(l_seq, 60)).astype(np.uint8)) + b"*ag=AC"
    parts = [b":%d" % l_seq]
    for _ in range(int(rng.integers(0, 6))):
        parts.append([b"*ag", b"+tt", b"-acg", b":12", b"*ct"][int(rng.integers(0, 5))])
    return b"".join(parts)


def _zoo_specs(rng):
    """Records of the zoo as dicts, unsorted (pos is set later for most)."""
    fill = _fillers(rng)
    specs = []

    def add(**kw):
        specs.append(kw)

    for c in FIXED_CIGARS:
        add(cigar=c, l_seq=_qlen(c))
    add(cigar="1M1I" * 100 + "1M1D" * 50, l_seq=250)                      # 300 ops
    add(cigar="2M1D" * 150, l_seq=300)
    for nl in range(1, 255):                                              # names of every length
        add(name_len=nl, l_seq=L_SEQS[nl % len(L_SEQS)])
    for l_seq in L_SEQS:                                                  # every length with every residue of the name length
        for nl in range(3, 19):
            add(name_len=nl, l_seq=l_seq)
    for k, _ in enumerate(fill):                                          # each filler kind alone before / after cs
        add(pre=[k], post=[], tp_where=k % 3)
        add(pre=[], post=[k], tp_where=(k + 1) % 3)
        add(pre=[k], post=[k], tp_where=(k + 2) % 3)
    for d in range(len(_DECOYS)):
        add(decoy_pre=[d], decoy_post=[], tp_where=d % 3)
        add(decoy_pre=[], decoy_post=[d], tp_where=(d + 1) % 3)
    add(decoy_pre=list(range(len(_DECOYS))), decoy_post=list(range(len(_DECOYS))), tp_where=2)
    for flag in (0x100, 0x800, 0x400, 0x200, 0x10, 0x910, 0x1, 0x4, 0x14, 0x104):
        for _ in range(3):
            add(flag=flag)
    while len(specs) < 2600:
        add()
    return specs, fill


def _pack(rng, sp, fill, ref_id, pos, k, names):
    l_seq = sp.get("l_seq", L_SEQS[int(rng.integers(0, len(L_SEQS)))] if rng.random() < 0.7 else int(rng.integers(1, 1500)))
    cigar = sp.get("cigar") or _rand_cigar(rng, l_seq)
    if "name" in sp:
        name = sp["name"]
    else:
        nl = sp.get("name_len", int(rng.integers(3, 40)))
        while True:
            name = bytes(rng.integers(33, 127, nl, dtype=np.uint8))
            if name not in names:
                break
    names.add(name)
    codes = rng.integers(0, 16, l_seq, dtype=np.uint8)
    codes[:min(16, l_seq)] = ((np.arange(16) + k) & 15)[:min(16, l_seq)]      # all 16 codes, early
    qual = rng.integers(0, 256, l_seq, dtype=np.uint8)
    qual[-1] = 255 if k & 1 else 0
    if l_seq >= 17:
        qual[15], qual[16] = 255, 254
    pre = [S.tag("x%d" % (j % 10), *[fill[j][0], fill[j][1]()]) for j in sp.get("pre", rng.integers(0, len(fill), int(rng.integers(0, 3))))]
    post = [S.tag("y%d" % (j % 10), *[fill[j][0], fill[j][1]()]) for j in sp.get("post", rng.integers(0, len(fill), int(rng.integers(0, 3))))]
    pre += [_DECOYS[d]() for d in sp.get("decoy_pre", [])]
    post = [_DECOYS[d]() for d in sp.get("decoy_post", [])] + post
    tp_where = sp.get("tp_where", k % 3)                                  # 0 before cs, 1 after cs, 2 absent
    tp = [S.tag("tp", "A", "PSIi"[k % 4])]
    cs = [S.tag("cs", "Z", _rand_cs(rng, l_seq, k))]
    tags = (tp if tp_where == 0 else []) + pre + cs + post + (tp if tp_where == 1 else [])
    if tp_where == 0 and k % 2:
        tags = pre + tp + cs + post
    flag = sp.get("flag", [0, 16, 0x100, 0x800][int(rng.integers(0, 4))] if rng.random() < 0.3 else 0)
    return S.record(ref_id, pos, name, int(rng.integers(0, 256)) if k % 5 else 60, flag, cigar, codes, qual.tobytes(), tags,
                    low_nibble=1 + k % 15)


def _block_sizes(rng, raw_len, forced):
    """Random BGZF block ends plus the forced ones; some blocks empty, none above the format's limit."""
    cuts = set(forced)
    at = 0
    while at < raw_len:
        u = rng.random()
        at += int(rng.integers(1, 64)) if u < 0.15 else int(rng.integers(64, 6000)) if u < 0.45 else int(rng.integers(6000, S.BGZF_MAX + 1))
        cuts.add(min(at, raw_len))
    cuts = sorted(c for c in cuts if 0 < c <= raw_len)
    sizes, prev = [], 0
    for c in cuts:
        while c - prev > S.BGZF_MAX:
            sizes.append(S.BGZF_MAX)
            prev += S.BGZF_MAX
        sizes.append(c - prev)
        prev = c
        if rng.random() < 0.08:
            sizes.append(0)
    return sizes


def build_zoo(path, seed=20240611):
    """Writes the zoo; returns (raw inflated bytes, block ends)."""
    rng = np.random.default_rng(seed)
    specs, fill = _zoo_specs(rng)
    ordered = [specs[j] for j in rng.permutation(len(specs))]
    n = len(ordered) + 8
    for k, sp in ((7, dict(name=b"zoo/pair")), (40, dict(name=b"zoo/triple")), (41, dict(name=b"zoo/triple")),
                  (43, dict(name=b"zoo/triple")), (300, dict(name=b"zoo/both-contigs")),
                  (500, dict(name=b"zoo/dropped-first", flag=0x4)),      # unmapped on the contig: a later kept record has its name
                  (520, dict(name=b"zoo/dropped-first", flag=0)), (n - 9, dict(name=b"zoo/pair"))):
        ordered.insert(k, sp)
    assert len(ordered) == n
    # positions: a run at 0, runs of equal positions, the last records near 2^29
    pos = np.sort(rng.integers(0, 3_000_000, n)).astype(np.int64)
    pos[:4] = 0
    pos[100:108] = pos[100]
    pos[-6:] = (1 << 29) + np.array([-5, -5, -1, 0, 0, 3])
    names = set()
    recs = [_pack(rng, sp, fill, 0, int(pos[k]), k, names) for k, sp in enumerate(ordered)]
    nC = 240
    posC = np.sort(rng.integers(0, 90_000, nC))
    for k in range(nC):
        sp = {"name": b"zoo/both-contigs"} if k == 17 else {}
        recs.append(_pack(rng, sp, fill, 2, int(posC[k]), n + k, names))
    for k in range(3):                                 # unplaced, at the end of the file
        recs.append(S.record(-1, -1, "unplaced%d" % k, 0, 4, "", "ACGTN"[:3 + k], bytes(3 + k), b""))
    hdr = S.header(ZOO_CONTIGS, "zooSample")
    raw = hdr + b"".join(recs)
    # block ends inside a length field, a fixed part, a CIGAR, a SEQ and the auxiliary fields of some records
    spans = S.field_spans(raw)
    forced = []
    for kind, step in (("len", 2), ("fixed", 9), ("cigar", 3), ("seq", 1), ("aux", 2), ("qual", 5), ("name", 1)):
        cand = [(a, b) for kd, a, b in spans if kd == kind and b - a > step]
        for a, b in cand[11::max(1, len(cand) // 7)]:
            forced.append(a + step)
    cuts = S.write_bgzf(path, raw, _block_sizes(rng, len(raw), forced))
    return raw, cuts


def build_stale(path, n=3200, l_seq=2048):
    """One contig larger than any of the zoo in every array: all-N bases, all-255 qualities, cs text of '~'."""
    recs = [S.record(0, 10 * k, "stale%06d" % k, 255, 0xfff & ~4, "%dM" % l_seq, np.full(l_seq, 15, np.uint8), b"\xff" * l_seq,
                     [S.tag("cs", "Z", b"~" * 250), S.tag("tp", "A", "\x7f")]) for k in range(n)]
    S.write_bgzf(path, S.header([("stale", 1_000_000)], "st") + b"".join(recs))


SHORT_REC_BYTES = 54


def short_records_count(head, window=1 << 20):
    """Enough short records to fill head / (0.15 * window) + 8 windows: a stream that leaves 15 % of every window to the
    next one has outgrown its head room by then."""
    return int((head / (0.15 * window) + 8) * window / SHORT_REC_BYTES) + 1


def build_short_records(path, n):
    """n records of 54 bytes (one base, cs ':1', five hex digits of name); returns (pos, flag) of the records."""
    tmpl = np.frombuffer(S.record(0, 0, "00000", 60, 0, "1M", "A", b"\x28", [S.tag("cs", "Z", b":1")]), np.uint8)
    assert tmpl.shape[0] == SHORT_REC_BYTES and n <= 16 ** 5
    a = np.tile(tmpl, (n, 1))
    k = np.arange(n, dtype=np.int64)
    pos = (k // 3).astype("<i4")
    a[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    for d in range(5):
        a[:, 36 + d] = hexd[(k >> (4 * (4 - d))) & 15]
    flag = np.where(k % 11 == 0, 16, 0).astype("<u2")
    a[:, 18:20] = flag.view(np.uint8).reshape(n, 2)
    S.write_bgzf(path, S.header([("short", 1 << 28)], "sh") + a.tobytes())
    return pos.astype(np.int32), flag.astype(np.uint16)


# ---- files a parser must refuse (or accept: kind None) ------------------------------------------------------------

def _plain(k, pos=None, tags=None, **kw):
    rng = np.random.default_rng(1000 + k)
    l_seq = 700 + k % 13
    t = [S.tag("NM", "C", 3), S.tag("cs", "Z", b":%d" % l_seq), S.tag("tp", "A", "P")] if tags is None else tags
    return S.record(0, 100 * k if pos is None else pos, "err/%d" % k, 60, 0, "%dM" % l_seq, rng.integers(0, 16, l_seq, dtype=np.uint8),
                    rng.integers(0, 94, l_seq, dtype=np.uint8).tobytes(), t, **kw)


ERR_N = 150
ERR_PER_BLOCK = 50              # ~53 KB: every 64 KB ingest window is one block and starts on a record


def _err_file(path, edit, tail=b"", cut=0):
    recs = [_plain(k) for k in range(ERR_N)]
    edit(recs)
    hdr = S.header([("errc", 1_000_000)], "er")
    sizes, k = [len(hdr)], 0
    while k < len(recs):
        sizes.append(sum(len(r) for r in recs[k:k + ERR_PER_BLOCK]))
        k += ERR_PER_BLOCK
    raw = hdr + b"".join(recs) + tail
    if cut:
        raw = raw[:-cut]
        sizes[-1] -= cut
    S.write_bgzf(path, raw, sizes)


def _set(k, rec):
    def edit(recs):
        recs[k] = rec
    return edit


_NOTAG_CS = [S.tag("NM", "C", 3), S.tag("tp", "A", "P")]
_CS = S.tag("cs", "Z", b":700")
F, M, L = ERR_PER_BLOCK, ERR_PER_BLOCK + 20, 2 * ERR_PER_BLOCK - 1         # first / middle / last record of the second window


def _several_no_cs(recs):
    for k in (F, M, L):
        recs[k] = _plain(k, tags=_NOTAG_CS)


# name -> (kind the spec parser reports, or None for a good file; builder)
ERROR_CASES = {
    "no_cs_first_of_window": ("no_cs", lambda p: _err_file(p, _set(F, _plain(F, tags=_NOTAG_CS)))),
    "no_cs_middle_of_window": ("no_cs", lambda p: _err_file(p, _set(M, _plain(M, tags=_NOTAG_CS)))),
    "no_cs_last_of_window": ("no_cs", lambda p: _err_file(p, _set(L, _plain(L, tags=_NOTAG_CS)))),
    "no_cs_last_of_contig_no_tags": ("no_cs", lambda p: _err_file(p, _set(ERR_N - 1, _plain(ERR_N - 1, tags=[])))),
    "no_cs_three_records": ("no_cs", lambda p: _err_file(p, _several_no_cs)),
    "unsorted_inside_window": ("unsorted", lambda p: _err_file(p, _set(M, _plain(M, pos=100 * M - 101)))),
    "unsorted_first_of_window": ("unsorted", lambda p: _err_file(p, _set(F, _plain(F, pos=100 * F - 101)))),
    "equal_positions": (None, lambda p: _err_file(p, _set(F, _plain(F, pos=100 * F - 100)))),
    "aux_unknown_type": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, tags=[_CS, b"xxx\x01\x02\x03\x04"])))),
    "aux_string_without_nul": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, tags=[_CS, b"xxZabcdef"])))),
    "aux_scalar_cut": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, tags=[_CS, b"xxi\x01\x02"])))),
    "aux_array_overlong": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, tags=[_CS, b"xxBi" + struct.pack("<I", 1000) + bytes(4)])))),
    "aux_array_header_cut": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, tags=[_CS, b"xxBi\x01"])))),
    "parts_exceed_block_size_l_seq": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, l_seq=900)))),
    "parts_exceed_block_size_n_cigar": ("malformed", lambda p: _err_file(p, _set(M, _plain(M, n_cigar=400)))),
    "block_size_below_32": ("malformed", lambda p: _err_file(p, _set(M, struct.pack("<I", 20) + bytes(20)))),
    "truncated_last_record": ("truncated", lambda p: _err_file(p, lambda recs: None, cut=333)),
}
# one or two bytes behind the last auxiliary field: both of our parsers take the record
STRAY_CASES = {
    "stray_one_byte": lambda p: _err_file(p, _set(M, _plain(M, tags=[_CS, S.tag("tp", "A", "S"), b"\x07"]))),
    "stray_two_bytes": lambda p: _err_file(p, _set(M, _plain(M, tags=[S.tag("tp", "A", "S"), _CS, b"cs"]))),
}


def expected_error(name, device):
    """(exception classes, text the message must contain) for a case of ERROR_CASES, None for a good file."""
    from himut_amd._ffi import HimutError
    kind = ERROR_CASES[name][0]
    if kind is None:
        return None
    if kind == "no_cs":
        return (KeyError,), "3 records" if name == "no_cs_three_records" else "1 records"
    if kind == "unsorted":
        return (ValueError,), "not coordinate sorted"
    if kind == "truncated":
        return (ValueError,), "truncated"
    if name == "block_size_below_32":
        return (ValueError,), "too short"
    return ((HimutError, ValueError) if device else (ValueError,)), "malformed BAM record"


def same_batch(got, want):
    """Field by field, exactly."""
    assert got.n == want.n
    for k in S.FIELDS:
        x, y = getattr(got, k), getattr(want, k)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), k


@functools.lru_cache(maxsize=None)
def cached(kind, directory):
    """Builds a file once per directory and parses it once: (path, Parsed or None, extra)."""
    path = os.path.join(directory, kind + ".bam")
    if kind == "zoo":
        raw, cuts = build_zoo(path)
        return path, S.parse(path), (raw, cuts)
    if kind == "stale":
        build_stale(path)
        return path, S.parse(path), None
    if kind == "short":
        from himut_amd import bamio
        n = short_records_count(bamio._load().bam_stream_head())
        return path, None, build_short_records(path, n)          # parsed by the one test that needs it
    raise KeyError(kind)
