"""A BAM packer and a BAM parser written from the SAM/BAM specification (section 4.2 of SAMv1: the BGZF container, the
header, the alignment record, the auxiliary fields), for tests: inputs that the project's own writer never emits, and an
expected read batch that owes nothing to the project's parsers.  Pure Python over struct, zlib and numpy; nothing of
the package under test is imported here."""
import struct
import zlib

import numpy as np

NIBBLES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
BGZF_MAX = 65280                    # the largest payload a BGZF block of this writer carries
_BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

FIELDS = ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "qid", "qoff", "cs_off", "seq", "bq", "cs", "tp")


class SpecError(Exception):
    """parse() refuses the file.  kind: no_cs (count = records without cs:Z), unsorted, malformed, truncated."""

    def __init__(self, kind, detail="", count=0):
        super().__init__("{}: {}".format(kind, detail))
        self.kind = kind
        self.count = count


# ---- packer ------------------------------------------------------------------------------------------------------

def header(contigs, sample):
    """contigs: [(name, length)]; the text carries @HD, one @SQ per contig and one @RG with SM:sample."""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:{}\tLN:{}\n".format(n, ln) for n, ln in contigs) + \
        "@RG\tID:rg1\tSM:{}\n".format(sample)
    out = [b"BAM\1", struct.pack("<i", len(text)), text.encode(), struct.pack("<i", len(contigs))]
    for n, ln in contigs:
        nm = n.encode() + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", ln)]
    return b"".join(out)


def cigar_ops(cigar):
    """'5H2S3M' or [(length, op)] -> [(length, op index)]."""
    if isinstance(cigar, str):
        out, num = [], ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                out.append((int(num), CIGAR_OPS.index(ch)))
                num = ""
        assert num == ""
        return out
    return [(int(ln), CIGAR_OPS.index(op) if isinstance(op, str) else int(op)) for ln, op in cigar]


_SCALAR = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def tag(name, typ, value):
    """One auxiliary field.  typ: A c C s S i I f Z H, or 'B' + subtype with a list of values.  Z and H take bytes
    (NUL appended here)."""
    nm = name.encode() if isinstance(name, str) else name
    assert len(nm) == 2
    if typ in _SCALAR:
        v = value.encode() if typ == "A" and isinstance(value, str) else value
        return nm + typ.encode() + struct.pack(_SCALAR[typ], v)
    if typ in ("Z", "H"):
        v = value.encode() if isinstance(value, str) else bytes(value)
        assert b"\0" not in v
        return nm + typ.encode() + v + b"\0"
    assert typ[0] == "B" and typ[1] in "cCsSiIf"
    return nm + b"B" + typ[1].encode() + struct.pack("<I", len(value)) + \
        b"".join(struct.pack(_SCALAR[typ[1]], v) for v in value)


def record(ref_id, pos, name, mapq, flag, cigar, seq, qual, tags, l_seq=None, n_cigar=None, block_size=None,
           low_nibble=0, next_ref_id=-1, next_pos=-1, tlen=0, bin_=4680):
    """One alignment record, length field included.  seq: a string over NIBBLES or a sequence of 4-bit codes; qual: bytes;
    tags: bytes, or a list of tag() results.  The raw overrides make records that disagree with themselves: l_seq and
    n_cigar replace the counts in the fixed part, block_size the length field, low_nibble the unused low half of an odd
    sequence's last byte (zero by the specification)."""
    nm = (name.encode() if isinstance(name, str) else bytes(name)) + b"\0"
    assert 2 <= len(nm) <= 255
    ops = cigar_ops(cigar)
    codes = np.array([NIBBLES.index(c) for c in seq], np.uint8) if isinstance(seq, str) else np.asarray(seq, np.uint8)
    n = int(codes.shape[0])
    assert len(qual) == n and (n == 0 or int(codes.max()) < 16)
    padded = np.zeros((n + 1) // 2 * 2, np.uint8)
    padded[:n] = codes
    if n & 1:
        padded[n] = low_nibble & 15
    packed = ((padded[0::2] << 4) | padded[1::2]).astype(np.uint8).tobytes()
    aux = tags if isinstance(tags, (bytes, bytearray)) else b"".join(tags)
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(nm), mapq, bin_, len(ops) if n_cigar is None else n_cigar, flag,
                       n if l_seq is None else l_seq, next_ref_id, next_pos, tlen) + nm + \
        b"".join(struct.pack("<I", (ln << 4) | op) for ln, op in ops) + packed + bytes(qual) + bytes(aux)
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def bgzf_block(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    assert len(data) <= BGZF_MAX and len(comp) + 26 <= 65536
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + \
        struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def write_bgzf(path, raw, block_sizes=()):
    """Cuts ``raw`` into BGZF blocks of the given inflated sizes (0 ... BGZF_MAX; a 0 is an empty block in the middle of the
    file), what is left after the list into blocks of BGZF_MAX, and ends with the empty end-of-file block.  No index is
    written.  Returns the offsets in ``raw`` at which blocks end."""
    cuts, at = [], 0
    with open(path, "wb") as o:
        for sz in block_sizes:
            sz = min(int(sz), len(raw) - at)
            assert 0 <= sz <= BGZF_MAX
            o.write(bgzf_block(raw[at:at + sz]))
            at += sz
            cuts.append(at)
        while at < len(raw):
            sz = min(BGZF_MAX, len(raw) - at)
            o.write(bgzf_block(raw[at:at + sz]))
            at += sz
            cuts.append(at)
        o.write(_BGZF_EOF)
    return cuts


# ---- parser ------------------------------------------------------------------------------------------------------

def inflate_bgzf(data):
    """The concatenated payloads of a BGZF file (a series of gzip members with a BC extra subfield)."""
    out, p = [], 0
    while p < len(data):
        if p + 18 > len(data):
            raise SpecError("truncated", "BGZF header")
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", data, p)
        if (id1, id2, cm) != (31, 139, 8) or not flg & 4:
            raise SpecError("malformed", "not a BGZF block")
        bsize, q = None, p + 12
        while q + 4 <= p + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, q)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, q + 4)[0]
            q += 4 + slen
        if bsize is None:
            raise SpecError("malformed", "BGZF block without BC")
        end = p + bsize + 1
        if end > len(data):
            raise SpecError("truncated", "BGZF block")
        payload = zlib.decompress(data[p + 12 + xlen:end - 8], -15)
        crc, isize = struct.unpack_from("<II", data, end - 8)
        if len(payload) != isize or zlib.crc32(payload) & 0xffffffff != crc:
            raise SpecError("malformed", "BGZF checksum")
        out.append(payload)
        p = end
    return b"".join(out)


def read_header(raw):
    """-> (text, [(name, length)], offset of the first record)."""
    if raw[:4] != b"BAM\1":
        raise SpecError("malformed", "magic")
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].rstrip(b"\0").decode()
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    contigs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]
        name = raw[p + 4:p + 4 + l_name].split(b"\0")[0].decode()
        length = struct.unpack_from("<i", raw, p + 4 + l_name)[0]
        contigs.append((name, length))
        p += 8 + l_name
    return text, contigs, p


_AUX_SIZE = {65: 1, 99: 1, 67: 1, 115: 2, 83: 2, 105: 4, 73: 4, 102: 4}     # A c C s S i I f


def walk_aux(raw, p, end):
    """The auxiliary fields in raw[p:end] -> (cs value or None, tp byte).  Every field lies inside the record."""
    cs, tp = None, 0
    while p < end:
        if p + 3 > end:
            raise SpecError("malformed", "bytes behind the last auxiliary field")
        t0, t1, ty = raw[p], raw[p + 1], raw[p + 2]
        p += 3
        sz = _AUX_SIZE.get(ty)
        if sz is not None:
            if p + sz > end:
                raise SpecError("malformed", "auxiliary value cut by the record's end")
            if ty == 65 and t0 == 116 and t1 == 112:                          # tp:A
                tp = raw[p]
            p += sz
        elif ty == 90 or ty == 72:                                              # Z, H
            q = raw.find(b"\0", p, end)
            if q < 0:
                raise SpecError("malformed", "string without NUL")
            if ty == 90 and t0 == 99 and t1 == 115:                           # cs:Z
                cs = (cs or b"") + raw[p:q]
            p = q + 1
        elif ty == 66:                                                          # B
            if p + 5 > end:
                raise SpecError("malformed", "array header cut by the record's end")
            es = _AUX_SIZE.get(raw[p])
            if es is None or raw[p] == 65:
                raise SpecError("malformed", "array subtype")
            cnt = struct.unpack_from("<I", raw, p + 1)[0]
            if p + 5 + es * cnt > end:
                raise SpecError("malformed", "array runs past the record's end")
            p += 5 + es * cnt
        else:
            raise SpecError("malformed", "auxiliary type {!r}".format(chr(ty)))
    return cs, tp


def field_spans(raw):
    """(kind, start, end) of the parts of every record of an inflated BAM stream, kinds 'len', 'fixed', 'name', 'cigar',
    'seq', 'qual', 'aux' (tests ask whether a block boundary falls inside one)."""
    _, _, p = read_header(raw)
    out = []
    while p + 4 <= len(raw):
        bs = struct.unpack_from("<I", raw, p)[0]
        l_name, n_cig, l_seq = raw[p + 12], struct.unpack_from("<H", raw, p + 16)[0], struct.unpack_from("<I", raw, p + 20)[0]
        a = p + 4
        b = a + 32
        c = b + l_name
        d = c + 4 * n_cig
        e = d + (l_seq + 1) // 2
        f = e + l_seq
        out += [("len", p, a), ("fixed", a, b), ("name", b, c), ("cigar", c, d), ("seq", d, e), ("qual", e, f),
                ("aux", f, a + bs)]
        p = a + bs
    return out


class Batch:
    """The arrays of a ReadBatch (himut_amd/readbatch.py) for one contig."""

    def __init__(self, name, length, **arrays):
        self.name, self.length = name, length
        for k in FIELDS:
            setattr(self, k, arrays[k])
        self.n = int(self.tstart.shape[0])

    def read_bases(self):
        return int(self.qlen.astype(np.int64).sum())


class Parsed:
    def __init__(self, text, contigs, batches):
        self.header_text, self.contigs, self.batches = text, contigs, batches
        self.tname2tsize = dict(contigs)

    def sample(self):
        for line in self.header_text.split("\n"):
            if line.startswith("@RG"):
                for f in line.split("\t"):
                    if f.startswith("SM:"):
                        return f[3:]
        return None


def parse(path):
    """The read batch of every contig as the reference sees the records through pysam: reference_end from M D N = X,
    query_alignment_start from the leading soft clip (hard clips skipped), the sequence and qualities as stored, cs:Z,
    tp:A.  Kept: mapped records (flag & 4 == 0) with 0 <= ref_id < n_ref.  Raises SpecError."""
    with open(path, "rb") as f:
        raw = inflate_bgzf(f.read())
    text, contigs, p = read_header(raw)
    n_ref = len(contigs)
    cols = [dict(rows=[], seq=[], bq=[], cs=[], names={}, last=None) for _ in range(n_ref)]
    no_cs = 0
    unsorted = False
    fixed = struct.Struct("<iiBBHHHI")
    cigar_of = {}
    size = len(raw)
    while p < size:
        if p + 4 > size:
            raise SpecError("truncated", "length field")
        bs = struct.unpack_from("<I", raw, p)[0]
        if bs < 32:
            raise SpecError("malformed", "block_size below the fixed part")
        a = p + 4
        end = a + bs
        if end > size:
            raise SpecError("truncated", "record")
        p = end
        ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq = fixed.unpack_from(raw, a)
        if flag & 4 or not 0 <= ref_id < n_ref:
            continue
        c0 = a + 32 + l_name
        s0 = c0 + 4 * n_cig
        q0 = s0 + (l_seq + 1) // 2
        x0 = q0 + l_seq
        if x0 > end:
            raise SpecError("malformed", "the record's parts are longer than block_size")
        ref_len = lead = 0
        in_lead = True
        if n_cig not in cigar_of:
            cigar_of[n_cig] = struct.Struct("<{}I".format(n_cig))
        for v in cigar_of[n_cig].unpack_from(raw, c0):
            op, ln = v & 15, v >> 4
            if op in (0, 2, 3, 7, 8):                  # M D N = X consume the reference
                ref_len += ln
            if op == 4:                                # S: counted while nothing but clips came before
                lead += ln if in_lead else 0
            elif op != 5:
                in_lead = False
        cs, tp = walk_aux(raw, x0, end)
        if cs is None:
            no_cs += 1
            continue
        C = cols[ref_id]
        if C["last"] is not None and pos < C["last"]:
            unsorted = True
        C["last"] = pos
        rows = C["rows"]
        qid = C["names"].setdefault(raw[a + 32:a + 32 + l_name].split(b"\0")[0], len(rows))
        rows.append((pos, pos + ref_len, lead, l_seq, mapq, flag, qid, tp, len(cs)))
        pad = -l_seq % 32
        sq = raw[s0:q0]
        if l_seq & 1:
            sq = sq[:-1] + bytes([sq[-1] & 0xf0])
        C["seq"].append(sq + bytes(pad // 2))
        C["bq"].append(raw[q0:x0] + bytes(pad))
        C["cs"].append(cs)
    if no_cs:
        raise SpecError("no_cs", "{} records".format(no_cs), no_cs)
    if unsorted:
        raise SpecError("unsorted")
    batches = {}
    for (name, length), C in zip(contigs, cols):
        r = np.array(C["rows"], np.int64).reshape(-1, 9)
        padded = (r[:, 3] + 31) & ~31
        batches[name] = Batch(
            name, length, tstart=r[:, 0].astype(np.int32), tend=r[:, 1].astype(np.int32), qstart=r[:, 2].astype(np.int32),
            qlen=r[:, 3].astype(np.int32), mapq=r[:, 4].astype(np.uint8), flag=r[:, 5].astype(np.uint16),
            qid=r[:, 6].astype(np.int32), tp=r[:, 7].astype(np.uint8), qoff=np.cumsum(padded) - padded,
            cs_off=np.concatenate([[0], np.cumsum(r[:, 8])]).astype(np.int64),
            seq=np.frombuffer(b"".join(C["seq"]), np.uint8), bq=np.frombuffer(b"".join(C["bq"]), np.uint8),
            cs=np.frombuffer(b"".join(C["cs"]), np.uint8))
    return Parsed(text, contigs, batches)
