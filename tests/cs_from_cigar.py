"""The derivation rule of DESIGN 11 restated in plain Python (the cs text of a record from its CIGAR, SEQ and the
reference bases under the alignment), the way back (a CIGAR from a cs text, in M form and in =/X form), and the inputs
the tests of the deriving ingest share: records written by hand with their texts as literals, the synthetic samples,
BAM files of a read batch packed through tests/bam_spec.py.  A helper: no test lives here, and nothing of the code under
test is used to work out an expected text."""
import numpy as np

from tests import bam_spec

M, I, D, N, S, H, P, EQ, X = range(9)
_LOW = {"A": "a", "C": "c", "G": "g", "T": "t"}
_NIB_LOW = {1: "a", 2: "c", 4: "g", 8: "t"}


def derive_cs(cigar, pos, codes, ref):
    """cigar: [(length, op index)] or a string; codes: the record's SEQ as 4-bit codes; ref: the contig (str or bytes).
    -> the short-form cs text, or None for a record whose text cannot be derived."""
    ops = bam_spec.cigar_ops(cigar)
    ref = ref.decode("latin-1") if isinstance(ref, (bytes, bytearray)) else ref
    codes = [int(c) for c in codes]
    if not ops or any(op in (N, P) or op > X for _, op in ops):
        return None
    if sum(ln for ln, op in ops if op in (M, I, S, EQ, X)) != len(codes):
        return None
    if pos < 0 or pos + sum(ln for ln, op in ops if op in (M, D, EQ, X)) > len(ref):
        return None
    out, t, q, run = [], pos, 0, 0

    def flush():
        nonlocal run
        if run > 0:
            out.append(":{}".format(run))
        run = 0

    for ln, op in ops:
        if op in (M, EQ, X):
            for _ in range(ln):
                r, b = ref[t].upper(), codes[q]
                if r in _LOW and _NIB_LOW.get(b) == _LOW[r]:
                    run += 1
                else:
                    flush()
                    out.append("*" + _LOW.get(r, "n") + _NIB_LOW.get(b, "n"))
                t += 1
                q += 1
        elif op == I:
            flush()
            out.append("+" + "".join(_NIB_LOW.get(b, "n") for b in codes[q:q + ln]))
            q += ln
        elif op == D:
            flush()
            out.append("-" + "".join(_LOW.get(c.upper(), "n") for c in ref[t:t + ln]))
            t += ln
        elif op == S:
            q += ln
    flush()
    return "".join(out)


def cs_to_cigar(cs, qstart, qlen, form):
    """The CIGAR an aligner would have written beside this cs text.  form "M": S, merged M, I, D, S; form "EQX": every
    *xy is 1X and every :n (or =ACGT) is n=, nothing merged."""
    cs = cs.decode() if isinstance(cs, (bytes, bytearray)) else cs
    ops, qcons = [], qstart
    if qstart > 0:
        ops.append((qstart, S))

    def push(op, ln):
        if ln == 0:
            return
        if form == "M" and ops and ops[-1][1] == op:
            ops[-1] = (ops[-1][0] + ln, op)
        else:
            ops.append((ln, op))

    i = 0
    while i < len(cs):
        c, j = cs[i], i + 1
        if c == ":":
            while j < len(cs) and cs[j].isdigit():
                j += 1
            ln = int(cs[i + 1:j])
            push(M if form == "M" else EQ, ln)
            qcons += ln
        elif c == "*":
            j = i + 3
            push(M if form == "M" else X, 1)
            qcons += 1
        else:
            while j < len(cs) and cs[j].isalpha():
                j += 1
            ln = j - i - 1
            if c == "=":
                push(M if form == "M" else EQ, ln)
                qcons += ln
            elif c == "+":
                push(I, ln)
                qcons += ln
            else:
                assert c == "-", cs[i:i + 10]
                push(D, ln)
        i = j
    if qlen > qcons:
        ops.append((qlen - qcons, S))
    return ops


def read_codes(batch, i):
    """The 4-bit codes of read i of a read batch."""
    o, n = int(batch.qoff[i]), int(batch.qlen[i])
    b = np.asarray(batch.seq[o // 2:o // 2 + (n + 1) // 2])
    return np.stack([b >> 4, b & 15], 1).reshape(-1)[:n]


def read_cs(batch, i):
    return bytes(batch.cs[int(batch.cs_off[i]):int(batch.cs_off[i + 1])]).decode()


def batch_records(batch, form, with_cs=False, ref_id=0, bare=()):
    """One contig's read batch as records packed by bam_spec: CIGARs in the given form from the cs texts, the tp tag kept,
    the cs tag only if asked for and never on the reads whose ordinals ``bare`` lists; names as bamio.write_bam gives
    them."""
    recs = []
    for i in range(batch.n):
        cs = read_cs(batch, i)
        tags = [bam_spec.tag("cs", "Z", cs)] if with_cs and i not in bare else []
        if batch.tp[i]:
            tags.append(bam_spec.tag("tp", "A", bytes([int(batch.tp[i])])))
        o, n = int(batch.qoff[i]), int(batch.qlen[i])
        recs.append(bam_spec.record(ref_id, int(batch.tstart[i]), "ccs/{}".format(int(batch.qid[i])), int(batch.mapq[i]),
                                    int(batch.flag[i]), cs_to_cigar(cs, int(batch.qstart[i]), n, form),
                                    read_codes(batch, i), bytes(batch.bq[o:o + n]), tags))
    return recs


def batch_bam(path, batch, form, with_cs=False, sample="syn"):
    """One contig's read batch as a BAM: batch_records under a header of its own."""
    recs = batch_records(batch, form, with_cs)
    bam_spec.write_bgzf(path, bam_spec.header([(batch.name, batch.length)], sample) + b"".join(recs))


# ---- the synthetic samples of the GPU tests

SYNTH_SEEDS = (41, 42, 43)
SYNTH_RATES = ((2e-3, 1e-3, 1e-3), (1e-2, 5e-3, 5e-3))          # substitutions, insertions, deletions
_samples = {}


def synth_sample(seed, rates):
    from himut_amd import synth
    key = (seed, rates)
    if key not in _samples:
        _samples[key] = synth.generate(synth.SynthConfig(
            seed=seed, contig_len=40_000, depth=12, read_len_mean=3000, read_len_sd=600, read_len_min=1000,
            read_len_max=6000, frac_softclip=0.3, softclip_max=50, sub_rate=rates[0], ins_rate=rates[1],
            del_rate=rates[2], name="chrD"), want_ref=True)
    return _samples[key]


# ---- records written by hand

def hand_reference(length=5000, seed=7):
    """ACGT from a seeded generator with a few stretches spelled out: the bases under the literal records below, an N
    run, a soft-masked stretch, one IUPAC code."""
    rs = np.random.RandomState(seed)
    ref = bytearray(bytes(rs.choice(np.frombuffer(b"ACGT", np.uint8), length)))
    ref[100:114] = b"ACGTACGTACGTAC"
    ref[200:217] = b"GATTACAGATTACAGAT"
    ref[300:312] = b"AACCGGTTAACC"
    ref[4500:4540] = b"N" * 40
    ref[4600:4700] = bytes(ref[4600:4700]).lower()
    ref[4650:4658] = b"acgtacgt"
    ref[4800] = ord("R")
    ref[4900:4908] = b"ACGTNNAC"
    return bytes(ref)


LONG_LEN = 10_200


def long_reference(seed=8):
    rs = np.random.RandomState(seed)
    return bytes(rs.choice(np.frombuffer(b"ACGT", np.uint8), LONG_LEN))


_COMP = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _query(ref, pos, cigar, mism=(), ins="ACGTTGCA", clip="TTGCA"):
    """A query for the CIGAR: the reference's bases (upper case; A where the reference has none of ACGT) under M = X, the
    columns listed in ``mism`` (counted over the M = X columns) replaced by another base, insertions and clips from
    fixed strings."""
    out, t, col = [], pos, 0
    for ln, op in bam_spec.cigar_ops(cigar):
        if op in (M, EQ, X):
            for _ in range(ln):
                r = chr(ref[t]).upper()
                r = r if r in _COMP else "A"
                out.append(_COMP[r] if col in mism else r)
                t += 1
                col += 1
        elif op == I:
            out.append((ins * (ln // len(ins) + 1))[:ln])
        elif op == S:
            out.append((clip * (ln // len(clip) + 1))[:ln])
        elif op == D:
            t += ln
    return "".join(out)


def hand_cases():
    """[(contig, pos, cigar, seq, literal or None, tags kept)] sorted by contig and position.  contig 0: the 5 kb
    reference, contig 1: the long one.  The literals were written by hand from the reference stretches spelled out in
    hand_reference."""
    ref, lref = hand_reference(), long_reference()
    c = []

    def add(contig, pos, cigar, seq=None, literal=None, mism=(), tags="tp"):
        r = ref if contig == 0 else lref
        c.append((contig, pos, cigar, _query(r, pos, cigar, mism) if seq is None else seq, literal, tags))

    # ref[100:114] = ACGTACGTACGTAC: 5M ACGTA (query ACCTA), 1I g, 3M CGT, 2D ac, 2M GT
    add(0, 100, "2S5M1I3M2D2M", "TT" + "ACCTA" + "G" + "CGT" + "GT", ":2*gc:2+g:3-ac:2")
    # ref[200:217] = GATTACAGATTACAGAT: adjacent M = X without a mismatch are one run
    add(0, 200, "5M5=3X4M", "GATTACAGATTACAGAT", ":17")
    # a mismatch in the first and in the last column; ref[300:312] = AACCGGTTAACC
    add(0, 300, "12M", "CACCGGTTAACC", "*ac:11")
    add(0, 300, "12M", "AACCGGTTAACA", ":11*ca")
    add(0, 300, "6=6M", "TACCGGTTAACG", "*at:10*cg")
    # the reference's N, an IUPAC code, query N (nibble 15) and another ambiguity code (M = 3)
    add(0, 4900, "8M", "ACGTACAC", ":4*na*nc:2")
    add(0, 4900, "4M", "ANGM", ":1*cn:1*tn")
    # soft-masked reference ref[4650:4658] = acgtacgt: the upper-cased letter decides
    add(0, 4650, "8M", "ACGTACCT", ":6*gc:1")
    add(0, 4648, "2S3I4M3D2M1S", "TT" + "NAC" + "ACGT" + "TC" + "G", None)
    # every digit count of a match run
    for k, ln in enumerate((9, 10, 99, 100, 999, 1000)):
        add(0, 400 + k, "{}M".format(ln), literal=":{}".format(ln))
    add(1, 0, "9999M", literal=":9999")
    add(1, 100, "10000M", literal=":10000")
    add(1, 150, "3S4000=2I3000=1D2999=", None)
    # mismatches at the borders of the 64-column steps
    for mm in ((63,), (64,), (65,), (63, 64, 65), (127, 128), (0, 129), (62, 63, 126, 127, 128, 129)):
        add(0, 1500, "130M", mism=mm)
    add(0, 1510, "60M10=70X", mism=(59, 60, 69, 70, 139))
    # indels at the ends, next to each other, beside clips; hard clips; an odd leading clip
    add(0, 1600, "3S2I10M")
    add(0, 1610, "10M3D4S")
    add(0, 1620, "5M2I3D5M", mism=(4, 5))
    add(0, 1630, "2H3S10M2S3H")
    add(0, 1640, "1S70M", mism=(0, 63, 64))
    add(0, 1650, "7S3M1D1I1D3M")
    # the shortest records; one with no auxiliary field at all whose text is three times its sequence
    add(0, 1700, "1M")
    add(0, 1701, "1M", mism=(0,))
    add(0, 1710, "33M", mism=(32,))
    add(0, 1720, "40M", mism=tuple(range(40)), tags="")
    # a record that carries a cs tag of its own (a wrong one): ignored
    add(0, 1800, "20M", mism=(7,), tags="tp,cs")
    # across the N run, the IUPAC code and the soft-masked stretch
    add(0, 4480, "80M", mism=(3,))
    add(0, 4590, "120M", mism=(5, 50))
    add(0, 4790, "5M4D8M")
    add(0, 4495, "3M10D3M")
    add(0, 4990, "10M")                                   # ends with the contig
    c.sort(key=lambda x: (x[0], x[1]))
    return c


def hand_bam(path, tagged):
    """The hand records as a BAM of two contigs.  tagged: every record carries the cs text derive_cs gives it (what the
    ingest reads without the derivation); else no record has a cs tag but the one whose tag is wrong.  -> per contig the
    list of expected texts."""
    refs = (hand_reference(), long_reference())
    recs, want = [], ([], [])
    for k, (contig, pos, cigar, seq, _lit, tags) in enumerate(hand_cases()):
        codes = [bam_spec.NIBBLES.index(ch) for ch in seq]
        cs = derive_cs(cigar, pos, codes, refs[contig])
        want[contig].append(cs)
        aux = []
        if tagged:
            aux.append(bam_spec.tag("cs", "Z", cs))
        elif "cs" in tags:
            aux.append(bam_spec.tag("cs", "Z", ":1"))
        if "tp" in tags:
            aux.append(bam_spec.tag("tp", "A", b"P"))
        recs.append(bam_spec.record(contig, pos, "h{}".format(k), 60, 0, cigar, seq, bytes([40 + k % 50] * len(seq)), aux))
    bam_spec.write_bgzf(path, bam_spec.header([("hand", len(refs[0])), ("long", LONG_LEN)], "hand") + b"".join(recs))
    return want
