"""The indels run's contract (himut_run_indels) in plain Python: nothing of the device side,
nothing of the package.

A read batch, a region list, the contig's string and the run's parameters in; records, the thirteen counters and the VCF
body out.  Events come from the cs text (a regular expression) and SEQ, the left shift looks at the string alone, the
alleles are counted in dictionaries, and the genotype performs the contract's five operations on Python floats."""
import math
import re

import numpy as np

RECORD_DTYPE = np.dtype([("anchor", "<i4"), ("len", "<i4"), ("type", "u1"), ("status", "u1"), ("gt_state", "u1"),
                         ("pad0", "u1"), ("gq", "<i4"), ("dp", "<u4"), ("n_alt", "<u4"), ("n_other", "<u4"),
                         ("pad1", "<u4"), ("bases", "u1", (16,)), ("reserved", "<u4", (4,))])
BASES = "ATGC"
DEL, INS = 0, 1
ST_PASS, ST_LOWGQ, ST_LOWDEPTH, ST_HIGHDEPTH = 0, 2, 9, 10                     # HIMUT_ST_*
FILTER_NAME = {ST_PASS: "PASS", ST_LOWGQ: "LowGQ", ST_LOWDEPTH: "LowDepth", ST_HIGHDEPTH: "HighDepth"}
LOG = ("events", "alleles", "num_edge", "num_long", "num_nbase", "num_dup", "homref", "het", "homalt", "PASS", "LowGQ",
       "LowDepth", "HighDepth")
LOG_SLOT = {ST_PASS: 9, ST_LOWGQ: 10, ST_LOWDEPTH: 11, ST_HIGHDEPTH: 12}
DEFAULTS = dict(min_mapq=0, min_gq=20, min_ref_count=2, min_alt_count=2, md_threshold=1 << 30, max_len=50,
                indel_error=0.01, germline_indel_prior=1 / (10 ** 4), report_homref=False)
_OP = re.compile(r":[0-9]+|\*[a-z][a-z]|[=+\-][A-Za-z]+")
_NIB_BYTES = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)


def logs(indel_error, germline_indel_prior):
    e, pi = indel_error, germline_indel_prior
    return (math.log10(1 - e), math.log10(e), math.log10(0.5), math.log10(1 - 1.5 * pi), math.log10(pi), math.log10(pi / 2))


def query(batch, i):
    """SEQ of read i as letters."""
    o, ql = int(batch.qoff[i]), int(batch.qlen[i])
    packed = np.asarray(batch.seq[o >> 1:(o + ql + 1) >> 1])
    nib = np.empty(packed.shape[0] * 2, np.uint8)
    nib[0::2] = packed >> 4
    nib[1::2] = packed & 15
    return _NIB_BYTES[nib[:ql]].tobytes().decode("ascii")


def raw_events(batch, i):
    """[(type, p, L, s)] of read i in text order: every deletion, every insertion (insertions in a row are one), bases
    from SEQ."""
    cs = bytes(batch.cs[int(batch.cs_off[i]):int(batch.cs_off[i + 1])]).decode("latin-1")
    seq = query(batch, i)
    t, q = int(batch.tstart[i]), int(batch.qstart[i])
    out = []
    prev_ins = False
    for op in _OP.findall(cs):
        k, body = op[0], op[1:]
        if k == ":":
            t += int(body); q += int(body)
        elif k == "=":
            t += len(body); q += len(body)
        elif k == "*":
            t += 1; q += 1
        elif k == "+":
            s = seq[q:q + len(body)]
            if prev_ins:
                ty, p, L, s0 = out.pop()
                out.append((INS, p, L + len(body), s0 + s))
            else:
                out.append((INS, t, len(body), s))
            q += len(body)
        else:
            out.append((DEL, t, len(body), ""))
            t += len(body)
        prev_ins = k == "+"
    return out


def ref_letter(refseq, i):
    """The upper-cased byte at i if it is one of ACGT, else None (a byte behind the end of the string is no letter)."""
    if 0 <= i < len(refseq):
        c = refseq[i].upper()
        if c in BASES:
            return c
    return None


def normalise(refseq, tstart, ty, p, L, s):
    """The left shift of one event of a read that starts at tstart: (p, s)."""
    while p - 1 > tstart:
        c = ref_letter(refseq, p - 1)
        if c is None:
            break
        if ty == DEL:
            if c != ref_letter(refseq, p + L - 1):
                break
        else:
            if c != s[L - 1]:
                break
            s = s[L - 1] + s[:L - 1]
        p -= 1
    return p, s


def apply_allele(refseq, ty, p, L, s):
    """The contig's string (upper case) with the event applied: what the left shift must not change."""
    u = refseq.upper()
    return u[:p] + u[p + L:] if ty == DEL else u[:p] + s + u[p:]


def genotype(n_non, n_alt, lg):
    """(state, gq, PLs): the contract's operations in its order."""
    l_hit, l_err, l_half, p0, p1, p2 = lg
    pls = []
    for prior, x, y in ((p0, l_hit, l_err), (p1, l_half, l_half), (p2, l_err, l_hit)):
        t = float(n_non) * x
        u = float(n_alt) * y
        total = prior + t
        total = total + u
        pls.append(-10.0 * total)
    order = sorted(range(3), key=lambda g: pls[g])              # stable: ties to the lower index
    gqf = pls[order[1]] - pls[order[0]]
    return order[0], (int(gqf) if gqf < 99.0 else 99), pls


def in_regions(regions, a):
    return any(s <= a <= e for s, e in regions)


def pack_bases(s):
    out = [0] * 16
    for i, b in enumerate(s):
        out[i >> 2] |= BASES.index(b) << (2 * (i & 3))
    return out


def unpack_bases(rec):
    return "".join(BASES[(int(rec["bases"][i >> 2]) >> (2 * (i & 3))) & 3] for i in range(int(rec["len"]))) if int(rec["type"]) == INS else ""


def collect(batch, regions, refseq, **kw):
    """What does not depend on the genotype's parameters: ([(allele, n_alt, n_other, dp)] in record order, the first six
    counters); allele = (a, type, L, codes)."""
    p = dict(DEFAULTS, **kw)
    assert 1 <= p["max_len"] <= 64
    regions = [(int(s), int(e)) for s, e in regions]
    log = [0] * 13
    pile = []                                                   # (tstart, tend) of the pile reads
    carriers = {}                                               # allele -> [read, ...] (a read once per event)
    at_anchor = {}                                              # anchor -> set of reads
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100 or int(batch.mapq[i]) < p["min_mapq"]:
            continue
        ts, te = int(batch.tstart[i]), int(batch.tend[i])
        pile.append((ts, te))
        for ty, pos, L, s in raw_events(batch, i):
            end = pos if ty == INS else pos + L
            if not (ts <= pos - 1 and end < te):
                log[2] += 1
                continue
            if L > p["max_len"]:
                log[3] += 1
                continue
            if any(b not in BASES for b in s):
                log[4] += 1
                continue
            pos, s = normalise(refseq, ts, ty, pos, L, s)
            a = pos - 1
            if not in_regions(regions, a):
                continue
            log[0] += 1
            carriers.setdefault((a, ty, L, tuple(BASES.index(b) for b in s)), []).append(i)
            at_anchor.setdefault(a, set()).add(i)
    items = []
    for allele in sorted(carriers):                             # anchor, deletions first, length, the string in code order
        a, ty, L, _codes = allele
        reads = carriers[allele]
        n_alt = len(set(reads))
        log[5] += len(reads) - n_alt
        end = a + 1 if ty == INS else a + 1 + L
        dp = sum(1 for ts, te in pile if ts <= a and end < te)
        assert dp >= n_alt
        items.append((allele, n_alt, len(at_anchor[a]) - n_alt, dp))
    return items, log


def evaluate(items, base_log, **kw):
    """(records, log[13]) of collect's alleles under the genotype's parameters."""
    p = dict(DEFAULTS, **kw)
    lg = logs(p["indel_error"], p["germline_indel_prior"])
    log = list(base_log)
    out = []
    for (a, ty, L, codes), n_alt, n_other, dp in items:
        n_non = dp - n_alt
        state, gq, _pls = genotype(n_non, n_alt, lg)
        log[1] += 1
        log[6 + state] += 1
        status = ST_PASS
        if state != 0:
            if gq < p["min_gq"]:
                status = ST_LOWGQ
            elif n_alt < p["min_alt_count"] or (state == 1 and n_non < p["min_ref_count"]):
                status = ST_LOWDEPTH
            elif dp > p["md_threshold"]:
                status = ST_HIGHDEPTH
            log[LOG_SLOT[status]] += 1
        if state == 0 and not p["report_homref"]:
            continue
        out.append((a, L, ty, status, state, 0, gq, dp, n_alt, n_other, 0, pack_bases("".join(BASES[c] for c in codes)),
                    [0, 0, 0, 0]))
    return np.array(out, RECORD_DTYPE) if out else np.zeros(0, RECORD_DTYPE), log


def run(batch, regions, refseq, **kw):
    """(records, log[13])."""
    items, log = collect(batch, regions, refseq, **kw)
    return evaluate(items, log, **kw)


def vcf_lines(chrom, recs, refseq):
    """The data lines of the records of one contig (homref records are not printed): chrom, anchor + 1, ".", REF, ALT, gq,
    FILTER, ".", GT:GQ:DP:AD:NO, sample; AD = n_ref,n_alt with n_ref = DP - n_alt - n_other, not below 0."""
    out = []
    u = refseq.upper()
    for r in recs:
        st = int(r["gt_state"])
        if st == 0:
            continue
        a, L = int(r["anchor"]), int(r["len"])
        if int(r["type"]) == DEL:
            ref, alt = u[a:a + 1 + L], u[a]
        else:
            ref, alt = u[a], u[a] + unpack_bases(r)
        dp, n_alt, n_other = int(r["dp"]), int(r["n_alt"]), int(r["n_other"])
        out.append("\t".join([chrom, str(a + 1), ".", ref, alt, str(int(r["gq"])), FILTER_NAME[int(r["status"])], ".",
                              "GT:GQ:DP:AD:NO", "{}:{}:{}:{},{}:{}".format("0/1" if st == 1 else "1/1", int(r["gq"]), dp,
                                                                          max(0, dp - n_alt - n_other), n_alt, n_other)]) + "\n")
    return out


def assert_same(got, got_log, want, want_log):
    assert [int(x) for x in got_log] == [int(x) for x in want_log], (dict(zip(LOG, got_log)), dict(zip(LOG, want_log)))
    assert len(got) == len(want), (len(got), len(want))
    for name in RECORD_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (name, got[name][:8], want[name][:8])
    assert got.tobytes() == want.tobytes()
