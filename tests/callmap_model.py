"""The callable run's contract (Row 9; himut_run_callable) in plain Python and numpy: the state
and the callable bases of every swept position, the runs of equal state, the fourteen counters.

It restates normcounts.get_callable_tricounts (normcounts.py:243-402) per position and keeps the verdict where the
reference folds it into counters.  Built from what the tests own already: the read filters and the per-base rule of
tests/callable_model.py (its tokenizer, mismatch list, window and trim functions; ``counted_mask`` below is its
``counted`` over numpy arrays, and tests/test_callmap_cpu.py holds the two against each other), and the pile of
tests/germline_model.PileRead (update_allelecounts).  The genotype is gtlib.get_germ_gt / get_germ_gq written out here:
the three tables from the formulas of gtlib.py:47-69, the sums per allele in fetch order, the ten PLs, numpy's stable
argsort.  Nothing of the library, of oracle.normcounts or of the device side."""
import bisect
import math

import numpy as np

from tests import callable_model as CM
from tests.germline_model import BASES, DEL, NONE, OTHER, ModelError, PileRead

NON_ACGT, NO_BASE, UNPHASED, HET, HETALT, HOMALT = 0, 1, 2, 3, 4, 5
INDEL, HIGH_DEPTH, ALLELE_BALANCE, LOW_GQ, PON, COMMON_SNP, CALLABLE = 7, 8, 9, 10, 11, 12, 13
STATE_NAMES = {0: "NON_ACGT", 1: "NO_BASE", 2: "UNPHASED", 3: "HET", 4: "HETALT", 5: "HOMALT", 7: "INDEL",
               8: "HIGH_DEPTH", 9: "ALLELE_BALANCE", 10: "LOW_GQ", 11: "PON", 12: "COMMON_SNP", 13: "CALLABLE"}
ERR_ARG, ERR_BASE, ERR_BQ0, ERR_COVER = 1, 4, 5, 7                     # HIMUT_ERR_*
RUN_DTYPE = np.dtype([("chunk", "<i4"), ("start", "<i4"), ("end", "<i4"), ("state", "<i4"), ("bases", "<i8")])
GT_LST = ["AA", "TA", "CA", "GA", "TT", "CT", "GT", "CC", "GC", "GG"]   # gtlib.py:9
GT_IDX = [(BASES.index(g[0]), BASES.index(g[1])) for g in GT_LST]
BLOCK = 2048                                                            # positions of a chunk laid out at a time
PURINE2PYRIMIDINE = {"A": "T", "T": "A", "G": "C", "C": "G", "N": "N"}


# ---------------------------------------------------------------------------------------------- genotype (gtlib.py)
def gt_tables():
    """[3][256]: log10(1 - e), log10(0.5 - e / 2), log10(e(bq / 3)) with e(bq) = 10 ** (-bq / 10); quality 0 (log10(0)
    in the reference) is left 0.0 and looked for by the caller."""
    t = np.zeros((3, 256))
    for bq in range(1, 256):
        eps = 10 ** (-bq / 10)
        t[0, bq] = math.log10(1 - eps) if eps < 1 else 0.0
        t[1, bq] = math.log10(0.5 - eps / 2.0)
        t[2, bq] = math.log10(10 ** (-(bq / 3) / 10))
    return t


def gt_priors(prior):
    """log10 prior of homref, het, hetalt, homalt (gtlib.init)."""
    return [math.log10(1 - ((1.5 * prior) + (prior * prior))), math.log10(prior), math.log10(prior * prior * 2),
            math.log10(prior / 2)]


def gt_state(b1, b2, ref):
    if b1 == b2 == ref:
        return 0
    if (b1 == ref) != (b2 == ref):
        return 1
    return 2 if b1 != b2 else 3


def gt_pls(S, ref, logp, skip=None):
    """The ten PLs of columns whose sums are S[table][allele] (arrays over columns or scalars), reference allele index
    ``ref`` (an array or a scalar); ``skip``: the allele get_germ_gq leaves out."""
    out = []
    for b1, b2 in GT_IDX:
        acc = 0
        for b in range(4):
            if b == skip:
                continue
            if b1 == b2 and b == b1:
                acc = acc + S[0][b]
            elif b1 != b2 and (b == b1 or b == b2):
                acc = acc + S[1][b]
            else:
                acc = acc + S[2][b]
        if np.ndim(ref) == 0:
            pr = logp[gt_state(b1, b2, int(ref))]
        else:
            pr = np.array([logp[gt_state(b1, b2, r)] for r in range(4)])[ref]
        out.append((acc + pr) * -10)
    return out


def gq_of(pls):
    """get_argmin_gt's gq for one column: the gap between the two smallest PLs, cut at 99."""
    s = sorted(pls)
    g = s[1] - s[0]
    return int(g) if g < 99 else 99


# ---------------------------------------------------------------------------------------------- the reads
def counted_mask(tstart, tend, qstart, qlen, bq, cs, p):
    """callable_model.counted over arrays: bool[tend - tstart + 1], True where the read's base over that reference
    position counts (update_tri2count)."""
    w, maxmm, min_bq = p["mismatch_window_size"], p["max_mismatch_count"], p["min_bq"]
    tuples = CM.cs_tuples(cs)
    mis = np.array(CM.mismatch_positions(tstart, tuples), np.int64)
    lo, hi = CM.trimmed_range(qlen, p["min_trim"])
    bq = np.asarray(bq, np.int64)
    out = np.zeros(tend - tstart + 1, bool)
    rpos, qpos = tstart, qstart
    for state, _ref, ref_len, alt_len in tuples:
        if state == 1:
            ts, te = CM.mismatch_range(rpos, qpos, qlen, w)
            j = np.arange(ref_len, dtype=np.int64)
            count = np.searchsorted(mis, te + j, side="right") - np.searchsorted(mis, ts + j, side="left")
            q = qpos + j
            ok = (bq[q] >= min_bq) & (count <= maxmm) & ~((q < lo) | (q > hi))
            out[rpos - tstart:rpos - tstart + ref_len] = ok
        elif state == 2:
            out[rpos - tstart] = True
        rpos += ref_len
        qpos += alt_len
    return out


def ccs_hap(r, hbit_lst, hpos_lst, hetsnp_lst):
    """haplib.get_ccs_hap for a pile read: "0", "1" or "."."""
    idx = bisect.bisect_right(hpos_lst, r.tstart)
    jdx = bisect.bisect_right(hpos_lst, r.real_tend)
    if jdx - idx < 2:
        return "."
    h0 = "".join(hbit_lst[k] for k in range(idx, jdx))
    h1 = "".join({"0": "1", "1": "0", "-": "-"}[b] for b in h0)
    bits = ""
    for k in range(idx, jdx):
        pos1, ref, alt = hetsnp_lst[k][0], hetsnp_lst[k][1], hetsnp_lst[k][2]
        o = pos1 - 1 - r.tstart
        cell = int(r.cell[o]) if 0 <= o < r.real_tend - r.tstart else NONE
        if cell == NONE:
            raise ModelError(ERR_COVER)                                    # KeyError in tpos2qbase
        qbase = "-" if cell == DEL else BASES[cell] if cell < 4 else "?"
        bits += "0" if qbase == ref else "1" if qbase == alt else "-"
    return "0" if h0 == bits else "1" if h1 == bits else "."


class Result:
    def __init__(self, chunks, state, bases, log):
        self.chunks, self.state, self.bases, self.log = chunks, state, bases, log
        self.mapoff = np.concatenate([[0], np.cumsum([max(e - s, 0) for s, e in chunks])]).astype(np.int64)
        self.runs = runs_of(chunks, state, bases)


def runs_of(chunks, state, bases):
    """The runs of a map (the chunks' positions one behind the other): per chunk the maximal stretches of equal state."""
    out, off = [], 0
    for k, (s, e) in enumerate(chunks):
        n = max(e - s, 0)
        st, bs = state[off:off + n], bases[off:off + n].astype(np.int64)
        if n:
            cut = np.concatenate([[0], np.flatnonzero(st[1:] != st[:-1]) + 1, [n]])
            csum = np.concatenate([[0], np.cumsum(bs)])
            for a, b in zip(cut[:-1], cut[1:]):
                out.append((k, s + int(a), s + int(b), int(st[a]), int(csum[b] - csum[a])))
        off += n
    return np.array(out, RUN_DTYPE) if out else np.zeros(0, RUN_DTYPE)


def merged_lines(runs):
    """What the BED writer makes of the runs: (start, end, state, bases), runs of equal state that abut across a chunk
    boundary joined and their bases added; everything else as it comes."""
    out = []
    for r in runs:
        if out and out[-1][4] != int(r["chunk"]) and out[-1][1] == int(r["start"]) and out[-1][2] == int(r["state"]):
            out[-1] = [out[-1][0], int(r["end"]), out[-1][2], out[-1][3] + int(r["bases"]), int(r["chunk"])]
        else:
            out.append([int(r["start"]), int(r["end"]), int(r["state"]), int(r["bases"]), int(r["chunk"])])
    return [tuple(x[:4]) for x in out]


def get_tri_context(seq, pos):
    """normcounts.get_tri_context."""
    tri = seq[max(pos - 1, 0):pos + 2] if pos - 1 >= 0 else ""
    if len(tri) == 3:
        if tri[1] in "AG":
            return "".join(PURINE2PYRIMIDINE.get(b, "N") for b in tri[::-1])
        return tri
    return "NNN"


def fold(res, refseq):
    """(log rows 1..13 from the map, ref_tri2count, ccs_tri2count): the sums the reference keeps."""
    seq = refseq.decode("latin-1") if isinstance(refseq, (bytes, bytearray)) else refseq
    rows = [0] * 14
    ref_tri, ccs_tri = {}, {}
    for k, (s, e) in enumerate(res.chunks):
        off = int(res.mapoff[k])
        st, bs = res.state[off:off + max(e - s, 0)], res.bases[off:off + max(e - s, 0)].astype(np.int64)
        for code in range(2, 14):
            rows[code] += int(bs[st == code].sum())
        for i in np.flatnonzero(st == CALLABLE):
            tri = get_tri_context(seq, s + int(i))
            ref_tri[tri] = ref_tri.get(tri, 0) + 1
            ccs_tri[tri] = ccs_tri.get(tri, 0) + int(bs[i])
    rows[1] = sum(rows[2:6]) + sum(rows[7:14])
    rows[6] = sum(rows[7:14])
    return rows, ref_tri, ccs_tri


def site_key_set(keys):
    return set() if keys is None else set(int(k) for k in keys)


def run(batch, refseq, chunks, p, pon_keys=None, com_keys=None, alt_order=None, non_human_sample=False, phase=None):
    """The map, the runs and the counters of one contig.  p: the worker's parameters (tests/util.params_of);
    pon_keys / com_keys: (tpos << 4 | ref << 2 | alt) in himut's allele indices; alt_order: {ref: [alt, alt, alt]}, the
    order python gave set("ATGC").difference(ref); phase: (hbit, hpos, hetsnp) dictionaries keyed by str(chunk start).
    Raises ModelError with the code the run returns."""
    seq = refseq.decode("latin-1") if isinstance(refseq, (bytes, bytearray)) else refseq
    chunks = [(int(s), int(e)) for s, e in chunks]
    pon, com = site_key_set(pon_keys), site_key_set(com_keys)
    order = alt_order if alt_order is not None else {r: list(set(BASES).difference(r)) for r in BASES}
    T, logp = gt_tables(), gt_priors(p["germline_snv_prior"])
    # the primary reads in file order: the pile of each, whether it passes the read filters, which of its bases count
    reads = []
    for i in range(batch.n):
        if int(batch.flag[i]) & 0x100:
            continue
        r = PileRead(batch, i)
        r.real_tend = r.tend
        r.index = i
        r.live = CM.read_is_live(batch, i, chunks, p)
        r.counted = None
        reads.append(r)
    if any(r.bad_base and any(s < r.tend and e > r.tstart for s, e in chunks) for r in reads):
        raise ModelError(ERR_BASE)
    N = sum(max(e - s, 0) for s, e in chunks)
    state, bases = np.zeros(N, np.uint8), np.zeros(N, np.uint16)
    log = [0] * 14
    seen = set()
    bq0 = False
    off = 0
    for (s, e) in chunks:
        if e > s and (s < 0 or e > len(seq)):
            raise ModelError(ERR_ARG)                                      # IndexError in the reference
        fetched = [r for r in reads if r.tstart < e and r.tend > s]         # file order = fetch order
        haps = {}
        if phase is not None:
            hbit, hpos, hetsnp = (d.get(str(s), []) for d in phase)
            haps = {id(r): ccs_hap(r, hbit, hpos, hetsnp) for r in fetched}
        for r in fetched:
            if r.live and (phase is None or haps[id(r)] in "01"):
                seen.add(batch.query_name(r.index))
                if r.counted is None:
                    r.counted = counted_mask(r.tstart, r.tend, int(batch.qstart[r.index]), int(batch.qlen[r.index]),
                                             batch.query_qualities(r.index), batch.cs_tag(r.index), p)
        for b0 in range(s, e, BLOCK):
            b1 = min(b0 + BLOCK, e)
            W = b1 - b0
            rows = [r for r in fetched if r.tstart < b1 and r.tend >= b0]
            cnt = np.zeros((6, W), np.int64)
            tri = np.zeros(W, np.int64)
            h0, h1 = np.zeros(W, np.int64), np.zeros(W, np.int64)
            S = np.zeros((3, 4, W))
            zero_q = np.zeros(W, bool)
            for r in rows:
                lo, hi = max(r.tstart, b0), min(r.tend + 1, b1)             # (a trailing insertion sits at tend)
                a, b = lo - r.tstart, hi - r.tstart
                cell, q = r.cell[a:b], r.bq[a:b]
                sl = slice(lo - b0, hi - b0)
                cnt[4, sl] += r.ins[a:b]
                cnt[5, sl] += cell == DEL
                base = cell < 4
                zero_q[sl] |= base & (q == 0)
                for al in range(4):
                    m = cell == al
                    if m.any():
                        cnt[al, sl] += m
                        for t in range(3):
                            S[t, al, sl] = np.where(m, S[t, al, sl] + T[t][q], S[t, al, sl])
                hap = haps.get(id(r), ".")
                if hap == "0":
                    h0[sl] += base
                elif hap == "1":
                    h1[sl] += base
                if r.live and (phase is None or hap in "01"):
                    tri[sl] += r.counted[a:b] & base
            refc = np.frombuffer(seq[b0:b1].encode("latin-1"), np.uint8)
            ref = np.full(W, -1, np.int64)
            for al, ch in enumerate(BASES):
                ref[refc == ord(ch)] = al
            st = np.full(W, NON_ACGT, np.int64)
            st[(ref >= 0) & (tri == 0)] = NO_BASE
            go = (ref >= 0) & (tri > 0)
            if phase is not None:
                unph = go & ~((h0 >= p["min_hap_count"]) & (h1 >= p["min_hap_count"]))
                st[unph] = UNPHASED
                go &= ~unph
            if (go & zero_q).any():
                bq0 = True                                                  # log10(0) in the reference
            refx = np.where(ref >= 0, ref, 0)
            pls = np.array(gt_pls(S, refx, logp))                           # [10][W]
            best = np.argmin(pls, axis=0)                                   # (the first of equal PLs, as the stable sort)
            srt = np.sort(pls, axis=0)
            gap = srt[1] - srt[0]
            gq = np.where(gap < 99, gap, 99).astype(np.int64)
            gstate = np.array([[gt_state(b1_, b2_, r_) for r_ in range(4)] for b1_, b2_ in GT_IDX])[best, refx]
            depth = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[5]
            ref_count = cnt[refx, np.arange(W)]
            for gs, code in ((1, HET), (2, HETALT), (3, HOMALT)):
                st[go & (gstate == gs)] = code
            hr = go & (gstate == 0)
            indel = hr & ((cnt[4] != 0) | (cnt[5] != 0))
            st[indel] = INDEL
            deep = hr & ~indel & (depth > p["md_threshold"])
            st[deep] = HIGH_DEPTH
            rest = hr & ~indel & ~deep
            plain = rest & (depth == ref_count)
            st[plain] = np.where(gq < p["min_gq"], LOW_GQ, np.where(ref_count < p["min_ref_count"], ALLELE_BALANCE, CALLABLE))[plain]
            for x in np.flatnonzero(rest & ~plain):                        # a column with another allele (normcounts.py:367-400)
                rch = BASES[ref[x]]
                alts = [BASES.index(a) for a in order[rch]]
                counts, verdict = [], None
                for al in alts:
                    counts.append(int(cnt[al, x]))
                    if counts[-1] == 0 or non_human_sample:
                        continue
                    key = ((b0 + int(x) + 1) << 4) | (int(ref[x]) << 2) | al
                    if key in pon:
                        verdict = PON
                        break
                    if key in com:
                        verdict = COMMON_SNP
                        break
                if verdict is None:
                    al = alts[counts.index(max(counts))]
                    g2 = gq_of(gt_pls([[S[t, b_, x] for b_ in range(4)] for t in range(3)], int(ref[x]), logp, skip=al))
                    if g2 < p["min_gq"]:
                        verdict = LOW_GQ
                    elif not (ref_count[x] >= p["min_ref_count"] and cnt[al, x] >= p["min_alt_count"]):
                        verdict = ALLELE_BALANCE
                    else:
                        verdict = CALLABLE
                st[x] = verdict
            state[off:off + W] = st
            bases[off:off + W] = np.where(st >= UNPHASED, tri, 0)
            assert tri.max(initial=0) <= 65535
            off += W
    if bq0:
        raise ModelError(ERR_BQ0)
    res = Result(chunks, state, bases, log)
    rows, _r, _c = fold(res, seq)
    res.log = [len(seen)] + rows[1:]
    return res
