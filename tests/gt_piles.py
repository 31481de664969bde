"""Genotype vectors as read piles, and a plain restatement of the genotyper's fp64 arithmetic.

A vector is one pileup column: the reference base, the alleles and base qualities of its reads in fetch order, and the
germline prior it is evaluated at (tests/golden/gt_edges.json, tests/golden/leaf_gtlib.json).  build() lays vectors out
on one synthetic contig, one column per vector, under read filters that every read passes, so that the call run and
normcounts genotype exactly the column the vector holds.  genotype() restates gtlib's sums (gtlib.py:72-174) in the
reference's order or in a perturbed one; tests/golden/make_golden.py keeps a boundary vector only if a perturbation
changes its outcome, and the CPU tests check that this still holds.

build_dbs() lays vectors out as halves of doublet candidates, so that the dbs run genotypes the same columns.

Used by the fixture generator and by the tests; nothing here reads the reference."""
import math
import random

from himut_amd.gtlib import GT_LST, GT_STATES, build_tables
from himut_amd.readbatch import batch_from_records

BASES = "ATGC"                                           # util.py:14, the order the sums run in
ORDERS = ("rise", "same", "pairs")                       # how a vector's reads start: see _starts
PERTURBATIONS = ("reverse", "fsum", "prior_first", "base_order")


def state_of(b1, b2, ref):
    """gtlib.get_germ_gt_state (gtlib.py:23-38)."""
    if b1 == b2 == ref:
        return "homref"
    if (b1 == ref) != (b2 == ref):
        return "het"
    return "hetalt" if b1 != b2 else "homalt"


def _tables(prior):
    hom, het, err, logp = build_tables(prior)
    return hom, het, err, dict(zip(GT_STATES, (float(x) for x in logp)))


def pls(ref, alleles, bqs, prior, how="ref", skip=None, tables=None):
    """The ten PLs.  how="ref" sums as gtlib does: per genotype, for base in ATGC the reads of that base in fetch order
    from 0, the four sums from 0 in that order, then the log prior, times -10.  The perturbations: "reverse" sums each
    base's reads last to first, "fsum" sums them with math.fsum, "prior_first" starts from the prior, "base_order" adds
    the bases as CGTA.  skip: a base left out (get_germ_gq, gtlib.py:151-152)."""
    hom, het, err, logp = tables or _tables(prior)
    per = {b: [q for a, q in zip(alleles, bqs) if a == b] for b in BASES}
    if how == "reverse":
        per = {b: v[::-1] for b, v in per.items()}
    out = []
    for gt in GT_LST:
        b1, b2 = gt
        lp = logp[state_of(b1, b2, ref)]
        acc = lp if how == "prior_first" else 0.0
        for base in ("CGTA" if how == "base_order" else BASES):
            if base == skip:
                continue
            if b1 == b2 and base == b1:
                lut = hom
            elif b1 != b2 and base in gt:
                lut = het
            else:
                lut = err
            terms = [float(lut[q]) for q in per[base]]
            s = math.fsum(terms) if how == "fsum" else 0.0
            if how != "fsum":
                for t in terms:
                    s = s + t
            acc = acc + s
        if how != "prior_first":
            acc = acc + lp
        out.append(-10 * acc)
    return out


def decide(pl):
    """np.argsort of the numpy the reference pins (ties -> lower index), then gtlib.py:113-135: (gt index, gqf)."""
    order = sorted(range(10), key=lambda i: (pl[i], i))
    return order[0], pl[order[1]] - pl[order[0]]


def gq_of(gqf):
    return int(gqf) if gqf < 99 else 99


def genotype(ref, alleles, bqs, prior, how="ref", tables=None):
    """get_germ_gt plus get_germ_gq for each single-base alt: dict of gt, gq, gqf, state, pls, germ_gq, germ_gqf."""
    tables = tables or _tables(prior)
    pl = pls(ref, alleles, bqs, prior, how, tables=tables)
    i, gqf = decide(pl)
    gt = GT_LST[i]
    state = state_of(gt[0], gt[1], ref)
    if gt[0] != ref and gt.count(ref) == 1:
        gt = gt[::-1]
    germ_gq, germ_gqf = {}, {}
    for alt in BASES:
        if alt != ref:
            germ_gqf[alt] = decide(pls(ref, alleles, bqs, prior, how, skip=alt, tables=tables))[1]
            germ_gq[alt] = gq_of(germ_gqf[alt])
    return dict(gt=gt, gq=gq_of(gqf), gqf=gqf, state=state, pls=pl, germ_gq=germ_gq, germ_gqf=germ_gqf)


def outcome(g, k):
    """What a kernel decides from a genotype: gt, state, gq, gq >= k, and the alt-omitted qualities against k."""
    return (g["gt"], g["state"], g["gq"], g["gq"] >= k, tuple(sorted(g["germ_gq"].items())),
            tuple(sorted((a, q >= k) for a, q in g["germ_gq"].items())))


def flips(v):
    """The perturbations that change the vector's outcome (an empty list: the vector tests nothing)."""
    tables = _tables(v["prior"])
    base = outcome(genotype(v["ref"], v["alleles"], v["bqs"], v["prior"], tables=tables), v["k"])
    return [how for how in PERTURBATIONS
            if outcome(genotype(v["ref"], v["alleles"], v["bqs"], v["prior"], how, tables=tables), v["k"]) != base]


def leaf_vectors(vectors, prior=1 / (10 ** 3), k=20):
    """leaf_gtlib's vectors carry the caller's germ_gq only (the plain gq): the same vectors with the alt-omitted
    qualities restated here (the CPU tests check them against the oracle), the prior and a k."""
    out = []
    for v in vectors:
        g = genotype(v["ref"], v["alleles"], v["bqs"], prior)
        out.append(dict(v, germ_gq=g["germ_gq"], prior=prior, k=k))
    return out


# ---- what the call run and normcounts make of one column ----

def counts(v):
    return {b: v["alleles"].count(b) for b in BASES}


def candidates(v):
    """{alt: True if the call run writes a record for (ref, alt), False if the germline rule drops it}
    (caller.py:111-147, 336-345): every alt allele in the column is a candidate."""
    ref, gt, st, c = v["ref"], v["gt"], v["state"], counts(v)
    out = {}
    for alt in BASES:
        if alt == ref or c[alt] == 0:
            continue
        if st == "het":
            germ = ref + alt == gt
        elif st == "hetalt":
            germ = sum(c.values()) == c[gt[0]] + c[gt[1]] and alt in gt
        elif st == "homalt":
            germ = c[ref] == 0 and gt.count(alt) == 2
        else:
            germ = False
        out[alt] = not germ
    return out


def norm_row(v, min_gq, alt_order, min_ref_count, min_alt_count):
    """The norm.log row the column's tri_sum (its depth) lands in (normcounts.py:334-402), with no indels, no depth
    filter and no site sets.  alt_order: {ref: [three alts]}, list(set("ATGC").difference(ref))."""
    st = v["state"]
    if st != "homref":
        return {"het": 3, "hetalt": 4, "homalt": 5}[st]
    c = counts(v)
    if c[v["ref"]] == len(v["alleles"]):
        gq, alt_count = v["gq"], None
    else:
        alts = alt_order[v["ref"]]
        ac = [c[a] for a in alts]
        alt = alts[ac.index(max(ac))]
        gq, alt_count = v["germ_gq"][alt], c[alt]
    if gq < min_gq:
        return 10
    if c[v["ref"]] < min_ref_count or (alt_count is not None and alt_count < min_alt_count):
        return 9
    return 13


def norm_log(vectors, min_gq, alt_order, min_ref_count, min_alt_count, copies=1):
    """The 14 counters of normcounts over chunks that hold the vectors' columns (each `copies` times) and no other
    covered position."""
    log = [0] * 14
    for v in vectors:
        d = len(v["alleles"]) * copies
        log[0] += d                     # every read is its own molecule and passes the filters
        log[1] += d
        row = norm_row(v, min_gq, alt_order, min_ref_count, min_alt_count)
        if row >= 6:
            log[6] += d
        log[row] += d
    return log


# ---- the pile ----

def params(min_gq, prior, depth):
    """Filters every read passes, every column base callable: only the genotype decides."""
    return dict(min_qv=0, min_mapq=0, qlen_lower_limit=0, qlen_upper_limit=1 << 20, min_sequence_identity=0.0,
                min_gq=int(min_gq), min_bq=1, min_trim=0.0, max_mismatch_count=1 << 20, mismatch_window_size=0,
                md_threshold=int(depth) + 1, min_ref_count=3, min_alt_count=1, min_hap_count=3,
                germline_snv_prior=prior)


def _starts(n, order, pos):
    """Read starts of a column of n reads at pos, in fetch (file) order: "rise" -- each read starts after the one
    before; "same" -- all at one position (file order decides); "pairs" -- two reads per start."""
    if order == "rise":
        return [pos - (n - k) for k in range(n)]
    if order == "same":
        return [pos - 3] * n
    return [pos - 1 - (n - 1 - k) // 2 for k in range(n)]


class Piles:
    pass


TWIN_GAP = 8


def _read(seq, s, e, c, allele, ref, q, qname):
    """A read over [s, e) holding `allele` at column c (quality q) and the contig's bases elsewhere (quality 93)."""
    left, right = c - s, e - c - 1
    rseq = "".join(seq[s:c]) + allele + "".join(seq[c + 1:e])
    if allele == ref:
        cs = ":{}".format(e - s)
    else:
        cs = (":{}".format(left) if left else "") + "*" + ref.lower() + allele.lower()
        cs += ":{}".format(right) if right else ""
    bq = [93] * len(rseq)
    bq[left] = int(q)
    return dict(tstart=s, tend=e, qstart=0, seq=rseq, bq=bq, cs=cs, qname=qname)


def build(vectors, spacing=None, seed=11, name="chrG", orders=ORDERS, twin=False):
    """One contig with vector i's column at position P_i = spacing * (i + 1) (0-based); its reads lie within
    (P_i - spacing / 2, P_i + spacing / 2) and start by the rule orders[i % len(orders)].  Returns a Piles with batch,
    refseq (str), cols (the column positions of each vector), call_chunks (one per vector, [P_i - spacing / 2,
    P_i + spacing / 2)), norm_chunks ((P_i, P_i + 1)) and orders.

    twin: the column twice, at P_i with reads that end there and at P_i + TWIN_GAP with reads that start there (all at
    one position, so file order is fetch order); the normcounts chunk (P_i, P_i + TWIN_GAP + 1) holds both and no other
    covered position.  Two columns that need the sweep's pool and its left-over list in one wave and one workgroup."""
    deep = max(len(v["alleles"]) for v in vectors)
    if spacing is None:
        spacing = 64
        while spacing // 2 < deep + 16:
            spacing *= 2
    assert spacing // 2 >= deep + 16, "spacing too small for the deepest column"
    rs = random.Random(seed)
    length = spacing * (len(vectors) + 1)
    seq = [rs.choice(BASES) for _ in range(length)]
    # a read at the contig's start that no chunk fetches holds the first bytes of the read arrays (a tile whose piece
    # starts there goes to k_norm_tile, which would hide the path the column takes)
    recs, cols, ords = [_read(seq, 1, 17, 1, seq[1], seq[1], 93, "pad")], [], []
    for i, v in enumerate(vectors):
        p = spacing * (i + 1)
        q = p + TWIN_GAP
        order = orders[i % len(orders)]
        ords.append(order)
        seq[p] = v["ref"]
        cols.append([p, q] if twin else [p])
        if twin:
            seq[q] = v["ref"]
        for k, (a, bq, s) in enumerate(zip(v["alleles"], v["bqs"], _starts(len(v["alleles"]), order, p))):
            e = p + 1 if twin else p + 3 + (k % 3)
            recs.append(_read(seq, s, e, p, a, v["ref"], bq, "v{}/r{}".format(i, k)))
            if twin:
                recs.append(_read(seq, q, q + 3 + (k % 3), q, a, v["ref"], bq, "v{}/t{}".format(i, k)))
    recs.sort(key=lambda r: r["tstart"])             # coordinate order; stable: equal starts keep the file order
    P = Piles()
    P.refseq = "".join(seq)
    P.batch = batch_from_records(name, length, recs)
    P.cols = cols
    P.orders = ords
    P.spacing = spacing
    P.call_chunks = [(c[0] - spacing // 2, c[0] + spacing // 2) for c in cols]
    P.norm_chunks = [(c[0], c[-1] + 1) for c in cols]
    return P


# ---- the pile of doublets ----

DBS_COMPANIONS = 14                                      # all-reference reads over the companion column alone
DBS_MARGIN = 24                                          # room beside a pair for the companions and the reads' tails


def dbs_params(min_gq, depth):
    """params() for the dbs run (the prior goes to the run on its own): every read passes, the mismatch window is shut
    and min_bq is 1, so only the genotype decides a half."""
    p = params(min_gq, None, depth + 20)
    del p["germline_snv_prior"]
    return p


def alts_of(v):
    """The distinct non-reference alleles of a column, in the order they come."""
    return [a for a in dict.fromkeys(v["alleles"]) if a != v["ref"]]


def build_dbs(vectors, alts, halves, spacing=None, seed=11, name="chrG", orders=ORDERS, straddle=None, extra=None):
    """One contig with vector i's column as half halves[i] (0: first, 1: second) of a doublet candidate whose allele
    at that column is alts[i].  The column is at p = spacing * (i + 1) (0-based), its companion at c = p + 1 (first
    half) or p - 1 (second half); straddle[i] moves the pair up so that min(p, c) % 256 == 255 and the two columns lie
    in two 256-position blocks.

    The vector's reads lie in fetch order by _starts(n, order, min(p, c)), end at max(p, c) + 3 + k % 3 and hold the
    vector's allele and quality at p and the contig's bases at quality 93 elsewhere.  The first of them that holds
    alts[i] also carries the next base in ATGC rotation of the contig's base at c (quality 93): the one proposer.
    DBS_COMPANIONS all-reference reads of quality 93 cover c and not p, so the companion half is a confident homref
    column whatever the vector's depth.  extra[i]: further all-reference reads of quality 93 over both columns, one per
    entry, "ins" with an inserted base in front of p, "del" with p deleted.

    Returns a Piles with batch, refseq, regions (the whole contig), cols ([p] per vector), doublets ((tpos, half) per
    vector: the record's 1-based position and the half that is the vector's) and spacing."""
    from tests.germline_model import make_read
    deep = max(len(v["alleles"]) for v in vectors)
    if spacing is None:
        spacing = 64
        while spacing // 2 < deep + DBS_MARGIN:
            spacing *= 2
    assert spacing // 2 >= deep + DBS_MARGIN, "spacing too small for the deepest column"
    straddle = straddle or [False] * len(vectors)
    ps, shift = [], 0
    for i, half in enumerate(halves):
        p = spacing * (i + 1) + shift
        if straddle[i]:
            lo = min(p, p + 1 - 2 * half)
            shift += (255 - lo) % 256
            p += (255 - lo) % 256
        ps.append(p)
    length = ps[-1] + spacing
    rs = random.Random(seed)
    seq = [rs.choice(BASES) for _ in range(length)]
    for v, p in zip(vectors, ps):
        seq[p] = v["ref"]
    seq = "".join(seq)
    recs = [make_read(seq, 1, 16, bq=93, qname="pad")]
    P = Piles()
    P.cols, P.doublets, P.orders = [], [], []
    for i, (v, alt, half, p) in enumerate(zip(vectors, alts, halves, ps)):
        assert alt != v["ref"] and alt in v["alleles"], (v, alt)
        c = p + 1 - 2 * half
        lo, hi = min(p, c), max(p, c)
        order = orders[i % len(orders)]
        carrier = v["alleles"].index(alt)
        for k, (a, bq, s) in enumerate(zip(v["alleles"], v["bqs"], _starts(len(v["alleles"]), order, lo))):
            subs = {p: a} if a != v["ref"] else {}
            if k == carrier:
                subs[c] = BASES[(BASES.index(seq[c]) + 1) % 4]
            recs.append(make_read(seq, s, hi + 3 + k % 3 - s, subs, bq=93, bq_at={p: int(bq)}, qname="v{}/r{}".format(i, k)))
        for k, kind in enumerate((extra or {}).get(i, ())):
            recs.append(make_read(seq, lo - 2 - k, hi + 5 + k - lo, ins={p: "G"} if kind == "ins" else None,
                                  dels={p: 1} if kind == "del" else None, bq=93, qname="v{}/x{}".format(i, k)))
        for k in range(DBS_COMPANIONS):
            s = c if c > p else c - 2 - k % 3
            e = c + 3 + k % 3 if c > p else c + 1
            recs.append(make_read(seq, s, e - s, bq=93, qname="v{}/c{}".format(i, k)))
        P.cols.append([p])
        P.doublets.append((lo + 1, half))
        P.orders.append(order)
    recs.sort(key=lambda r: r["tstart"])             # coordinate order; stable: equal starts keep the file order
    P.refseq = seq
    P.batch = batch_from_records(name, length, recs)
    P.regions = [(1, length)]
    P.spacing = spacing
    return P
