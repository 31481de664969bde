"""Hand-built alignments for the haplotag run: one case per place where the kernels can go wrong -- the lane and turn
edges, the segment and quality rules, the choice among sets, the verdict's boundaries, the pile rule, the empty inputs --
each with the rows that can be written down by hand.  A case is (name, batch, hetSNPs [(pos1, ref, alt, bit, set)],
parameters, rows {read: (set, n0, n1, n_other, n_del, n_lowbq, n_sets, hap, status)}, hetSNP rows {index: (n_ref, n_alt,
n_other, n_del, n_lowbq, agree, disagree)}).  The CPU test holds the model to the expectations, the GPU test the device
to the model."""
from collections import namedtuple

import numpy as np

from himut_amd.readbatch import batch_from_records
from tests.germline_model import make_read

N = 6000
CONTIG = "chrH"
ALT = {"A": "C", "C": "G", "G": "T", "T": "A"}
THIRD = {"A": "G", "C": "T", "G": "A", "T": "C"}
A_, NIP, NOSNP, NOVOTE, LOW, CONF = range(6)          # the statuses

Case = namedtuple("Case", "name batch snps kw rows snp_rows")


def contig(seed=5, n=N):
    rs = np.random.RandomState(seed)
    return "".join("ACGT"[k] for k in rs.randint(0, 4, n))


REF = contig()


def snp(p0, bit=0, st=0, ref=REF):
    """The hetSNP at the 0-based position."""
    return (p0 + 1, ref[p0], ALT[ref[p0]], bit, st)


def shows(snps, start, length, hap, flip=(), third=(), ref=REF):
    """The substitutions of a read of haplotype ``hap`` over [start, start + length): at each spanned hetSNP the allele
    hap XOR bit; at the 0-based positions of ``flip`` the other one, at those of ``third`` a third base."""
    subs = {}
    for pos1, r, a, bit, _st in snps:
        p = pos1 - 1
        if start <= p < start + length:
            allele = hap ^ bit ^ (1 if p in flip else 0)
            if p in third:
                subs[p] = THIRD[ref[p]]
            elif allele:
                subs[p] = a
    return subs


def read(snps, start, length, hap, flip=(), third=(), subs=None, ref=REF, **kw):
    s = shows(snps, start, length, hap, flip, third, ref)
    s.update(subs or {})
    return make_read(ref, start, length, s, **kw)


def with_n(rec, q):
    """The record with an N at query offset q of SEQ, under a match run of its cs text: the short form names no bases, and
    the decode leaves such a base alone (a substitution to n it refuses, HIMUT_ERR_BASE, in every run)."""
    assert ":" in rec["cs"] and "=" not in rec["cs"]
    return dict(rec, seq=rec["seq"][:q] + "N" + rec["seq"][q + 1:])


def batch(records, ref=REF):
    assert [r["tstart"] for r in records] == sorted(r["tstart"] for r in records), "the cases number their reads by hand"
    return batch_from_records(CONTIG, len(ref), records)


def _cases():
    out = []

    def case(name, records, snps, rows, snp_rows=None, **kw):
        out.append(Case(name, batch(records), list(snps), kw, rows, snp_rows or {}))

    # ---- lanes and turns: reads over 0, 1, 2, 15, 16, 17 and 33 hetSNPs of one set, both bit values; the reads over 17
    # and 33 carry the other allele at their last hetSNP (the second and the third turn's only lane)
    rs = np.random.RandomState(3)
    grid = [snp(1000 + 40 * k, int(rs.randint(0, 2))) for k in range(40)]
    recs, rows = [], {}
    for i, k in enumerate((0, 1, 2, 15, 16, 17, 33)):
        start = 990 - 7 + i                                  # ascending starts; every read begins in front of the first hetSNP
        length = (1000 + 40 * (k - 1) + 1 - start) if k else 5
        last = 1000 + 40 * (k - 1)
        off = k in (17, 33)
        recs.append(read(grid, start, length, i & 1, flip={last} if off else ()))
        h = i & 1
        n_h, n_o = (k - 1, 1) if off else (k, 0)
        rows[i] = (0, n_h if h == 0 else n_o, n_o if h == 0 else n_h, 0, 0, 0, 1, h, A_) if k else (-1, 0, 0, 0, 0, 0, 0, 2, NOSNP)
    case("lanes", recs, grid, rows)

    # ---- the segment and quality rules, a read per rule; one set, bit 0, so allele = haplotype
    S = [snp(p) for p in (200, 260, 300, 301, 400, 402, 403, 500, 600, 700, 800, 820, 900, 905, 1000, 1010, 1020)]
    recs = [
        read(S, 200, 60, 1),                                     # 0: a hetSNP at tstart; the one at tend (260) is not spanned
        read(S, 250, 51, 1),                                     # 1: hetSNPs at tstart + 10 and at tend - 1 (300); 301 is tend
        read(S, 390, 30, 1, dels={400: 3}),                      # 2: the deletion's first (400) and last (402) base; 403 behind it votes
        read(S, 480, 40, 1, ins={500: "GAT"}),                   # 3: the base right behind an insertion
        read(S, 580, 40, 1, softclip=("ACGTACG", "TT")),         # 4: soft clips: query offsets include the leading one
        read(S, 680, 40, 1, long_cs=True),                       # 5: a long-form cs text
        read(S, 790, 40, 0, bq_at={800: 19, 820: 20}),           # 6: bq == min_bq - 1 and == min_bq
        with_n(read(S, 890, 30, 0, third={900}), 905 - 890),     # 7: a third base, and an N in SEQ
        read(S, 990, 40, 1, dels={1000: 1}, bq_at={1010: 3}, third={1020}),   # 8: nothing but del / lowbq / other
    ]
    rows = {0: (0, 0, 1, 0, 0, 0, 1, 1, A_), 1: (0, 0, 2, 0, 0, 0, 1, 1, A_), 2: (0, 0, 1, 0, 2, 0, 1, 1, A_),
            3: (0, 0, 1, 0, 0, 0, 1, 1, A_), 4: (0, 0, 1, 0, 0, 0, 1, 1, A_), 5: (0, 0, 1, 0, 0, 0, 1, 1, A_),
            6: (0, 1, 0, 0, 0, 1, 1, 0, A_), 7: (-1, 0, 0, 2, 0, 0, 0, 2, NOVOTE), 8: (-1, 0, 0, 1, 1, 1, 0, 2, NOVOTE)}
    srows = {0: (0, 1, 0, 0, 0, 1, 0), 1: (0, 1, 0, 0, 0, 1, 0), 2: (0, 1, 0, 0, 0, 1, 0), 3: (0, 0, 0, 0, 0, 0, 0),
             4: (0, 0, 0, 1, 0, 0, 0), 5: (0, 0, 0, 1, 0, 0, 0), 6: (0, 1, 0, 0, 0, 1, 0), 10: (0, 0, 0, 0, 1, 0, 0),
             11: (1, 0, 0, 0, 0, 1, 0), 12: (0, 0, 1, 0, 0, 0, 0), 13: (0, 0, 1, 0, 0, 0, 0), 14: (0, 0, 0, 1, 0, 0, 0),
             15: (0, 0, 0, 0, 1, 0, 0), 16: (0, 0, 1, 0, 0, 0, 0)}
    case("segments", recs, S, rows, srows)

    # ---- sets.  A (0) and B (1) interleave hetSNP by hetSNP; C (2) and D (3) follow; E (4) lies under a secondary read only
    T = [snp(2000 + 20 * k, k & 1, k & 1) for k in range(6)] + [snp(2200, 1, 2), snp(2220, 0, 2), snp(2300, 0, 3)] + \
        [snp(2500, 0, 4), snp(2520, 1, 4)]
    recs = [
        read(T[:6], 1990, 120, 0),                               # 0: three votes each in A and B: the tie goes to A
        read([s if s[4] == 0 else s[:3] + (1 - s[3], s[4]) for s in T[:6]], 1995, 120, 0),   # 1: haplotype 0 in A, 1 in B; tie
        read(T, 2015, 320, 1),                                   # 2: B 3, A 2, C 2, D 1 votes: B, four sets
        read(T, 2075, 200, 0),                                   # 3: A 1, B 1, C 2: C, three sets
        read(T, 2095, 200, 0, flip={2220}),                      # 4: B 1 vote, C 1:1, no A: C by its two votes, a Conflict
        read(T, 2150, 160, 1),                                   # 5: C 2, D 1: C, two sets
        read(T, 2490, 60, 0, flag=0x100),                        # 6: secondary, over E alone
    ]
    rows = {0: (0, 3, 0, 0, 0, 0, 2, 0, A_), 1: (0, 3, 0, 0, 0, 0, 2, 0, A_), 2: (1, 0, 3, 0, 0, 0, 4, 1, A_),
            3: (2, 2, 0, 0, 0, 0, 3, 0, A_), 4: (2, 1, 1, 0, 0, 0, 2, 2, CONF), 5: (2, 0, 2, 0, 0, 0, 2, 1, A_),
            6: (-1, 0, 0, 0, 0, 0, 0, 2, NIP)}
    srows = {9: (0, 0, 0, 0, 0, 0, 0), 10: (0, 0, 0, 0, 0, 0, 0),
             # D's hetSNP (index 8): reads 2 and 5 voted there, both assigned to another set: neither agrees nor disagrees
             8: (0, 2, 0, 0, 0, 0, 0)}
    case("sets", recs, T, rows, srows)

    # ---- the verdict.  Twelve hetSNPs of one set, both bit values; votes h0:h1 by flipping
    V = [snp(3000 + 30 * k, (k * 7 // 3) & 1) for k in range(12)]

    def votes(start, a, b, hap=0):
        """A read of haplotype ``hap`` over the first a + b hetSNPs from ``start`` on, b of them flipped."""
        first = next(i for i, s in enumerate(V) if s[0] - 1 >= start)
        ps = [V[first + j][0] - 1 for j in range(a + b)]
        return read(V, start, ps[-1] + 1 - start, hap, flip=set(ps[:b]))
    recs = [votes(2990, 4, 1), votes(2991, 3, 1), votes(2992, 1, 1), votes(2993, 5, 0), votes(2994, 1, 0, hap=1),
            votes(2995, 9, 1, hap=1), votes(2996, 4, 1, hap=1)]
    at800 = {0: (0, 4, 1, 0, 0, 0, 1, 0, A_), 1: (0, 3, 1, 0, 0, 0, 1, 2, CONF), 2: (0, 1, 1, 0, 0, 0, 1, 2, CONF),
             3: (0, 5, 0, 0, 0, 0, 1, 0, A_), 4: (0, 0, 1, 0, 0, 0, 1, 1, A_), 5: (0, 1, 9, 0, 0, 0, 1, 1, A_),
             6: (0, 1, 4, 0, 0, 0, 1, 1, A_)}
    case("verdict_800", recs, V, at800, min_agree_permille=800)
    case("verdict_min_snps_2", recs, V, {**at800, 4: (0, 0, 1, 0, 0, 0, 1, 2, LOW)}, min_snps=2)
    case("verdict_1000", recs, V, {**at800, 0: (0, 4, 1, 0, 0, 0, 1, 2, CONF), 5: (0, 1, 9, 0, 0, 0, 1, 2, CONF),
                                   6: (0, 1, 4, 0, 0, 0, 1, 2, CONF)}, min_agree_permille=1000)
    case("verdict_750", recs, V, {**at800, 1: (0, 3, 1, 0, 0, 0, 1, 0, A_)}, min_agree_permille=750)

    # ---- the pile: a secondary read and one a mapping quality short of min_mapq over voted hetSNPs
    P = [snp(4000 + 50 * k, k & 1) for k in range(4)]
    recs = [read(P, 3990, 200, 0, mapq=20), read(P, 3991, 200, 1, flag=0x100), read(P, 3992, 200, 1, mapq=19),
            read(P, 3993, 200, 0, flag=0x800, mapq=60), read(P, 3994, 200, 0, flag=0x10, mapq=20, flip={4050})]
    rows = {0: (0, 4, 0, 0, 0, 0, 1, 0, A_), 1: (-1, 0, 0, 0, 0, 0, 0, 2, NIP), 2: (-1, 0, 0, 0, 0, 0, 0, 2, NIP),
            3: (0, 4, 0, 0, 0, 0, 1, 0, A_), 4: (0, 3, 1, 0, 0, 0, 1, 2, CONF)}
    # hetSNP 1 (bit 1): haplotype 0 shows alt; read 4 shows ref there and is no Assigned read
    case("pile", recs, P, rows, {0: (3, 0, 0, 0, 0, 2, 0), 1: (1, 2, 0, 0, 0, 2, 0)}, min_mapq=20)
    case("pile_mapq_0", recs, P, {**rows, 2: (0, 0, 4, 0, 0, 0, 1, 1, A_)}, {0: (3, 1, 0, 0, 0, 3, 0)})

    # ---- agree and disagree: a read assigned to A that votes at B's hetSNP; an assigned read with one vote against its haplotype
    G = [snp(4500, 0, 0), snp(4520, 1, 0), snp(4540, 0, 0), snp(4560, 0, 1), snp(4580, 1, 0), snp(4600, 0, 0), snp(4620, 1, 0)]
    recs = [read(G, 4490, 80, 0),                                # 0: A 3 votes, B 1 vote (for haplotype 0)
            read(G, 4495, 130, 1, flip={4500}),                  # 1: A 1:5, B 1: assigned to A, haplotype 1; disagrees at 4500
            read(G, 4550, 20, 1)]                                # 2: B alone: assigned to B
    rows = {0: (0, 3, 0, 0, 0, 0, 2, 0, A_), 1: (0, 1, 5, 0, 0, 0, 2, 1, A_), 2: (1, 0, 1, 0, 0, 0, 1, 1, A_)}
    # hetSNP 3 is B's: reads 0 and 1 vote there and are assigned to A, so only read 2 moves its agree
    case("agree", recs, G, rows, {0: (2, 0, 0, 0, 0, 1, 1), 1: (1, 1, 0, 0, 0, 2, 0), 3: (1, 2, 0, 0, 0, 1, 0), 4: (1, 0, 0, 0, 0, 1, 0)})

    # ---- empty and degenerate inputs
    case("no_snps", [read(P, 3990, 200, 0)], [], {0: (-1, 0, 0, 0, 0, 0, 0, 2, NOSNP)})
    case("no_reads", [], P, {}, {k: (0,) * 7 for k in range(4)})
    case("snps_outside_the_reads", [read([], 1000, 100, 0), read([], 1200, 100, 0)], [snp(10), snp(999), snp(1100), snp(1300), snp(5000)],
         {0: (-1, 0, 0, 0, 0, 0, 0, 2, NOSNP), 1: (-1, 0, 0, 0, 0, 0, 0, 2, NOSNP)}, {k: (0,) * 7 for k in range(5)})
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
ROW_FIELDS = ("set", "n0", "n1", "n_other", "n_del", "n_lowbq", "n_sets", "hap", "status")
SNP_FIELDS = ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq", "agree", "disagree")


def check_expectations(case, rows, snp_rows):
    """The hand-computed rows of a case against a result's."""
    for i, want in case.rows.items():
        got = tuple(int(rows[i][f]) for f in ROW_FIELDS)
        assert got == want, (case.name, "read", i, got, want)
    for k, want in case.snp_rows.items():
        got = tuple(int(snp_rows[k][f]) for f in SNP_FIELDS)
        assert got == want, (case.name, "hetSNP", k, got, want)
