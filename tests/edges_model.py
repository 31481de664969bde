"""phaselib.get_edges (phaselib.py:16-67) in plain Python: dictionaries and lists, nothing of k_edges or orc_edges.

Per read a dictionary position (1-based) -> (base, quality) as cslib.cs2tpos2qbase (cslib.py:153-170) builds it from
the cs operations (oracle.cs_ops, the tokenizer the other models use), then the reference's double loop over the
hetSNPs with tstart < pos <= tend.  ``rules`` switches single rules to a deliberately wrong variant: the CPU tests
use them to show that the hand-built inputs of tests/edges_cases.py tell the right rule from the wrong one."""
import bisect

from oracle import oracle as O

ERR_ARG, ERR_COVER = 1, 7                                                      # HIMUT_ERR_*

# one switch per rule under test; every one of them makes the model wrong
RULES = ("bq_gt",          # bq > min_bq in place of bq >= min_bq
         "left_start",     # bisect_left at tstart: a hetSNP on tstart (1-based: the base in front of the read) is in
         "left_end",       # bisect_left at tend: a hetSNP on the read's last base is out
         "del_ref",        # a deleted position counts with state 0
         "trans_swap",     # trans1 and trans2 exchanged
         "no_clip",        # the query offset starts at 0, not behind the leading soft clip
         "drop_supp",      # supplementary reads (0x800) skipped
         "next_lane")      # the state of the second hetSNP of a pair read from its neighbour within its block of 64


class ModelError(Exception):
    def __init__(self, code):
        super().__init__("edges model error {}".format(code))
        self.code = code


def tpos2qbase(batch, i, no_clip=False):
    """cslib.cs2tpos2qbase of read i: a match or substituted base maps to (base from SEQ, quality), a deleted position
    to ('-', 0), an insertion adds nothing."""
    seq, q = batch.query_sequence(i), batch.query_qualities(i)
    tpos, qpos = int(batch.tstart[i]), 0 if no_clip else int(batch.qstart[i])
    out = {}
    for state, ref_len, alt_len, _ref, _alt in O.cs_ops(batch, i):
        if state == 1:
            for k in range(ref_len):
                out[tpos + k + 1] = (seq[qpos + k], int(q[qpos + k]))
        elif state == 2:
            out[tpos + 1] = (seq[qpos], int(q[qpos]))
        elif state == 4:
            for k in range(ref_len):
                out[tpos + k + 1] = ("-", 0)
        tpos += ref_len
        qpos += alt_len
    return out


def edges(batch, hetsnp_lst, min_bq, min_mapq, rules=()):
    """(edge_lst, {(i, j): [cis1, cis2, trans1, trans2]}) over the keys that got a count, edge_lst in natural order.
    hetsnp_lst: [(pos1, ref, alt)] ascending.  Raises ModelError(ERR_COVER) where the reference raises KeyError."""
    rules = set(rules)
    assert rules <= set(RULES), rules - set(RULES)
    hpos_lst = [h[0] for h in hetsnp_lst]
    edge2counts = {}
    for r in range(batch.n):
        flag = int(batch.flag[r])
        if flag & 0x100 or ("drop_supp" in rules and flag & 0x800):
            continue
        if int(batch.mapq[r]) < min_mapq:
            continue
        lo = (bisect.bisect_left if "left_start" in rules else bisect.bisect_right)(hpos_lst, int(batch.tstart[r]))
        hi = (bisect.bisect_left if "left_end" in rules else bisect.bisect_right)(hpos_lst, int(batch.tend[r]))
        if hi - lo < 2:
            continue
        t2q = tpos2qbase(batch, r, "no_clip" in rules)
        sub = list(range(lo, hi))
        seen = []                                            # (state, usable) per spanned hetSNP
        for g in sub:
            if hpos_lst[g] not in t2q:
                raise ModelError(ERR_COVER)
            base, bq = t2q[hpos_lst[g]]
            usable = bq > min_bq if "bq_gt" in rules else bq >= min_bq
            state = 0 if base == hetsnp_lst[g][1] or ("del_ref" in rules and base == "-") else 1
            seen.append((state, usable))
        for a, i in enumerate(sub):
            i_state, i_ok = seen[a]
            if not i_ok:
                continue
            for b in range(a + 1, len(sub)):
                j = sub[b]
                j_state, j_ok = seen[b]
                if not j_ok:
                    continue
                if "next_lane" in rules:
                    n = (b & ~63) + ((b + 1) & 63)
                    j_state = seen[n][0] if n < len(sub) else 0
                if not i_state and not j_state:
                    k = 0
                elif i_state and j_state:
                    k = 1
                elif not i_state and j_state:
                    k = 3 if "trans_swap" in rules else 2
                else:
                    k = 2 if "trans_swap" in rules else 3
                edge2counts.setdefault((i, j), [0, 0, 0, 0])[k] += 1
    return sorted(edge2counts), edge2counts


def band_table(edge2counts, n_het, band):
    """The counts as himut_run_edges lays them out: [(i * band + (j - i - 1)) * 4 + k], n_het * band * 4 entries (one
    row of band edges for n_het = 0)."""
    import numpy as np
    t = np.zeros(max(1, n_het) * band * 4, np.uint32)
    for (i, j), c in edge2counts.items():
        assert 0 <= i < j < n_het and j - i - 1 < band, (i, j, band)
        t[(i * band + (j - i - 1)) * 4:(i * band + (j - i - 1)) * 4 + 4] = c
    return t


def flat(edge_lst, edge2counts):
    """[i, j, c0, c1, c2, c3, ...] in edge order: how the fixtures store a result."""
    out = []
    for e in edge_lst:
        out.extend([int(e[0]), int(e[1])] + [int(x) for x in edge2counts[tuple(e)]])
    return out
