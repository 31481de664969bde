"""The call, dbs, sites and germline runs genotype a column through one walk and one verdict cascade
(himut_amd/csrc/himut_column.h): the same substitutions through all four runs on one context say the same.

One small contig (tests/gt_piles.build_dbs): every vector's column is one half of a doublet candidate, so the call run
proposes both halves as single-base candidates, the dbs run genotypes them as halves, the sites run is asked for them,
and the germline run reports both positions.  The columns hold 1, 7, 8, 9, 16 and 17 reads (the edges of the walk's
batch of eight slots), second halves whose companion reads lie between the column's own in fetch order (empty slots
between filled ones), a read with an insertion in front of the column, a read with the column deleted, and -- for the
sites run, which alone can be asked about it -- a position inside the reads' span that no read covers."""
import functools

import numpy as np
import pytest

from tests import dbs_model as D
from tests import germline_model as GM
from tests import gt_piles as G
from tests import sites_model as S

PARAM_NAMES = ("min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq", "min_bq", "max_mismatch_count",
               "mismatch_window_size", "md_threshold", "min_ref_count", "min_alt_count", "min_hap_count", "min_sequence_identity",
               "min_trim")
PRIOR = 1 / (10 ** 3)


def _vector(ref, n_ref, alt, alt_bqs, ref_bq=93):
    """A column of n_ref reference reads with the alt reads spread between them."""
    alleles, bqs = [ref] * n_ref, [ref_bq] * n_ref
    for k, q in enumerate(alt_bqs):
        at = (k + 1) * len(alleles) // (len(alt_bqs) + 1)
        alleles.insert(at, alt)
        bqs.insert(at, q)
    return dict(ref=ref, alleles=alleles, bqs=bqs)


# (vector, half, extra reads, site set): depths 1, 7, 8, 9, 16, 17
COLUMNS = [
    (_vector("A", 0, "T", [93]), 0, (), None),                     # 1: one alt read
    (_vector("C", 6, "G", [93]), 1, (), None),                     # 7, companions between its reads
    (_vector("G", 4, "A", [93] * 4), 0, (), None),                 # 8: a het column
    (_vector("T", 1, "C", [93] * 7, ref_bq=2), 1, (), None),       # 8: a homalt column with a reference read
    (_vector("A", 7, "C", [93]), 1, ("ins",), None),               # 8 + the insertion read = 9
    (_vector("T", 8, "G", [93]), 0, (), "com"),                    # 9
    (_vector("C", 14, "A", [93]), 0, ("del",), None),              # 15 + the deletion read = 16
    (_vector("G", 15, "T", [93]), 1, (), "pon"),                   # 16
    (_vector("A", 16, "G", [5]), 0, (), None),                     # 17: the alt read below min_bq
    (_vector("T", 15, "A", [93, 93]), 1, (), None),                # 17
    (_vector("C", 2, "T", [93] * 15), 0, (), None),                # 17: a het column
]


@functools.lru_cache(maxsize=None)
def case():
    """(pile, parameters, sites, the uncovered site): the sites are both halves of every doublet and one position between
    two piles that no read covers."""
    vs = [c[0] for c in COLUMNS]
    P = G.build_dbs(vs, [G.alts_of(v)[0] for v in vs], [c[1] for c in COLUMNS], orders=["rise"],
                    extra={i: c[2] for i, c in enumerate(COLUMNS)})
    kw = dict(G.dbs_params(20, 17), min_bq=20)
    sites, sets = [], {"pon": [], "com": []}
    for (tpos, half), col in zip(P.doublets, COLUMNS):
        reads = [D.ReadInfo(P.batch, i) for i in range(P.batch.n)]
        for j in (0, 1):
            subs = {(e[2], e[3]) for r in reads for e in r.mismatch if e[1] and e[0] == tpos + j}
            assert len(subs) == 1                                  # one alt allele per column: no HetAltSite pair
            (ref, alt), = subs
            sites.append((tpos + j, ref, alt))
            if j == half and col[3]:
                sets[col[3]].append((tpos + j) << 4 | D.BASES.index(ref) << 2 | D.BASES.index(alt))
    empty = (P.doublets[0][0] + P.spacing // 2, "A", "C")
    kw.update(pon_keys=sorted(sets["pon"]), com_keys=sorted(sets["com"]))
    return P, kw, sorted(sites + [empty]), empty


def _half(r, j):
    """What a dbs record says about half j, in the order of _single."""
    return (tuple(int(x) for x in r["counts"][j]), bytes(r["gt"][j]).decode(), int(r["gt_state"][j]), int(r["half_gq"][j]),
            int(r["alt_bqsum"][j]), int(r["half_status"][j]))


def _single(r, alt_bqsum):
    gt = bytes(r["gt"]).decode() if "gt" in r.dtype.names else chr(r["gt0"]) + chr(r["gt1"])
    return (tuple(int(x) for x in r["counts"]), gt, int(r["gt_state"]), int(r["gq"]), int(alt_bqsum), int(r["status"]))


def check(P, sites, empty, crecs, clog, drecs, dlog, srecs, grecs):
    """The four runs' records of one input against each other.  Returns the sites' status names in site order."""
    germline, nocov = S.ST["Germline"], S.ST["NoCoverage"]
    site = {s: _single(r, r["alt_bqsum"]) for s, r in zip(sites, srecs)}
    call = {(int(r["tpos"]), chr(r["ref"]), chr(r["alt"])): _single(r, r["bqsum"][D.BASES.index(chr(r["alt"]))]) for r in crecs}
    dbs = {}
    for r in drecs:
        for j in (0, 1):
            dbs[int(r["tpos"]) + j, chr(r["ref"][j]), chr(r["alt"][j])] = _half(r, j)
    assert len(call) == len(crecs) and len(dbs) == 2 * len(drecs)
    assert site[empty] == ((0,) * 6, "\0\0", 0, 0, 0, nocov)       # every slot of its column is empty
    n_germ = 0
    for k in range(0, len(P.doublets)):
        tpos = P.doublets[k][0]
        pair = [s for s in sites if s[0] in (tpos, tpos + 1) and s != empty]
        assert len(pair) == 2
        dropped = [s for s in pair if site[s][5] == germline]
        n_germ += bool(dropped)
        for s in pair:
            if s in dropped:                                      # dropped as germline: no call record, no doublet
                assert s not in call and s not in dbs, s
                continue
            assert site[s][5] not in (germline, nocov)
            assert call[s] == site[s], (s, call[s], site[s])
            if dropped:
                assert s not in dbs, s
            else:
                assert dbs[s] == site[s], (s, dbs[s], site[s])
    assert set(call) | set(dbs) <= set(site)
    assert dlog[D.LOG_ROWS.index("num_germ")] == n_germ and dlog[D.LOG_ROWS.index("num_dbs")] == len(P.doublets)
    assert len(drecs) == len(P.doublets) - n_germ
    assert clog[1] == len(sites) - 1                               # num_sbs: every half was a candidate of the call run
    # the germline run under thresholds every read passes: the same pile at every position, whatever the alt
    germ = {int(r["tpos"]): (tuple(int(x) for x in r["counts"]), chr(r["gt0"]) + chr(r["gt1"]), int(r["gt_state"]), int(r["gq"]))
            for r in grecs}
    assert len(germ) == len(grecs)
    for s in sites:
        if s != empty:
            assert germ[s[0]] == site[s][:4], (s, germ[s[0]], site[s])
    assert set(germ) == {s[0] for s in sites if s != empty}
    return [S.STATUS[site[s][5]] for s in sites]


def _germline_kw(kw):
    return dict(report_homref=True, min_mapq=0, min_gq=kw["min_gq"], min_bq=kw["min_bq"], min_ref_count=kw["min_ref_count"],
                min_alt_count=kw["min_alt_count"], md_threshold=kw["md_threshold"])


def test_models_put_every_column_in_every_run():
    """The plain models on the test's input: every column is in all four runs, and the statuses cover the cascade."""
    from oracle import oracle as O
    P, kw, sites, empty = case()
    assert sorted(len(v["alleles"]) + len(x) for v, _h, x, _s in COLUMNS) == [1, 7, 8, 8, 9, 9, 16, 16, 17, 17, 17]
    p = {k: v for k, v in kw.items() if k not in ("pon_keys", "com_keys")}
    crecs, clog = O.call(P.batch, [(0, P.batch.length)], p, PRIOR, pon_keys=kw["pon_keys"], com_keys=kw["com_keys"])
    drecs, dlog = D.run(P.batch, P.regions, prior=PRIOR, **kw)
    srecs, _slog = S.run(P.batch, sites, prior=PRIOR, **kw)
    grecs, _glog = GM.run(P.batch, P.regions, PRIOR, **_germline_kw(kw))
    crecs = crecs[(crecs["flags"] & 7) == 0] if "flags" in crecs.dtype.names else crecs
    seen = check(P, sites, empty, crecs, clog, drecs, dlog, srecs, grecs)
    assert set(seen) >= {"NoCoverage", "Germline", "HomAltSite", "IndelSite", "LowGQ", "LowBQ", "PanelOfNormal", "ComSnp", "PASS"}, seen
    assert seen.count("Germline") >= 2
    # empty slots between filled ones: a second half's companion reads start among the column's own
    i = next(k for k, c in enumerate(COLUMNS) if c[1] == 1 and len(c[0]["alleles"]) >= 7)
    col = P.cols[i][0]
    over = [col >= int(P.batch.tstart[r]) and col < int(P.batch.tend[r]) for r in range(P.batch.n)]
    inside = over[over.index(True):len(over) - over[::-1].index(True)]
    assert not all(inside)


@pytest.mark.gpu
def test_four_runs_say_the_same():
    from himut_amd import _ffi, gtlib
    P, kw, sites, empty = case()
    prm = dict(D.DEFAULTS, **kw)
    with _ffi.Context(0) as c:
        c.set_params(**{k: prm[k] for k in PARAM_NAMES})
        c.set_gt_lut(*gtlib.build_tables(PRIOR))
        c.set_site_set(0, np.array(kw["pon_keys"], np.uint64))
        c.set_site_set(1, np.array(kw["com_keys"], np.uint64))
        c.push_reads(P.batch)
        c.set_chunks([(0, P.batch.length)])
        c.run()
        crecs, clog = c.records(), c.log()
        c.set_chunks(P.regions)
        c.run_dbs()
        drecs, dlog = c.dbs()
        c.run_sites(np.array([s[0] for s in sites], np.int32), "".join(s[1] for s in sites).encode(), "".join(s[2] for s in sites).encode())
        srecs, slog = c.sites()
        c.run_germline(**_germline_kw(kw))
        grecs, _glog = c.germline()
    seen = check(P, sites, empty, crecs, clog, drecs, dlog, srecs, grecs)
    assert seen.count("Germline") >= 2 and "IndelSite" in seen and "NoCoverage" in seen
    S.assert_same(srecs, slog, *S.run(P.batch, sites, prior=PRIOR, **kw))
    D.assert_same(drecs, dlog, *D.run(P.batch, P.regions, prior=PRIOR, **kw))
