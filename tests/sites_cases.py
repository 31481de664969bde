"""Hand-built inputs for the sites contract (tests/sites_model.py), shared by the CPU tests (the model against what each
rule says) and the GPU tests (the run against the model).  A case is (name, batch, sites, keyword parameters of
sites_model.run, expect) where sites is [(pos1, ref, alt)] in non-decreasing position and expect(records, log) asserts
what the rule says (None: the shape alone matters, the model is the expectation)."""
import random

from tests import sites_model as M
from tests.dbs_cases import A1, A2, A3, N, OPEN, REF, batch

KW = dict(OPEN, min_mapq=20)


def stack(p, n, subs=None, length=200, bq=93, low_mapq=(), **kw):
    """n reads that all cover 0-based p; read k carries subs.get(k) ({pos: base}); the reads of low_mapq map at 10."""
    out = []
    for k in range(n):
        start = max(0, p - length // 2 + (k % 41) - 20)
        out.append(M.make_read(REF, start, length, dict((subs or {}).get(k, {})), bq=bq, mapq=10 if k in low_mapq else 60, **kw))
    return out


def site(p, alt=A1):
    """The site (pos1, ref, alt) at 0-based p."""
    return (p + 1, REF[p], alt[p])


def statuses(recs):
    return [M.STATUS[int(r["status"])] for r in recs]


def _case(name, reads, sites, expect=None, pon=(), com=(), **kw):
    sites = sorted(sites, key=lambda s: s[0]) if kw.pop("sort", True) else list(sites)
    return name, batch(reads), sites, dict(dict(KW, **kw), pon_keys=list(pon), com_keys=list(com)), expect


def _key(s):
    return (s[0] << 4) | ("ATGC".index(s[1]) << 2) | "ATGC".index(s[2])


def _want(*names):
    def expect(recs, log):
        assert statuses(recs) == list(names), (statuses(recs), names, log)
    return expect


def shape_cases():
    """The shapes at which the kernels can go wrong (the model does not care)."""
    out = []
    # pos1 = 1, the first bit of the bitmap
    r = [M.make_read(REF, 0, 150 + k, {0: A1[0]} if k == 0 else {}, bq=93) for k in range(9)]
    out.append(_case("pos1_is_1", r, [site(0), site(0, A2), site(1)]))
    # block positions 255 / 256 / 257 and bitmap-word positions 31 / 32 / 33: two blocks, two words
    r = [M.make_read(REF, 3 * k, 400, {31: A1[31], 256: A1[256]} if k == 2 else {}, bq=93) for k in range(10)]
    r += [M.make_read(REF, 100 + 5 * k, 156 - 5 * k, bq=93) for k in range(4)]          # end at 256: cover rpos 255, not 256
    r += [M.make_read(REF, 256, 120 + k, bq=93) for k in range(3)]                      # start at 256
    out.append(_case("block_and_word_edges", r, [site(p) for p in (31, 32, 33, 255, 256, 257)]))
    # a read's first base, its last base, its tend (not covered); a gap between reads; behind every read, inside the span
    # and far behind it
    r = [M.make_read(REF, 1000, 200, {1000: A1[1000], 1199: A1[1199]}, bq=93), M.make_read(REF, 1600, 100, bq=93)]

    def edges(recs, log, span=M.span_of(batch(r))):
        assert statuses(recs)[2:] == ["NoCoverage"] * 6 and [M.depth_of(x) for x in recs] == [1, 1, 0, 0, 0, 0, 0, 0], recs
        assert [int(x["counts"]["ATGC".index(chr(x["alt"]))]) for x in recs[:2]] == [1, 1]
        assert (log[0], log[1], log[14]) == (8, 6, 2)
        assert log[15] == 5 and span == 2048      # the three sites behind the span mark nothing
    far = [site(N - 1), (1 << 20, "A", "C"), ((1 << 31) - 1, "G", "T")]
    out.append(_case("read_edges_and_gaps", r, [site(1000), site(1199), site(1200), site(1400), site(1900)] + far, edges))
    # column depths 0, 1, 7, 8, 9 (the in-flight batch), 64, 65 (a wave) and 300; an alt read in each, both a seen and an
    # unseen alt asked
    r, s = [], []
    for i, n in enumerate((0, 1, 7, 8, 9, 64, 65, 300)):
        p = 250 + 450 * i
        r += stack(p, n, {0: {p: A1[p]}}, low_mapq=(0,) if n in (7, 65) else ())
        s += [site(p), site(p, A2)]

    def depths(recs, log):
        assert [M.depth_of(x) for x in recs[0::2]] == [0, 1, 7, 8, 9, 64, 65, 300]
        assert [int(x["alt_mq"]) for x in recs[0::2]] == [0, 1, 0, 1, 1, 1, 0, 1]
    out.append(_case("column_depths", r, s, depths))
    # an insertion in front of the site, a deletion over it, a soft-clipped read, a trailing insertion at tend
    p = 2000
    r = stack(p, 10) + [M.make_read(REF, p - 80, 200, ins={p: "AC"}, bq=93), M.make_read(REF, p - 70, 200, dels={p - 1: 3}, bq=93),
                        M.make_read(REF, p - 60, 200, {p: A1[p]}, bq=93, softclip=("ACGTACGTAC", "TTT")),
                        M.make_read(REF, p - 150, 150, ins={p: "GG"}, bq=93)]

    def indels(recs, log):
        assert [int(x) for x in recs[0]["counts"][4:]] == [2, 1] and statuses(recs) == ["IndelSite"] * 2
    out.append(_case("indels_and_soft_clip", r, [site(p), site(p, A3)], indels))
    # three alleles at one position, all three alts asked, one triple twice
    p = 3000
    r = stack(p, 14, {0: {p: A1[p]}, 1: {p: A2[p]}, 2: {p: A3[p]}, 3: {p: A2[p]}})

    def three(recs, log):
        assert [int(x["counts"]["ATGC".index(chr(x["alt"]))]) for x in recs] == [1, 2, 1, 1] and log[15] == 1
        assert recs[0].tobytes()[4:] == recs[3].tobytes()[4:] and [int(x) for x in recs["site"]] == [0, 1, 2, 3]
    out.append(_case("three_alleles", r, [site(p), site(p, A2), site(p, A3), site(p)], three, sort=False))
    # all 256 positions of a block and both neighbours
    rs = random.Random(11)
    r = [M.make_read(REF, 400 + 9 * k, 420, {512 + 37 * k: A1[512 + 37 * k]} if k < 7 else {}, bq=93) for k in range(11)]
    out.append(_case("whole_block", r, [site(p, rs.choice((A1, A2, A3))) for p in range(511, 769)]))
    # 255 / 256 / 257 sites: the workgroup's edge
    r = [M.make_read(REF, 100 * k, 330, {100 * k + 150: A1[100 * k + 150]}, bq=93) for k in range(36)]
    for n in (255, 256, 257):
        out.append(_case("sites_{}".format(n), r, [site(120 + 13 * k, (A1, A2, A3)[k % 3]) for k in range(n)]))
    return out


def status_cases():
    """One case per status."""
    out = []
    p = 500

    def add(name, reads, sites, want, **kw):
        out.append(_case(name, reads, sites, _want(*want), **kw))
    one = {0: {p: A1[p]}}
    add("pass", stack(p, 12, one), [site(p)], ["PASS"])
    add("low_bq_no_alt_read", stack(p, 12, one), [site(p, A2)], ["LowBQ"])
    add("low_bq", stack(p, 12, one, bq=93) + [], [site(p)], ["LowBQ"], min_bq=94)
    add("germline_het", stack(p, 12, {k: {p: A1[p]} for k in range(6)}), [site(p)], ["Germline"])
    add("het_site", stack(p, 12, {k: {p: A2[p]} for k in range(6)}), [site(p)], ["HetSite"])
    hetalt = {k: {p: (A2 if k % 2 else A3)[p]} for k in range(12)}
    add("hetalt_site", stack(p, 12, hetalt), [site(p), site(p, A2)], ["HetAltSite", "Germline"])
    hom = {k: {p: A2[p]} for k in range(12)}
    add("homalt_site", stack(p, 12, hom), [site(p), site(p, A2)], ["HomAltSite", "Germline"])
    add("no_coverage", stack(p, 12, one), [site(p + 900)], ["NoCoverage"])
    add("indel_site", stack(p, 12, one) + [M.make_read(REF, p - 50, 200, dels={p: 1}, bq=93)], [site(p)], ["IndelSite"])
    add("low_gq", stack(p, 4, one), [site(p)], ["LowGQ"], min_gq=99)
    add("panel_of_normals", stack(p, 12, one), [site(p)], ["PanelOfNormal"], pon=[_key(site(p))], com=[_key(site(p))])
    add("common_snp", stack(p, 12, one), [site(p)], ["ComSnp"], com=[_key(site(p))], pon=[_key(site(p, A2))])
    add("low_depth_ref", stack(p, 12, one), [site(p)], ["LowDepth"], min_ref_count=12)
    add("low_depth_alt", stack(p, 12, one), [site(p)], ["LowDepth"], min_alt_count=2)
    add("high_depth", stack(p, 14, one), [site(p)], ["HighDepth"], md_threshold=13)
    add("at_depth_threshold", stack(p, 14, one), [site(p)], ["PASS"], md_threshold=14)
    return out


def cases():
    return shape_cases() + status_cases()
