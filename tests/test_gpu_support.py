"""The support run (himut_run_support / himut_get_support) through the C ABI against the plain-Python model of its
contract (tests/support_model.py): np.array_equal on every field of the rows and on the site counts.  Hand-built
alignments pin the rules of the contract, a grid of single reads the mismatch window, two piles the lane and ordering
limits of the kernels, a synthetic sample and the twelve golden fixtures the run as a whole, and sequences on one
context the state a support run and the other runs leave each other."""
import os
import random
import re

import numpy as np
import pytest

from tests import germline_model as GM
from tests import support_model as M
from tests import util
from tests.test_support_cpu import CASES, check_fixture, fixture_sites

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _run(c, sites, batch=None, **kw):
    if batch is not None:
        c.push_reads(batch)
    c.run_support(np.array([s[0] for s in sites], np.int32), "".join(s[1] for s in sites).encode(),
                  "".join(s[2] for s in sites).encode(), **kw)
    return c.support()


def _both(c, batch, sites, push=True, **kw):
    """The run and the model on the same input: equal; returns (rows, site_counts)."""
    got = _run(c, sites, batch if push else None, **kw)
    M.assert_same(got, M.support(batch, sites, **kw))
    return got


def _contig(n=6000, seed=5):
    rs = random.Random(seed)
    ref = "".join(rs.choice("ATGC") for _ in range(n))
    nxt = lambda p, k: "ATGC"[("ATGC".index(ref[p]) + k) % 4]
    return ref, nxt


def _read(ref, start, length, subs=None, clip=0, swap_case=False, **kw):
    """germline_model.make_read with a leading soft clip of ``clip`` bases and, on request, the letters of the cs text's
    ``= + -`` operations in the other case (a substitution's two letters are lower-case by the pattern)."""
    r = GM.make_read(ref, start, length, subs, **kw)
    if clip:
        r["seq"] = "G" * clip + r["seq"]
        r["bq"] = [7] * clip + list(r["bq"])
        r["qstart"] = clip
    if swap_case:
        r["cs"] = "".join(k + (v if k in ":*" else v.swapcase()) for k, v in M.cs_operations(r["cs"]))
    return r


def _batch(ref, recs):
    from himut_amd.readbatch import batch_from_records
    return batch_from_records("chrU", len(ref), sorted(recs, key=lambda r: r["tstart"]))


def _site(ref, nxt, p, k=1):
    """The site of the substitution ref[p] -> the k-th next letter at 0-based p."""
    return (p + 1, ref[p], nxt(p, k))


# ---- 1. rules on hand-built alignments

def test_cover_and_support_at_the_ends_and_around_indels(ctx):
    ref, nxt = _contig()
    r0 = _read(ref, 100, 400, {100: nxt(100, 1), 499: nxt(499, 1), 300: nxt(300, 1)}, dels={200: 5}, ins={300: "AC", 350: "T"},
               bq_at={300: 11})
    r1 = _read(ref, 501, 100)
    b = _batch(ref, [r0, r1])
    sites = [_site(ref, nxt, 100), (203, ref[202], nxt(202, 1)), _site(ref, nxt, 300), (351, ref[350], nxt(350, 2)),
             _site(ref, nxt, 499), (501, ref[500], nxt(500, 1))]
    rows, counts = _both(ctx, b, sites)
    assert list(rows["site"]) == [0, 2, 4] and list(rows["read"]) == [0, 0, 0]
    assert counts.tolist() == [[1, 1], [1, 0], [1, 1], [1, 0], [1, 1], [0, 0]]     # tend itself is not covered
    assert list(rows["qpos"]) == [0, 200 - 5 + 2, 399 - 5 + 3] and int(rows[1]["bq"]) == 11
    assert list(rows["n_sub"]) == [3] * 3 and list(rows["n_indel"]) == [3] * 3
    assert int(rows[0]["bq_sum"]) == sum(r0["bq"])


def test_soft_clip_cs_forms_and_n_reference(ctx):
    ref, nxt = _contig()
    subs = {1010: nxt(1010, 1), 1200: nxt(1200, 2)}
    reads = [_read(ref, 1000, 300, subs, clip=37), _read(ref, 1001, 300, subs, long_cs=True),
             _read(ref, 1002, 300, subs, swap_case=True, ins={1100: "AC"}, dels={1150: 2}),
             _read(ref, 1003, 300, subs, long_cs=True, swap_case=True),
             _read(ref, 1004, 300, subs, nref=(1010,))]
    b = _batch(ref, reads)
    rows, counts = _both(ctx, b, [_site(ref, nxt, 1010), _site(ref, nxt, 1200, 2)])
    assert counts.tolist() == [[5, 4], [5, 5]]                            # the *n? substitution: covered, no row
    assert int(rows[0]["qpos"]) == 37 + 10 and int(rows[1]["qpos"]) == 9
    last = rows[rows["read"] == 4]
    assert list(last["site"]) == [1] and int(last[0]["n_sub"]) == 1      # ... and not in n_sub


def test_reads_in_play(ctx):
    """Secondary: neither row nor cover; supplementary: in; mapq at min_mapq in, one below out; both strands; two
    alignments of one name are two reads."""
    ref, nxt = _contig()
    s = {2100: nxt(2100, 1)}
    reads = [_read(ref, 2000, 300, s, flag=0x100), _read(ref, 2001, 300, s, flag=0x800, mapq=20),
             _read(ref, 2002, 300, s, flag=0x10, mapq=19), _read(ref, 2003, 300, s, mapq=20, qname="twice"),
             _read(ref, 2004, 300, s, flag=0x810, mapq=60, qname="twice"), _read(ref, 2005, 300, {}, mapq=60)]
    b = _batch(ref, reads)
    site = [_site(ref, nxt, 2100)]
    rows, counts = _both(ctx, b, site)
    assert counts.tolist() == [[5, 4]] and list(rows["read"]) == [1, 2, 3, 4]
    assert list(rows["flag"]) == [0x800, 0x10, 0, 0x810] and list(rows["qid"]) == [1, 2, 3, 3]
    rows, counts = _both(ctx, b, site, push=False, min_mapq=20)
    assert counts.tolist() == [[4, 3]] and list(rows["read"]) == [1, 3, 4] and list(rows["mapq"]) == [20, 20, 60]


def test_alleles_at_one_position_repeats_and_a_wrong_ref(ctx):
    ref, nxt = _contig()
    p = 3100
    reads = [_read(ref, 3000 + k, 300, {p: nxt(p, 1 + k % 2)}) for k in range(6)]
    b = _batch(ref, reads)
    a, c = (p + 1, ref[p], nxt(p, 1)), (p + 1, ref[p], nxt(p, 2))
    wrong = (p + 1, nxt(p, 3), nxt(p, 1))                                  # a ref the reads disagree with
    sites = [a, c, a, wrong, c]
    rows, counts = _both(ctx, b, sites)
    assert counts.tolist() == [[6, 3], [6, 3], [6, 3], [6, 0], [6, 3]]
    assert list(rows["site"]) == [0] * 3 + [1] * 3 + [2] * 3 + [4] * 3
    assert list(rows["read"]) == [0, 2, 4, 1, 3, 5, 0, 2, 4, 1, 3, 5]


# ---- 2. the mismatch window, one read per case

def _window_reads(ref, nxt, w, start):
    """Reads of one window size: the target with other mismatches at distance w - 1, w, w + 1 on either side, near the
    read's start, near its end, in a read shorter than 2 w, and with an insertion in front of the target itself."""
    L = 2 * w + 40
    out, sites = [], []

    def add(length, t, others, ins=None):
        nonlocal start
        if not 0 <= t < length:
            return
        subs = {start + t: nxt(start + t, 1)}
        subs.update({start + o: nxt(start + o, 2) for o in others if 0 <= o < length and o != t})
        out.append(_read(ref, start, length, subs, ins={start + k: v for k, v in (ins or {}).items()}))
        sites.append(_site(ref, nxt, start + t))
        start += length + 3
    mid = L // 2
    for d in (w - 1, w, w + 1):
        add(L, mid, [mid - d])
        add(L, mid, [mid + d])
        add(L, mid, [mid - d, mid + d])
    for t in (0, max(w - 1, 0), w):                                        # qpos < w, and the first qpos that is not
        add(L, t, [t + w, t + 2 * w - t, t + 2 * w - t + 1, t - 1])
    for t in (L - 1, L - w, L - w - 1):                                    # qpos + w > qlen, and the last qpos that is not
        add(L, t, [t - w, t - w - (t + w - L), t - w - (t + w - L) - 1, L - 1])
    if w > 1:
        S = 2 * w - 3                                                      # qlen < 2 w
        for t in (0, S // 2, S - 1):
            add(S, t, [0, S - 1, S // 3])
    add(L, mid, [mid + 1], ins={mid: "AC"})                               # an insertion and a substitution at one position
    add(L, mid, [], ins={mid: "A", mid + max(w, 1): "G"})
    return out, sites, start


def test_window_grid(ctx):
    ref, nxt = _contig(9000, 9)
    for w in (0, 1, 20, 100):
        reads, sites, _ = _window_reads(ref, nxt, w, 50)
        b = _batch(ref, reads)
        rows, counts = _both(ctx, b, sites, mismatch_window_size=w)
        assert len(rows) == len(sites) and np.all(counts[:, 1] == 1)
        assert len(set(rows["window_mismatches"].tolist())) >= (2 if w else 1)
        # the window rule against a direct count over the read's mismatch list
        for row in rows:
            _subs, mm = M.cs_walk(b, int(row["read"]))
            s, e = M.mismatch_range(sites[int(row["site"])][0], int(row["qpos"]), int(row["qlen"]), w)
            assert int(row["window_mismatches"]) == sum(s <= p <= e for p in mm) - 1


# ---- 3. lane and ordering limits

def test_one_read_over_200_sites(ctx):
    ref, nxt = _contig()
    ps = [400 + 7 * k for k in range(200)]
    carried = {p: nxt(p, 1) for p in ps[::3]}
    b = _batch(ref, [_read(ref, 350, 1600, carried), _read(ref, 2500, 200, {2600: nxt(2600, 1)})])
    sites = [(5, "A", "C"), (349, "A", "C")] + [_site(ref, nxt, p) for p in ps] + [(2800, "A", "C"), (5999, "C", "T")]
    rows, counts = _both(ctx, b, sites)
    assert len(rows) == 67 and counts[:2].tolist() == [[0, 0]] * 2 and counts[-2:].tolist() == [[0, 0]] * 2
    assert np.all(counts[2:-2, 0] == 1)


def test_one_site_under_300_reads(ctx):
    ref, nxt = _contig()
    rs = random.Random(2)
    p = 1500
    reads = [_read(ref, 1200 + (k * 37) % 170, 400, {p: nxt(p, 1)} if k >= 40 else {}, mapq=rs.randrange(0, 61)) for k in range(340)]
    b = _batch(ref, reads)
    rows, counts = _both(ctx, b, [_site(ref, nxt, p)])
    assert counts.tolist() == [[340, 300]] and np.all(np.diff(rows["read"]) > 0)
    rows, counts = _both(ctx, b, [_site(ref, nxt, p)], push=False, min_mapq=30)
    assert 100 < len(rows) < 200


# ---- 4. a synthetic sample

@pytest.fixture(scope="module")
def sample():
    from himut_amd import synth
    return synth.generate(synth.SynthConfig(seed=11, contig_len=100_000, depth=30.0, frac_softclip=0.3, softclip_max=200)).batch


def _sample_sites(b):
    rs = random.Random(4)
    real = set()
    for i in range(b.n):
        real.update((p, r, a) for (p, r, a, _q) in M.cs_walk(b, i)[0])
    decoys = set()
    while len(decoys) < len(real):
        p, r, a = rs.randrange(1, b.length + 1), rs.choice("ATGC"), rs.choice("ATGC")
        if r != a and (p, r, a) not in real:
            decoys.add((p, r, a))
    return sorted(real | decoys)


def test_synthetic_sample(ctx, sample):
    sites = _sample_sites(sample)
    assert len(sites) > 1500 and int(sample.qstart.max()) > 0
    rows, _ = _both(ctx, sample, sites)
    hi, _ = _both(ctx, sample, sites, push=False, min_mapq=60)
    assert 0 < len(hi) < len(rows)


def _call(c, batch, chunks, push=True):
    from himut_amd import gtlib
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=0, qlen_upper_limit=1 << 30, md_threshold=1 << 30, phase=0)
    c.set_params(**{k: v for k, v in p.items() if not k.endswith("_prior")})
    c.set_gt_lut(*gtlib.build_tables(p["germline_snv_prior"]))
    c.set_site_set(0, np.zeros(0, np.uint64)); c.set_site_set(1, np.zeros(0, np.uint64))
    c.set_chunks(chunks)
    if push:
        c.push_reads(batch)
    c.run()
    return c.records(), c.log()


def test_alt_reads_equal_the_call_runs_counts(ctx, sample):
    recs, _ = _call(ctx, sample, [(0, sample.length)])
    bi = recs[recs["gt_state"] != 2]
    assert len(bi) > 50
    sites = [(int(r["tpos"]), chr(r["ref"]), chr(r["alt"])) for r in bi]
    _rows, counts = _both(ctx, sample, sites, push=False)
    want = [int(r["counts"]["ATGC".index(chr(r["alt"]))]) for r in bi]
    assert counts[:, 1].tolist() == want


# ---- 5. the golden fixtures on the device

def test_golden_fixtures(ctx):
    total = left_out = 0
    for case in CASES:
        batch, exp = util.load_case(case)
        sites, site_of = fixture_sites(exp)
        ctx.push_reads(batch)
        rows, counts = _run(ctx, sites, mismatch_window_size=util.params_of(exp)["mismatch_window_size"])
        n, out = check_fixture(exp, rows, counts, site_of)
        total += n
        left_out += out
    assert total == 5687 and left_out <= 6


# ---- 6. sequences on one context

def test_call_support_call(ctx, sample):
    recs, log = _call(ctx, sample, [(0, sample.length)])
    sites = [(int(r["tpos"]), chr(r["ref"]), chr(r["alt"])) for r in recs[recs["gt_state"] != 2]]
    got = _run(ctx, sites)
    again, log2 = _call(ctx, sample, [(0, sample.length)], push=False)
    assert again.tobytes() == recs.tobytes() and log2 == log
    M.assert_same(_run(ctx, sites), got)
    assert ctx.records().tobytes() == recs.tobytes()                       # the call run's records are still served


def test_support_germline_support(ctx, sample):
    from himut_amd import gtlib
    sites = _sample_sites(sample)[::5]
    ctx.push_reads(sample)
    first = _run(ctx, sites)
    ctx.set_gt_lut(*gtlib.build_tables(1 / (10 ** 3)))
    ctx.set_chunks([(1, sample.length)])
    ctx.run_germline()
    germ, glog = ctx.germline()
    assert len(germ) > 0
    second = _run(ctx, sites)
    assert second[0].tobytes() == first[0].tobytes() and np.array_equal(second[1], first[1])
    again, alog = ctx.germline()
    assert again.tobytes() == germ.tobytes() and alog == glog


def test_buffer_growth_and_reuse(ctx, sample):
    sites = _sample_sites(sample)
    ctx.push_reads(sample)
    for part in (sites[::2], sites[:7], sites, []):
        got = _run(ctx, part)
        M.assert_same(got, M.support(sample, part))
    assert got[0].shape == (0,) and got[1].shape == (0, 2) and ctx.stats()["n_records"] == 0
    # a smaller batch after a larger one
    ref, nxt = _contig()
    small = _batch(ref, [_read(ref, 10 + k, 100, {50: nxt(50, 1)}) for k in range(3)])
    mixed = sorted([_site(ref, nxt, 50)] + sites[:50])
    rows, counts = _both(ctx, small, mixed)
    assert counts[mixed.index(_site(ref, nxt, 50))].tolist() == [3, 3] and len(rows) == 3
    st = ctx.stats()
    assert st["n_records"] == 3 and st["n_reads"] == 3 and st["read_bases"] == 300 and st["ms_total"] > 0


def test_bad_site_lists_leave_the_context_usable(ctx):
    from himut_amd._ffi import Context, HimutError
    ref, nxt = _contig()
    b = _batch(ref, [_read(ref, 10, 100, {50: nxt(50, 1)})])
    good = [_site(ref, nxt, 50)]
    want = _both(ctx, b, good)
    for bad in ([(60, "A", "C"), (50, "A", "C")], [(50, "a", "C")], [(50, "A", "c")], [(50, "A", "A")], [(50, "N", "A")],
                [(0, "A", "C")]):
        with pytest.raises(HimutError) as e:
            _run(ctx, bad)
        assert e.value.code == 1
        M.assert_same(ctx.support(), want)                                 # the last good run is still served
    M.assert_same(_run(ctx, good), want)
    with Context(0) as fresh, pytest.raises(HimutError) as e:             # no reads
        _run(fresh, good)
    assert e.value.code == 1


def test_two_runs_give_the_same_bytes(ctx, sample):
    sites = _sample_sites(sample)
    a = _run(ctx, sites, sample)
    b = _run(ctx, sites)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 7. ABI

def test_row_layout_and_exports():
    import ctypes
    from himut_amd import _ffi, build
    assert _ffi.SUPPORT_ROW_DTYPE.itemsize == 48 and ctypes.sizeof(_ffi.SupportParams) == 16
    text = open(os.path.join(os.path.dirname(build.INCLUDE), "include", "himut_hip.h")).read()
    body = re.search(r"typedef struct himut_support_row \{(.*?)\} himut_support_row;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(_ffi.SUPPORT_ROW_DTYPE.names)
    L = ctypes.CDLL(build.HIP_LIB)
    assert hasattr(L, "himut_run_support") and hasattr(L, "himut_get_support")
