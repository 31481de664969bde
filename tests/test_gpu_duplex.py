"""The duplex run (himut_run_duplex / himut_get_duplex) through the C ABI against the plain-Python model of its contract
(tests/duplex_model.py): equal record bytes, equal single-strand spectrum, equal counters, on the hand-built reads of
tests/duplex_cases.py and on a small seeded sweep; every record's site fields against himut_run_sites on the same
context; two runs with equal bytes; the malformed mate arrays; what the run leaves of the other runs' results."""
import numpy as np
import pytest

from tests import duplex_cases as C
from tests import duplex_model as M
from tests import sites_model as S

pytestmark = pytest.mark.gpu

PARAM_NAMES = ("min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq", "min_bq", "max_mismatch_count",
               "mismatch_window_size", "md_threshold", "min_ref_count", "min_alt_count", "min_hap_count", "min_sequence_identity",
               "min_trim")
CASES = C.cases()


@pytest.fixture(scope="module")
def ctx():
    from himut_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _configure(c, kw, prior=1 / (10 ** 3)):
    from himut_amd import gtlib
    p = dict(M.DEFAULTS, **kw)
    c.set_params(**{k: p[k] for k in PARAM_NAMES})
    c.set_gt_lut(*gtlib.build_tables(prior))
    c.set_site_set(0, np.array(sorted(kw.get("pon_keys", ())), np.uint64))
    c.set_site_set(1, np.array(sorted(kw.get("com_keys", ())), np.uint64))


def _duplex(c, batch, mate, chunks, kw, push=True):
    _configure(c, kw)
    c.set_chunks(chunks)
    if push:
        c.push_reads(batch)
    c.run_duplex(mate)
    return c.duplex()


def _site_arrays(recs):
    return recs["tpos"].astype(np.int32), bytes(recs["ref"]), bytes(recs["alt"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(ctx, case):
    """Records, spectrum and counters are the model's and say what the rule says; the first 64 bytes of every record are
    the sites run's record of the candidate on the same context; a second run gives the same bytes."""
    _name, b, mate, chunks, kw, expect = case
    got = _duplex(ctx, b, mate, chunks, kw)
    M.assert_same(got, M.run(b, mate, chunks, **kw))
    recs, ss, log = got
    M.check_identities(recs, ss, log)
    if expect:
        expect(recs, ss, M.logd(log))
    ctx.run_sites(*_site_arrays(recs))
    sites, _slog = ctx.sites()
    assert len(sites) == len(recs)
    for name in S.SITE_RECORD_DTYPE.names:
        assert np.array_equal(sites[name], recs[name]), name
    again = _duplex(ctx, b, mate, chunks, kw, push=False)
    assert again[0].tobytes() == recs.tobytes() and again[1] == ss and again[2] == log
    st = ctx.stats()
    assert st["n_records"] == len(recs) and st["n_reads"] == b.n and st["reran"] == 0


@pytest.mark.parametrize("seed", range(6))
def test_seeded_sweep(ctx, seed):
    b, mate, chunks, kw = C.random_case(seed)
    M.assert_same(_duplex(ctx, b, mate, chunks, kw), M.run(b, mate, chunks, **kw))


def test_site_sets_reach_the_verdict(ctx):
    """The panel of normals and the common SNPs apply to a candidate as they do to a site."""
    _name, b, mate, chunks, kw, _e = next(c for c in CASES if c[0] == "one_molecule_two_sites")
    plain = M.run(b, mate, chunks, **kw)[0]
    keys = [(int(r["tpos"]) << 4) | ("ATGC".index(chr(r["ref"])) << 2) | "ATGC".index(chr(r["alt"])) for r in plain]
    kw = dict(kw, pon_keys=keys[:1], com_keys=keys[1:])
    got = _duplex(ctx, b, mate, chunks, kw)
    M.assert_same(got, M.run(b, mate, chunks, **kw))
    assert [S.STATUS[int(x)] for x in got[0]["status"]] == ["PanelOfNormal", "ComSnp"]


def test_malformed_mate(ctx):
    """Every malformed mate array is HIMUT_ERR_ARG with a message, and a good run follows on the same context."""
    from himut_amd import _ffi
    _name, b, mate, chunks, kw, _e = next(c for c in CASES if c[0] == "two_molecules_one_site")
    want = M.run(b, mate, chunks, **kw)
    M.assert_same(_duplex(ctx, b, mate, chunks, kw), want)
    i = int(np.flatnonzero(mate >= 0)[0])
    lone = int(np.flatnonzero(mate < 0)[0])
    bad = {"outside": (i, b.n), "below": (i, -2), "itself": (i, i), "one_sided": (lone, i)}
    for what, (k, v) in bad.items():
        m = mate.copy()
        m[k] = v
        with pytest.raises(ValueError):
            M.check_mate(m, b.n)
        with pytest.raises(_ffi.HimutError) as e:
            ctx.run_duplex(m)
        assert e.value.code == 1 and "mate" in e.value.message, (what, e.value.message)
    for m in (mate[:-1], np.append(mate, -1)):
        with pytest.raises(_ffi.HimutError) as e:
            ctx.run_duplex(m)
        assert e.value.code == 1 and "n_mate" in e.value.message
    ctx.run_duplex(mate)
    M.assert_same(ctx.duplex(), want)


def test_other_getters_keep_their_runs(ctx):
    """A duplex run changes nothing the sites, support and haplotag getters serve."""
    _name, b, mate, chunks, kw, _e = next(c for c in CASES if c[0] == "alt_on_unpaired_reads")
    _configure(ctx, kw)
    ctx.push_reads(b)
    p = 501
    ctx.run_sites(np.array([p, p + 3], np.int32), b"AA", b"CC")
    ctx.run_support(np.array([p], np.int32), C.REF[p - 1].encode(), C.A1[p - 1].encode(), min_mapq=0)
    ctx.run_haplotag(np.array([p], np.int32), b"A", b"C", [0], [0])
    before = (ctx.sites(), ctx.support(), ctx.haplotag())
    M.assert_same(_duplex(ctx, b, mate, chunks, kw, push=False), M.run(b, mate, chunks, **kw))
    after = (ctx.sites(), ctx.support(), ctx.haplotag())
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert (u.tobytes() == v.tobytes()) if isinstance(u, np.ndarray) else u == v


def test_runs_on_kept_capacities():
    """On a context of its own: the second run goes on the capacities the first one kept; a batch that needs more column
    slots than were kept (eighty candidates under 2 kb reads after one under 300-base reads) is run again with exact
    sizes, says so, and gives the model's bytes all the same."""
    small = next(c for c in CASES if c[0] == "full_overlap")
    large = next(c for c in CASES if c[0] == "long_lists")
    from himut_amd import _ffi
    with _ffi.Context(0) as c:
        for _name, b, mate, chunks, kw, _e in (small, small):
            M.assert_same(_duplex(c, b, mate, chunks, kw), M.run(b, mate, chunks, **kw))
            assert c.stats()["reran"] == 0
        _name, b, mate, chunks, kw, _e = large
        M.assert_same(_duplex(c, b, mate, chunks, kw), M.run(b, mate, chunks, **kw))
        M.assert_same(_duplex(c, b, mate, chunks, kw, push=False), M.run(b, mate, chunks, **kw))
