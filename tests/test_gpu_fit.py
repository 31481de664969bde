"""himut_fit_exposures on the device: k_fit_resample and k_fit_em against the plain model of
tests/fit_model.py.  The exposures are compared as uint64 views -- equality is of the bits -- and the resampled counts with
array_equal: shapes around the wave and the workgroup, more replicates than the grid, S read from global memory, the
hand-built cases, the seeds, repeatability, a call between two call runs, and the invariants at ten million draws."""
import numpy as np
import pytest

from himut_amd import fit
from tests import fit_cases as C, fit_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from himut_amd._ffi import Context
    with Context(0) as c:
        yield c


def _problem(C_, K, seed, mean=6):
    """(sig[C, K] with columns summing to 1 and a fifth of its entries 0, counts with zero channels): seeded."""
    rs = np.random.RandomState(seed)
    raw = rs.rand(C_, K)
    raw[rs.rand(C_, K) < 0.2] = 0.0
    raw[rs.randint(0, C_), :] = 1.0                      # no column sums to 0, one channel is never set aside
    rows, _ = fit.normalise_columns(raw.tolist(), ["s{}".format(k) for k in range(K)])
    counts = rs.poisson(mean, C_).astype(np.int64)
    counts[rs.rand(C_) < 0.15] = 0
    if C_ > 2:
        counts[0] = counts[C_ - 1] = 0
        counts[1] = max(int(counts[1]), 1)
    return np.array(rows, np.float64).reshape(C_, K), counts


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(ctx, sig, counts, n_boot, seed, iters):
    want_e, want_m = M.fit(sig, counts, n_boot=n_boot, seed=seed, iters=iters)
    expo, res = ctx.fit_exposures(sig, counts, n_boot=n_boot, seed=seed, iters=iters)
    assert res.dtype == np.int32 and np.array_equal(res, np.array(want_m, np.int64).reshape(n_boot + 1, -1))
    same = _bits(expo) == _bits(np.array(want_e, np.float64).reshape(n_boot + 1, -1))
    assert same.all(), (np.argwhere(~same)[:5], expo[~same][:5])
    none_e, none_m = ctx.fit_exposures(sig, counts, n_boot=n_boot, seed=seed, iters=iters, want_resampled=False)
    assert none_m is None and np.array_equal(_bits(none_e), _bits(expo))         # resampled = NULL
    return expo, res


def _budget(C_, K):
    """(iters, n_boot) that keep 2 * C * K * T * (B + 1) near two million model operations: T repeats the same code."""
    n_boot = 3
    return max(4, min(25, 2_000_000 // (2 * C_ * K * (n_boot + 1)))), n_boot


# the corners of C in {1, 63, 64, 65, 96, 255, 256, 257} x K in {1, 2, 63, 64, 65, 96}, a diagonal through it, and 1536 x 3
SHAPES = [(1, 1), (1, 96), (257, 1), (257, 96), (63, 2), (64, 63), (65, 64), (96, 65), (255, 96), (256, 2), (96, 96), (1536, 3)]


@pytest.mark.parametrize("C_,K", SHAPES)
def test_shapes(ctx, C_, K):
    sig, counts = _problem(C_, K, 1000 * C_ + K, mean=6 if C_ < 1000 else 1)
    iters, n_boot = _budget(C_, K)
    _check(ctx, sig, counts, n_boot, 11, iters)
    st = ctx.stats()
    assert st["n_candidates"] == n_boot + 1 and st["ms_total"] > 0
    # S is held in LDS exactly when it fits the default budget beside one replicate's arrays
    in_lds = (12 * C_ + 8 * K) + C_ * (K | 1) * 8 <= 65536
    assert (st["positions"] == C_ * (K | 1) * 8) if in_lds else (st["positions"] == 0)
    assert 1 <= st["n_records"] <= 4 and st["column_slots"] <= 65536


def test_fewer_replicates_share_a_workgroup_to_keep_s_in_lds(ctx):
    """100 x 75: S takes 100 * 75 * 8 = 60,000 bytes and a replicate 1,800, so three replicates fit 65,536 beside it and
    four do not."""
    sig, counts = _problem(100, 75, 10075)
    _check(ctx, sig, counts, 6, 2, 10)
    st = ctx.stats()
    assert st["n_records"] == 3 and st["positions"] == 60000 and st["column_slots"] == 65400
    assert st["n_unique_positions"] == 3                      # seven replicates: the last workgroup has two idle waves


def test_more_replicates_than_the_grid(ctx):
    """Both kernels stride.  Seventeen replicates on two workgroups: k_fit_resample makes nine trips, and k_fit_em, four
    replicates a workgroup, makes three on the first workgroup and two on the second -- a second trip re-initialises a
    wave's arrays, and the last trip of the first workgroup has one replicate and three waves without.  Then one
    replicate a workgroup (a budget of one byte: S from global memory), seven replicates on two workgroups."""
    sig, counts = _problem(65, 5, 7)
    ctx.debug_fit(2, 0)
    try:
        _check(ctx, sig, counts, 16, 3, 20)
        st = ctx.stats()
        assert st["n_unique_positions"] == 2 and st["n_records"] == 4 and st["n_candidates"] == 17
        assert -(-17 // st["n_records"]) > 2 * st["n_unique_positions"]          # more than two trips somewhere
        ctx.debug_fit(2, 1)
        _check(ctx, sig, counts, 6, 3, 20)
        st = ctx.stats()
        assert st["n_unique_positions"] == 2 and st["n_records"] == 1 and st["positions"] == 0
    finally:
        ctx.debug_fit(0, 0)


def test_global_memory_path_gives_the_same_bits(ctx):
    sig, counts = _problem(96, 30, 9630)
    lds_e, lds_m = _check(ctx, sig, counts, 3, 5, 17)
    assert ctx.stats()["positions"] == 96 * 31 * 8
    for budget in (4096, 1):                 # two replicates a workgroup, then one: S does not fit either way
        ctx.debug_fit(0, budget)
        try:
            e, m = ctx.fit_exposures(sig, counts, n_boot=3, seed=5, iters=17)
            st = ctx.stats()
        finally:
            ctx.debug_fit(0, 0)
        assert st["positions"] == 0 and st["n_records"] == (2 if budget == 4096 else 1)
        assert np.array_equal(_bits(e), _bits(lds_e)) and np.array_equal(m, lds_m)


def test_hand_built_cases(ctx):
    n = len(C.IDENTITY_COUNTS)
    e, _ = _check(ctx, np.array(C.identity(n)), C.IDENTITY_COUNTS, 0, 1, 25)
    assert e[0].tolist() == [float(m) for m in C.IDENTITY_COUNTS]
    e, _ = _check(ctx, np.array(C.DISJOINT_SIG), C.DISJOINT_COUNTS, 2, 1, 50)
    assert all(abs(got - want) <= 1e-12 * want for got, want in zip(e[0], C.DISJOINT_EXPECT))
    e, _ = _check(ctx, np.array(C.SUBNORMAL_SIG), C.SUBNORMAL_COUNTS, 1, 1, C.SUBNORMAL_ITERS)
    assert e[0][1] == 0.0 and e[1][1] == 0.0 and abs(e[0][0] - 1000.0) <= 1e-9
    # on the way there the device holds the same subnormals as the model
    e, _ = _check(ctx, np.array(C.SUBNORMAL_SIG), C.SUBNORMAL_COUNTS, 0, 1, 105)
    assert 0.0 < e[0][1] < 2.2250738585072014e-308
    e, m = _check(ctx, np.array(C.SMALL_SIG), C.ZERO_COUNTS, 3, 1, 10)
    assert not e.any() and not np.isnan(e).any() and not m.any()
    e, m = _check(ctx, np.array(C.SMALL_SIG), C.ONE_COUNTS, 3, 5, 10)
    assert (m == np.array(C.ONE_COUNTS)).all() and not np.isnan(e).any()
    e, m = _check(ctx, np.array(C.GAPS_SIG), C.GAPS_COUNTS, 9, 4, 12)
    assert not m[:, C.GAPS_ZERO].any() and (m.sum(axis=1) == sum(C.GAPS_COUNTS)).all()


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
def test_seeds(ctx, seed):
    sig, counts = _problem(40, 4, 404, mean=20)
    _e, m = _check(ctx, sig, counts, 4, seed, 8)
    assert len({tuple(r) for r in m.tolist()}) == 5            # the spectrum and four different replicates


def test_two_calls_give_the_same_bytes(ctx):
    sig, counts = _problem(96, 30, 77, mean=100)
    a = ctx.fit_exposures(sig, counts, n_boot=50, seed=8, iters=200)
    b = ctx.fit_exposures(sig, counts, n_boot=50, seed=8, iters=200)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.allclose(a[0].sum(axis=1), counts.sum(), rtol=1e-9)       # EM keeps the total
    assert (a[1].sum(axis=1) == counts.sum()).all()


def test_a_fit_between_two_call_runs_changes_nothing():
    from himut_amd import caller, synth, util as hutil
    cfg = synth.SynthConfig(seed=20, contig_len=60_000, read_len_mean=6000, read_len_sd=1200, read_len_min=2000,
                            read_len_max=12000, som_rate=2e-4, name="chrFit")
    b = synth.generate(cfg).batch
    chunks = [(c[1], c[2]) for c in hutil.chunkloci((b.name, 0, b.length))]
    w = caller.Worker(0)
    try:
        w.configure(germline_snv_prior=1 / (10 ** 3), phase=False, min_qv=30, min_mapq=60, qlen_lower_limit=3000,
                    qlen_upper_limit=9500, min_sequence_identity=0.99, min_gq=20, min_bq=93, min_trim=0.01,
                    max_mismatch_count=0, mismatch_window_size=20, md_threshold=52, min_ref_count=3, min_alt_count=1,
                    min_hap_count=3)
        recs, log = w.call_contig(b, chunks)
        sig, counts = _problem(96, 30, 5)
        first = w.ctx.fit_exposures(sig, counts, n_boot=5, seed=2, iters=10)
        w.ctx.run()                                   # the same reads, tables and regions: the fit touched none of them
        again, log2 = w.ctx.records(), w.ctx.log()
        assert len(recs) > 0 and again.tobytes() == np.asarray(recs).tobytes() and list(log2) == list(log)
        second = w.ctx.fit_exposures(sig, counts, n_boot=5, seed=2, iters=10)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    finally:
        w.close()


def test_ten_million_draws_keep_the_invariants(ctx):
    counts = np.array([4_000_000, 0, 5_999_999, 1], np.int64)
    sig = np.array([[0.5, 0.1], [0.2, 0.2], [0.2, 0.3], [0.1, 0.4]])
    e, m = ctx.fit_exposures(sig, counts, n_boot=2, seed=1, iters=2)
    assert (m.sum(axis=1) == 10_000_000).all() and not m[:, 1].any() and (m[0] == counts).all()
    assert (m[1] != m[2]).any() and abs(int(m[1][0]) - 4_000_000) < 20_000          # ten standard deviations
    assert not np.isnan(e).any()
