"""`himut fit` without a device: the plain model of tests/fit_model.py on the hand-built cases
of tests/fit_cases.py, its likelihood over the iterations, its resampling; the host side of himut_amd/fit.py -- parsers,
--select, every error message, prepare's normalisation and set-aside, the --opp normcounts weights, the writers."""
import math

import numpy as np
import pytest

from himut_amd import fit
from tests import fit_cases as C, fit_model as M


def test_identity_exposures_equal_the_counts():
    e = M.em(C.identity(len(C.IDENTITY_COUNTS)), C.IDENTITY_COUNTS, sum(C.IDENTITY_COUNTS), 25)
    assert e == [float(m) for m in C.IDENTITY_COUNTS]


def test_disjoint_support_sums_its_channels():
    for iters in (1, 2, 50):
        e = M.em(C.DISJOINT_SIG, C.DISJOINT_COUNTS, sum(C.DISJOINT_COUNTS), iters)
        for got, want in zip(e, C.DISJOINT_EXPECT):
            assert abs(got - want) <= 1e-12 * want, (iters, e)


def test_subnormal_exposure_reaches_exactly_zero():
    steps = list(M.em_steps(C.SUBNORMAL_SIG, C.SUBNORMAL_COUNTS, 1000, C.SUBNORMAL_ITERS))
    b = [e[1] for e in steps]
    assert b[-1] == 0.0 and not math.isnan(steps[-1][0])
    assert any(0.0 < x < 2.2250738585072014e-308 for x in b)         # it passed through the subnormals on the way
    assert abs(steps[-1][0] - 1000.0) <= 1e-12 * 1000.0
    assert all(x >= y for x, y in zip(b, b[1:]))


def test_no_mutations_and_one_mutation():
    e = M.em(C.SMALL_SIG, C.ZERO_COUNTS, 0, 10)
    assert e == [0.0, 0.0, 0.0]
    expo, res = M.fit(C.SMALL_SIG, C.ONE_COUNTS, n_boot=3, seed=5, iters=10)
    assert res == [C.ONE_COUNTS] * 4
    assert all(not math.isnan(x) and x >= 0.0 for row in expo for x in row)
    assert abs(sum(expo[0]) - 1.0) < 1e-12 and expo[1] == expo[0]


def test_zero_channels_are_never_drawn():
    for seed in (0, 1, 2 ** 64 - 1):
        for b in range(1, 6):
            m = M.resample(C.GAPS_COUNTS, b, seed)
            assert sum(m) == sum(C.GAPS_COUNTS) and all(m[c] == 0 for c in C.GAPS_ZERO), (seed, b, m)


def test_resampled_counts_sum_to_n_and_differ_by_seed_and_replicate():
    counts = [3, 0, 40, 7, 1, 0, 0, 25]
    seen = set()
    for seed in (0, 1, 7, 2 ** 63, 2 ** 64 - 1, 2 ** 64 + 1):
        for b in (1, 2, 1000, 100000):
            m = M.resample(counts, b, seed)
            assert sum(m) == sum(counts) and m[1] == m[5] == m[6] == 0
            seen.add((seed & M.MASK, tuple(m)))
    assert len(seen) >= 18                                              # seed 2^64 + 1 is seed 1
    assert M.resample(counts, 0, 9) == counts
    assert M.resample(counts, 3, 1) == M.resample(counts, 3, 2 ** 64 + 1)
    # the generator, worked by hand for its first value: splitmix64's first output from state 0 is 0xE220A8397B1DCDAF
    assert M.draw(0, 0, 0, 1 << 32) == 0xE220A8397B1DCDAF >> 32


def test_loglik_is_non_decreasing():
    rs = np.random.RandomState(20)
    sig = rs.rand(40, 5)
    sig[rs.rand(40, 5) < 0.2] = 0.0
    prep_rows, _ = fit.normalise_columns(sig.tolist(), ["s{}".format(k) for k in range(5)])
    counts = [int(x) for x in rs.poisson(30, 40)]
    counts[3] = counts[17] = 0
    prev = None
    for e in M.em_steps(prep_rows, counts, sum(counts), 60):
        ll = M.loglik(prep_rows, counts, e)
        if prev is not None:
            assert ll >= prev - 1e-9 * abs(prev), (prev, ll)
        prev = ll


# ---- the host side

def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@pytest.mark.parametrize("layout", sorted(C.SPECTRA))
def test_read_spectrum_layouts(tmp_path, layout):
    s = fit.read_spectrum(_write(tmp_path, "s.tsv", C.SPECTRA[layout]))
    assert s.labels == C.LABELS and s.counts == C.COUNTS
    assert s.header[s.label_column + 1] == "counts"


def test_tables_the_package_writes_are_read_back(tmp_path):
    from himut_amd import mutlib, spectra, strands
    counts = {k: i for i, k in enumerate(mutlib.SBS96_LST)}
    mutlib.write_sbs96_counts(counts, str(tmp_path / "a.tsv"))
    s = fit.read_spectrum(str(tmp_path / "a.tsv"))
    assert s.labels == list(mutlib.SBS96_LST) and s.counts == list(range(96))
    spectra.write_counts("id83", spectra.ID83_LST, list(range(83)), str(tmp_path / "b.tsv"))
    s = fit.read_spectrum(str(tmp_path / "b.tsv"))
    assert s.labels == list(spectra.ID83_LST) and s.counts == list(range(83))
    # sbs384 and sbs192 go through strands.write_counts: a label column, then counts -- the rule covers them
    strands.write_counts("sbs192", ["T:A[C>A]A", "U:A[C>A]A"], {"T:A[C>A]A": 4, "U:A[C>A]A": 9}, str(tmp_path / "c.tsv"))
    s = fit.read_spectrum(str(tmp_path / "c.tsv"))
    assert s.labels == ["T:A[C>A]A", "U:A[C>A]A"] and s.counts == [4, 9]


def test_read_spectrum_errors(tmp_path):
    for text, word in (("a\tb\n1\t2\n", "no header line with a field named counts"),
                       ("counts\tx\n1\t2\n", "no label column"),
                       ("k\tcounts\nA\t1\nA\t2\n", "label A appears twice"),
                       ("k\tcounts\nA\t1.5\n", "is not an integer"),
                       ("k\tcounts\nA\t-1\n", "the count of A is negative"),
                       ("k\tcounts\nA\n", "fewer fields")):
        with pytest.raises(fit.FitError) as e:
            fit.read_spectrum(_write(tmp_path, "bad.tsv", text))
        assert word in str(e.value), text


def test_read_signatures_and_select_order(tmp_path):
    p = _write(tmp_path, "sig.tsv", C.SIGNATURES)
    labels, names, rows = fit.read_signatures(p)
    assert labels == C.SIG_LABELS and names == ["SigA", "SigB", "SigC"] and rows == C.SIG_ROWS
    labels, names, rows = fit.read_signatures(p, ["SigC", "SigA"])
    assert names == ["SigC", "SigA"] and rows == [[r[2], r[0]] for r in C.SIG_ROWS]
    for select, word in ((["SigQ"], "no signature named SigQ"), (["SigA", "SigA"], "--select names SigA twice")):
        with pytest.raises(fit.FitError) as e:
            fit.read_signatures(p, select)
        assert word in str(e.value)
    for text, word in ((C.SIG_NEGATIVE, "SigB of A[C>T]G is negative or not finite"), (C.SIG_TEXT, "SigB of A[C>T]G is not a number"),
                       ("Type\n", "no signature column"), ("", "empty"), ("Type\tA\tA\nx\t1\t2\n", "appears twice"),
                       ("Type\tA\nx\t1\t2\n", "has 3 fields"), ("Type\tA\nx\t1\nx\t1\n", "label x appears twice"),
                       ("Type\tA\nx\tinf\n", "negative or not finite")):
        with pytest.raises(fit.FitError) as e:
            fit.read_signatures(_write(tmp_path, "bad.tsv", text))
        assert word in str(e.value), text


def test_prepare_normalises_matches_and_sets_aside():
    prep = fit.prepare(C.LABELS, C.COUNTS, C.SIG_LABELS, ["SigA", "SigB", "SigC"], C.SIG_ROWS)
    assert prep.labels == C.LABELS and prep.counts == C.COUNTS and prep.aside == [] and not prep.weighted
    assert prep.sig.dtype == np.float64 and prep.sig.shape == (6, 3)
    # the sums run in ascending channel order: 0.5 + 0.2 + 0.1 + 0.1 + 0.1 + 0.0 and so on, as floats
    raw = [C.SIG_ROWS[C.SIG_LABELS.index(k)] for k in C.LABELS]
    sums = [0.0, 0.0, 0.0]
    for row in raw:
        for k in range(3):
            sums[k] += row[k]
    assert prep.sig.tolist() == [[row[k] / sums[k] for k in range(3)] for row in raw]
    assert np.allclose(prep.sig, C.PREPARED_ALL, rtol=1e-15, atol=0) and prep.scale == [1.0, 1.0, 1.0]
    ab = fit.prepare(C.LABELS, C.COUNTS, C.SIG_LABELS, ["SigA", "SigB"], [r[:2] for r in C.SIG_ROWS])
    assert ab.labels == C.SELECT_AB_LABELS and ab.counts == C.SELECT_AB_COUNTS and ab.aside == [("T[T>G]T", 5)]
    assert ab.N == 95 and ab.unexplained == 5 and ab.all_labels == C.LABELS


def test_prepare_with_weights():
    prep = fit.prepare(C.LABELS, C.COUNTS, C.SIG_LABELS, ["SigA", "SigB"], [r[:2] for r in C.SIG_ROWS], C.OPP_WEIGHTS)
    base = fit.prepare(C.LABELS, C.COUNTS, C.SIG_LABELS, ["SigA", "SigB"], [r[:2] for r in C.SIG_ROWS])
    w = [C.OPP_WEIGHTS[k] for k in C.SELECT_AB_LABELS]
    for k in range(2):
        d = 0.0
        for c in range(5):
            d += base.sig[c][k] * w[c]
        assert prep.scale[k] == d
        assert [prep.sig[c][k] for c in range(5)] == [base.sig[c][k] * w[c] / d for c in range(5)]
    assert prep.weighted and prep.aside == [("T[T>G]T", 5)]
    # a weight of 0 sets a channel aside even where a signature is not 0 there
    w0 = dict(C.OPP_WEIGHTS, **{"A[C>A]A": 0.0})
    p0 = fit.prepare(C.LABELS, C.COUNTS, C.SIG_LABELS, ["SigA", "SigB"], [r[:2] for r in C.SIG_ROWS], w0)
    assert p0.aside == [("A[C>A]A", 30), ("T[T>G]T", 5)] and p0.N == 65


def test_prepare_errors():
    ab = [r[:2] for r in C.SIG_ROWS]
    cases = (
        (dict(labels=C.LABELS + ["G[T>A]G"], counts=C.COUNTS + [1]), "label G[T>A]G of the spectrum is not in the signature matrix"),
        (dict(labels=C.LABELS[:-1], counts=C.COUNTS[:-1]), "label T[T>G]T of the signature matrix is not in the spectrum"),
        (dict(weights={k: 1.0 for k in C.LABELS[1:]}), "label A[C>A]A of the spectrum has no opportunity weight"),
        (dict(weights=dict(C.NORMCOUNTS_WEIGHTS), names=["SigA", "SigB", "SigC"], rows=C.SIG_ROWS), "signature SigC sums to 0"),
        (dict(names=["SigA", "SigZ"], rows=[[r[0], 0.0] for r in C.SIG_ROWS]), "signature SigZ sums to 0"),
    )
    for kw, word in cases:
        with pytest.raises(fit.FitError) as e:
            fit.prepare(kw.get("labels", C.LABELS), kw.get("counts", C.COUNTS), C.SIG_LABELS, kw.get("names", ["SigA", "SigB"]),
                        kw.get("rows", ab), kw.get("weights"))
        assert word in str(e.value), word
    with pytest.raises(fit.FitError) as e:
        fit.prepare(["x"], [1], ["x"], ["s{}".format(k) for k in range(97)], [[1.0] * 97])
    assert "97 signatures" in str(e.value)
    for bad in ((-1, 10, 5), (100001, 10, 5), (1, 0, 5), (1, 100001, 5), (1, 10, 2 ** 31)):
        with pytest.raises(fit.FitError):
            fit.check_limits(*bad)
    fit.check_limits(0, 1, 0)
    fit.check_limits(100000, 100000, 2 ** 31 - 1)


def test_opportunity_tables(tmp_path):
    assert fit.read_opportunities(_write(tmp_path, "o.tsv", C.OPPORTUNITIES)) == C.OPP_WEIGHTS
    assert fit.read_opportunities(_write(tmp_path, "o2.tsv", "a\t1\nb\t0.5\n")) == {"a": 1.0, "b": 0.5}     # no header
    for text, word in (("a\t1\na\t2\n", "label a appears twice"), ("a\t1\nb\t-2\n", "the weight of b is negative"),
                       ("a\t1\nb\tx\n", "the weight of b is not a number"), ("a\t1\nb\n", "without a weight")):
        with pytest.raises(fit.FitError) as e:
            fit.read_opportunities(_write(tmp_path, "bad.tsv", text))
        assert word in str(e.value)


def test_normcounts_weights_from_the_tables_own_columns(tmp_path):
    s = fit.read_spectrum(_write(tmp_path, "n.tsv", C.SPECTRUM_NORMCOUNTS))
    assert fit.normcounts_weights(s) == C.NORMCOUNTS_WEIGHTS
    plain = fit.read_spectrum(_write(tmp_path, "p.tsv", C.SPECTRUM_SBS96))
    with pytest.raises(fit.FitError) as e:
        fit.normcounts_weights(plain, "p.tsv")
    assert "p.tsv is not a normcounts table" in str(e.value)
    prep = fit.load_inputs(str(tmp_path / "n.tsv"), _write(tmp_path, "sig.tsv", C.SIGNATURES), "SigB,SigA", "normcounts")
    assert prep.names == ["SigB", "SigA"] and prep.weighted and prep.aside == [("T[T>G]T", 5)]


def _prep_ab(weights=None):
    return fit.prepare(C.LABELS, C.COUNTS, C.SIG_LABELS, ["SigA", "SigB"], [r[:2] for r in C.SIG_ROWS], weights)


def test_summarise_and_writers(tmp_path):
    prep = _prep_ab()
    expo, _ = M.fit(prep.sig, prep.counts, n_boot=4, seed=3, iters=30)
    res = fit.summarise(prep, expo, min_fraction=0.3)
    e = expo[0]
    assert res["exposure"] == e and res["exposure_genome"] == e
    assert res["fraction"] == [e[0] / (e[0] + e[1]), e[1] / (e[0] + e[1])]
    assert res["recon"] == [prep.sig[c][0] * e[0] + prep.sig[c][1] * e[1] for c in range(5)]
    assert 0.9 < res["cosine"] <= 1.0 and res["loglik"] == M.loglik(prep.sig.tolist(), prep.counts, e)
    reps = np.array(expo[1:])
    for name, q in (("lo", 2.5), ("median", 50.0), ("hi", 97.5)):
        assert res["boot"][name] == [float(x) for x in np.percentile(reps, q, axis=0)]
    assert res["boot"]["presence"] == [sum(1 for r in expo[1:] if r[k] / (r[0] + r[1]) >= 0.3) / 4.0 for k in range(2)]
    out = str(tmp_path / "e.tsv")
    fit.write_exposures(prep, res, out)
    lines = open(out).read().split("\n")
    assert lines[:5] == ["# N\t100", "# fitted_N\t95", "# unexplained\t5", "# cosine\t" + repr(res["cosine"]),
                         "# loglik\t" + repr(res["loglik"])]
    assert lines[5] == "signature\texposure\tfraction\texposure_genome\tlo\tmedian\thi\tpresence"
    assert lines[6].split("\t") == ["SigA"] + [repr(x) for x in (e[0], res["fraction"][0], e[0], res["boot"]["lo"][0],
                                                                 res["boot"]["median"][0], res["boot"]["hi"][0],
                                                                 res["boot"]["presence"][0])]
    assert [float(x) for x in lines[7].split("\t")[1:4]] == [e[1], res["fraction"][1], e[1]] and lines[8:] == [""]
    # without replicates: four columns
    res0 = fit.summarise(prep, expo[:1])
    assert res0["boot"] is None
    fit.write_exposures(prep, res0, out)
    assert open(out).read().split("\n")[5:7] == ["signature\texposure\tfraction\texposure_genome",
                                                 "SigA\t{!r}\t{!r}\t{!r}".format(e[0], res["fraction"][0], e[0])]
    fit.write_recon(prep, res, out)
    want = ["label\tcounts\treconstructed"] + ["{}\t{}\t{!r}".format(k, n, r) for k, n, r in
                                               zip(C.LABELS, C.COUNTS, res["recon"] + [0.0])]
    assert open(out).read() == "\n".join(want) + "\n"
    fit.write_boot(prep, expo, out)
    assert open(out).read() == "replicate\tSigA\tSigB\n" + "".join("{}\t{!r}\t{!r}\n".format(b, r[0], r[1]) for b, r in enumerate(expo))
    fit.write_log(prep, 4, 30, out)
    assert open(out).read() == C.log_text(5, 1, 2, 95, 5, 30)


def test_genome_exposures_under_weights():
    prep = _prep_ab(C.OPP_WEIGHTS)
    expo, _ = M.fit(prep.sig, prep.counts, iters=40)
    res = fit.summarise(prep, expo)
    e = expo[0]
    g = [e[0] / prep.scale[0], e[1] / prep.scale[1]]
    t = g[0] + g[1]
    assert res["exposure_genome"] == [g[0] * (95.0 / t), g[1] * (95.0 / t)]
    assert abs(sum(res["exposure_genome"]) - 95.0) < 1e-9 and res["exposure"] == e
    # N = 0: nothing divides by zero
    z = fit.prepare(C.LABELS, [0] * 6, C.SIG_LABELS, ["SigA", "SigB"], [r[:2] for r in C.SIG_ROWS], C.OPP_WEIGHTS)
    rz = fit.summarise(z, [[0.0, 0.0], [0.0, 0.0]])
    assert rz["fraction"] == [0.0, 0.0] and rz["exposure_genome"] == [0.0, 0.0] and rz["cosine"] == 0.0
    assert rz["boot"]["presence"] == [0.0, 0.0]


def test_subparser_and_no_cpu_fallback(monkeypatch):
    from himut_amd import _ffi
    from himut_amd.parse_args import parse_args
    _parser, o = parse_args("x", ["fit", "-i", "s.tsv", "--signatures", "sig.tsv", "-o", "e.tsv"])
    assert (o.sub, o.bootstrap, o.seed, o.iters, o.min_fraction, o.device) == ("fit", 1000, 1, 1000, 0.05, 0)
    assert o.select is None and o.opp is None and o.recon is None and o.boot is None
    _parser, o = parse_args("x", ["fit", "-i", "s.tsv", "--signatures", "sig.tsv", "-o", "e.tsv", "--select", "SBS1,SBS5", "--opp",
                                  "normcounts", "--bootstrap", "0", "--seed", "9", "--iters", "7", "--min_fraction", "0.1",
                                  "--recon", "r.tsv", "--boot", "b.tsv", "--device", "2"])
    assert (o.select, o.opp, o.bootstrap, o.seed, o.iters, o.min_fraction, o.recon, o.boot, o.device) == \
        ("SBS1,SBS5", "normcounts", 0, 9, 7, 0.1, "r.tsv", "b.tsv", 2)

    def no_lib():
        raise ImportError("libhimut_hip.so is not there")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    with pytest.raises(ImportError):
        fit.dump_exposures("s.tsv", "sig.tsv", "e.tsv")
