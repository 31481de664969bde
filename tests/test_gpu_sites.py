"""The sites run (himut_run_sites / himut_get_sites) through the C ABI against the plain-Python model of its contract
(tests/sites_model.py): equal record bytes and equal counters.  The hand-built alignments of tests/sites_cases.py pin
the rules and the shapes at which the kernels can go wrong; a synthetic sample pins the run at size and against the call
run of the same context; randomised rounds vary everything at once; sequences on one context pin the state the runs
leave each other; then errors and the command line."""
import os
import random

import numpy as np
import pytest

from tests import dbs_cases as C
from tests import sites_cases as S
from tests import sites_model as M
from tests.test_sites_cpu import CASES, assert_twins, call_params, read_substitutions, sample_model

pytestmark = pytest.mark.gpu

PARAM_NAMES = ("min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq", "min_bq", "max_mismatch_count",
               "mismatch_window_size", "md_threshold", "min_ref_count", "min_alt_count", "min_hap_count", "min_sequence_identity",
               "min_trim")


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


def _arrays(sites):
    return (np.array([s[0] for s in sites], np.int32), "".join(s[1] for s in sites).encode(), "".join(s[2] for s in sites).encode())


def _sites(c, batch, sites, kw, push=True, prior=1 / (10 ** 3)):
    _configure(c, kw, prior)
    if push:
        c.push_reads(batch)
    c.run_sites(*_arrays(sites))
    return c.sites()


def _both(c, batch, sites, kw, prior=1 / (10 ** 3), push=True):
    got, glog = _sites(c, batch, sites, kw, push=push, prior=prior)
    want, wlog = M.run(batch, sites, prior=prior, **kw)
    M.assert_same(got, glog, want, wlog)
    return got, glog


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(ctx, case):
    """Every rule of the contract and every shape: the run's bytes are the model's, and say what the rule says."""
    _name, b, sites, kw, expect = case
    recs, log = _both(ctx, b, sites, kw)
    if expect:
        expect(recs, log)


def test_synthetic_sample(ctx):
    """The 200 kb sample (eleven thousand sites: forty-odd workgroups of the evaluation) equals the model, twice with the
    same bytes; with the mismatch window open, himut_run on one chunk (0, length) on the same context gives the twin of
    every site record it has a record for, and leaves the site records alone."""
    b, sites, kw, want, wlog = sample_model()
    got, glog = _sites(ctx, b, sites, kw)
    M.assert_same(got, glog, want, wlog)
    again, alog = _sites(ctx, b, sites, kw, push=False)
    assert again.tobytes() == got.tobytes() and alog == glog
    st = ctx.stats()
    assert st["n_records"] == st["n_candidates"] == len(sites) and st["ms_total"] > 0 and st["reran"] == 0
    assert st["n_reads"] == b.n and st["column_slots"] > 0
    _configure(ctx, call_params(kw) | {k: kw[k] for k in ("pon_keys", "com_keys")})
    ctx.set_chunks([(0, b.length)])
    ctx.run()
    crecs = ctx.records()
    from tests import dbs_model as D
    n_germ = assert_twins(sites, got, crecs, read_substitutions(b, dict(D.DEFAULTS, **call_params(kw))))
    assert len(crecs) >= 1000 and n_germ >= 20
    served, slog = ctx.sites()                             # the call run left the site records alone
    assert served.tobytes() == got.tobytes() and slog == glog


def _small(seed, length, depth):
    from tests.test_gpu_germline import _sample
    return _sample(seed, length, depth=depth, read_len_mean=500, read_len_sd=200, read_len_min=60, read_len_max=1500,
                   snp_rate=5e-3, hetalt_frac=0.2, sub_rate=5e-3, ins_rate=2e-3, del_rate=2e-3).batch


def _random_sites(rs, b, n):
    """n sites at random positions up to 700 behind the contig, a third of them at a position a read substitutes, some
    repeated; sorted by position, the alleles of one position in random order."""
    real = sorted(read_substitutions(b))
    out = []
    for _ in range(n):
        if real and rs.random() < 0.35:
            s = rs.choice(real)
            out.append(s if rs.random() < 0.7 else (s[0], s[1], rs.choice([x for x in "ATGC" if x != s[1]])))
        else:
            r = rs.choice("ATGC")
            out.append((rs.randrange(1, b.length + 700), r, rs.choice([x for x in "ATGC" if x != r])))
        if rs.random() < 0.05:
            out.append(out[-1])
    rs.shuffle(out)
    return sorted(out, key=lambda s: s[0])


def test_randomised_rounds(ctx):
    """Thirty small contigs of varying length and depth with random site lists and thresholds, on one context."""
    rs = random.Random(23)
    for k in range(30):
        b = _small(300 + k, rs.choice((900, 2500, 6000)), rs.choice((2.0, 9.0, 40.0)))
        sites = _random_sites(rs, b, rs.choice((1, 40, 300, 700)))
        kw = dict(C.OPEN, min_mapq=rs.choice((0, 20, 60)), min_bq=rs.choice((1, 30, 93)), min_gq=rs.choice((0, 20, 60)),
                  md_threshold=rs.choice((5, 30, 1 << 30)), min_ref_count=rs.choice((0, 3)), min_alt_count=rs.choice((1, 2)))
        keys = sorted({(s[0] << 4) | ("ATGC".index(s[1]) << 2) | "ATGC".index(s[2]) for s in sites})
        kw = dict(kw, pon_keys=keys[0::5], com_keys=keys[2::5])
        _both(ctx, b, sites, kw, prior=rs.choice((1e-3, 1e-2)))


def test_sequences_on_one_context():
    """call -> sites -> call returns the first call's records and log; sites -> germline -> sites and dbs -> sites -> dbs
    serve each run's own records; a small site list, then a large one that overflows the column store the small one left
    (reran), then the small one again."""
    from himut_amd import _ffi
    from tests import dbs_model as D
    from tests import germline_model as G
    b, sites, kw, want, wlog = sample_model()
    few = sites[::400]
    fwant, flog = M.run(b, few, **kw)
    ckw = call_params(kw) | {k: kw[k] for k in ("pon_keys", "com_keys")}
    with _ffi.Context(0) as c:
        _configure(c, ckw)
        c.set_chunks([(0, b.length)])
        c.push_reads(b)
        c.run()
        crecs, clog = c.records(), c.log()
        assert len(crecs) > 1000
        got, glog = _sites(c, b, few, kw, push=False)
        M.assert_same(got, glog, fwant, flog)
        assert c.stats()["reran"] == 0
        assert c.records().tobytes() == crecs.tobytes() and c.log() == clog          # the getter serves the call run
        _configure(c, ckw)
        c.run()                                                                      # the chunks are as the call run left them
        assert c.records().tobytes() == crecs.tobytes() and c.log() == clog
        # small -> large: the large list needs more column slots than the small one left room for
        got, glog = _sites(c, b, sites, kw, push=False)
        M.assert_same(got, glog, want, wlog)
        assert c.stats()["reran"] == 1
        got, glog = _sites(c, b, sites, kw, push=False)
        M.assert_same(got, glog, want, wlog)
        assert c.stats()["reran"] == 0
        got, glog = _sites(c, b, few, kw, push=False)
        M.assert_same(got, glog, fwant, flog)
        assert c.stats()["reran"] == 0
        # sites -> germline -> sites
        c.run_germline()
        grecs, gl = c.germline()
        G.assert_same(grecs, gl, *G.run(b, [(0, b.length)]))
        served, slog = c.sites()
        assert served.tobytes() == fwant.tobytes() and slog == flog
        got, glog = _sites(c, b, few, kw, push=False)
        M.assert_same(got, glog, fwant, flog)
        assert c.germline()[0].tobytes() == grecs.tobytes()
        # dbs -> sites -> dbs
        dkw = dict(C.OPEN, min_bq=30, max_mismatch_count=3)
        _configure(c, dkw)
        c.set_chunks([(1, b.length)])
        c.run_dbs()
        drecs, dlog = c.dbs()
        D.assert_same(drecs, dlog, *D.run(b, [(1, b.length)], **dkw))
        got, glog = _sites(c, b, few, kw, push=False)
        M.assert_same(got, glog, fwant, flog)
        assert c.dbs()[0].tobytes() == drecs.tobytes()
        _configure(c, dkw)
        c.run_dbs()
        again, alog = c.dbs()
        assert again.tobytes() == drecs.tobytes() and alog == dlog
        served, slog = c.sites()
        assert served.tobytes() == fwant.tobytes() and slog == flog


def test_argument_errors():
    from himut_amd import _ffi, gtlib
    p = 500
    b = C.batch(S.stack(p, 12, {0: {p: C.A1[p]}}))
    good = [S.site(p), S.site(p + 3)]
    prm = dict(M.DEFAULTS, **S.KW)
    with _ffi.Context(0) as c:
        for step in (lambda: c.set_params(**{k: prm[k] for k in PARAM_NAMES}), lambda: c.set_gt_lut(*gtlib.build_tables(1e-3)),
                     lambda: c.push_reads(b)):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_sites(*_arrays(good))
            assert e.value.code == 1
            step()
        c.run_sites(*_arrays(good))            # no chunks, the site sets never set: allowed
        recs, log = c.sites()
        M.assert_same(recs, log, *M.run(b, good, **S.KW))
        ref, alt = C.REF[p], C.A1[p]
        for bad in ([S.site(p + 3), S.site(p)],                                   # unsorted
                    [(p + 1, ref, ref)], [(p + 1, ref.lower(), alt)], [(p + 1, ref, alt.lower())], [(p + 1, "N", alt)],
                    [(0, ref, alt)], [(-5, ref, alt)]):
            with pytest.raises(_ffi.HimutError) as e:
                c.run_sites(*_arrays(bad))
            assert e.value.code == 1, bad
        # n_sites == 0: a run with zero records; phase = 1 without phase sets: ignored
        c.run_sites(np.zeros(0, np.int32), b"", b"")
        recs, log = c.sites()
        assert len(recs) == 0 and log == [0] * 20 and c.stats()["n_records"] == 0
        c.set_params(**dict({k: prm[k] for k in PARAM_NAMES}, phase=1))
        c.run_sites(*_arrays(good))
        M.assert_same(*c.sites(), *M.run(b, good, **S.KW))
        # a batch without reads: every site NoCoverage
        from himut_amd.readbatch import batch_from_records
        c.push_reads(batch_from_records("chrD", C.N, []))
        c.run_sites(*_arrays(good))
        recs, log = c.sites()
        M.assert_same(recs, log, *M.run(batch_from_records("chrD", C.N, []), good, **S.KW))
        assert S.statuses(recs) == ["NoCoverage"] * 2 and log[15] == 0


def test_errors_then_a_good_contig(ctx):
    """Quality 0 in an A/T/G/C cell of a site's column: HIMUT_ERR_BQ0; a query N in a cell of a site's column:
    HIMUT_ERR_BASE; either one position beside the site is no error (the capture's region-based check has no regions);
    the same context runs a good contig right afterwards.  (Inputs the library rejects cleanly.)"""
    from himut_amd._ffi import HimutError
    p = 500
    good = S.stack(p, 12, {0: {p: C.A1[p]}})
    gb = C.batch(good)
    sites = [S.site(p), S.site(p, C.A2)]
    want, wlog = M.run(gb, sites, **S.KW)
    for what, code in (("bq0", M.ERR_BQ0), ("bq0_beside", 0), ("n", M.ERR_BASE), ("n_beside", 0)):
        reads = [dict(r) for r in good]
        pos = p if what in ("bq0", "n") else p + 1
        k = pos - reads[5]["tstart"]
        if what.startswith("bq0"):
            reads[5]["bq"] = list(reads[5]["bq"]); reads[5]["bq"][k] = 0
        else:
            s = reads[5]["seq"]
            reads[5]["seq"] = s[:k] + "N" + s[k + 1:]
        b = C.batch(reads)
        if code:
            with pytest.raises(HimutError) as e:
                _sites(ctx, b, sites, S.KW)
            assert e.value.code == code
            with pytest.raises(M.ModelError) as me:
                M.run(b, sites, **S.KW)
            assert me.value.code == code
        else:
            _both(ctx, b, sites, S.KW)
        got, glog = _sites(ctx, gb, sites, S.KW)
        M.assert_same(got, glog, want, wlog)


def _write_vcf(path, chrom2lines, contigs):
    with open(path, "w") as o:
        o.write("##fileformat=VCFv4.2\n")
        for c, n in contigs:
            o.write("##contig=<ID={},length={}>\n".format(c, n))
        o.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSMP\n")
        for c, _n in contigs:
            for pos, ref, alt, flt in chrom2lines.get(c, []):
                o.write("{}\t{}\t.\t{}\t{}\t.\t{}\t.\tGT\t./.\n".format(c, pos, ref, alt, flt))


def test_cli_sites(tmp_path, capsys):
    """`sites` on a two-contig BAM written by the package's own writer: the model's TSV and log, --unseen against the
    model, --devices 0,0 and --cs_from_ref give the same files."""
    from himut_amd import __main__ as cli
    from himut_amd import bamio, bamlib, sites as sites_mod, support, synth, util as hutil
    from tests import cs_from_cigar
    cfg = dict(depth=20.0, read_len_mean=6000, read_len_sd=1200, read_len_min=2000, read_len_max=12000, snp_rate=1e-3,
               hetalt_frac=0.1, sub_rate=1e-3)
    s1 = synth.generate(synth.SynthConfig(seed=95, contig_len=60_000, name="chr2", **cfg), want_ref=True)
    s2 = synth.generate(synth.SynthConfig(seed=96, contig_len=40_000, name="chr10", **cfg), want_ref=True)
    batches = {"chr2": s1.batch, "chr10": s2.batch}
    sizes = {"chr10": 40_000, "chr2": 60_000}
    bam, bare, fa = str(tmp_path / "in.bam"), str(tmp_path / "bare.bam"), str(tmp_path / "g.fa")
    bamio.write_bam(bam, [s2.batch, s1.batch], sample="SMP")
    from tests import bam_spec                # the same two contigs without cs tags, CIGARs from the cs texts
    bam_spec.write_bgzf(bare, bam_spec.header([("chr10", 40_000), ("chr2", 60_000)], "SMP") +
                        b"".join(cs_from_cigar.batch_records(s2.batch, "M", ref_id=0) + cs_from_cigar.batch_records(s1.batch, "M", ref_id=1)))
    with open(fa, "w") as o:
        for s, name in ((s2, "chr10"), (s1, "chr2")):
            text = bytes(s.ref).decode()
            o.write(">{}\n".format(name) + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    # the "other sample's calls": what this sample's reads carry (seen here), random triples (mostly unseen here), a
    # HetAlt line, non-PASS lines, an indel line and a contig the BAM lacks
    rs = random.Random(8)
    lines = {}
    for c, b in batches.items():
        real = sorted(read_substitutions(b))[::3]
        at = {s[0] for s in real}
        rows = [(p, r, a, "PASS" if k % 4 else "LowBQ") for k, (p, r, a) in enumerate(real)]
        while len(rows) < 2 * len(real):
            p = rs.randrange(1, b.length + 1)
            if p not in at:
                at.add(p)
                r = rs.choice("ATGC")
                two = [x for x in "ATGC" if x != r]
                rows.append((p, r, rs.choice(two) if rs.random() < 0.9 else ",".join(rs.sample(two, 2)), "PASS"))
        rows.append((77, "AC", "A", "PASS"))
        lines[c] = sorted(rows)
    lines["chrZ"] = [(5, "A", "C", "PASS")]
    vcf = str(tmp_path / "calls.vcf")
    _write_vcf(vcf, lines, [("chr10", 40_000), ("chr2", 60_000), ("chrZ", 100)])

    chrom_lst, _c2c = hutil.load_loci(None, None, sizes)
    _ql, _qu, md = bamlib.get_thresholds(batches, chrom_lst, sizes)
    flags = ["--min_mapq", "20", "--min_bq", "30"]
    kw = dict(C.OPEN, min_mapq=20, min_bq=30, md_threshold=md, min_gq=20, min_ref_count=3, min_alt_count=1)
    for all_filters in (False, True):
        c2s, _skipped = support.load_sites(vcf, all_filters)
        body, logs, unseen = [], {}, {}
        for c in chrom_lst:
            recs, logs[c] = M.run(batches[c], [s[:3] for s in c2s[c]], **kw)
            body += sites_mod.format_rows(c, c2s[c], recs)
            unseen[c] = {s[:3] for s, r in zip(c2s[c], recs) if int(r["counts"]["ATGC".index(s[2])]) == 0 and M.depth_of(r) >= 12}
        assert len(body) > 200 and any(len(u) > 20 for u in unseen.values())
        runs = [("one", bam, ["--devices", "0"]), ("two", bam, ["--devices", "0,0"])]
        if not all_filters:
            runs.append(("bare", bare, ["--ref", fa, "--cs_from_ref"]))
        out, cwd = {}, os.getcwd()
        for name, path, extra in runs:
            d = tmp_path / (name + str(int(all_filters)))
            d.mkdir()
            os.chdir(d)
            try:
                cli.main(["sites", "-i", path, "--sbs", vcf, "-o", str(d / "s.tsv"), "--unseen", str(d / "u.vcf"), "--min_depth", "12"]
                         + flags + extra + (["--all_filters"] if all_filters else []))
            finally:
                os.chdir(cwd)
            printed = capsys.readouterr().out
            assert "contig chrZ" in printed and "1 lines of" in printed
            tsv = open(d / "s.tsv").read().splitlines()
            assert tsv[0].split("\t") == list(sites_mod.COLUMNS) and tsv[1:] == body
            rows = [l.split() for l in open(d / "himut_sites.log")]
            assert rows[0] == chrom_lst + ["total"] and [r[0] for r in rows[1:]] == M.LOG_ROWS
            assert [[int(x) for x in r[1:3]] for r in rows[1:]] == [[logs[c][k] for c in chrom_lst] for k in range(20)]
            u = open(d / "u.vcf").read().splitlines()
            head = [l for l in u if l.startswith("#")]
            assert head[:-2] == open(vcf).read().splitlines()[:len(head) - 2] and head[-1].startswith("#CHROM")
            assert head[-2].startswith("##himut_sites_command=himut sites -i {} --sbs {} ".format(path, vcf))
            kept = [l.split("\t") for l in u if not l.startswith("#")]
            want = [(c, pos, ref, alt) for c in ("chr10", "chr2") for pos, ref, alt, flt in lines[c]
                    if (all_filters or flt == "PASS") and len(ref) == 1
                    and all((pos, ref, a) in unseen[c] for a in alt.split(","))]
            assert [(f[0], int(f[1]), f[3], f[4]) for f in kept] == want and len(want) > 20
            out[name] = (tsv, [l for l in u if not l.startswith("##himut_sites_command")])
        assert out["one"] == out["two"]
        if "bare" in out:
            assert out["bare"] == out["one"]


def test_gt_rounding_boundaries(ctx):
    """The genotype and the min_gq cut at fp64 rounding boundaries: the 400 leaf columns in one contig and every boundary
    vector of gt_edges.json in a pile of its own, as site columns -- the run's bytes are the model's and carry the
    fixture's gt, gq and state."""
    from tests.test_callmap_cpu import LEAF_K, edge_vectors
    from tests.test_sites_cpu import check_vectors, edge_site_model, leaf_site_model
    vs, P, kw, prior, sites, want, wlog = leaf_site_model()
    got, glog = _sites(ctx, P.batch, sites, kw, prior=prior)
    M.assert_same(got, glog, want, wlog)
    check_vectors(got, vs, LEAF_K)
    for i in range(len(edge_vectors())):
        v, P, kw, prior, sites, want, wlog = edge_site_model(i)
        got, glog = _sites(ctx, P.batch, sites, kw, prior=prior)
        M.assert_same(got, glog, want, wlog)
        check_vectors(got, [v], None)
