"""`himut id83` and `himut dbs78` on the device: himut_id83_classify (k_id83) and
himut_dbs78_counts (k_dbs78) against the plain model of tests/spectra_model.py -- the hand-built cases, a string of planted
repeats with every short deletion at every position, list sizes around the workgroup and a strided grid, the bad arguments
-- and the two subcommands as child processes on the hand-written VCF and FASTA."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from himut_amd import normcounts as N, spectra
from tests import spectra_cases as C, spectra_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _set_reference(ctx, seq):
    chars, cls = N.tri_classes(seq)
    ctx.set_reference(seq, cls, len(chars))


def _arrays(alleles):
    """(anchor, type, len, bases) of a list of (a, kind, L, ins)."""
    n = len(alleles)
    bases = np.zeros((n, 16), np.uint8)
    for i, (_a, kind, _L, ins) in enumerate(alleles):
        if kind == "ins":
            bases[i] = spectra.pack_bases(ins)
    return (np.array([al[0] for al in alleles], np.int32), np.array([al[1] == "ins" for al in alleles], np.uint8),
            np.array([al[2] for al in alleles], np.int32), bases)


def _want_cls(labels):
    return [255 if k in (M.NBASE, M.RANGE) else M.ID83_LABELS.index(k) for k in labels]


def test_cases_classes_and_bins(worker):
    by_seq = {}
    for name, seq, a, kind, L, ins, label in C.CASES:
        by_seq.setdefault(seq, []).append((name, (a, kind, L, ins), label))
    total = np.zeros(88, np.int64)
    for seq, group in by_seq.items():
        _set_reference(worker.ctx, seq)
        alleles = [g[1] for g in group]
        cls, bins = worker.ctx.id83_classify(*_arrays(alleles))
        want = _want_cls([g[2] for g in group])
        assert [int(x) for x in cls] == want, [(g[0], int(c), w) for g, c, w in zip(group, cls, want) if int(c) != w]
        assert [int(x) for x in bins] == M.id83_bins(seq, alleles)[1], seq
        total += bins
    assert np.all(total[:85] > 0) and not total[85:].any()          # every class and both counters, nothing in the reserved words


def _planted_string(rs, n=4000):
    """About ``n`` letters: random stretches, homopolymers and tandem repeats (unit 1-6, 1-8 copies), lower-case islands, a few N."""
    parts, size = [], 0
    while size < n:
        k = rs.rand()
        if k < 0.35:
            p = "".join(rs.choice(list("ACGT"), rs.randint(1, 25)))
        elif k < 0.9:
            p = "".join(rs.choice(list("ACGT"), rs.randint(1, 7))) * rs.randint(1, 9)
        elif k < 0.93:
            p = "N" * rs.randint(1, 3)
        else:
            p = "".join(rs.choice(list("acgt"), rs.randint(1, 7))) * rs.randint(1, 6)
        parts.append(p)
        size += len(p)
    return "".join(parts)[:n]


@pytest.fixture(scope="module")
def planted():
    """(string, alleles, the model's labels and bins): every deletion of length 1-6 at every anchor from -1 to the end, and
    about 3,000 insertions of length 1-8 and 63-64, most of them copies of what follows the anchor, rotated at random."""
    rs = np.random.RandomState(83)
    seq = _planted_string(rs)
    alleles = [(a, "del", L, "") for a in range(-1, len(seq)) for L in range(1, 7)]
    for _ in range(3000):
        a = int(rs.randint(-1, len(seq) + 1))
        L = int(rs.choice([1, 1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 63, 64]))
        ins = seq[a + 1:a + 1 + L].upper() if 0 <= a and rs.rand() < 0.7 else ""
        if len(ins) < L or any(ch not in "ACGT" for ch in ins):
            ins = "".join(rs.choice(list("ACGT"), L))
        s = int(rs.randint(0, L))
        alleles.append((a, "ins", L, ins[s:] + ins[:s]))
    labels, bins = M.id83_bins(seq, alleles)
    return seq, alleles, labels, bins


def test_planted_string_every_deletion_and_random_insertions(worker, planted):
    seq, alleles, labels, bins = planted
    _set_reference(worker.ctx, seq)
    cls, got = worker.ctx.id83_classify(*_arrays(alleles))
    want = _want_cls(labels)
    wrong = [(al, int(c), w) for al, c, w in zip(alleles, cls, want) if int(c) != w]
    assert not wrong, wrong[:10]
    assert [int(x) for x in got] == bins
    assert sum(1 for b in bins[:83] if b) >= 70 and bins[83] > 0 and bins[84] > 0       # the list reaches most classes


@pytest.mark.parametrize("n,max_wgs", [(0, 0), (1, 0), (255, 0), (256, 0), (257, 0), (1500, 2), (1500, 1)])
def test_list_sizes_and_strided_grid(worker, planted, n, max_wgs):
    seq, alleles, labels, _bins = planted
    rs = np.random.RandomState(n + max_wgs)
    pick = [int(i) for i in rs.choice(len(alleles), n, replace=False)]
    sub = [alleles[i] for i in pick]
    _set_reference(worker.ctx, seq)
    worker.ctx.debug_spectra(max_wgs)
    try:
        cls, got = worker.ctx.id83_classify(*_arrays(sub))
        none, got2 = worker.ctx.id83_classify(*_arrays(sub), want_classes=False)       # cls = NULL
    finally:
        worker.ctx.debug_spectra(0)
    assert [int(x) for x in cls] == _want_cls([labels[i] for i in pick])
    assert [int(x) for x in got] == M.id83_bins(seq, sub)[1] and sum(got) == n
    assert none is None and list(got2) == list(got)


def test_bad_arguments_leave_the_context_usable():
    from himut_amd._ffi import Context, HimutError
    with Context(0) as ctx:
        one = (np.zeros(1, np.int32), np.zeros(1, np.uint8), np.ones(1, np.int32))
        with pytest.raises(HimutError) as e:            # no reference yet
            ctx.id83_classify(*one)
        assert e.value.code == 1 and "himut_set_reference" in e.value.message
        seq = "GTAAAAACGT"
        _set_reference(ctx, seq)
        assert int(ctx.id83_classify(*one)[0][0]) == M.ID83_LABELS.index("1:Del:T:0")       # the T at 1 goes
        L, h = ctx._L, ctx._h
        a, t, ln, b = np.zeros(4, np.int32), np.zeros(4, np.uint8), np.ones(4, np.int32), np.zeros((4, 16), np.uint8)
        out = np.zeros(88, np.int64)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        assert L.himut_id83_classify(h, p(a), p(t), p(ln), p(b), -1, None, p(out)) == 1
        assert L.himut_id83_classify(h, p(a), p(t), p(ln), p(b), 4, None, None) == 1
        for hole in range(4):
            args = [p(a), p(t), p(ln), p(b)]
            args[hole] = None
            assert L.himut_id83_classify(h, *args, 4, None, p(out)) == 1, hole
            assert b"himut_id83_classify" in L.himut_last_error(h)
        assert L.himut_id83_classify(h, None, None, None, None, 0, None, p(out)) == 0       # nothing to read with n = 0
        for bad in (0, 65, -3, 1 << 20):
            ln2 = ln.copy()
            ln2[2] = bad
            assert L.himut_id83_classify(h, p(a), p(t), p(ln2), p(b), 4, None, p(out)) == 1, bad
            assert b"length outside 1..64" in L.himut_last_error(h)
        t2 = t.copy()
        t2[3] = 2
        assert L.himut_id83_classify(h, p(a), p(t2), p(ln), p(b), 4, None, p(out)) == 1
        r2 = np.frombuffer(b"ACGT", np.uint8).copy()
        o80 = np.zeros(80, np.int64)
        assert L.himut_dbs78_counts(h, p(r2), p(r2), -1, None, p(o80)) == 1
        assert L.himut_dbs78_counts(h, None, p(r2), 2, None, p(o80)) == 1
        assert L.himut_dbs78_counts(h, p(r2), None, 2, None, p(o80)) == 1
        assert L.himut_dbs78_counts(h, p(r2), p(r2), 2, None, None) == 1
        assert L.himut_debug_spectra(h, -1) == 1
        # the context goes on: the spectra, and an SBS96 count over the same string
        assert int(ctx.id83_classify(*one)[0][0]) == M.ID83_LABELS.index("1:Del:T:0")
        h96 = ctx.sbs96_counts([7], [ord("C")], [ord("T")])          # A[C>T]G
        assert int(h96.sum()) == 1 and int(h96[2 * 16 + 0 * 4 + 2]) == 1


def test_dbs78_on_the_256_ordered_pairs(worker):
    pairs = [a + b for a in "ACGT" for b in "ACGT"]
    ref = [r for r in pairs for _ in pairs] + ["ac", "Gt", "NC", "AC", "AC", "nn", "A-"]
    alt = [a for _ in pairs for a in pairs] + ["gt", "aC", "GT", "GR", "AT", "nn", "CT"]
    labels = [M.dbs78_label(r, a) for r, a in zip(ref, alt)]
    want_cls = [255 if k in (M.NLETTER, M.UNCHANGED) else M.DBS78_LABELS.index(k) for k in labels]
    want = [labels.count(k) for k in M.DBS78_LABELS] + [labels.count(M.NLETTER), labels.count(M.UNCHANGED)]
    r2 = np.frombuffer("".join(ref).encode(), np.uint8).reshape(-1, 2)
    a2 = np.frombuffer("".join(alt).encode(), np.uint8).reshape(-1, 2)
    for max_wgs in (0, 1):
        worker.ctx.debug_spectra(max_wgs)
        try:
            cls, got = worker.ctx.dbs78_counts(r2, a2)
            none, got2 = worker.ctx.dbs78_counts(r2, a2, want_classes=False)
        finally:
            worker.ctx.debug_spectra(0)
        assert [int(x) for x in cls] == want_cls
        assert [int(x) for x in got] == want and none is None and list(got2) == want
    assert sum(want[:78]) == 146 and want[78] == 4 and want[79] == 256 - 144 + 1
    cls, got = worker.ctx.dbs78_counts(np.zeros((0, 2), np.uint8), np.zeros((0, 2), np.uint8))
    assert len(cls) == 0 and not got.any()


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "himut_amd"] + args, cwd=str(cwd), env=env, capture_output=True,
                          text=True, timeout=300)


def _log_text(rows, chroms, cells):
    text = "{:30}{}\n".format("", "\t".join(list(chroms) + ["total"]))
    for k, name in enumerate(rows):
        row = [cells[c][k] for c in chroms]
        text += "{:30}{}\n".format(name, "\t".join(str(x) for x in row + [sum(row)]))
    return text


def _table(name, labels, counts):
    return "{}\tcounts\n".format(name) + "".join("{}\t{}\n".format(k, counts.get(k, 0)) for k in labels)


@pytest.mark.parametrize("all_filters", [False, True])
def test_cli_id83_and_dbs78(tmp_path, all_filters):
    with open(tmp_path / "in.vcf", "w") as o:
        o.write(C.VCF_TEXT)
    with open(tmp_path / "ref.fa", "w") as o:
        o.write(C.FASTA_TEXT)
    flag = ["--all_filters"] if all_filters else []
    r = _cli(["id83", "-i", "in.vcf", "--ref", "ref.fa", "-o", "id83.tsv", "--classes", "classes.tsv"] + flag, tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, lines, log = C.ID83_EXPECT[all_filters]
    assert open(tmp_path / "id83.tsv").read() == _table("id83", M.ID83_LABELS, counts)
    assert open(tmp_path / "classes.tsv").read() == "chrom\tpos\tref\talt\tid83\n" + "".join(x + "\n" for x in lines)
    assert open(tmp_path / "himut_id83.log").read() == _log_text(spectra.ID83_LOG_ROWS, ["c1", "c2"], log)
    assert "contig c3 of in.vcf is not in ref.fa: its 1 alleles are skipped" in r.stdout
    r = _cli(["dbs78", "-i", "in.vcf", "-o", "dbs78.tsv"] + flag, tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, log = C.DBS78_EXPECT[all_filters]
    assert open(tmp_path / "dbs78.tsv").read() == _table("dbs78", M.DBS78_LABELS, counts)
    assert open(tmp_path / "himut_dbs78.log").read() == _log_text(spectra.DBS78_LOG_ROWS, ["c1", "c2", "c3"], log)
    if not all_filters:
        # a region narrows both to one contig
        r = _cli(["id83", "-i", "in.vcf", "--ref", "ref.fa", "-o", "c2.tsv", "--region", "c2"], tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(tmp_path / "c2.tsv").read() == _table("id83", M.ID83_LABELS, {"3:Ins:R:3": 1, "3:Del:R:2": 1})
        assert open(tmp_path / "himut_id83.log").read() == _log_text(spectra.ID83_LOG_ROWS, ["c2"], C.ID83_EXPECT[False][2])
