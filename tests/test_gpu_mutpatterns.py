"""`tricount`, `sbs96`, `sbs1536` and `burden` on the device: himut_fasta_tricounts (k_fasta_tricounts) against the
reference's files and the host mirror over FASTA layouts and staging windows, himut_sbs1536_counts (k_sbs<2>) against
the host mirror and the reference, and the four subcommands as child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from himut_amd import mutlib, normcounts as N, reflib
from tests.test_mutpatterns_cpu import _raises, _write, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden()
WS = b"\n\r\t "
WSB = np.frombuffer(WS, np.uint8)


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.close()


def _bins(d):
    return [d[t] for t in N.TRI_LST]


def _host(body):
    return _bins(N.get_chrom_tricount(bytes(body).translate(None, WS)))


@pytest.mark.parametrize("case", G["tricount"], ids=[c["name"] for c in G["tricount"]])
def test_tricount_device_golden(case, tmp_path):
    fa = _write(tmp_path / "g.fa", case["fasta"])
    rl = _write(tmp_path / "r.list", case["region_list"]) if "region_list" in case else None
    out = str(tmp_path / "o.tsv")
    if case["raises"]:
        with pytest.raises(_raises(case["raises"])):
            reflib.get_ref_tricount(fa, case.get("region"), rl, 1, out)
    else:
        reflib.get_ref_tricount(fa, case.get("region"), rl, 1, out)
    assert (open(out).read() if os.path.exists(out) else None) == case["tsv"]


def _random_layout(rs, n):
    """A record body of about n letters: mixed case, N runs, IUPAC letters, random line widths and whitespace runs of
    every kind, some longer than a tile (4096 bytes)."""
    letters = np.frombuffer(b"ACGTACGTACGTACGTacgtNNRY", np.uint8)
    seq = letters[rs.randint(0, letters.shape[0], n)]
    out, i = [], 0
    while i < n:
        w = int(rs.choice([1, 2, 3, 60, 61, rs.randint(1, 200)]))
        out.append(seq[i:i + w].tobytes())
        i += w
        r = rs.rand()
        if r < 0.01:
            out.append(WSB[rs.randint(0, 4, rs.randint(4097, 9000))].tobytes())
        elif r < 0.2:
            out.append(WSB[rs.randint(0, 4, rs.randint(1, 8))].tobytes())
        else:
            out.append(b"\r\n" if r < 0.3 else b"\n")
    return b"".join(out)


@pytest.mark.parametrize("window", [0, 1, 2, 3, 17, 4096])
def test_fasta_tricounts_windows_against_host(worker, window):
    rs = np.random.RandomState(11 + window)
    ctx = worker.ctx
    ctx.debug_fasta_window(window)
    try:
        sizes = [0, 1, 2, 3, 5, 4095, 4096, 4097] if window in (1, 2, 3) else [0, 1, 2, 3, 4097, 20_000, 150_000]
        for n in sizes:
            body = _random_layout(rs, n)
            assert _bins(reflib.tricount_dict(ctx.fasta_tricounts(body))) == _host(body), n
        # hand-made: a base and its two followers split by whitespace runs around every window end
        body = b"AC\n\n\r\nG" + b" " * 5000 + b"T\tC" + b"\r\n" * 3000 + b"AGT"
        assert _bins(reflib.tricount_dict(ctx.fasta_tricounts(body))) == _host(body)
        assert sum(_host(body)) == 6
    finally:
        ctx.debug_fasta_window(0)


def test_fasta_tricounts_large_record(worker, tmp_path):
    """One 300 Mb record, more than four default staging windows, mapped from a file; the host count goes chunk by
    chunk (triplets starting in each chunk)."""
    rs = np.random.RandomState(3)
    rows = 5_000_000
    letters = np.frombuffer(b"ACGTACGTACGTACGTACGTacgtN", np.uint8)
    seq = letters[rs.randint(0, letters.shape[0], rows * 60, dtype=np.uint8)]
    seq[1000:5000] = ord("N")
    lines = np.concatenate([seq.reshape(rows, 60), np.full((rows, 1), ord("\n"), np.uint8)], axis=1)
    fa = tmp_path / "big.fa"
    with open(fa, "wb") as o:
        o.write(b">big\n")
        o.write(lines.tobytes())
    del lines
    got = reflib.get_genome_tricounts_device(str(fa), ["big"])
    want = {t: 0 for t in N.TRI_LST}
    C = 20_000_000
    raw = seq.tobytes()
    for i in range(0, len(raw), C):
        for t, c in N.get_chrom_tricount(raw[i:i + C + 2]).items():
            want[t] += c
    assert got == want and sum(got.values()) > 100_000_000


def test_ref_tricounts_same_kernel_on_resident_string(worker):
    rs = np.random.RandomState(8)
    body = _random_layout(rs, 300_000)
    seq = body.translate(None, WS).decode("latin-1")
    chars, cls = N.tri_classes(seq)
    worker.ctx.set_reference(seq, cls, len(chars))
    res = worker.ctx.ref_tricounts()
    assert list(res) == list(worker.ctx.fasta_tricounts(body))
    assert _bins(reflib.tricount_dict(res)) == _host(body)


def test_fasta_tricounts_refused_while_ingest_open(worker):
    from himut_amd.caller import Worker
    other = Worker(0)
    try:
        other.ctx.ingest_begin(0, 1 << 16)
        with pytest.raises(Exception):
            worker.ctx.fasta_tricounts(b"ACGT\n")
        other.ctx.ingest_end(True)
        assert sum(worker.ctx.fasta_tricounts(b"ACGT\n")) == 2
    finally:
        other.close()


def test_fasta_tricounts_refused_while_own_ingest_open():
    """A context whose own ingest is open is refused the count, and its ingest keeps the windows."""
    from himut_amd.caller import Worker
    a, b = Worker(0), Worker(0)
    try:
        a.ctx.ingest_begin(0, 1 << 16)
        with pytest.raises(Exception):
            a.ctx.fasta_tricounts(b"ACGT\n")
        with pytest.raises(Exception):
            b.ctx.ingest_begin(0, 1 << 16)
        a.ctx.ingest_end(True)
        assert sum(a.ctx.fasta_tricounts(b"ACGT\n")) == 2
    finally:
        a.close()
        b.close()


def test_sbs1536_counts_against_host_mirror(worker):
    rs = np.random.RandomState(6)
    seq = "".join(rs.choice(list("ACGT"), 3000))
    seq = seq[:400] + "N" * 5 + seq[405:800] + seq[800:860].lower() + seq[860:1000] + "RY" + seq[1002:]
    ref = {"c": seq}
    pos, rr, aa = [], [], []
    want = {k: 0 for k in mutlib.SBS1536_LST}
    n_drop = n_key = 0
    for p in range(0, len(seq) - 2):
        r = seq[p]
        if r not in "ACGT":
            continue
        for a in "ACGT":
            if a == r:
                continue
            k = mutlib.get_sbs1536("c", p, r, a, ref)
            pos.append(p); rr.append(ord(r)); aa.append(ord(a))
            if "N" in k:
                n_drop += 1
            elif k in want:
                want[k] += 1
            else:
                n_key += 1
    chars, cls = N.tri_classes(seq)
    worker.ctx.set_reference(seq, cls, len(chars))
    h = worker.ctx.sbs1536_counts(pos, rr, aa)
    dev = {k: int(h[i]) for i, k in enumerate(mutlib.SBS1536_LST)}
    assert dev == want and int(h[1536]) == n_drop and int(h[1537]) == n_key and n_drop > 0 and n_key > 0
    assert int(h[1538]) == 0
    for p in (len(seq) - 2, len(seq) - 1):                     # IndexError in the reference
        assert int(worker.ctx.sbs1536_counts([p], [ord("C")], [ord("T")])[1538]) == 1
    # positions 0 and 1 read the end of the string
    for p in (0, 1):
        r = seq[p]
        a = "A" if r != "A" else "C"
        k = mutlib.get_sbs1536("c", p, r, a, ref)
        h = worker.ctx.sbs1536_counts([p], [ord(r)], [ord(a)])
        assert (int(h[mutlib.SBS1536_LST.index(k)]) if k in want else int(h[1536] + h[1537])) == 1
    # sbs96 through the same template agrees with its host mirror at the wrapped position
    k96 = N.get_sbs96("c", 0, seq[0], "A" if seq[0] != "A" else "C", ref)
    h96 = worker.ctx.sbs96_counts([0], [ord(seq[0])], [ord("A" if seq[0] != "A" else "C")])
    assert int(h96[N.SUB_LST.index(k96[2:5]) * 16 + "ACGT".index(k96[0]) * 4 + "ACGT".index(k96[6])]) == 1


@pytest.mark.parametrize("case", G["sbs"], ids=[c["name"] for c in G["sbs"]])
def test_sbs_device_golden(case, tmp_path, worker):
    fa = _write(tmp_path / "g.fa", case["fasta"])
    vcf = _write(tmp_path / "s.vcf", case["vcf"])
    rl = _write(tmp_path / "r.list", case["region_list"]) if case["region_list"] is not None else None
    _, tname2tsize = mutlib.get_sample(vcf)
    for kind, dump in (("sbs96", mutlib.dump_sbs96_counts), ("sbs1536", mutlib.dump_sbs1536_counts)):
        out = str(tmp_path / (kind + ".tsv"))
        if case[kind + "_raises"]:
            with pytest.raises(_raises(case[kind + "_raises"])):
                dump(vcf, fa, case["region"], rl, tname2tsize, out)
        else:
            dump(vcf, fa, case["region"], rl, tname2tsize, out)
        assert (open(out).read() if os.path.exists(out) else None) == case[kind + "_tsv"], kind


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "himut_amd"] + args, cwd=str(cwd), env=env, capture_output=True,
                          text=True, timeout=300)


def test_cli_subcommands_match_golden(tmp_path):
    tri = {c["name"]: c for c in G["tricount"]}
    for name in ("unselected_between", "crlf_blank", "region_and_list"):
        c = tri[name]
        fa = _write(tmp_path / (name + ".fa"), c["fasta"])
        args = ["tricount", "-i", fa, "-o", str(tmp_path / (name + ".tri"))]
        if "region" in c:
            args += ["--region", c["region"]]
        if "region_list" in c:
            args += ["--region_list", _write(tmp_path / (name + ".list"), c["region_list"])]
        r = _cli(args, tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(tmp_path / (name + ".tri")).read() == c["tsv"], name
    r = _cli(["tricount", "-i", fa, "-o", str(tmp_path / "none.tri")], tmp_path)
    assert r.returncode == 0 and "Please provide --region or --region_list" in r.stdout
    sbs = {c["name"]: c for c in G["sbs"]}
    for name in ("dense", "dense_list", "sparse"):
        c = sbs[name]
        fa = _write(tmp_path / (name + ".s.fa"), c["fasta"])
        vcf = _write(tmp_path / (name + ".vcf"), c["vcf"])
        for kind in ("sbs96", "sbs1536"):
            out = tmp_path / "{}.{}.tsv".format(name, kind)
            args = [kind, "-i", vcf, "--ref", fa, "-o", str(out)]
            if c["region_list"] is not None:
                args += ["--region_list", _write(tmp_path / (name + ".slist"), c["region_list"])]
            r = _cli(args, tmp_path)
            assert (r.returncode == 0) == (c[kind + "_raises"] is None), r.stderr[-2000:]
            if c[kind + "_raises"]:
                assert c[kind + "_raises"] in r.stderr
            assert open(out).read() == c[kind + "_tsv"], (name, kind)
    for c in G["burden"][:2]:
        args = ["burden", "-i", _write(tmp_path / "n.tsv", c["table"]), "--region_list",
                _write(tmp_path / "b.list", c["region_list"]), "-o", str(tmp_path / (c["name"] + ".burden"))]
        if c["tri"] is not None:
            args += ["--tri", _write(tmp_path / "t.tsv", c["tri"])]
        if c["fasta"] is not None:
            args += ["--ref", _write(tmp_path / "b.fa", c["fasta"])]
        r = _cli(args, tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(tmp_path / (c["name"] + ".burden")).read() == c["out"]
