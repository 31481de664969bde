"""Golden vectors of `himut tricount`, `sbs96`, `sbs1536` and `burden`, captured from the reference's own functions
(reflib.get_ref_tricount, mutlib.dump_sbs96_counts / dump_sbs1536_counts / get_burden_per_cell) through
ref_harness.load_reference_norm_host(), which serves pyfastx.Fasta from FakeFasta.  Writes mutpatterns.json.

Run from the repository root, where the reference checkout exists:  python tests/golden/make_golden_mutpatterns.py
Texts of 256 characters or more are stored once under "blobs" and named "@<sha1[:12]>" where they are used.
Inputs avoid spaces inside sequence lines and empty headers (FakeFasta strips lines; read_fasta deletes those bytes)."""
import gc
import hashlib
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402


def rand_seq(rng, n, lower=0.0, nrun=0.0, iupac=0.0):
    """Seeded sequence with soft-masked stretches, N runs and IUPAC letters."""
    out = []
    while len(out) < n:
        x = rng.random()
        if x < nrun:
            out.extend("N" * rng.randint(1, 12))
        elif x < nrun + lower:
            out.extend(c.lower() for c in rng.choices("ACGT", k=rng.randint(1, 15)))
        elif x < nrun + lower + iupac:
            out.append(rng.choice("RYKMSWBDHV"))
        else:
            out.extend(rng.choices("ACGT", k=rng.randint(1, 30)))
    return "".join(out[:n])


def lines_of(seq, widths):
    """Split seq into lines whose widths cycle through ``widths``."""
    out, i, k = [], 0, 0
    while i < len(seq):
        w = widths[k % len(widths)]
        out.append(seq[i:i + w])
        i += w
        k += 1
    return out


def fasta_text(recs, eol="\n", blank_every=0, final_newline=True):
    parts = []
    for header, seq, widths in recs:
        parts.append(">" + header + eol)
        for j, ln in enumerate(lines_of(seq, widths)):
            parts.append(ln + eol)
            if blank_every and j % blank_every == blank_every - 1:
                parts.append(eol * (1 + j % 3))
    text = "".join(parts)
    if not final_newline:
        text = text.rstrip("\r\n")
    return text


def tricount_cases(rng):
    cases = []
    mixed = dict(lower=0.05, nrun=0.02, iupac=0.01)
    for w in (1, 2, 3, 60, 61):
        s = rand_seq(rng, 700, **mixed)
        cases.append(dict(name="width{}".format(w), fasta=fasta_text([("chr1", s, [w])]), region="chr1"))
    s = rand_seq(rng, 1500, **mixed)
    cases.append(dict(name="irregular", fasta=fasta_text([("chr1", s, [7, 60, 1, 33, 2, 80])]), region="chr1"))
    cases.append(dict(name="crlf", fasta=fasta_text([("chr1", s, [60])], eol="\r\n"), region="chr1"))
    cases.append(dict(name="blank_lines", fasta=fasta_text([("chr1", s, [13, 5])], blank_every=4), region="chr1"))
    cases.append(dict(name="crlf_blank", fasta=fasta_text([("chr1", s, [11])], eol="\r\n", blank_every=3), region="chr1"))
    cases.append(dict(name="no_final_newline", fasta=fasta_text([("chr1", s, [61])], final_newline=False), region="chr1"))
    cases.append(dict(name="masked_heavy", fasta=fasta_text([("chr1", rand_seq(rng, 3000, lower=0.3, nrun=0.1, iupac=0.05),
                                                              [60])]), region="chr1"))
    short = [("s0", "", [60]), ("s1", "A", [60]), ("s2", "CT", [1]), ("s3", "ACG", [2]), ("s4", "TCA", [1])]
    text = fasta_text(short)
    for name, _, _ in short:
        cases.append(dict(name="short_" + name, fasta=text, region=name))
    a, b, c = rand_seq(rng, 900, **mixed), rand_seq(rng, 400, **mixed), rand_seq(rng, 650, **mixed)
    text = fasta_text([("chrA some description here", a, [60]), ("chrB", b, [50]), ("chrA", c, [61]),
                       ("chrC\tlen=650 x", c[::-1], [70])])
    cases.append(dict(name="duplicate_name", fasta=text, region="chrA"))
    cases.append(dict(name="description", fasta=text, region="chrC"))
    cases.append(dict(name="region_list", fasta=text, region_list="chrA\nchrC\n"))
    cases.append(dict(name="region_and_list", fasta=text, region="chrB", region_list="chrC\nchrA\n"))
    cases.append(dict(name="missing_name", fasta=text, region="chrZ"))
    cases.append(dict(name="neither", fasta=text))
    multi = [("c{}".format(k), rand_seq(rng, rng.randint(50, 900), **mixed), [rng.choice([1, 3, 60, 61])]) for k in range(6)]
    cases.append(dict(name="unselected_between", fasta=fasta_text(multi), region_list="c1\nc4\nc2\n"))
    return cases


def put(tmp, name, text):
    """Write text (if any) to tmp/name and return the path (or None)."""
    if text is None:
        return None
    path = os.path.join(tmp, name)
    with open(path, "w", newline="") as o:
        o.write(text)
    return path


def capture(exp, key, fn, out):
    """Run fn; exp[key + "raises"] = what it raised (None, "KeyError", "SystemExit(0)", ...), exp[out_key] = the file."""
    try:
        fn()
        exp[key + "raises"] = None
    except SystemExit as e:
        exp[key + "raises"] = "SystemExit({})".format(e.code)
    except Exception as e:  # noqa: BLE001
        exp[key + "raises"] = type(e).__name__
    gc.collect()                       # the reference leaves a file open when it raises: flush it
    return open(out).read() if os.path.exists(out) else None


def run_tricount(NH, case, tmp):
    fa, rl = put(tmp, case["name"] + ".fa", case["fasta"]), put(tmp, case["name"] + ".list", case.get("region_list"))
    out = os.path.join(tmp, case["name"] + ".tri.tsv")
    exp = dict(case)
    exp["tsv"] = capture(exp, "", lambda: NH.reflib.get_ref_tricount(fa, case.get("region"), rl, 1, out), out)
    return exp


VCF_HEAD = ("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n{contigs}"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsyn1\n")


def vcf_text(contigs, recs):
    head = VCF_HEAD.format(contigs="".join("##contig=<ID={},length={}>\n".format(n, l) for n, l in contigs))
    body = "".join("{}\t{}\t.\t{}\t{}\t60\t{}\t.\tGT\t0/1\n".format(*r) for r in recs)
    return head + body


def sbs_inputs(rng, dense, lower_pyr=False):
    """Two contigs (plus an unselected third) and PASS SNVs on them: dense fills all 96 (tri, sub) groups.  N
    neighbours on both strands and lower-case neighbours of a purine (read as N) are dropped; a lower-case neighbour
    of a pyrimidine (lower_pyr) is a KeyError in the reference."""
    seqs = {"chr1": rand_seq(rng, 6000, nrun=0.003), "chr2": rand_seq(rng, 3000, nrun=0.003), "chrX": rand_seq(rng, 300)}
    s2 = list(seqs["chr2"])
    s2[100:105] = list("ANGNA")
    s2[200:205] = list("AgAtA")
    s2[300:305] = list("TNCNT")
    s2[400:405] = list("gaGct")
    if lower_pyr:
        s2[500:505] = list("AcCgT")
    seqs["chr2"] = "".join(s2)
    recs = []
    nsnv = 900 if dense else 40
    alts = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}
    for _ in range(nsnv):
        chrom = "chr1" if rng.random() < 0.75 else "chr2"
        s = seqs[chrom]
        p = rng.randrange(2, len(s) - 2)
        r = s[p]
        if r not in "ACGT":
            continue
        recs.append((chrom, p + 1, r, rng.choice(alts[r]), "PASS"))
    for chrom, p in (("chr2", 103), ("chr2", 203), ("chr2", 303), ("chr2", 403), ("chr2", 503)):
        r = seqs[chrom][p - 1]
        if r in "ACGT":
            recs.append((chrom, p, r, alts[r][0], "PASS"))
    for p in (1, 2):                                   # the first positions: upstream wraps to the end of the string
        r = seqs["chr2"][p - 1]
        if r in "ACGT":
            recs.append(("chr2", p, r, alts[r][1], "PASS"))
    recs.append(("chr1", 500, seqs["chr1"][499], "A" if seqs["chr1"][499] != "A" else "C", "LowQual"))   # not PASS
    recs.append(("chr1", 600, "C", "A,T", "PASS"))     # multi-allelic
    recs.append(("chr1", 700, "CA", "C", "PASS"))      # indel
    recs.sort(key=lambda r: (r[0], r[1]))
    contigs = [(n, len(s)) for n, s in seqs.items()]
    return seqs, vcf_text(contigs, recs)


def end_inputs(rng, k):
    """One PASS SNV at 1-based position len - k + 1 (len, len - 1): IndexError in the reference where the context runs
    past the end of the string."""
    s = "".join(rng.choices("ACGT", k=300))
    p = len(s) - k + 1
    r = s[p - 1]
    return {"chr1": s}, vcf_text([("chr1", len(s))], [("chr1", p, r, "A" if r != "A" else "C", "PASS")])


def run_sbs(NH, name, seqs, vcf, tmp, region=None, region_list=None):
    fa = put(tmp, name + ".fa", fasta_text([(n, s, [60]) for n, s in seqs.items()]))
    vf, rl = put(tmp, name + ".vcf", vcf), put(tmp, name + ".list", region_list)
    _, tname2tsize = NH.vcflib.get_sample(vf)
    exp = dict(name=name, fasta=open(fa).read(), vcf=vcf, region=region, region_list=region_list)
    for kind, fn in (("sbs96", NH.mutlib.dump_sbs96_counts), ("sbs1536", NH.mutlib.dump_sbs1536_counts)):
        out = os.path.join(tmp, "{}.{}.tsv".format(name, kind))
        exp[kind + "_tsv"] = capture(exp, kind + "_", lambda: fn(vf, fa, region, rl, tname2tsize, out), out)
    return exp


def run_burden(NH, name, table, tmp, tri_text=None, fasta=None, region_list="chr9\n"):
    inf, tri, fa = put(tmp, name + ".norm.tsv", table), put(tmp, name + ".tri", tri_text), put(tmp, name + ".fa", fasta)
    rl = put(tmp, name + ".list", region_list)
    out = os.path.join(tmp, name + ".burden")
    # the FASTA is norm_host.json's "fasta_text": named, not stored again
    exp = dict(name=name, table=table, tri=tri_text, fasta="norm_host" if fasta is not None else None, region_list=region_list)
    exp["out"] = capture(exp, "", lambda: NH.mutlib.get_burden_per_cell(inf, fa, tri, rl, 1, out), out)
    return exp


def main():
    NH = H.load_reference_norm_host()
    rng = random.Random(20261016)
    golden = {"tri_lst": list(NH.mutlib.tri_lst), "sbs96_lst": list(NH.mutlib.sbs96_lst),
              "sbs1536_lst": list(NH.mutlib.sbs1536_lst)}
    with tempfile.TemporaryDirectory() as tmp:
        golden["tricount"] = [run_tricount(NH, c, tmp) for c in tricount_cases(rng)]
        sbs = []
        seqs, vcf = sbs_inputs(rng, dense=True)
        sbs.append(run_sbs(NH, "dense", seqs, vcf, tmp))
        sbs.append(run_sbs(NH, "dense_chr2", seqs, vcf, tmp, region="chr2"))
        sbs.append(run_sbs(NH, "dense_list", seqs, vcf, tmp, region_list="chr2\nchr1\n"))
        seqs, vcf = sbs_inputs(rng, dense=False)
        sbs.append(run_sbs(NH, "sparse", seqs, vcf, tmp))
        seqs, vcf = sbs_inputs(rng, dense=False, lower_pyr=True)
        sbs.append(run_sbs(NH, "lower_pyrimidine", seqs, vcf, tmp))
        for k in (1, 2):
            seqs, vcf = end_inputs(rng, k)
            sbs.append(run_sbs(NH, "end{}".format(k), seqs, vcf, tmp))
        golden["sbs"] = sbs
        norm = json.load(open(os.path.join(HERE, "norm_host.json")))
        table = norm["normcounts_tsv"]
        fasta = norm["fasta_text"]
        tri = run_tricount(NH, dict(name="norm_host", fasta=fasta, region=norm["contig"]), tmp)["tsv"]
        rl = norm["contig"] + "\n"
        rows = table.splitlines(True)
        k = next(i for i, ln in enumerate(rows) if ln.startswith("sub")) + 5
        f = rows[k].rstrip("\n").split("\t")
        f[-1] = "0"
        zero = "".join(rows[:k]) + "\t".join(f) + "\n" + "".join(rows[k + 1:])
        golden["burden"] = [
            run_burden(NH, "tri", table, tmp, tri_text=tri, region_list=rl),
            run_burden(NH, "ref", table, tmp, fasta=fasta, region_list=rl),
            run_burden(NH, "tri_and_ref", table, tmp, tri_text=tri, fasta=fasta, region_list=rl),
            run_burden(NH, "neither", table, tmp, region_list=rl),
            run_burden(NH, "zero_callable", zero, tmp, tri_text=tri, region_list=rl),
        ]
    # every text of 256 characters or more is stored once, under "blobs", and named by "@" + its hash where it is used
    blobs = {}

    def share(x):
        if isinstance(x, dict):
            return {k: share(v) for k, v in x.items()}
        if isinstance(x, list):
            return [share(v) for v in x]
        if isinstance(x, str) and len(x) >= 256:
            key = "@" + hashlib.sha1(x.encode()).hexdigest()[:12]
            blobs[key] = x
            return key
        return x
    out = share({k: v for k, v in golden.items() if k.endswith("_lst") is False})
    out.update({k: v for k, v in golden.items() if k.endswith("_lst")})
    out["blobs"] = blobs
    with open(os.path.join(HERE, "mutpatterns.json"), "w") as o:
        json.dump(out, o, sort_keys=True)
    print("tricount", [(c["name"], c["raises"]) for c in golden["tricount"]])
    print("sbs", [(c["name"], c["sbs96_raises"], c["sbs1536_raises"]) for c in golden["sbs"]])
    print("burden", [(c["name"], c["raises"], c["out"]) for c in golden["burden"]])


if __name__ == "__main__":
    main()
