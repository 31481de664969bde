#!/usr/bin/env python3
"""Regenerates the golden fixtures in this directory by running the REFERENCE
(read-only checkout at /root/reference) through tests/golden/ref_harness.py.

Run in the build container only:  python tests/golden/make_golden.py
The outputs (*.json expected values, *.npz inputs) are committed; the tests
never need the reference.  Inputs come from the repo's own synthetic generator
or from hand-written records, never from reference files.
"""
import json
import os
import sys

_FEATS = "AVX512F AVX512CD AVX512VL AVX512BW AVX512DQ AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX2 FMA3"
if os.environ.get("NPY_DISABLE_CPU_FEATURES") != _FEATS:
    # numpy must come up with its SIMD sorts off so np.argsort breaks ties the
    # way the numpy pinned by the reference does.
    env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=_FEATS)
    import subprocess
    sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))

import random  # noqa: E402

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402
from himut_amd.readbatch import ReadBatch, batch_from_records  # noqa: E402
from himut_amd import synth  # noqa: E402


def _canon(v):
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    return v


def canon_records(recs):
    return [[_canon(x) for x in r[1:]] for r in recs]  # chrom dropped (constant)


def save(case, expected, batch=None, extra_npz=None):
    with open(os.path.join(HERE, case + ".json"), "w") as o:
        json.dump(expected, o, indent=0, sort_keys=True)
    d = {}
    if batch is not None:
        d.update(batch.to_npz_dict())
    if extra_npz:
        d.update(extra_npz)
    if d:
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **d)
    print("wrote", case, "records" in expected and len(expected["records"]))


def thresholds_of(ref, bam, chroms, sizes):
    return ref.bamlib.get_thresholds(bam, chroms, sizes)


def worker_case(case, cfg, chunks=None, tmpdir="/tmp", with_sets=False, phase_block=0, overrides=None,
                md_threshold=None, qlen_limits=None, mutate=None, create_pon=False):
    ref = H.load_reference()
    s = synth.generate(cfg)
    b = s.batch
    if mutate is not None:
        mutate(b)
    bam = "/fake/{}.bam".format(case)
    H.register_bam(bam, {b.name: b})
    sizes = {b.name: b.length}
    ql, qu, md = thresholds_of(ref, bam, [b.name], sizes)
    if md_threshold is not None:
        md = md_threshold
    if qlen_limits is not None:
        ql, qu = qlen_limits
    if chunks is None:
        _, c2c = ref.util.load_loci(None, None, sizes)
        chunks = [(s_, e_) for (_, s_, e_) in c2c[b.name]]
    exp = {"chunks": chunks, "qlen_lower_limit": ql, "qlen_upper_limit": qu, "md_threshold": md,
           "overrides": overrides or {}, "contig": b.name, "length": b.length}
    common = pon = None
    if with_sets:
        common = os.path.join(tmpdir, case + ".common.vcf")
        pon = os.path.join(tmpdir, case + ".pon.vcf")
        # a first pass without sets gives true candidates to seed the side files with
        recs0, _ = H.run_reference_worker(bam, b.name, chunks, ql, qu, md, **(overrides or {}))
        passing = [(r[1], r[2], r[3]) for r in recs0 if r[4] in ("PASS", "LowDepth", "HighDepth")]
        synth.write_common_snps_vcf(common, s, seed=cfg.seed, extra_sites=passing[3::5])
        synth.write_pon_vcf(pon, s, seed=cfg.seed, extra_sites=passing[::7])
        exp["common_vcf"] = open(common).read()
        exp["pon_vcf"] = open(pon).read()
        exp["common_set"] = sorted([list(t) for t in ref.vcflib.load_common_snp(b.name, common)])
        exp["pon_set"] = sorted([list(t) for t in ref.vcflib.load_pon(b.name, pon)])
    phase_sets = None
    if phase_block:
        pv = os.path.join(tmpdir, case + ".phased.vcf")
        synth.write_phased_vcf(pv, s, block=phase_block)
        hb, hp, hs, c2c = ref.vcflib.load_phased_hetsnps(pv, [b.name], sizes)
        phase_sets = (dict(hb[b.name]), dict(hp[b.name]), dict(hs[b.name]))
        chunks = [(s_, e_) for (_, s_, e_) in c2c[b.name]]
        exp["chunks"] = chunks
        exp["phased_vcf"] = open(pv).read()
        exp["phase_sets"] = {"hbit": phase_sets[0], "hpos": phase_sets[1],
                             "hetsnp": {k: [list(t) for t in v] for k, v in phase_sets[2].items()}}
    recs, log = H.run_reference_worker(bam, b.name, chunks, ql, qu, md, common_snps=common, panel_of_normals=pon,
                                       phase=bool(phase_block), phase_sets=phase_sets,
                                       create_panel_of_normals=create_pon, **(overrides or {}))
    exp["create_panel_of_normals"] = create_pon
    exp["records"] = canon_records(recs)
    exp["log"] = [int(x) for x in log]
    # formatted VCF body as the reference's own writer prints it
    out = os.path.join(tmpdir, case + ".out.vcf")
    cwd = os.getcwd()
    os.chdir(tmpdir)
    try:
        if phase_block:
            ref.vcflib.dump_phased_sbs(out, "#HEADER", [b.name], {b.name: recs})
        else:
            ref.vcflib.dump_sbs(out, "#HEADER", [b.name], {b.name: recs})
        ref.vcflib.dump_call_log([b.name], {b.name: log})
        exp["log_text"] = open("himut.log").read()
    finally:
        os.chdir(cwd)
    exp["vcf_text"] = open(out).read()
    exp["sm_vcf_text"] = open(out.replace(".vcf", ".single_molecule_mutations.vcf")).read()
    from collections import Counter
    exp["status_histogram"] = dict(Counter(r[4] for r in recs))
    print("   ", case, exp["status_histogram"], log)
    save(case, exp, batch=b)
    return exp


def norm_case(case, cfg, chunks=None, tmpdir="/tmp", with_sets=False, overrides=None, md_threshold=None,
              qlen_limits=None, mutate_ref=None, non_human_sample=False, phase_block=0, mutate_batch=None,
              both_sets_at_multiallelic=False, do_save=True):
    """normcounts.get_callable_tricounts (non-phased) on a synthetic contig + its reference sequence."""
    ref = H.load_reference()
    s = synth.generate(cfg, want_ref=True)
    b = s.batch
    if mutate_batch is not None:
        mutate_batch(b)
    seq = bytes(s.ref).decode()
    if mutate_ref is not None:
        seq = mutate_ref(seq)
    bam = "/fake/{}.bam".format(case)
    H.register_bam(bam, {b.name: b})
    sizes = {b.name: b.length}
    ql, qu, md = thresholds_of(ref, bam, [b.name], sizes)
    if md_threshold is not None:
        md = md_threshold
    if qlen_limits is not None:
        ql, qu = qlen_limits
    if chunks is None:
        _, c2c = ref.util.load_loci(None, None, sizes)
        chunks = [(s_, e_) for (_, s_, e_) in c2c[b.name]]
    exp = {"chunks": chunks, "qlen_lower_limit": ql, "qlen_upper_limit": qu, "md_threshold": md,
           "overrides": overrides or {}, "contig": b.name, "length": b.length, "non_human_sample": non_human_sample}
    common = pon = None
    if with_sets:
        common = os.path.join(tmpdir, case + ".common.vcf")
        pon = os.path.join(tmpdir, case + ".pon.vcf")
        # sites where some read carries a non-reference base: candidates of the call worker seed the side files
        recs0, _ = H.run_reference_worker(bam, b.name, chunks, ql, qu, md, **(overrides or {}))
        hits = [(r[1], r[2], r[3]) for r in recs0 if len(r[3]) == 1]
        extra_com, extra_pon = hits[3::4], hits[::5]
        if both_sets_at_multiallelic:
            # positions where the pile shows two alternative alleles: one goes to the panel of normals, the other to
            # the common SNPs, so which filter counts the position (normcounts.py:367-383: the first alternative with
            # reads, in the order python iterates set("ATGC").difference(ref)) depends on the interpreter's hash seed
            from collections import defaultdict
            by_pos = defaultdict(list)
            for (p_, r_, a_) in hits:
                by_pos[(p_, r_)].append(a_)
            multi = sorted(k for k, v in by_pos.items() if len(set(v)) >= 2)
            extra_com, extra_pon = [], []
            for n_, (p_, r_) in enumerate(multi):
                a1, a2 = sorted(set(by_pos[(p_, r_)]))[:2]
                if n_ % 2:
                    a1, a2 = a2, a1
                extra_pon.append((p_, r_, a1))
                extra_com.append((p_, r_, a2))
            exp["multiallelic_positions"] = len(multi)
        synth.write_common_snps_vcf(common, s, seed=cfg.seed, extra_sites=extra_com)
        synth.write_pon_vcf(pon, s, seed=cfg.seed, extra_sites=extra_pon)
        exp["common_set"] = sorted([list(t) for t in ref.vcflib.load_common_snp(b.name, common)])
        exp["pon_set"] = sorted([list(t) for t in ref.vcflib.load_pon(b.name, pon)])
    phase_sets = None
    if phase_block:
        pv = os.path.join(tmpdir, case + ".phased.vcf")
        synth.write_phased_vcf(pv, s, block=phase_block)
        hb, hp, hs, c2c = ref.vcflib.load_phased_hetsnps(pv, [b.name], sizes)
        phase_sets = (dict(hb[b.name]), dict(hp[b.name]), dict(hs[b.name]))
        chunks = [(s_, e_) for (_, s_, e_) in c2c[b.name]]
        exp["chunks"] = chunks
        exp["phase_sets"] = {"hbit": phase_sets[0], "hpos": phase_sets[1],
                             "hetsnp": {k: [list(t) for t in v] for k, v in phase_sets[2].items()}}
    ccs, rf, log, order = H.run_reference_normcounts(bam, b.name, seq, chunks, ql, qu, md, common_snps=common,
                                                     panel_of_normals=pon, non_human_sample=non_human_sample,
                                                     phase_sets=phase_sets, **(overrides or {}))
    exp["ccs_tri2count"] = {k: int(v) for k, v in ccs.items()}
    exp["ref_tri2count"] = {k: int(v) for k, v in rf.items()}
    exp["log"] = [int(x) for x in log]
    exp["alt_order"] = order
    print("   ", case, exp["log"], "keys", len(ccs))
    if do_save:
        save(case, exp, batch=b, extra_npz={"refseq": np.frombuffer(seq.encode("ascii"), np.uint8)})
    exp["_batch"], exp["_seq"] = b, seq
    return exp


def nsub_batch(b, every=3):
    """Rewrites the cs tags of every ``every``-th read so that its substitutions name the reference base as 'n'
    (minimap2 writes that where the reference has an N): cslib.cs2subindel keeps such a substitution out of the
    mismatch list (cslib.py:54-56) while update_tri2count still counts its base unconditionally (normcounts.py:97-109)."""
    cs = b.cs
    for r in range(0, b.n, every):
        a, z = int(b.cs_off[r]), int(b.cs_off[r + 1])
        seg = cs[a:z]
        star = np.nonzero(seg == ord("*"))[0]
        seg[star + 1] = ord("n")


def dup_names_batch(b, every=7):
    """Gives every ``every``-th read the query name of the read before it (a supplementary alignment, flag 0x800): the
    phased vote of caller.py:552-603 goes by query NAME."""
    for r in range(1, b.n, every):
        b.qid[r] = b.qid[r - 1]
        b.flag[r] |= 0x800


def norm_order_case(tmpdir="/tmp"):
    """normcounts where the panel of normals and the common SNPs both hold an alternative allele of the same
    position, run under two PYTHONHASHSEED values: the two interpreters iterate set("ATGC").difference(ref) in
    different orders, and the fixture keeps the expected outcome of each."""
    import subprocess
    variants = []
    base = None
    for seed in ("1", "2", "3", "4", "5", "6"):
        out = os.path.join(tmpdir, "norm_order.{}.json".format(seed))
        env = dict(os.environ, PYTHONHASHSEED=seed, HIMUT_GOLDEN_PART=out)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "norm_order_part"], env=env)
        part = json.load(open(out))
        if base is None:
            base = part
        key = json.dumps(part["alt_order"], sort_keys=True)
        if all(json.dumps(v["alt_order"], sort_keys=True) != key for v in variants):
            variants.append({k: part[k] for k in ("alt_order", "log", "ccs_tri2count", "ref_tri2count", "hashseed")})
    assert len(variants) >= 2, "every hash seed tried gave the same set order"
    pon_pop = {(v["log"][11], v["log"][12]) for v in variants}
    assert len(pon_pop) >= 2, "the order never decided PoN vs common: " + str(pon_pop)
    exp = {k: v for k, v in base.items() if k not in ("alt_order", "log", "ccs_tri2count", "ref_tri2count", "hashseed")}
    exp["variants"] = variants
    # inputs: regenerate in this process (identical: the generator is seeded)
    full = norm_order_part(do_save=False)
    save("norm_order", exp, batch=full["_batch"], extra_npz={"refseq": np.frombuffer(full["_seq"].encode("ascii"), np.uint8)})


def norm_order_part(do_save=True):
    exp = norm_case("norm_order", small_cfg(206, contig_len=20000, depth=70.0, name="chrD", som_rate=1e-3, snp_rate=4e-3,
                                            sub_rate=2e-3, ins_rate=5e-4, del_rate=5e-4),
                    with_sets=True, md_threshold=200, both_sets_at_multiallelic=True, do_save=False,
                    overrides=dict(min_bq=40, min_gq=10, max_mismatch_count=2, mismatch_window_size=15, min_ref_count=2,
                                   min_alt_count=1, min_sequence_identity=0.95))
    exp["hashseed"] = os.environ.get("PYTHONHASHSEED", "")
    part = os.environ.get("HIMUT_GOLDEN_PART")
    if part and do_save:
        with open(part, "w") as o:
            json.dump({k: v for k, v in exp.items() if not k.startswith("_")}, o)
    return exp


def small_cfg(seed, **kw):
    d = dict(seed=seed, contig_len=30000, read_len_mean=3000, read_len_sd=500, read_len_min=1200, read_len_max=5000,
             name="chr7")
    d.update(kw)
    return synth.SynthConfig(**d)


def leaf_gtlib(n=400):
    """get_germ_gt / get_germ_gq over random and tie-heavy columns (gtlib.py:122-174)."""
    ref = H.load_reference()
    rs = random.Random(5)
    ref.gtlib.init(1 / (10 ** 3))
    out = []
    for k in range(n):
        depth = rs.choice([1, 2, 3, 5, 8, 13, 30, 60])
        refb = rs.choice("ATGC")
        mode = k % 5
        alleles, bqs = [], []
        for _ in range(depth):
            if mode == 0:
                a = refb if rs.random() < 0.9 else rs.choice("ATGC")
            elif mode == 1:
                a = rs.choice([refb, "ATGC"[(("ATGC".index(refb)) + 1) % 4]])
            elif mode == 2:
                a = rs.choice("ATGC")
            elif mode == 3:
                a = rs.choice([x for x in "ATGC" if x != refb][:2])
            else:
                a = rs.choice([x for x in "ATGC" if x != refb][:1])
            alleles.append(a)
            bqs.append(93 if (mode in (1, 3) or rs.random() < 0.8) else rs.randint(1, 92))
        a2b = {0: [], 1: [], 2: [], 3: [], 4: [], 5: []}
        for a, q in zip(alleles, bqs):
            a2b[ref.util.base2idx[a]].append(q)
        gt, gq, state, gt2state = ref.gtlib.get_germ_gt(refb, a2b)
        alt = rs.choice([x for x in "ATGC" if x != refb])
        germ_gq = ref.gtlib.get_germ_gq(refb + alt, gt2state, a2b)
        pls, _ = ref.gtlib.get_germ_gt_pD(refb, a2b)
        out.append({"ref": refb, "alleles": "".join(alleles), "bqs": bqs, "gt": gt, "gq": int(gq), "state": state,
                    "germ_gq": int(germ_gq), "pls": [float(x) for x in pls]})
    tables = {"hom": [ref.gtlib.get_log10_one_minus_epsilon(q) for q in range(1, 94)],
              "het": [ref.gtlib.get_log10_one_half_minus_epsilon(q) for q in range(1, 94)],
              "err": [ref.gtlib.get_log10_epsilon(q / 3) for q in range(1, 94)],
              "prior": {k: ref.gtlib.get_log10_germ_gt_prior(k) for k in ("homref", "het", "hetalt", "homalt")}}
    save("leaf_gtlib", {"vectors": out, "tables": tables})


GT_DEPTHS = [2, 3, 4, 5, 8, 12, 20, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
PRIOR_LO, PRIOR_HI = 1e-4, 1e-2        # the human default and the non-human priors of germline_priors.json lie within


def _bits(x):
    import struct
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b):
    import struct
    return struct.unpack("<d", struct.pack("<q", b))[0]


def _crossing(pred, lo=PRIOR_LO, hi=PRIOR_HI):
    """Adjacent doubles (a, b) in [lo, hi] with pred(a) != pred(b), by bisection on the bit patterns; None if pred is
    the same at both ends."""
    plo = pred(lo)
    if plo == pred(hi):
        return None
    a, b = _bits(lo), _bits(hi)
    while b - a > 1:
        m = (a + b) // 2
        if pred(_from_bits(m)) == plo:
            a = m
        else:
            b = m
    return _from_bits(a), _from_bits(b)


def _gq_value(col, p, target):
    """second - best at prior p of the column's plain PLs (target None) or of the PLs with base `target` left out."""
    from tests import gt_piles as G
    ref, al, bq = col
    return G.decide(G.pls(ref, al, bq, p, skip=target))[1]


def _reference_vector(ref_mod, kind, col, prior, k, pair):
    """The reference's own outputs for one column (gtlib.init, get_germ_gt, get_germ_gt_pD, get_germ_gq), checked
    against the restatement in tests/gt_piles.py, which must agree bit for bit."""
    from tests import gt_piles as G
    refb, alleles, bqs = col
    g = ref_mod.gtlib
    g.init(prior)
    a2b = {0: [], 1: [], 2: [], 3: [], 4: [], 5: []}
    for a, q in zip(alleles, bqs):
        a2b[ref_mod.util.base2idx[a]].append(q)
    gt, gq, state, gt2state = g.get_germ_gt(refb, a2b)
    pls, _ = g.get_germ_gt_pD(refb, a2b)
    germ = {alt: int(g.get_germ_gq(alt, gt2state, a2b)) for alt in "ATGC" if alt != refb}
    v = {"kind": kind, "ref": refb, "alleles": "".join(alleles), "bqs": [int(q) for q in bqs], "prior": prior,
         "k": int(k), "pair": pair, "gt": gt, "gq": int(gq), "state": state, "pls": [float(x) for x in pls],
         "germ_gq": germ}
    m = G.genotype(refb, v["alleles"], bqs, prior)
    assert (m["gt"], m["gq"], m["state"], m["pls"], m["germ_gq"]) == (gt, int(gq), state, v["pls"], germ), v
    return v


def _mixed_column(rs, ref, depth, bq_pick, want="homref", lo=3.0, hi=90.0, alt2=False, tries=4000):
    """ref and alt1 reads (and one alt2 read) whose plain genotype at prior 1e-3 is `want` with second - best in
    [lo, hi]: reads flip between ref and alt1 until it is.  None if that does not happen."""
    from tests import gt_piles as G
    alts = [b for b in "ATGC" if b != ref]
    rs.shuffle(alts)
    al = [ref if rs.random() < 0.7 else alts[0] for _ in range(depth)]
    bq = [bq_pick(rs) for _ in range(depth)]
    if alt2 and depth >= 3:
        al[rs.randrange(depth)] = alts[1]
    for _ in range(tries):
        g = G.genotype(ref, al, bq, 1e-3)
        if g["state"] == want and lo <= g["gqf"] <= hi:
            return ref, al, bq
        refs = [i for i, a in enumerate(al) if a == ref]
        alt1 = [i for i, a in enumerate(al) if a == alts[0]]
        if (g["state"] == "homref") == (want == "homref") and g["gqf"] > hi:
            pool = refs if want == "homref" else alt1
            to = alts[0] if want == "homref" else ref
        else:
            pool = alt1 if want == "homref" else refs
            to = ref if want == "homref" else alts[0]
        if len(pool) <= 1:
            return None
        al[rs.choice(pool)] = to
    return None


def gt_edges():
    """Genotype vectors at fp64 decision boundaries, evaluated by the reference's gtlib (tests/gt_piles.py holds the
    layout and the restatement).  Each kind but assoc is a crossing: two priors one ulp apart in [1e-4, 1e-2] between
    which second - best (or the alt-omitted one) passes the integer k.  A side is kept only if it discriminates: summing
    a base's reads in reverse, with math.fsum, with the prior first or in another base order changes its outcome (gt,
    state, gq, gq >= k, or an alt-omitted quality).  A depth-1 column never does, so none is kept."""
    from tests import gt_piles as G
    ref_mod = H.load_reference()
    rs = random.Random(97)
    out = []
    need = {"gq_int": 64, "cap99": 12, "germ_gq_int": 24, "assoc": 32, "order": 12, "qual": 24, "state": 24}
    got = {k: 0 for k in need}
    pair = [0]

    def keep(kind, col, prior, k):
        return _reference_vector(ref_mod, kind, col, prior, k, pair[0])

    def crossing_pair(kind, col, target=None, ks=None, state=None):
        f_lo, f_hi = _gq_value(col, PRIOR_LO, target), _gq_value(col, PRIOR_HI, target)
        a, b = sorted((f_lo, f_hi))
        cands = [k for k in (ks or range(1, 99)) if a < k <= b]
        if not cands:
            return False
        k = rs.choice(cands)
        x = _crossing(lambda p: _gq_value(col, p, target) >= k)
        if x is None:
            return False
        vs = []
        for p in x:
            v = {"ref": col[0], "alleles": "".join(col[1]), "bqs": col[2], "prior": p, "k": k}
            g = G.genotype(col[0], col[1], col[2], p)
            if state is not None and g["state"] != state:
                return False
            pure = col[0] * len(col[1]) == "".join(col[1])
            if target is None and kind != "qual" and g["state"] != "homref" and not pure and \
                    not any(G.candidates(dict(v, gt=g["gt"], state=g["state"])).values()):
                return False                     # a gq the call run never shows and normcounts never reads
            if G.flips(v):
                vs.append((p, k))
        if not vs:
            return False
        for p, k_ in vs:
            out.append(keep(kind, col, p, k_))
        got[kind] += len(vs)
        pair[0] += 1
        return True

    def any_bq(rs):
        return rs.choice([93, 93, rs.randint(1, 92), rs.randint(1, 40), rs.randint(20, 93)])

    def low_bq(rs):
        return rs.choice([rs.randint(1, 12), rs.randint(1, 30), rs.randint(5, 25)])

    # gq_int: pure-reference columns (depth <= 20: deeper ones sit at 99) and ref + alt columns at every depth
    pure_depths = [3, 4, 5, 8, 12, 20]        # (a pure depth-2 column never discriminates: a + b is b + a)
    i = 0
    while got["gq_int"] < need["gq_int"] // 2:
        d = pure_depths[i % len(pure_depths)]
        i += 1
        ref = rs.choice("ATGC")
        crossing_pair("gq_int", (ref, [ref] * d, [any_bq(rs) for _ in range(d)]))
    i = 0
    while got["gq_int"] < need["gq_int"]:
        d = GT_DEPTHS[i % len(GT_DEPTHS)]
        i += 1
        col = _mixed_column(rs, rs.choice("ATGC"), d, low_bq if d > 20 else any_bq, alt2=bool(i % 2))
        if col is not None:
            crossing_pair("gq_int", col)
    # cap99: second - best on either side of 99.0
    i = 0
    while got["cap99"] < need["cap99"]:
        d = [20, 21, 22, 23, 24, 64, 128, 256][i % 8]
        i += 1
        ref = rs.choice("ATGC")
        if d < 30:
            col = (ref, [ref] * d, [rs.choice([93, rs.randint(30, 93)]) for _ in range(d)])
        else:
            col = _mixed_column(rs, ref, d, low_bq, lo=80.0, hi=99.0)
        if col is not None:
            crossing_pair("cap99", col, ks=[99])
    # germ_gq_int: ref reads plus reads of one alt allele at low quality (homref stays the genotype, normcounts leaves
    # the alt out: the ref reads and the priors decide); the alt's reads pad the column to the deep depths
    i = 0
    while got["germ_gq_int"] < need["germ_gq_int"]:
        d = GT_DEPTHS[i % len(GT_DEPTHS)]
        i += 1
        ref = rs.choice("ATGC")
        alt = rs.choice([b for b in "ATGC" if b != ref])
        nref = min(d - 1, rs.randint(3, 16)) if d > 1 else 0
        if nref < 1:
            continue
        al = [ref] * nref + [alt] * (d - nref)
        bq = [any_bq(rs) for _ in range(nref)] + [rs.randint(1, 4) for _ in range(d - nref)]
        z = list(zip(al, bq))
        rs.shuffle(z)
        crossing_pair("germ_gq_int", (ref, [a for a, _ in z], [q for _, q in z]), target=alt, state="homref")
    # qual: qualities 1-3 (homalt / hetalt best or second) and 94-255 (the hom term is 0.0 from about 163 up)
    i = 0
    while got["qual"] < need["qual"]:
        i += 1
        ref = rs.choice("ATGC")
        if i % 2:
            d = rs.choice([3, 4, 5, 8, 12, 20, 63])
            al = [rs.choice("ATGC") for _ in range(d)]
            bq = [rs.choice([1, 2, 3, 1, 2, 3, rs.randint(4, 30)]) for _ in range(d)]
            g = G.genotype(ref, al, bq, 1e-3)
            order = sorted(range(10), key=lambda j: (g["pls"][j], j))
            sts = [G.state_of(G.GT_LST[j][0], G.GT_LST[j][1], ref) for j in order[:2]]
            if not set(sts) & {"homalt", "hetalt"}:
                continue
        else:
            d = rs.choice([2, 3, 5, 8, 12, 20])
            al = [ref] * d
            if d >= 5 and i % 4 == 0:
                al[rs.randrange(d)] = rs.choice([b for b in "ATGC" if b != ref])
            bq = [rs.randint(163 if i % 4 == 2 else 94, 255) for _ in range(d)]
        crossing_pair("qual", (ref, al, bq))
    # assoc: ref with two alts whose reads carry the same quality multiset: the two het genotypes are equal in exact
    # maths; their fp64 PLs differ in the last bits (the lower one is the genotype) or tie bit for bit (the lower index)
    ties = {"tie": 0, "ulp": 0}
    i = 0
    while got["assoc"] < need["assoc"]:
        i += 1
        ref = "ATGC"[i % 4]
        x, y = rs.sample([b for b in "ATGC" if b != ref], 2)
        n = rs.randint(2, 12)
        qs = [rs.randint(10, 93) for _ in range(n)]
        qx, qy = qs[:], qs[:]
        rs.shuffle(qx)
        rs.shuffle(qy)
        m = n + rs.randint(0, 4)
        reads = [(ref, rs.randint(20, 93)) for _ in range(m)] + [(x, q) for q in qx] + [(y, q) for q in qy]
        rs.shuffle(reads)
        col = (ref, [a for a, _ in reads], [q for _, q in reads])
        p = _from_bits(_bits(1e-3) + rs.randint(-2 ** 40, 2 ** 40))
        g = G.genotype(ref, col[1], col[2], p)
        gx, gy = (G.GT_LST.index(t) if t in G.GT_LST else G.GT_LST.index(t[::-1]) for t in (ref + x, ref + y))
        if {gx, gy} != set(sorted(range(10), key=lambda j: (g["pls"][j], j))[:2]):
            continue
        sort = "tie" if g["pls"][gx] == g["pls"][gy] else "ulp"
        if ties[sort] >= need["assoc"] // 2 + 2 or got["assoc"] >= need["assoc"]:
            continue
        v = {"ref": ref, "alleles": "".join(col[1]), "bqs": col[2], "prior": p, "k": 20}
        if not G.flips(v) or ties[sort] >= (need["assoc"] + 1) // 2:
            continue
        ties[sort] += 1
        out.append(keep("assoc", col, p, 20))
        got["assoc"] += 1
        pair[0] += 1
    # state: ref + alt columns whose best genotype changes state (hom-ref against het or hom-alt) between two adjacent
    # priors: second - best crosses 0.0.  normcounts reads nothing else of the ten PLs of a column with another allele
    # (its quality is the alt-omitted one), and for a pure-reference column the prior's place in the sum makes no
    # difference, so these keep only sides that adding the prior first flips
    i = 0
    while got["state"] < need["state"]:
        d = GT_DEPTHS[i % len(GT_DEPTHS)]
        i += 1
        col = _mixed_column(rs, rs.choice("ATGC"), d, low_bq if d > 20 else any_bq, lo=0.0, hi=8.0, alt2=not i % 3)
        if col is None:
            continue

        def best_state(p):
            g = G.decide(G.pls(col[0], col[1], col[2], p))[0]
            return G.state_of(G.GT_LST[g][0], G.GT_LST[g][1], col[0])
        x = _crossing(lambda p: best_state(p) == "homref")
        if x is None:
            continue
        vs = [p for p in x if "prior_first" in G.flips({"ref": col[0], "alleles": "".join(col[1]), "bqs": col[2],
                                                         "prior": p, "k": 1})]
        for p in vs:
            out.append(keep("state", col, p, 1))
        got["state"] += len(vs)
        pair[0] += bool(vs)
    # order: one quality multiset in two fetch orders with different outcomes, at a crossing's prior
    base = [v for v in out if v["kind"] == "gq_int" and len(v["alleles"]) >= 8]
    i = 0
    while got["order"] < need["order"]:
        v = base[i % len(base)]
        i += 1
        z = list(zip(v["alleles"], v["bqs"]))
        for _ in range(200):
            rs.shuffle(z)
            col2 = (v["ref"], [a for a, _ in z], [q for _, q in z])
            w = {"ref": v["ref"], "alleles": "".join(col2[1]), "bqs": col2[2], "prior": v["prior"], "k": v["k"]}
            g = G.genotype(w["ref"], w["alleles"], w["bqs"], w["prior"])
            if (g["gt"], g["gq"], g["state"]) != (v["gt"], v["gq"], v["state"]) and G.flips(w) and G.flips(v):
                out.append(keep("order", (v["ref"], list(v["alleles"]), v["bqs"]), v["prior"], v["k"]))
                out.append(keep("order", col2, w["prior"], w["k"]))
                got["order"] += 2
                pair[0] += 1
                break
    print("    gt_edges:", got, ties, "depths", sorted({len(v["alleles"]) for v in out}))
    path = os.path.join(HERE, "gt_edges.json")
    with open(path, "w") as o:
        o.write('{"vectors": [\n')
        o.write(",\n".join(json.dumps(v, sort_keys=True, separators=(",", ":")) for v in out))
        o.write("\n]}\n")
    print("wrote gt_edges", len(out), "vectors", os.path.getsize(path), "bytes")


class _Obj:
    pass


def leaf_cs():
    """cs2tuple / cs2subindel / identity / window helpers on hand-written tags."""
    ref = H.load_reference()
    cases = [
        (":10*ag:5+tt:3-ac:7", "ACGTACGTACGTACGTAGTTCCCAAAAAAAG", 0, 100),
        ("=ACGTA*ct=GG+a=T-gg=C", "ACGTATGGATC", 0, 5),
        (":4*na:4", "NNACGTAACGTT", 2, 50),
        (":3+acgt:3", "ACGACGTACG", 0, 0),
        (":2-a:2*ga*ct:1", "ACGTACT", 0, 9),
    ]
    out = []
    for cs, seq, qstart, tstart in cases:
        o = _Obj()
        o.qstart = qstart
        o.qseq = seq
        o.tstart = tstart
        o.bq_int_lst = list(range(10, 10 + len(seq)))
        ref.cslib.cs2tuple(o, cs)
        ref.cslib.cs2subindel(o)
        o.qlen = len(seq)
        ident = ref.bamlib.BAM.get_blast_sequence_identity(o)
        out.append({"cs": cs, "seq": seq, "qstart": qstart, "tstart": tstart, "bq": o.bq_int_lst,
                    "tuples": [list(t) for t in o.cstuple_lst], "tsbs": [list(t) for t in o.tsbs_lst],
                    "qsbs": [list(t) for t in o.qsbs_lst], "mismatch": [list(t) for t in o.mismatch_lst],
                    "identity": ident})
    grid = []
    for qlen in (100, 1000, 15000):
        for qpos in (0, 5, 19, 20, 21, qlen - 21, qlen - 20, qlen - 19, qlen - 1, qlen // 2):
            for w in (20, 7):
                grid.append({"tpos": 1000, "qpos": qpos, "qlen": qlen, "window": w,
                             "range": list(ref.bamlib.get_mismatch_range(1000, qpos, qlen, w))})
    trims = []
    for qlen in (99, 100, 101, 3333, 15000, 15001, 24999):
        for mt in (0.01, 0.0, 0.05):
            a, b = ref.bamlib.get_trimmed_range(qlen, mt)
            trims.append({"qlen": qlen, "min_trim": mt, "start": a, "end": b})
    chunks = {}
    for L in (1000, 200000, 200002, 400002, 1000000, 64444167):
        chunks[str(L)] = [list(t[1:]) for t in ref.util.chunkloci(("c", 0, L))]
    save("leaf_cs", {"cs": out, "mismatch_range": grid, "trim": trims, "chunkloci": chunks})


def boundary_case():
    """Chunk-boundary candidates at tpos == 200000: column seen
    with full counts in the earlier chunk, with reads that end at the boundary
    missing in the later one, and som_seen carried across."""
    ref = H.load_reference()
    rs = random.Random(11)
    L = 400002
    recs = []
    genome = {}

    def refbase(p):
        if p not in genome:
            genome[p] = rs.choice("ACGT")
        return genome[p]

    def mk(tstart, tend, subs, name, bq=93):
        seq = []
        cs = []
        run = 0
        for p in range(tstart, tend):
            rb = refbase(p)
            if p in subs:
                if run:
                    cs.append(":{}".format(run))
                    run = 0
                cs.append("*{}{}".format(rb.lower(), subs[p].lower()))
                seq.append(subs[p])
            else:
                run += 1
                seq.append(rb)
        if run:
            cs.append(":{}".format(run))
        return dict(tstart=tstart, tend=tend, qstart=0, seq="".join(seq), bq=[bq] * len(seq), cs="".join(cs),
                    qname=name)

    def other(b, k=1):
        return "ACGT"[("ACGT".index(b) + k) % 4]

    k = 0
    # site A: rpos 199999 (tpos 200000). 8 reads span it, 4 of them END at 200000
    # (tend == 200000): they are fetched by chunk 0 but not by chunk 1.
    pA = 199999
    for i in range(4):
        recs.append(mk(199000 + 10 * i, 200000, {pA: other(refbase(pA))} if i == 0 else {}, "a{}".format(k))); k += 1
    for i in range(4):
        recs.append(mk(199500 + 10 * i, 200900, {}, "a{}".format(k))); k += 1
    # site B: tpos 400000, het-like column in chunk 1 (dropped as germline there),
    # different column in chunk 2 because three ref reads end at 400000.
    pB = 399999
    altB = other(refbase(pB), 2)
    for i in range(3):
        recs.append(mk(399000 + 7 * i, 400000, {}, "b{}".format(k))); k += 1
    for i in range(3):
        recs.append(mk(399100 + 7 * i, 400001, {pB: altB}, "b{}".format(k))); k += 1
    for i in range(2):
        recs.append(mk(399200 + 7 * i, 400002, {}, "b{}".format(k))); k += 1
    # ordinary candidates inside the chunks
    recs.append(mk(100000, 101500, {100700: other(refbase(100700))}, "c0"))
    for i in range(5):
        recs.append(mk(100100 + i, 101400, {}, "c{}".format(i + 1)))
    recs.sort(key=lambda r: r["tstart"])
    b = batch_from_records("chr3", L, recs)
    bam = "/fake/boundary.bam"
    H.register_bam(bam, {"chr3": b})
    _, c2c = ref.util.load_loci(None, None, {"chr3": L})
    chunks = [(s_, e_) for (_, s_, e_) in c2c["chr3"]]
    ov = dict(min_trim=0.0, min_ref_count=1)
    out, log = H.run_reference_worker(bam, "chr3", chunks, 100, 5000, 52, **ov)
    exp = {"chunks": chunks, "qlen_lower_limit": 100, "qlen_upper_limit": 5000, "md_threshold": 52, "overrides": ov,
           "records": canon_records(out), "log": [int(x) for x in log], "contig": "chr3", "length": L,
           "reads": recs}
    print("    boundary", chunks, [r[:6] for r in out], log)
    save("worker_boundary", exp, batch=b)


def thresholds_case():
    ref = H.load_reference()
    out = []
    for seed, L, depth in ((21, 300000, 8.0), (22, 150000, 16.0)):
        cfg = synth.SynthConfig(seed=seed, contig_len=L, depth=depth, read_len_mean=4000, read_len_sd=900,
                                read_len_min=1000, read_len_max=9000, name="chr9")
        s = synth.generate(cfg)
        bam = "/fake/thr{}.bam".format(seed)
        H.register_bam(bam, {"chr9": s.batch})
        ql, qu, md = ref.bamlib.get_thresholds(bam, ["chr9"], {"chr9": L})
        random.seed(10)
        starts = random.sample(range(L), 100)
        out.append({"cfg": cfg.__dict__, "qlen_lower_limit": ql, "qlen_upper_limit": qu, "md_threshold": md,
                    "first_starts": starts[:5]})
    save("thresholds", {"cases": out})


def header_case():
    ref = H.load_reference()
    b = synth.generate(small_cfg(31)).batch
    bam = "/fake/header.bam"
    H.register_bam(bam, {"chr7": b, "chr10": b, "chr2": b})
    hdr = ref.vcflib.get_himut_vcf_header(
        bam, None, None, None, None, {"chr7": 30000, "chr10": 5, "chr2": 7}, "c.vcf", "p.vcf", 30, 60, 2000, 4100, 0.99,
        20, 93, 0.01, 0, 20, 52, 3, 1, 3, 1, 1 / (10 ** 6), 1 / (10 ** 3), 1 / (10 ** 4), False, False, False, False,
        "1.0.4", "out.vcf")
    hdr_phase = ref.vcflib.get_himut_vcf_header(
        bam, None, "ph.vcf", "chr7", None, {"chr7": 30000}, "c.vcf", "p.vcf", 30, 60, 2000, 4100, 0.99,
        20, 93, 0.01, 0, 20, 52, 3, 1, 3, 4, 1 / (10 ** 6), 1 / (10 ** 3), 1 / (10 ** 4), True, False, False, False,
        "1.0.4", "out.vcf")
    save("vcf_header", {"header": hdr, "header_phase": hdr_phase})


def edges_case(case, cfg, min_bq=20, min_mapq=20, mutate=None):
    """phaselib.get_edges on a synthetic contig and its heterozygous SNPs."""
    s = synth.generate(cfg)
    b = s.batch
    if mutate is not None:
        mutate(b)
    bam = "/fake/{}.bam".format(case)
    H.register_bam(bam, {b.name: b})
    het = s.snp_gt == 1 if hasattr(s, "snp_gt") else None
    hets = [(int(p) + 1, chr(r), chr(a)) for p, r, a, g in zip(s.snp_pos, s.snp_ref, s.snp_alt, s.snp_gt) if g in (1, 2)]
    hets = sorted(set(hets))
    edge_lst, e2c = H.run_reference_edges(bam, b.name, hets, min_bq, min_mapq)
    exp = {"contig": b.name, "hetsnps": [list(h) for h in hets], "min_bq": min_bq, "min_mapq": min_mapq,
           "edge_lst": edge_lst, "edge2counts": e2c}
    print("   ", case, len(hets), "hetSNPs", len(edge_lst), "edges")
    save(case, exp, batch=b)


def _flat_edges(edge_lst, e2c):
    """[i, j, c0, c1, c2, c3, ...] in edge order: a result of run_reference_edges, compactly."""
    out = []
    for i, j in edge_lst:
        out.extend([int(i), int(j)] + [int(x) for x in e2c["{},{}".format(i, j)]])
    return out


def edges_hand_case(case, built, params):
    """phaselib.get_edges on a hand-built batch of tests/edges_cases.py, once per (min_bq, min_mapq) of ``params``: all
    runs go into one fixture, each as a flat integer list."""
    from tests import edges_cases as C
    b = C.batch_of(built)
    bam = "/fake/{}.bam".format(case)
    H.register_bam(bam, {b.name: b})
    hets = [tuple(h) for h in built.hets]
    runs = []
    for min_bq, min_mapq in params:
        edge_lst, e2c = H.run_reference_edges(bam, b.name, hets, min_bq, min_mapq)
        runs.append({"min_bq": min_bq, "min_mapq": min_mapq, "edges": _flat_edges(edge_lst, e2c)})
    exp = {"contig": b.name, "length": b.length, "hetsnps": [list(h) for h in hets], "runs": runs}
    with open(os.path.join(HERE, case + ".json"), "w") as o:
        json.dump(exp, o, sort_keys=True, separators=(",", ":"))
        o.write("\n")
    d = b.to_npz_dict()
    d["refseq"] = np.frombuffer(built.ref.encode("ascii"), np.uint8)
    np.savez_compressed(os.path.join(HERE, case + ".npz"), **d)
    print("   ", case, b.n, "reads", len(hets), "hetSNPs", [len(r["edges"]) // 6 for r in runs], "edges")


CALLABLE_CRC_ARRAYS = ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "qid", "qoff", "cs_off", "seq", "bq", "cs", "tp")


def callable_hand_case(case="callable_cases"):
    """normcounts.update_tri2count of the reference on the hand-built reads of tests/callable_cases.py: once per read (a
    BAM object over the harness's stand-in for a pysam record) with a fresh rpos2count, at every parameter set of the
    read's case.  Stored per (case, parameter set, read), in that order: the counted reference positions of [tstart,
    tend) as packed bits, all in one byte array; the inputs are the builders' (the JSON holds checksums of their
    arrays).  The archive is written with fixed time stamps, so that a rerun gives the same bytes."""
    import io
    import zipfile
    import zlib
    from collections import defaultdict
    from tests import callable_cases as C
    ref = H.load_reference()
    import himut.normcounts as N
    exp = {"contig": C.CONTIG, "order": list(C.FIXTURE_CASES), "cases": {}}
    packed = []
    for name in C.FIXTURE_CASES:
        built = C.build(name)
        b = C.batch_of(built)
        reads = H._reads_of(b)
        keep = [i for i, r in enumerate(built.records) if C.in_fixture(name, r)]
        for ov in built.params:
            p = C.params_of(ov)
            for i in keep:
                ccs = ref.bamlib.BAM(reads[i])
                rpos2count = defaultdict(lambda: 0)
                N.update_tri2count(ccs, p["min_bq"], p["min_trim"], p["mismatch_window_size"], p["max_mismatch_count"],
                                   rpos2count)
                ts, te = int(b.tstart[i]), int(b.tend[i])
                bits = np.zeros(te - ts, np.uint8)
                for rpos, n in rpos2count.items():
                    assert n == 1 and ts <= rpos < te, (name, i, rpos, n)
                    bits[rpos - ts] = 1
                packed.append(np.packbits(bits))
        exp["cases"][name] = {"reads": [built.records[i]["qname"] for i in keep], "params": built.params,
                              "crc32": {k: zlib.crc32(np.ascontiguousarray(getattr(b, k)).view(np.uint8).tobytes())
                                        for k in CALLABLE_CRC_ARRAYS}}
    counted = np.concatenate(packed)
    with open(os.path.join(HERE, case + ".json"), "w") as o:
        json.dump(exp, o, sort_keys=True, separators=(",", ":"))
        o.write("\n")
    buf = io.BytesIO()
    np.lib.format.write_array(buf, counted, allow_pickle=False)
    with zipfile.ZipFile(os.path.join(HERE, case + ".npz"), "w", zipfile.ZIP_DEFLATED) as z:
        info = zipfile.ZipInfo("counted.npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        info.external_attr = 0o644 << 16
        z.writestr(info, buf.getvalue())
    print("   ", case, len(packed), "read runs", counted.shape[0], "bytes of bits")


def phase_edges_case(case="phase_edges"):
    """The call worker and the normcounts worker, both under --phase, on every hand-built case of tests/phase_cases.py.
    Stored per case: the canonical record tuples, the call log, the two trinucleotide tables (non-zero entries) and the
    normcounts log; the inputs are rebuilt from the builders."""
    from tests import phase_cases as C
    exp = {"contig": C.CONTIG, "order": [c.name for c in C.CASES], "cases": {}}
    for c in C.CASES:
        bam = "/fake/{}.{}.bam".format(case, c.name)
        H.register_bam(bam, {c.batch.name: c.batch})
        p = C.params_of(c)
        ov = {k: v for k, v in p.items() if k in H.CALL_DEFAULTS}
        recs, log = H.run_reference_worker(bam, c.batch.name, c.chunks, p["qlen_lower_limit"], p["qlen_upper_limit"],
                                           p["md_threshold"], phase=True, phase_sets=c.phase_sets, **ov)
        ccs, rf, nlog, order = H.run_reference_normcounts(bam, c.batch.name, c.refseq, c.chunks, p["qlen_lower_limit"],
                                                          p["qlen_upper_limit"], p["md_threshold"],
                                                          phase_sets=c.phase_sets, **ov)
        exp["cases"][c.name] = {"records": canon_records(recs), "log": [int(x) for x in log],
                                "ccs_tri2count": {k: int(v) for k, v in sorted(ccs.items()) if v},
                                "ref_tri2count": {k: int(v) for k, v in sorted(rf.items()) if v},
                                "norm_log": [int(x) for x in nlog], "alt_order": order}
        del H._FAKE_BAMS[bam]
    with open(os.path.join(HERE, case + ".json"), "w") as o:
        json.dump(exp, o, sort_keys=True, separators=(",", ":"))
        o.write("\n")
    from collections import Counter
    print("   ", case, len(C.CASES), "cases", dict(Counter(r[3] for e in exp["cases"].values() for r in e["records"])))


def write_unphased_vcf(path, s, other_contig="chrOther"):
    """A germline VCF as `himut phase` reads it: the sample's SNPs with unphased genotypes (0/1 for the
    heterozygous ones), plus records the phaser must skip (1/1, a failed filter, an indel, a tri-allelic site,
    hetSNPs of another contig)."""
    name = s.batch.name
    rows = []
    for k, (p, r, a, g) in enumerate(zip(s.snp_pos, s.snp_ref, s.snp_alt, s.snp_gt)):
        gt = "0/1" if g in (1, 2) else "1/1"
        if g in (1, 2) and k % 7 == 3:
            gt = "1/0"
        flt = "q5" if k % 23 == 11 else "PASS"
        rows.append((int(p) + 1, "{}\t{}\t.\t{}\t{}\t{}\t{}\t.\tGT:GQ:DP\t{}:{}:{}".format(
            name, int(p) + 1, chr(r), chr(a), 30 + k % 20 if k % 5 else ".", flt, gt, 20 + k % 50, 25 + k % 11)))
    first = int(s.snp_pos[0]) + 1
    rows.append((first + 1, "{}\t{}\t.\tAC\tA\t40\tPASS\t.\tGT:GQ:DP\t0/1:30:31".format(name, first + 1)))
    rows.append((first + 2, "{}\t{}\t.\tA\tC,G\t40\tPASS\t.\tGT:GQ:DP\t1/2:30:31".format(name, first + 2)))
    rows.sort()
    with open(path, "w") as o:
        o.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsyn\n")
        for _, line in rows:
            o.write(line + "\n")
        o.write("{}\t777\t.\tA\tG\t50\tPASS\t.\tGT:GQ:DP\t0/1:40:30\n".format(other_contig))


def phase_case(case, cfg, min_bq=20, min_mapq=20, min_p_value=0.0001, min_phase_proportion=0.2, tmpdir="/tmp"):
    """`himut phase` on one synthetic contig: haplotype blocks, statistics and the phased VCF."""
    s = synth.generate(cfg)
    b = s.batch
    bam = "/fake/{}.bam".format(case)
    H.register_bam(bam, {b.name: b})
    vcf = os.path.join(tmpdir, case + ".germline.vcf")
    write_unphased_vcf(vcf, s)
    out = os.path.join(tmpdir, case + ".phased.vcf")
    sizes = {b.name: b.length, "chrOther": 1000}
    blocks, stats, text = H.run_reference_phase(bam, b.name, b.length, vcf, min_bq, min_mapq, min_p_value,
                                                min_phase_proportion, out, sizes)
    ref = H.load_reference()
    hb, hp, hs, c2c = ref.vcflib.load_phased_hetsnps(out, [b.name], sizes)
    exp = {"contig": b.name, "length": b.length, "sizes": sizes, "vcf_text": open(vcf).read(), "min_bq": min_bq,
           "min_mapq": min_mapq, "min_p_value": min_p_value, "min_phase_proportion": min_phase_proportion,
           "hblock_lst": blocks, "statistics": stats,
           "phased_vcf_text": text.replace(tmpdir + "/", "").replace(bam, "in.bam"),
           "phase_chunks": [[int(x) for x in c[1:]] for c in c2c[b.name]]}
    print("   ", case, len(blocks), "blocks", stats)
    save(case, exp, batch=b)


def germline_priors_case(tmpdir="/tmp"):
    """vcflib.get_germline_priors / load_germline_counts / util.get_truncated_float (the --non_human_sample priors)."""
    ref = H.load_reference_norm_host()
    rs = np.random.RandomState(5)
    fa = os.path.join(tmpdir, "gp.fa")
    sizes = {"chrA": 120_000, "chrB": 45_000, "chrC": 9_000}
    with open(fa, "w") as o:
        for name, L in sizes.items():
            seq = "".join("ACGT"[i] for i in rs.randint(0, 4, L))
            o.write(">{} some description\n".format(name))
            for k in range(0, L, 70):
                o.write(seq[k:k + 70] + "\n")
    vcf = os.path.join(tmpdir, "gp.germline.vcf")
    rows = []
    for name, L in sizes.items():
        for k in range(int(L * 2e-3)):
            pos = int(rs.randint(1, L))
            kind = rs.rand()
            gt = ["0/1", "1/1", "1/0", "0|1", "1/2"][int(rs.choice(5, p=[0.5, 0.3, 0.08, 0.07, 0.05]))]
            flt = "PASS" if rs.rand() < 0.9 else "RefCall"
            if kind < 0.75:
                r_, a_ = "ACGT"[rs.randint(4)], "ACGT"[rs.randint(4)]
            elif kind < 0.85:
                r_, a_ = "A" + "C" * int(rs.randint(1, 4)), "A"
            elif kind < 0.95:
                r_, a_ = "G", "G" + "T" * int(rs.randint(1, 4))
            elif kind < 0.98:
                r_, a_ = "AC", "GT"
            else:
                r_, a_ = "A", "C,G"
            rows.append((name, pos, r_, a_, flt, gt))
    rows.sort()
    with open(vcf, "w") as o:
        o.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsyn\n")
        for name, pos, r_, a_, flt, gt in rows:
            o.write("{}\t{}\t.\t{}\t{}\t33\t{}\t.\tGT:GQ\t{}:30\n".format(name, pos, r_, a_, flt, gt))
    exp = {"fasta_text": open(fa).read(), "vcf_text": open(vcf).read(), "cases": []}
    for chroms in (["chrA"], ["chrA", "chrB"], ["chrB", "chrC"], ["chrC"]):
        for refsample in (False, True):
            counts = ref.vcflib.load_germline_counts(vcf, chroms)
            try:
                pri = [float(x) for x in ref.vcflib.get_germline_priors(chroms, fa, vcf, refsample)]
            except (ValueError, IndexError) as e:       # a frequency of 0 (or >= 0.05) has no truncation
                pri = type(e).__name__
            exp["cases"].append({"chrom_lst": chroms, "reference_sample": refsample, "counts": [int(c) for c in counts],
                                 "priors": pri})
    core = H.load_reference()
    exp["truncated"] = [[f, core.util.get_truncated_float(f)] for f in
                        (0.0012345, 0.00099, 0.0409, 1e-6, 3.3e-5, 0.0005, 0.00149, 7.5e-9, 0.0449)]
    save("germline_priors", exp)


def norm_host_case(tmpdir="/tmp"):
    """The host side of `himut normcounts` around the worker: thresholds from the SBS file's header, SBS96 counts,
    genome trinucleotide counts, the output table and norm.log, the command line."""
    ref = H.load_reference()
    NH = H.load_reference_norm_host()
    cfg = small_cfg(301, contig_len=30000, name="chr9", som_rate=4e-4)
    s = synth.generate(cfg, want_ref=True)
    b = s.batch
    seq = list(bytes(s.ref).decode())
    seq[100:140] = ["N"] * 40
    seq[5000:5020] = [c.lower() for c in seq[5000:5020]]
    seq = "".join(seq)
    fa = os.path.join(tmpdir, "norm_host.fa")
    with open(fa, "w") as o:
        o.write(">chr9 test\n")
        for i in range(0, len(seq), 60):
            o.write(seq[i:i + 60] + "\n")
    bam = "/fake/norm_host.bam"
    H.register_bam(bam, {b.name: b})
    sizes = {b.name: b.length}
    ql, qu, md = thresholds_of(ref, bam, [b.name], sizes)
    _, c2c = ref.util.load_loci(None, None, sizes)
    chunks = [(s_, e_) for (_, s_, e_) in c2c[b.name]]
    recs, _ = H.run_reference_worker(bam, b.name, chunks, ql, qu, md)
    args = dict(H.CALL_DEFAULTS)
    header = ref.vcflib.get_himut_vcf_header(
        bam, None, None, None, None, sizes, "common.vcf", "pon.vcf", args["min_qv"], args["min_mapq"], ql, qu,
        args["min_sequence_identity"], args["min_gq"], args["min_bq"], args["min_trim"], args["max_mismatch_count"],
        args["mismatch_window_size"], md, args["min_ref_count"], args["min_alt_count"], args["min_hap_count"], 1,
        args["somatic_snv_prior"], args["germline_snv_prior"], args["germline_indel_prior"], False, False, False, False,
        "1.0.4", os.path.join(tmpdir, "norm_host.vcf"))
    sbs = os.path.join(tmpdir, "norm_host.vcf")
    cwd = os.getcwd()
    os.chdir(tmpdir)
    try:
        ref.vcflib.dump_sbs(sbs, header, [b.name], {b.name: recs})
        exp = {"contig": b.name, "fasta_text": open(fa).read(), "sbs_vcf_text": open(sbs).read()}
        exp["thresholds"] = list(NH.vcflib.get_thresholds(sbs))
        exp["sbs96_counts"] = NH.mutlib.load_sbs96_counts(sbs, fa, [b.name])
        d = {}
        NH.reflib.get_chrom_tricount(b.name, seq, d)
        exp["chrom_tricount"] = {k: int(v) for k, v in d[b.name].items() if k in NH.mutlib.tri_lst}
        ccs, rf, log, order = H.run_reference_normcounts(bam, b.name, seq, chunks, ql, qu, md)
        ref_tri2count = {t: d[b.name][t] for t in NH.mutlib.tri_lst}
        out = os.path.join(tmpdir, "norm_host.tsv")
        cmd = NH.mutlib.get_normcounts_cmdline(bam, fa, sbs, None, None, 30, 60, 0.99, 20, 93, 0.01, 20, 0, 3, 1, 3,
                                               "common.vcf", "pon.vcf", 1e-6, 1e-3, 1e-4, 4, False, False, False, out)
        NH.mutlib.dump_normcounts(exp["sbs96_counts"], ref_tri2count, {b.name: rf}, {b.name: ccs}, cmd, out)
        NH.mutlib.dump_norm_log([b.name], {b.name: log})
        exp["cmdline"] = cmd
        exp["cmdline_phase"] = NH.mutlib.get_normcounts_cmdline(bam, fa, sbs, "g.vcf", "p.vcf", 30, 60, 0.99, 20, 93,
                                                                0.01, 20, 0, 3, 1, 3, "c.vcf", "n.vcf", 1e-6, 1e-3,
                                                                1e-4, 2, True, False, False, out)
        exp["cmdline_nonhuman"] = NH.mutlib.get_normcounts_cmdline(bam, fa, sbs, "g.vcf", "p.vcf", 30, 60, 0.99, 20,
                                                                   93, 0.01, 20, 0, 3, 1, 3, None, None, 1e-6, 1e-3,
                                                                   1e-4, 2, True, True, True, out)
        exp["normcounts_tsv"] = open(out).read()
        exp["norm_log_text"] = open("norm.log").read()
        exp["ccs_tri2count"] = {k: int(v) for k, v in ccs.items()}
        exp["ref_tri2count"] = {k: int(v) for k, v in rf.items()}
        exp["log"] = [int(x) for x in log]
        exp["bam"] = bam
        exp["out"] = out
        exp["fa"] = fa
        exp["sbs"] = sbs
    finally:
        os.chdir(cwd)
    save("norm_host", exp)


def main():
    only = set(sys.argv[1:])

    def want(name):
        return not only or name in only

    if only == {"norm_order_part"}:        # one hash-seed variant of norm_order (norm_order_case runs these)
        norm_order_part()
        return
    if want("leaf_gtlib"):
        leaf_gtlib()
    if want("gt_edges"):
        gt_edges()
    if want("leaf_cs"):
        leaf_cs()
    if want("thresholds"):
        thresholds_case()
    if want("vcf_header"):
        header_case()
    if want("worker_basic"):
        worker_case("worker_basic", small_cfg(101), md_threshold=52)
    if want("worker_sets"):
        worker_case("worker_sets", small_cfg(102, name="chr12", som_rate=2e-4), with_sets=True, md_threshold=52)
    if want("worker_dense"):
        # many coincidences: every filter status shows up
        worker_case("worker_dense",
                    small_cfg(103, contig_len=6000, read_len_mean=700, read_len_sd=150, read_len_min=300,
                              read_len_max=1500, depth=40.0, snp_rate=1.5e-2, sub_rate=4e-3, ins_rate=1e-3,
                              del_rate=1e-3, som_rate=0.0, frac_noisy=0.0, bq93_prob=0.7, frac_softclip=0.3,
                              softclip_max=40, hetalt_frac=0.15, het_frac=0.55, name="chrD"),
                    overrides=dict(min_sequence_identity=0.9, max_mismatch_count=3, min_trim=0.0), md_threshold=45,
                    qlen_limits=(350, 1300))
    if want("worker_dense_sets"):
        worker_case("worker_dense_sets",
                    small_cfg(104, contig_len=6000, read_len_mean=700, read_len_sd=150, read_len_min=300,
                              read_len_max=1500, depth=35.0, snp_rate=1.5e-2, sub_rate=4e-3, ins_rate=5e-4,
                              del_rate=5e-4, som_rate=0.0, frac_noisy=0.0, bq93_prob=0.8, hetalt_frac=0.1, het_frac=0.6,
                              name="chrE"),
                    overrides=dict(min_sequence_identity=0.9, max_mismatch_count=2, min_alt_count=2, min_ref_count=5),
                    md_threshold=44,
                    qlen_limits=(350, 1300), with_sets=True)
    if want("worker_longcs"):
        worker_case("worker_longcs", small_cfg(105, contig_len=12000, cs_long=True, name="chrL"), md_threshold=52)
    if want("worker_phase"):
        worker_case("worker_phase", small_cfg(106, contig_len=40000, snp_rate=3e-3, som_rate=3e-4, name="chr5"),
                    phase_block=25, md_threshold=52)
    if want("worker_phase_dense"):
        worker_case("worker_phase_dense",
                    small_cfg(107, contig_len=8000, read_len_mean=900, read_len_sd=150, read_len_min=400,
                              read_len_max=1600, depth=40.0, snp_rate=1.2e-2, sub_rate=3e-3, ins_rate=8e-4,
                              del_rate=8e-4, frac_noisy=0.0, name="chrP"),
                    overrides=dict(min_sequence_identity=0.9, max_mismatch_count=3, min_hap_count=2),
                    qlen_limits=(400, 1500), phase_block=12, md_threshold=70)
    if want("worker_flags"):
        def mutate(b):
            rs = np.random.RandomState(7)
            idx = rs.choice(b.n, 24, replace=False)
            b.flag[idx[:8]] |= 0x100      # secondary: skipped (bamlib.py:17)
            b.flag[idx[8:16]] |= 0x800    # supplementary: kept
            for k in range(16, 24, 2):    # shared query names (supplementary pairs)
                i, j = sorted((int(idx[k]), int(idx[k + 1])))
                b.qid[j] = b.qid[i]
        worker_case("worker_flags", small_cfg(108, contig_len=20000, name="chrF", som_rate=2e-4), md_threshold=52,
                    mutate=mutate)
    if want("germline_priors"):
        germline_priors_case()
    if want("phase_blocks"):
        phase_case("phase_blocks", small_cfg(131, contig_len=60000, snp_rate=3e-3, name="chr9"))
    if want("phase_sparse"):
        # few reads per edge: most edges fail the binomial test, blocks break up, conflicting evidence appears
        phase_case("phase_sparse", small_cfg(132, contig_len=50000, depth=9.0, snp_rate=4e-3, sub_rate=3e-3, name="chr4"),
                   min_p_value=0.05, min_phase_proportion=0.1)
    if want("worker_pon_params"):
        # the thresholds --create_panel_of_normals switches to (util.py:44-63)
        worker_case("worker_pon_params", small_cfg(109, contig_len=20000, name="chrN", som_rate=2e-4), md_threshold=52,
                    overrides=dict(min_bq=20, min_gq=10, min_qv=20, min_trim=0, min_mapq=30, min_hap_count=0,
                                   min_sequence_identity=0.8), create_pon=True)
    if want("edges_basic"):
        edges_case("edges_basic", small_cfg(401, contig_len=40000, snp_rate=4e-3, name="chr6"))
    if want("edges_lowq"):
        def lowmapq(b):
            b.mapq[::5] = 10
        edges_case("edges_lowq", small_cfg(402, contig_len=30000, snp_rate=6e-3, name="chr8", del_rate=2e-3, ins_rate=1e-3),
                   min_bq=93, min_mapq=60, mutate=lowmapq)
    if want("edges_blocks"):
        from tests import edges_cases as C
        edges_hand_case("edges_blocks", C.blocks(C.BLOCKS_FIXTURE_K), [C.BLOCKS_PARAMS])
    if want("edges_rules"):
        from tests import edges_cases as C
        edges_hand_case("edges_rules", C.rules(), [(q, m) for q in C.RULES_MIN_BQ for m in C.RULES_MIN_MAPQ])
    if want("callable_cases"):
        callable_hand_case()
    if want("phase_edges"):
        phase_edges_case()
    if want("norm_host"):
        norm_host_case()
    if want("norm_basic"):
        norm_case("norm_basic", small_cfg(201, contig_len=40000, name="chrA"), md_threshold=52)
    if want("norm_sets"):
        norm_case("norm_sets", small_cfg(202, contig_len=40000, name="chr7", som_rate=3e-4, snp_rate=3e-3),
                  with_sets=True, md_threshold=52, chunks=[(1, 15000), (15000, 30000), (30000, 39998)])
    if want("norm_dense"):
        # deep pile, noisy reads, relaxed filters: every branch of the position loop fires
        norm_case("norm_dense", small_cfg(203, contig_len=20000, depth=70.0, name="chrD", som_rate=1e-3, snp_rate=4e-3,
                                          sub_rate=2e-3, ins_rate=5e-4, del_rate=5e-4),
                  with_sets=True, md_threshold=60,
                  overrides=dict(min_bq=40, min_gq=70, max_mismatch_count=2, mismatch_window_size=15, min_ref_count=5,
                                 min_alt_count=2, min_sequence_identity=0.95))
    if want("norm_phase"):
        norm_case("norm_phase", small_cfg(205, contig_len=40000, snp_rate=3e-3, som_rate=3e-4, name="chr5"),
                  md_threshold=52, phase_block=12, with_sets=True)
    if want("norm_nsub"):
        # cs substitutions with an 'n' reference base against a FASTA that holds a real base there
        norm_case("norm_nsub", small_cfg(207, contig_len=30000, name="chrN", sub_rate=1.5e-3, read_len_mean=1800, read_len_sd=500,
                                         read_len_min=700), md_threshold=60, mutate_batch=nsub_batch,
                  overrides=dict(max_mismatch_count=1, mismatch_window_size=20, min_trim=0.005))
    if want("norm_order"):
        norm_order_case()
    if want("worker_phase_dup"):
        worker_case("worker_phase_dup", small_cfg(111, contig_len=60000, snp_rate=3e-3, som_rate=4e-4, name="chr5"),
                    phase_block=15, mutate=dup_names_batch, md_threshold=200)
    if want("norm_softmask"):
        # lower-case (soft-masked) and N stretches in the reference: skipped positions, odd trinucleotide keys
        def mask(seq):
            t = list(seq)
            for a, z in ((3000, 3400), (9000, 9100), (15000, 15002)):
                t[a:z] = [c.lower() for c in t[a:z]]
            for a, z in ((5000, 5050), (12000, 12001)):
                t[a:z] = ["N"] * (z - a)
            return "".join(t)
        norm_case("norm_softmask", small_cfg(204, contig_len=20000, name="chrM"), md_threshold=52, mutate_ref=mask)
    if want("worker_boundary"):
        boundary_case()
    if want("worker_insins") or want("norm_insins"):
        def split_insertions(b):
            """every other insertion of two or more bases becomes two insertion operations in a row (+acg -> +a+cg): the
            tokenizer (cslib.py:7-10) splits them, cs2tuple (:13-44) emits two state-3 tuples, the pile counts two insertions
            at the position and the mismatch list holds two entries"""
            import re
            out, offs, k = [], [0], 0
            for i in range(b.n):
                cs = bytes(b.cs[b.cs_off[i]:b.cs_off[i + 1]]).decode()
                def rep(m):
                    nonlocal k
                    k += 1
                    return "+" + m.group(1)[0] + "+" + m.group(1)[1:] if k & 1 else m.group(0)
                cs = re.sub(r"\+([a-z]{2,})", rep, cs)
                out.append(cs.encode())
                offs.append(offs[-1] + len(cs))
            b.cs = np.frombuffer(b"".join(out), np.uint8).copy()
            b.cs_off = np.array(offs, np.int64)
        cfg = dict(contig_len=30000, ins_rate=2e-3, del_rate=5e-4, sub_rate=1e-3, som_rate=3e-4, frac_noisy=0.0)
        if want("worker_insins"):
            worker_case("worker_insins", small_cfg(131, name="chrI", **cfg), md_threshold=52, mutate=split_insertions,
                        overrides=dict(min_sequence_identity=0.9, max_mismatch_count=2, mismatch_window_size=12))
        if want("norm_insins"):
            norm_case("norm_insins", small_cfg(132, name="chrJ", **cfg), md_threshold=52, mutate_batch=split_insertions,
                      overrides=dict(min_sequence_identity=0.9, max_mismatch_count=2, mismatch_window_size=12))


if __name__ == "__main__":
    main()
