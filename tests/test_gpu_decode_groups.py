"""The grouped cs decode (k_parse_cs: one wave per group of consecutive reads) against the per-read path of the same
kernel, the CPU oracle and itself on a reused context.  The inputs are tests/decode_cases.py's.

The oracle half of the error cases (test_oracle_raises_too) runs without a GPU.  The reference never compares a tag's
reference span with tend outside a phased run; there a tend past the span leaves a hetSNP under the read that its tag
does not cover (KeyError in tpos2qbase, haplib.py:51), so the cs/tend case is a phased run on both sides."""
import functools

import numpy as np
import pytest

from himut_amd import caller, normcounts, synth, vcflib
from himut_amd._ffi import HimutError
from tests import decode_cases as DC
from tests import util

PARAMS = dict(util.CALL_DEFAULTS, qlen_lower_limit=30, qlen_upper_limit=250, md_threshold=400, min_sequence_identity=0.9,
              min_bq=20, min_ref_count=0)
WIDE = dict(PARAMS, qlen_upper_limit=5000)


def _configure(w, p, phase=False):
    w.configure(p["min_qv"], p["min_mapq"], p["qlen_lower_limit"], p["qlen_upper_limit"], p["min_sequence_identity"], p["min_gq"],
                p["min_bq"], p["min_trim"], p["max_mismatch_count"], p["mismatch_window_size"], p["md_threshold"], p["min_ref_count"],
                p["min_alt_count"], p["min_hap_count"], p["germline_snv_prior"], phase)


def read_pass(batch, mode, p, w=None):
    """(records, log, copied-out read pass) of a call run over the whole contig, in a fresh context unless one is given."""
    own = w is None
    if own:
        w = caller.Worker(0)
        w.ctx.debug_decode(mode)
    try:
        _configure(w, p)
        recs, log = w.call_contig(batch, [(1, batch.length)])
        return recs, log, w.ctx.read_pass()
    finally:
        if own:
            w.close()


def check_both_modes(batch, p, what):
    r0, l0, a = read_pass(batch, 0, p)
    r1, l1, b = read_pass(batch, 1, p)
    DC.assert_same_read_pass(batch, a, b, what)
    assert l0 == l1 and np.array_equal(r0, r1), what
    # the grouped path ran: the counters are the plan's, nothing was redone
    assert a["counters"] == DC.plan_counters(batch) + [0], (what, a["counters"])
    assert b["counters"] == DC.plan_counters(batch, 1) + [0], (what, b["counters"])
    want = DC.exact_marks(batch, b, p)
    got0, got1 = DC.bits_set(a["bits"]), DC.bits_set(b["bits"])
    over = any(int(b["nmis"][r]) > DC.MARK_CAP for r in range(batch.n))
    if not over:
        assert got0 == got1 == want, what
    else:                                    # the per-read path may set a long read's bits before it knows the identity
        assert want <= got0 and want <= got1, what
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DC.trap_batches()))
def test_trap_grouped_equals_per_read(name):
    recs, ref = DC.trap_batches()[name]
    batch = DC.batch_of(recs, ref)
    a = check_both_modes(batch, PARAMS, name)
    if batch.n > 1:
        assert a["counters"][1] > 0, name
    if name == "secondary_in_group":         # never validated: RF_SECONDARY and zeros
        assert a["rflag"][1] == 1 and a["nseg"][1] == 0 and a["nmis"][1] == 0 and a["nnsub"][1] == 0
    if name == "n_reference":
        assert list(a["nnsub"]) == [0, 3, 1, 0] and list(a["nmis"]) == [1, 1, 0, 1]
    if name == "long_form_per_read":
        assert [int(f) & 8 for f in a["rflag"]] == [0, 8, 0, 8]
    if name == "double_insertion":           # one more mismatch entry, no segment of its own
        assert a["nmis"][1] == 2 and a["nseg"][1] == 2
    if name == "filters_per_read":           # marks only from the reads that pass
        got = DC.bits_set(a["bits"])
        assert got == set(int(batch.tstart[r]) + 40 for r in (0, 2, 4, 6)), got
    if name == "text_of_1024":
        assert int(batch.cs_off[5]) == 1024 and DC.plan_groups(batch.cs_off)[0] == (0, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(10))
def test_random_batches_grouped_equals_per_read(block):
    multi = 0
    for seed in range(20 * block, 20 * block + 20):
        batch, _ = DC.random_batch(1000 + seed, n_reads=None if seed % 4 else 40)
        a = check_both_modes(batch, WIDE, "seed {}".format(1000 + seed))
        multi += a["counters"][1]
    assert multi > 0


def test_random_batches_share_groups():
    """The random batches put 1-12 and more reads into a group (no GPU: the plan's model)."""
    sizes = []
    for seed in range(0, 200, 10):
        batch, _ = DC.random_batch(1000 + seed)
        sizes += [b - a for a, b in DC.plan_groups(batch.cs_off)]
    assert min(sizes) == 1 and max(sizes) >= 12 and sum(1 for s in sizes if 2 <= s <= 12) > 50


# ---- errors: each kind in the first, a middle and the last read of one group

def _error_batch(kind, idx):
    """(batch, phase sets or None): five reads of one group, read idx broken."""
    rng = np.random.default_rng(5)
    ref = DC.reference(rng, 5000)
    recs = [DC._short(ref, rng, 100 + 10 * i) for i in range(5)]       # ":40*xy:30" each
    r = recs[idx]
    phase = None
    if kind == "bad_byte":
        r["cs"] = r["cs"][:2] + "!" + r["cs"][3:]
    elif kind == "non_acgt_base":
        r["cs"] = r["cs"][:5] + "n" + r["cs"][6:]
    elif kind == "empty_tag":                # ZeroDivisionError in the reference; two heads on one byte, or a head at the text's end
        r["cs"] = ""
    elif kind == "head_not_start":           # "40*xy:30": absorbed into the previous read's ":30" unless the head is checked
        r["cs"] = r["cs"][1:]
    elif kind == "alt_vs_seq":               # the base cs names for the substitution is not the base SEQ holds
        alt = r["seq"][40]
        r["seq"] = r["seq"][:40] + [c for c in "ACGT" if c not in (alt, ref[r["tstart"] + 40])][0] + r["seq"][41:]
    elif kind == "seq":                      # the tag walks past the end of SEQ
        r["seq"], r["bq"] = r["seq"][:-10], r["bq"][:-10]
    elif kind == "tend":                     # tend 300 past the tag's span, and a hetSNP of the read's phase set out there
        r["tend"] += 300
        hpos = [150, r["tstart"] + 201]
        phase = ({"1": ["0", "0"]}, {"1": hpos}, {"1": [(q, ref[q - 1], DC._OTHER[ref[q - 1]][0]) for q in hpos]})
    batch = DC.batch_of(recs, ref)
    assert DC.plan_groups(batch.cs_off) == [(0, 5)]
    return batch, phase


ERROR_KINDS = {"bad_byte": 3, "non_acgt_base": 4, "seq": 3, "tend": 3, "empty_tag": 3, "head_not_start": 3,
               "alt_vs_seq": 3}              # HIMUT_ERR_CS, HIMUT_ERR_BASE
# No oracle half for two kinds.  The reference takes a substitution's base from cs and never looks at SEQ there (DESIGN
# section 5).  For an empty tag the reference divides 0 by 0 (bamlib.py:62); the oracle's restatement computes the identity
# in C doubles, gets a NaN that passes the filter, and goes on: it does not restate that exception.
ORACLE_KINDS = sorted(k for k in ERROR_KINDS if k not in ("alt_vs_seq", "empty_tag"))


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 2, 4])
@pytest.mark.parametrize("kind", sorted(ERROR_KINDS))
def test_errors_same_code_in_both_modes(kind, idx):
    batch, phase = _error_batch(kind, idx)
    codes = []
    for mode in (0, 1):
        w = caller.Worker(0)
        try:
            w.ctx.debug_decode(mode)
            _configure(w, WIDE, phase is not None)
            with pytest.raises(HimutError) as e:
                w.call_contig(batch, [(1, batch.length)], None, None, phase)
            codes.append(e.value.code)
            counters = w.ctx.read_pass()["counters"]
            assert counters == ([1, 1, 0, 5] if mode == 0 else [5, 0, 5, 0])     # the whole group was taken read by read
        finally:
            w.close()
    assert codes == [ERROR_KINDS[kind]] * 2


@pytest.mark.parametrize("idx", [0, 2, 4])
@pytest.mark.parametrize("kind", ORACLE_KINDS)
def test_oracle_raises_too(kind, idx):
    from oracle import oracle as O
    batch, phase = _error_batch(kind, idx)
    with pytest.raises(O.OracleError):
        O.call(batch, [(1, 5000)], WIDE, WIDE["germline_snv_prior"], None, None, phase)


# ---- whole pipelines on one mixed batch, with and without phase sets

@functools.lru_cache(maxsize=None)
def _mixed():
    """A small contig of short, noisy reads from the generator: groups of one to a dozen reads, long reads between short
    ones, soft clips, reads that fail mapq, the length limits or the identity beside reads that pass, in long form too."""
    cfg = synth.SynthConfig(seed=77, contig_len=40_000, depth=25.0, read_len_mean=700.0, read_len_sd=500.0, read_len_min=60,
                            read_len_max=2000, sub_rate=2e-3, ins_rate=2e-3, del_rate=2e-3, som_rate=3e-4, snp_rate=3e-3,
                            frac_noisy=0.1, noisy_mult=20.0, frac_lowmapq=0.1, frac_lowbq=0.05, frac_softclip=0.3, softclip_max=40,
                            name="chrM1")
    return synth.generate(cfg, want_ref=True)


def _phase_sets(s, tmp_path):
    pv = str(tmp_path / "p.vcf")
    synth.write_phased_vcf(pv, s, block=8)
    b = s.batch
    hb, hp, hs, c2c = vcflib.load_phased_hetsnps(pv, [b.name], {b.name: b.length})
    return (dict(hb[b.name]), dict(hp[b.name]), dict(hs[b.name])), [(c[1], c[2]) for c in c2c[b.name]]


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [False, True])
def test_pipelines_against_oracle(phase, tmp_path):
    from oracle import oracle as O
    s = _mixed()
    b = s.batch
    sizes = [y - x for x, y in DC.plan_groups(b.cs_off)]
    assert max(sizes) >= 6 and sizes.count(1) > 0 and DC.plan_counters(b)[1] > 20
    p = dict(util.CALL_DEFAULTS, qlen_lower_limit=100, qlen_upper_limit=1800, md_threshold=400)
    phase_sets, chunks = _phase_sets(s, tmp_path) if phase else (None, [(1, 15_000), (15_000, b.length)])
    w = caller.Worker(0)
    try:
        w.ctx.debug_decode(0)
        _configure(w, p, phase)
        orecs, olog = O.call(b, chunks, p, p["germline_snv_prior"], None, None, phase_sets)
        hrecs, hlog = w.call_contig(b, chunks, None, None, phase_sets)
        c = w.ctx.read_pass()["counters"]
        assert c == DC.plan_counters(b) + [0] and c[1] > 0
        assert hlog == olog and len(hrecs) == len(orecs) > 0
        for k in ("tpos", "chunk", "phase_set", "gq", "ref", "alt", "gt0", "gt1", "status", "gt_state", "counts", "bqsum"):
            assert np.array_equal(hrecs[k], orecs[k]), k
        refseq = bytes(s.ref)
        order = {"A": ["T", "G", "C"], "T": ["C", "A", "G"], "G": ["A", "C", "T"], "C": ["G", "T", "A"]}
        want = O.normcounts(b, chunks, p, refseq, p["germline_snv_prior"], None, None, alt_order=order, non_human_sample=False,
                            phase=phase_sets)
        got = normcounts.norm_contig(w, b, chunks, refseq, None, None, False, order, phase_sets=phase_sets)
        assert (got[2], got[0], got[1]) == (want[2], want[0], want[1])
        if not phase:
            hets = sorted(set((int(pp) + 1, chr(r), chr(al)) for pp, r, al, g in zip(s.snp_pos, s.snp_ref, s.snp_alt, s.snp_gt)
                              if g in (1, 2)))
            o_lst, o_e2c = O.edges(b, hets, 20, 20)
            hpos = np.array([h[0] for h in hets], np.int32)
            href = np.array([ord(h[1]) for h in hets], np.uint8)
            band = O.edge_band(b, hpos)
            w.ctx.push_reads(b)
            cnt = w.ctx.run_edges(hpos, href, 20, 20, band).reshape(-1, 4)
            h_e2c = {}
            for e in np.flatnonzero(cnt.sum(1)):
                i, d = int(e) // band, int(e) % band
                h_e2c[(i, i + 1 + d)] = [float(x) for x in cnt[e]]
            assert sorted(h_e2c) == o_lst and h_e2c == o_e2c
    finally:
        w.close()


# ---- a context reused for another batch: stale column-store cells, a stale plan

@pytest.mark.gpu
def test_second_batch_in_one_context_equals_fresh():
    a, _ = DC.random_batch(5001, n_reads=250)
    b, _ = DC.random_batch(5002, n_reads=120)
    assert DC.plan_groups(a.cs_off) != DC.plan_groups(b.cs_off)
    want_recs, want_log, want = read_pass(b, 0, WIDE)
    w = caller.Worker(0)
    try:
        w.ctx.debug_decode(0)
        read_pass(a, 0, WIDE, w)
        read_pass(a, 0, WIDE, w)             # a second run: on the capacities the first one left
        recs, log, got = read_pass(b, 0, WIDE, w)
        DC.assert_same_read_pass(b, want, got, "reused context")
        assert got["counters"] == want["counters"] == DC.plan_counters(b) + [0]
        assert log == want_log and np.array_equal(recs, want_recs)
        assert np.array_equal(got["bits"][:len(want["bits"])], want["bits"]) or DC.bits_set(got["bits"]) == DC.bits_set(want["bits"])
    finally:
        w.close()
