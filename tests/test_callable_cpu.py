"""The callable bits of `normcounts` without a GPU: the plain model (tests/callable_model.py) against what the reference's
update_tri2count gave for the hand-built reads of tests/callable_cases.py (tests/golden/callable_cases.*, made by
tests/golden/make_golden.py callable_cases), proof that those reads tell every rule from its wrong variant, the trim
bounds over 20,000 query lengths, and the C oracle's counters on every case.  tests/test_gpu_callable.py holds
k_callable to the same model, bit by bit."""
import math
import os
import zlib

import numpy as np
import pytest

from tests import callable_cases as C
from tests import callable_model as M
from tests import util

CRC_ARRAYS = ("tstart", "tend", "qstart", "qlen", "mapq", "flag", "qid", "qoff", "cs_off", "seq", "bq", "cs", "tp")
ORDER = {"A": ["T", "G", "C"], "T": ["C", "A", "G"], "G": ["A", "C", "T"], "C": ["G", "T", "A"]}


@pytest.fixture(scope="module")
def built():
    """name -> (case, batch), built once."""
    out = {}
    for name in C.CASES:
        case = C.build(name)
        out[name] = (case, C.batch_of(case))
    return out


@pytest.fixture(scope="module")
def fixture():
    """(json, {(case, parameter set number, read name): packed bits of [tstart, tend)})."""
    exp = util.load_json("callable_cases")
    with np.load(os.path.join(util.GOLDEN, "callable_cases.npz")) as z:
        counted = z["counted"]
    assert tuple(exp["order"]) == C.FIXTURE_CASES
    runs, o = {}, 0
    for name in exp["order"]:
        case = C.build(name)
        span = {r["qname"]: r["tend"] - r["tstart"] for r in case.records}
        for k in range(len(exp["cases"][name]["params"])):
            for q in exp["cases"][name]["reads"]:
                n = (span[q] + 7) // 8
                runs[(name, k, q)] = counted[o:o + n]
                o += n
    assert o == counted.shape[0]
    return exp, runs


def ref_to_query(batch, i):
    """{reference position: query offset} of the match and substituted bases of read i, from its cs operations."""
    out = {}
    rpos, qpos = int(batch.tstart[i]), int(batch.qstart[i])
    for state, _ref, ref_len, alt_len in M.cs_tuples(batch.cs_tag(i)):
        if state in (1, 2):
            for j in range(ref_len):
                assert rpos + j not in out
                out[rpos + j] = qpos + j
        rpos += ref_len
        qpos += alt_len
    assert rpos == int(batch.tend[i]) and qpos <= int(batch.qlen[i])
    return out


def read_bits(batch, words, i):
    """The query offsets of read i whose bit is set."""
    qoff, qlen = int(batch.qoff[i]), int(batch.qlen[i])
    return {q for q in range(qlen) if (int(words[(qoff + q) >> 5]) >> (q & 31)) & 1}


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_model_equals_the_reference_made_fixture(built, fixture, name):
    exp, runs = fixture
    case, batch = built[name]
    want = exp["cases"][name]
    # the fixture's input is what the builders give today
    for k in CRC_ARRAYS:
        assert zlib.crc32(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).tobytes()) == want["crc32"][k], k
    assert want["params"] == case.params
    assert want["reads"] == [r["qname"] for r in case.records if C.in_fixture(name, r)]
    index = {r["qname"]: i for i, r in enumerate(case.records)}
    n_set = 0
    for k, ov in enumerate(case.params):
        p = C.params_of(ov)
        live, words = M.callable_bits(batch, case.chunks, p)
        assert live.all()
        for q in want["reads"]:
            i = index[q]
            ts, te = int(batch.tstart[i]), int(batch.tend[i])
            bits = np.unpackbits(runs[(name, k, q)])[:te - ts]
            positions = [ts + int(x) for x in np.flatnonzero(bits)]
            # the model's counted positions are the reference's ...
            mine = M.read_counted(batch, i, p)
            assert sorted(mine) == positions, (ov, q)
            # ... and through the read's segments they are the bits of the hook's layout
            t2q = ref_to_query(batch, i)
            assert read_bits(batch, words, i) == {t2q[t] for t in positions}, (ov, q)
            n_set += len(positions)
    assert n_set > 1000


# rule -> the case written for it, the number of its parameter set, a read that tells
SENSITIVITY = [("window_at_base", "read_start", 0, "start0_clip_sub45"), ("list_0based", "word_edges", 0, "sub_0"),
               ("sub_tested", "trim", 1, "subs100"), ("nsub_listed", "nsub", 0, "bit0"),
               ("nsub_same_op", "nsub", 0, "first_w"), ("bq_le", "quality", 2, "passA_low"),
               ("trim_strict", "trim", 2, "plain100"), ("minus_one", "counts", 1, "entries2"),
               ("dr_w_at_start", "read_start", 0, "start1_clip_sub45"), ("trim_end_floor", "trim", 3, "plain180")]


@pytest.mark.parametrize("rule,name,k,qname", SENSITIVITY)
def test_cases_tell_the_rule_from_its_wrong_variant(built, rule, name, k, qname):
    case, batch = built[name]
    p = C.params_of(case.params[k])
    i = [r["qname"] for r in case.records].index(qname)
    right, wrong = M.callable_bits(batch, case.chunks, p), M.callable_bits(batch, case.chunks, p, rules=(rule,))
    assert read_bits(batch, right[1], i) != read_bits(batch, wrong[1], i)


def test_every_switch_has_a_case_but_the_one_that_changes_nothing():
    """qe >= qlen in place of qe > qlen differs only where osq + w == qlen, and there the branch it takes gives ur = w +
    (qe - qlen) = w and dr = qlen - osq = w: the window of the branch it leaves.  The switch is a restatement, no case can
    tell it, and k_callable's choice between the two is free."""
    assert {r for r, _n, _k, _q in SENSITIVITY} == set(M.RULES) - {"qe_ge"}
    for w in range(0, 70):
        for qlen in range(1, 200):
            for qpos in range(qlen):
                assert M.mismatch_range(1000, qpos, qlen, w, ("qe_ge",)) == M.mismatch_range(1000, qpos, qlen, w)


def test_trim_bounds_over_20000_query_lengths():
    """bamlib.get_trimmed_range's two expressions, as the model and (in double arithmetic) k_callable evaluate them; the
    lengths at which ceil((1 - t) qlen) is not qlen - floor(t qlen) are in the trim case."""
    differ = set()
    for t in C.TRIM_VALUES + (C.DEFAULT_TRIM,):
        for qlen in range(1, 20001):
            lo, hi = M.trimmed_range(qlen, t)
            assert lo == math.floor(t * qlen) and hi == math.ceil((1 - t) * qlen)
            assert lo == int(np.floor(np.float64(t) * np.float64(qlen))) and hi == int(np.ceil((1.0 - np.float64(t)) * np.float64(qlen)))
            assert M.is_trimmed(lo - 1, lo, hi) and M.is_trimmed(hi + 1, lo, hi)
            assert lo > hi or not (M.is_trimmed(lo, lo, hi) or M.is_trimmed(hi, lo, hi))
            if hi != qlen - lo and qlen in C.TRIM_QLEN:
                differ.add((t, qlen))
    assert {(0.35, 180), (0.35, 340), (0.45, 100), (0.45, 180)} <= differ


def test_probe_bases_with_0_to_9_entries_in_their_window(built):
    """counts: for every k in 0 ... 9 some match base has exactly k list entries in its window (it counts at
    max_mismatch_count k and, for k > 0, not at k - 1)."""
    case, batch = built["counts"]
    by_m = {ov["max_mismatch_count"]: M.callable_bits(batch, case.chunks, C.params_of(ov))[1] for ov in case.params}
    more = M.callable_bits(batch, case.chunks, C.params_of(dict(max_mismatch_count=6)))[1]
    by_m[6] = more
    for k in range(1, 10):
        assert (by_m[k] & ~by_m[k - 1]).any(), k
    assert by_m[0].any()


def oracle_link(case, batch, ov, copies):
    """What the oracle's counters must be for the batch with every read laid down ``copies`` times, from the model on the
    batch itself (the copies differ in their names alone): log[0] (num_ccs) is the number of reads that stay, and log[1]
    (num_bases, normcounts.py:317-325) the number of their counted bases on upper-case ACGT positions of the chunks --
    every such position has tri_sum > 0, whatever its classification."""
    p = C.params_of(ov)
    live, _words = M.callable_bits(batch, case.chunks, p)
    bases = 0
    for i in range(batch.n):
        if live[i]:
            bases += sum(1 for t in M.read_counted(batch, i, p)
                         if case.ref[t] in "ACGT" and any(s <= t < e for s, e in case.chunks))
    return copies * int(live.sum()), copies * bases


@pytest.mark.parametrize("name", C.CASES)
def test_oracle_counters_follow_from_the_model(built, name):
    """Every read ten times at the same start under distinct names (positions deep enough to classify) through the C
    oracle: num_ccs and num_bases are the model's; the classified bases are a part of them."""
    from oracle import oracle as O
    case, batch = built[name]
    b10 = C.batch_of(case, copies=10)
    if name == "padding":
        batch, b10 = C.poison_padding(batch), C.poison_padding(b10)
    for ov in case.params[:2] + case.params[-1:]:
        p = C.params_of(ov)
        ccs, _rf, log = O.normcounts(b10, case.chunks, p, case.ref.encode(), p["germline_snv_prior"], alt_order=ORDER)
        assert (log[0], log[1]) == oracle_link(case, batch, ov, 10), ov
        assert sum(ccs.values()) == log[13] <= log[1]
        assert log[13] > 0
