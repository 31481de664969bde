"""The transcription-strand calls (himut_set_strands, himut_sbs384_counts, himut_strand_tricounts, himut_strand_callable)
through the C ABI against the plain model (tests/strands_model.py), by equality: strings and segment lists placed where
a lane, a wave or a tile of the reference pass can go wrong, substitutions at every segment edge and at the string's ends,
the map pass over the callable run's hand-built scenes, the error paths, and every result a second time with the grids
capped at one workgroup (himut_debug_spectra)."""
import functools

import numpy as np
import pytest

from tests import intervals_cases as IK
from tests import strands_cases as K
from tests import strands_model as SM
from tests.test_gpu_callmap import ORDER, Device, _configure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worker():
    from himut_amd.caller import Worker
    w = Worker(0)
    yield w
    w.ctx.debug_spectra(0)
    w.close()


@pytest.fixture(params=[0, 1], ids=["default", "one_workgroup"])
def ctx(worker, request):
    worker.ctx.debug_spectra(request.param)
    yield worker.ctx
    worker.ctx.debug_spectra(0)


def set_string(ctx, seq):
    from himut_amd import normcounts
    chars, cls = normcounts.tri_classes(seq)
    ctx.set_reference(seq, cls, len(chars))


def fold64(h):
    """himut_ref_tricounts' 64 bins as the 32 classes first * 8 + (centre == T) * 4 + last."""
    return np.array([h[f * 16 + m * 4 + l] for f in range(4) for m in (1, 3) for l in range(4)], np.int64)


@functools.lru_cache(maxsize=None)
def _wanted(length, name):
    """The model's results for one string and one of its segment lists, computed once for both grid settings."""
    seq = K.random_string(length)
    start, mask = K.segment_lists(length)[name]
    pos0, ref, alt = K.substitutions(seq, start, seed=length)
    return SM.strand_tricounts(seq, start, mask), (pos0, ref, alt), SM.sbs384(seq, start, mask, pos0, ref, alt)


@pytest.mark.parametrize("length", K.LENGTHS)
def test_reference_pass_and_substitutions(ctx, length):
    seq = K.random_string(length)
    set_string(ctx, seq)
    whole = fold64(ctx.ref_tricounts())
    for name, (start, mask) in K.segment_lists(length).items():
        want_tri, (pos0, ref, alt), (want_cls, want_out) = _wanted(length, name)
        ctx.set_strands(start, mask)
        got = ctx.strand_tricounts()
        assert got.shape == (4, 32) and got.dtype == np.int64
        assert np.array_equal(got, want_tri), name
        assert np.array_equal(got.sum(axis=0), whole), name
        assert ctx.strand_tricounts().tobytes() == got.tobytes()
        r8, a8 = [ord(x) for x in ref], [ord(x) for x in alt]
        cls, out = ctx.sbs384_counts(pos0, r8, a8)
        assert cls.dtype == np.uint16 and np.array_equal(cls, want_cls), name
        assert np.array_equal(out, want_out), name
        flat = ctx.sbs96_counts(pos0, r8, a8)
        assert np.array_equal(out[:384].reshape(4, 96).sum(axis=0), flat[:96]) and np.array_equal(out[384:], flat[96:])
        none, again = ctx.sbs384_counts(pos0, r8, a8, want_classes=False)
        assert none is None and again.tobytes() == out.tobytes()


def test_hand_built_contigs(ctx):
    labels, names = SM.bin_labels(), SM.tri_names()
    for seq, start, mask, subs, opp in ((K.CHR1, K.CHR1_SEG_START, K.CHR1_SEG_MASK, K.CHR1_SUBS, K.CHR1_OPP),
                                        (K.CHR2, K.CHR2_SEG_START, K.CHR2_SEG_MASK, K.CHR2_SUBS, K.CHR2_OPP)):
        set_string(ctx, seq)
        ctx.set_strands(start, mask)
        tri = ctx.strand_tricounts()
        assert {(SM.CATS[c], names[t]): int(tri[c, t]) for c in range(4) for t in range(32) if tri[c, t]} == opp
        cls, out = ctx.sbs384_counts([p - 1 for p, *_ in subs], [ord(s[1]) for s in subs], [ord(s[2]) for s in subs])
        assert [None if k == SM.NO_CLASS else labels[k] for k in cls.tolist()] == [s[4] if s[3] else None for s in subs]
        assert int(out.sum()) == len(subs)


def test_many_substitutions_and_none(ctx):
    """More substitutions than one workgroup holds, so the default grid has several workgroups; then n == 0."""
    import random
    length = 2 * K.TILE + 5
    seq = K.random_string(length, seed=9)
    start, mask = K.segment_lists(length)["sixteens"]
    set_string(ctx, seq)
    ctx.set_strands(start, mask)
    rs = random.Random(384)
    pos0 = [rs.randrange(-1, length + 1) for _ in range(3001)]
    ref = [seq[p].upper() if 0 <= p < length and seq[p].upper() in "ACGT" else "G" for p in pos0]
    alt = [rs.choice("ACGT") for _ in pos0]
    cls, out = ctx.sbs384_counts(pos0, [ord(x) for x in ref], [ord(x) for x in alt])
    want_cls, want_out = SM.sbs384(seq, start, mask, pos0, ref, alt)
    assert np.array_equal(cls, want_cls) and np.array_equal(out, want_out)
    assert int(out[:384].sum()) > 1000 and all(int(out[c * 96:(c + 1) * 96].sum()) > 0 for c in range(4))
    st = ctx.stats()
    assert st["ms_total"] > 0 and st["n_candidates"] == 3001
    cls, out = ctx.sbs384_counts([], [], [])
    assert cls.shape == (0,) and not out.any()


def _map_case(worker, case):
    sc = case.scene
    _configure(worker, sc.params)
    return Device(worker, sc.batch, sc.chunks, sc.ref.encode(), order=ORDER)


def _map_segments(case):
    """Segment lists for a scene: boundaries inside chunks (a chunk then starts inside a segment), at chunk starts and ends
    and one base either side, all four masks; and the single segment."""
    sc = case.scene
    n = len(sc.ref)
    at = {n // 3, n // 2}
    for s, e in sc.chunks:
        at.update((s - 1, s, s + 1, (s + e) // 2, e - 1, e, e + 1))
    starts = [0] + sorted(p for p in at if 0 < p < n)
    return [(starts, [(3 * k + 1) % 4 for k in range(len(starts))]), ([0], [1])]


@pytest.mark.parametrize("scene", ["hetalt", "hetalt_unordered", "string_ends", "boundary"])
def test_map_pass(worker, scene):
    """hetalt_unordered: chunks that overlap and go back; boundary: gaps between chunks, an N and lower-case letters, more
    entries than one workgroup takes; string_ends: entries at positions 0 and len - 1.  A position held by two chunks
    counts twice: the model walks the entries, not the positions."""
    case = getattr(IK, scene)()
    dev = _map_case(worker, case)
    sc = case.scene
    worker.ctx.run_intervals([0], [len(sc.ref)])
    whole = worker.ctx.intervals()[0]
    for start, mask in _map_segments(case):
        want = SM.strand_callable(dev.state, dev.bases, dev.chunks, sc.ref, start, mask)
        assert int(want[0].sum()) > 0
        results = []
        for cap in (0, 1):
            worker.ctx.debug_spectra(cap)
            worker.ctx.set_strands(start, mask)
            pos, bases = worker.ctx.strand_callable()
            assert np.array_equal(pos, want[0]) and np.array_equal(bases, want[1]), (scene, cap)
            assert np.array_equal(pos.sum(axis=0), whole["ref_tri"][:32]) and np.array_equal(bases.sum(axis=0), whole["ccs_tri"][:32])
            results.append(pos.tobytes() + bases.tobytes())
            st = worker.ctx.stats()
            assert st["ms_total"] > 0 and st["positions"] == dev.n
        worker.ctx.debug_spectra(0)
        assert results[0] == results[1]


def test_error_paths():
    from himut_amd import _ffi
    from himut_amd.caller import Worker
    w = Worker(0)
    try:
        ctx = w.ctx
        with pytest.raises(_ffi.HimutError) as e:              # no reference string
            ctx.set_strands([0], [0])
        assert e.value.code == 1 and "himut_set_reference" in e.value.message
        seq = K.random_string(100)
        set_string(ctx, seq)
        for call in (ctx.strand_tricounts, lambda: ctx.sbs384_counts([1], [67], [84]), ctx.strand_callable):
            with pytest.raises(_ffi.HimutError) as e:          # no segment list
                call()
            assert e.value.code == 1
        good = ([0, 10, 50], [1, 2, 3])
        ctx.set_strands(*good)
        want = SM.strand_tricounts(seq, *good)
        assert np.array_equal(ctx.strand_tricounts(), want)
        bad = (([], []), ([1, 10], [0, 0]), ([0, 10, 10], [0, 1, 2]), ([0, 20, 10], [0, 1, 2]), ([0, 100], [0, 1]),
               ([0, 99, 100], [0, 1, 1]), ([0, 10], [0, 4]), ([0, 10], [255, 0]))
        for start, mask in bad:
            with pytest.raises(_ffi.HimutError) as e:
                ctx.set_strands(start, mask)
            assert e.value.code == 1 and "himut_set_strands" in e.value.message, (start, mask)
            assert np.array_equal(ctx.strand_tricounts(), want)             # the context is usable, the list is the old one
        L = _ffi.lib()
        assert L.himut_set_strands(ctx.handle, None, None, 1) == 1 and L.himut_set_strands(None, None, None, 1) == 1
        assert L.himut_strand_tricounts(ctx.handle, None) == 1 and L.himut_sbs384_counts(ctx.handle, None, None, None, 1, None, None) == 1
        ctx.set_strands([0, 99], [0, 3])                                        # a start at len - 1 is the last one allowed
        assert np.array_equal(ctx.strand_tricounts(), SM.strand_tricounts(seq, [0, 99], [0, 3]))
        with pytest.raises(_ffi.HimutError) as e:                               # no callable run has completed
            ctx.strand_callable()
        assert e.value.code == 1 and "himut_run_callable" in e.value.message
        set_string(ctx, seq)                                                    # himut_set_reference drops the list
        for call in (ctx.strand_tricounts, lambda: ctx.sbs384_counts([1], [67], [84])):
            with pytest.raises(_ffi.HimutError) as e:
                call()
            assert e.value.code == 1 and "himut_set_strands" in e.value.message
        # behind a callable run: a list is needed, and a string as long as the run's
        case = IK.hetalt()
        _map_case(w, case)
        with pytest.raises(_ffi.HimutError) as e:
            ctx.strand_callable()
        assert e.value.code == 1 and "himut_set_strands" in e.value.message
        ctx.set_strands([0], [2])
        pos, _bases = ctx.strand_callable()
        assert int(pos.sum()) > 0
        set_string(ctx, case.scene.ref[:-1])
        ctx.set_strands([0], [2])
        with pytest.raises(_ffi.HimutError) as e:
            ctx.strand_callable()
        assert e.value.code == 1 and "reference" in e.value.message
    finally:
        w.close()
