"""The fit's entry points (himut_fit_exposures, himut_debug_fit) in the header, the export list and the ffi table; the ABI
version; a null context; and, on a device, every limit rejected with a message and the context usable afterwards."""
import ctypes

import numpy as np
import pytest

from himut_amd import _ffi, build
from tests.test_abi import declared_prototypes

SYMBOLS = {"himut_fit_exposures": 10, "himut_debug_fit": 3}


def test_symbols_are_declared_exported_and_bound():
    protos = declared_prototypes()
    lib = ctypes.CDLL(build.build_hip())
    for name, n_params in SYMBOLS.items():
        assert protos[name] == ("int", n_params), name
        assert name in _ffi.EXPORTS
        restype, argtypes = _ffi._ABI[name]
        assert restype is ctypes.c_int and len(argtypes) == n_params, name
        assert hasattr(lib, name), name
    assert _ffi._ABI["himut_fit_exposures"][1][6] is ctypes.c_uint64          # the seed: all 64 bits
    assert hasattr(_ffi.Context, "fit_exposures") and hasattr(_ffi.Context, "debug_fit")


def test_abi_version_stays_2():
    lib = ctypes.CDLL(build.build_hip())
    lib.himut_abi_version.restype = ctypes.c_int
    assert lib.himut_abi_version() == 2
    assert _ffi.lib().himut_abi_version() == 2


def test_null_context_is_rejected():
    L = _ffi.lib()
    sig, m, e = (ctypes.c_double * 1)(1.0), (ctypes.c_int64 * 1)(1), (ctypes.c_double * 1)()
    assert L.himut_fit_exposures(None, sig, 1, 1, m, 0, 1, 1, e, None) != 0
    assert L.himut_debug_fit(None, 0, 0) != 0


@pytest.mark.gpu
def test_each_limit_is_rejected_with_a_message():
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    with _ffi.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        sig, m, e = np.full((4, 2), 0.25), np.array([1, 2, 3, 4], np.int64), np.zeros((3, 2))

        def call(sig=sig, C=4, K=2, m=m, B=2, T=5, e=e):
            return L.himut_fit_exposures(h, None if sig is None else p(sig), C, K, None if m is None else p(m), B, 1, T,
                                         None if e is None else p(e), None)
        big = np.full((1537, 97), 0.5)
        bigm = np.zeros(1537, np.int64)
        bad = [(dict(C=0), b"C outside 1..1536"), (dict(C=1537, sig=big, m=bigm), b"C outside 1..1536"),
               (dict(K=0), b"K outside 1..96"), (dict(K=97, sig=big), b"K outside 1..96"),
               (dict(B=-1), b"n_boot outside 0..100000"), (dict(B=100001), b"n_boot outside 0..100000"),
               (dict(T=0), b"iters outside 1..100000"), (dict(T=100001), b"iters outside 1..100000"),
               (dict(m=np.array([1, -2, 3, 4], np.int64)), b"count 1 is negative"),
               (dict(m=np.array([2 ** 30, 2 ** 30, 0, 0], np.int64)), b"sum to 2^31 or more"),
               (dict(m=np.array([0, 0, 2 ** 40, 0], np.int64)), b"sum to 2^31 or more"),
               (dict(sig=None), b"a null array"), (dict(m=None), b"a null array"), (dict(e=None), b"a null array")]
        for value, at in ((-0.25, b"sig[2][1]"), (float("nan"), b"sig[2][1]"), (float("inf"), b"sig[2][1]")):
            s2 = sig.copy()
            s2[2, 1] = value
            bad.append((dict(sig=s2), at))
        for kw, word in bad:
            assert call(**kw) == 1, kw
            msg = L.himut_last_error(h)
            assert b"himut_fit_exposures" in msg and word in msg, (kw, msg)
        assert L.himut_debug_fit(h, -1, 0) == 1 and b"himut_debug_fit" in L.himut_last_error(h)
        assert L.himut_debug_fit(h, 0, -1) == 1 and L.himut_debug_fit(h, 0, 65537) == 1
        # the largest values pass the checks, and the context goes on
        assert L.himut_debug_fit(h, 2048, 65536) == 0 and L.himut_debug_fit(h, 0, 0) == 0
        assert call() == 0
        assert np.allclose(e.sum(axis=1), 10.0)
        top = np.array([2 ** 31 - 1, 0, 0, 0], np.int64)
        assert call(m=top, B=0, T=1) == 0 and abs(e[0].sum() - (2 ** 31 - 1)) < 1e-3
