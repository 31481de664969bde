"""The spectra's entry points (himut_id83_classify, himut_dbs78_counts, himut_debug_spectra) in the header, the export list
and the ffi table; the ABI version; a null context.  No compute calls here."""
import ctypes

from himut_amd import _ffi, build
from tests.test_abi import declared_prototypes

SYMBOLS = {"himut_id83_classify": 8, "himut_dbs78_counts": 6, "himut_debug_spectra": 2}


def test_symbols_are_declared_exported_and_bound():
    protos = declared_prototypes()
    lib = ctypes.CDLL(build.build_hip())
    for name, n_params in SYMBOLS.items():
        assert protos[name] == ("int", n_params), name
        assert name in _ffi.EXPORTS
        restype, argtypes = _ffi._ABI[name]
        assert restype is ctypes.c_int and len(argtypes) == n_params, name
        assert hasattr(lib, name), name


def test_abi_version_stays_2():
    lib = ctypes.CDLL(build.build_hip())
    lib.himut_abi_version.restype = ctypes.c_int
    assert lib.himut_abi_version() == 2
    assert _ffi.lib().himut_abi_version() == 2


def test_null_context_is_rejected():
    L = _ffi.lib()
    out = (ctypes.c_int64 * 88)()
    assert L.himut_id83_classify(None, None, None, None, None, 0, None, out) != 0
    assert L.himut_dbs78_counts(None, None, None, 0, None, out) != 0
    assert L.himut_debug_spectra(None, 0) != 0
