"""The duplex run's entries of the C ABI: exported by the built library, declared in include/himut_hip.h, rows of the
table behind _ffi.py; the 80-byte record and the parameter block as the header states them.  No compute calls."""
import ctypes
import os
import re

from himut_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("himut_run_duplex", "himut_get_duplex")


def header_text():
    return open(os.path.join(ROOT, "include", "himut_hip.h")).read()


def struct_fields(name):
    """[(type, field, count or None)] of a typedef struct of the header, comments dropped."""
    body = re.search(r"typedef struct {0} \{{(.*?)\}} {0};".format(name), header_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, f, int(n) if n else None) for t, f, n in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_symbols_resolve_and_are_in_the_table():
    from himut_amd import _ffi
    lib = ctypes.CDLL(build.build_hip())
    text = header_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _ffi._ABI and name in _ffi.EXPORTS, name
        assert re.search(r"^int\s+{}\(".format(name), text, flags=re.M), name
    assert [len(_ffi._ABI[n][1]) for n in SYMBOLS] == [4, 5]
    L = _ffi.lib()
    for name in SYMBOLS:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.himut_abi_version() == 2


def test_null_arguments_are_rejected():
    from himut_amd import _ffi
    L = _ffi.lib()
    assert L.himut_run_duplex(None, None, 0, None) == 1
    assert L.himut_get_duplex(None, None, None, None, None) == 1


def test_record_and_params_match_the_header():
    from himut_amd import _ffi
    from tests import duplex_model as M
    fields = struct_fields("himut_duplex_record")
    assert [(t, f, n) for t, f, n in fields] == [("himut_site_record", "site", None), ("uint32_t", "n_ds", None),
                                                 ("uint32_t", "n_ss", None), ("uint32_t", "n_alt_unpaired", None),
                                                 ("uint32_t", "reserved", None)]
    d = _ffi.DUPLEX_RECORD_DTYPE
    assert d == M.RECORD_DTYPE and d.itemsize == 80
    for name in _ffi.SITE_RECORD_DTYPE.names:                        # the site record's fields at their offsets
        assert d.fields[name] == _ffi.SITE_RECORD_DTYPE.fields[name], name
    assert [d.fields[k][1] for k in ("n_ds", "n_ss", "n_alt_unpaired", "reserved2")] == [64, 68, 72, 76]
    assert struct_fields("himut_duplex_params") == [("int32_t", "reserved", 8)]
    assert ctypes.sizeof(_ffi.DuplexParams) == 32
    assert tuple(_ffi.DUPLEX_LOG_NAMES) == M.LOG and len(M.LOG) == 40 and tuple(_ffi.DUPLEX_SS_CLASSES) == M.SS_CLASSES
    assert "int64_t ss[12], int64_t log[40]" in header_text()
