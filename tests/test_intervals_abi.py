"""The intervals run's entries of the C ABI: exported by the built library, declared in include/himut_hip.h, rows of the
table behind _ffi.py; the row as the header states it.  No compute calls."""
import ctypes
import os
import re

from himut_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("himut_run_intervals", "himut_get_intervals")


def header_text():
    return open(os.path.join(ROOT, "include", "himut_hip.h")).read()


def test_symbols_resolve_and_are_in_the_table():
    from himut_amd import _ffi
    lib = ctypes.CDLL(build.build_hip())
    text = header_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _ffi._ABI and name in _ffi.EXPORTS, name
        assert re.search(r"^int\s+{}\(".format(name), text, flags=re.M), name
    assert [len(_ffi._ABI[n][1]) for n in SYMBOLS] == [4, 3]
    L = _ffi.lib()
    for name in SYMBOLS:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.himut_abi_version() == 2


def test_null_arguments_are_rejected():
    from himut_amd import _ffi
    L = _ffi.lib()
    assert L.himut_run_intervals(None, None, None, 0) == 1
    assert L.himut_get_intervals(None, None, None) == 1


def test_row_matches_the_header():
    """The fields of himut_interval_row in the header's order, all int64, 128 of them."""
    from himut_amd import _ffi
    body = re.search(r"typedef struct himut_interval_row \{(.*?)\} himut_interval_row;", header_text(), flags=re.S).group(1)
    fields = re.findall(r"int64_t\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [name for name, _n in fields] == list(_ffi.INTERVAL_ROW_DTYPE.names)
    offset = 0
    for name, count in fields:
        dt, off = _ffi.INTERVAL_ROW_DTYPE.fields[name][:2]
        assert off == offset, name
        assert dt.base == "<i8" and dt.shape == ((int(count),) if count else ()), name
        offset += 8 * (int(count) if count else 1)
    assert offset == _ffi.INTERVAL_ROW_DTYPE.itemsize == 1024
    assert len(_ffi.INTERVAL_TRI_NAMES) == 33 and _ffi.INTERVAL_TRI_NAMES[-1] == "other"
    assert _ffi.INTERVAL_TRI_NAMES[:9] == ("ACA", "ACC", "ACG", "ACT", "ATA", "ATC", "ATG", "ATT", "CCA")
