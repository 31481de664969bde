"""The callable run's entries of the C ABI: exported by the built library, declared in include/himut_hip.h, rows of the
table behind _ffi.py; the record and the two block constants as the header states them.  No compute calls."""
import ctypes
import os
import re

from himut_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("himut_run_callable", "himut_get_callable", "himut_get_callable_map")


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
    assert [len(_ffi._ABI[n][1]) for n in SYMBOLS] == [3, 4, 4]
    L = _ffi.lib()
    for name in SYMBOLS:
        assert getattr(L, name).restype is ctypes.c_int


def test_null_arguments_are_rejected():
    from himut_amd import _ffi
    L = _ffi.lib()
    assert L.himut_run_callable(None, None, 0) == 1
    assert L.himut_get_callable(None, None, None, None) == 1
    assert L.himut_get_callable_map(None, None, None, 0) == 1


def test_record_and_constants_match_the_header():
    from himut_amd import _ffi
    text = header_text()
    assert _ffi.CALLABLE_RUN_DTYPE.itemsize == 24
    assert _ffi.CALLABLE_RUN_DTYPE.names == ("chunk", "start", "end", "state", "bases")
    assert [_ffi.CALLABLE_RUN_DTYPE.fields[n][1] for n in _ffi.CALLABLE_RUN_DTYPE.names] == [0, 4, 8, 12, 16]
    assert int(re.search(r"#define HIMUT_CALLMAP_TILE (\d+)", text).group(1)) == _ffi.CALLMAP_TILE
    assert int(re.search(r"#define HIMUT_CALLMAP_BLOCK (\d+)", text).group(1)) == _ffi.CALLMAP_BLOCK
    codes = {name: int(v) for name, v in re.findall(r"HIMUT_CM_(\w+) = (\d+)", text)}
    assert codes == {name: code for code, name in _ffi.CALLABLE_STATES.items()}
    assert 6 not in _ffi.CALLABLE_STATES
