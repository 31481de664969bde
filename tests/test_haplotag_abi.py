"""The haplotag run's entries of the C ABI: exported by the built library, declared in include/himut_hip.h, rows of the
table behind _ffi.py; the two 32-byte rows and the parameter block as the header states them.  No compute calls."""
import ctypes
import os
import re

from himut_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("himut_run_haplotag", "himut_get_haplotag", "himut_get_read_info")
CTYPES = {"int32_t": "<i4", "uint32_t": "<u4", "uint16_t": "<u2", "uint8_t": "u1"}


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
    assert [len(_ffi._ABI[n][1]) for n in SYMBOLS] == [9, 6, 5]
    L = _ffi.lib()
    for name in SYMBOLS:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.himut_abi_version() == 2


def test_null_arguments_are_rejected():
    from himut_amd import _ffi
    L = _ffi.lib()
    assert L.himut_run_haplotag(None, None, None, None, None, None, 0, 0, None) == 1
    assert L.himut_get_haplotag(None, None, None, None, None, None) == 1
    assert L.himut_get_read_info(None, None, None, None, None) == 1


def _check_layout(fields, dtype):
    assert [f for _t, f, _n in fields] == list(dtype.names)
    offset = 0
    for t, f, n in fields:
        dt, off = dtype.fields[f][:2]
        assert off == offset and n is None and dt == CTYPES[t], f
        offset += dt.itemsize
    assert offset == dtype.itemsize == 32


def test_rows_match_the_header():
    from himut_amd import _ffi
    _check_layout(struct_fields("himut_haplotag_row"), _ffi.HAPLOTAG_ROW_DTYPE)
    _check_layout(struct_fields("himut_haplotag_snp"), _ffi.HAPLOTAG_SNP_DTYPE)
    assert all(_ffi.HAPLOTAG_SNP_DTYPE.fields[k][0] == "<u4" for k in _ffi.HAPLOTAG_SNP_DTYPE.names)


def test_params_and_codes_match_the_header():
    from himut_amd import _ffi
    fields = struct_fields("himut_haplotag_params")
    assert [(f, n) for _t, f, n in fields] == [("min_mapq", None), ("min_bq", None), ("min_snps", None),
                                               ("min_agree_permille", None), ("reserved", 4)]
    assert [k for k, _ in _ffi.HaplotagParams._fields_] == [f for _t, f, _n in fields]
    assert ctypes.sizeof(_ffi.HaplotagParams) == 32
    text = header_text()
    for code, name in enumerate(_ffi.HAPLOTAG_STATUS_NAMES):
        assert re.search(r"HIMUT_HT_{} = {}\b".format(name.upper(), code), text), name
    assert len(_ffi.HAPLOTAG_LOG_NAMES) == 13
