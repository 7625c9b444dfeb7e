"""CPU checks of the training-log calls at the C-ABI boundary (include/td3.h: td3_log_*): exported, bound
with the argument types of ``SIGNATURES``, the ctypes structs and the numpy dtype laid out as the header's,
and the documented argument checks that precede the handle -- in the header's order -- made before any GPU
work, so a null handle reaches them without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_SYMBOLS = ("td3_log_entry_size", "td3_log_enable", "td3_log_info", "td3_log_read", "td3_log_set")
C_SIZES = {"int64_t": 8, "int32_t": 4, "int": 4, "double": 8}


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_log_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    for s in LOG_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0]
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
        assert re.search(r"^(int|size_t) %s\(" % s, txt, flags=re.M), f"{s} not declared in include/td3.h"
    assert _lib.SIGNATURES["td3_log_entry_size"][0] is C.c_size_t
    assert all(_lib.SIGNATURES[s][0] is C.c_int for s in LOG_SYMBOLS[1:])
    assert "csrc/trainlog.hip" in __import__("td3_amd.build", fromlist=["SOURCES"]).SOURCES


def _header_struct(name):
    """[(field, C type)] of a struct of plain scalars in include/td3.h, in order."""
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for d in (d.strip() for d in body.split(";")):
        if d:                                            # "type a, b"
            ctype, first = d.split(",")[0].split()
            out += [(n.strip(), ctype) for n in [first] + d.split(",")[1:]]
    return out


def _c_layout(fields):
    """Offsets and size under the C rules for naturally aligned scalars."""
    off, offsets, align = 0, {}, 1
    for name, ctype in fields:
        sz = C_SIZES[ctype]
        off = (off + sz - 1) // sz * sz
        offsets[name] = off
        off += sz
        align = max(align, sz)
    return offsets, (off + align - 1) // align * align


@pytest.mark.parametrize("name,size", [("td3_log_entry", 136), ("td3_log_info_t", 24)])
def test_log_structs_match_header(lib, name, size):
    from td3_amd import _lib
    st = getattr(_lib, name)
    fields = _header_struct(name)
    assert [f[0] for f in st._fields_] == [f[0] for f in fields]
    offsets, total = _c_layout(fields)
    for f, _ in st._fields_:
        assert getattr(st, f).offset == offsets[f], f
        assert getattr(st, f).size == C_SIZES[dict(fields)[f]], f
    assert C.sizeof(st) == total == size
    if name == "td3_log_entry":
        assert lib.td3_log_entry_size() == size


def test_entry_dtype_is_the_struct(lib):
    from td3_amd import _lib
    from td3_amd.train_log import ENTRY_DTYPE
    assert ENTRY_DTYPE.itemsize == C.sizeof(_lib.td3_log_entry) == lib.td3_log_entry_size()
    assert list(ENTRY_DTYPE.names) == [f[0] for f in _lib.td3_log_entry._fields_]
    for f, t in _lib.td3_log_entry._fields_:
        assert ENTRY_DTYPE.fields[f][1] == getattr(_lib.td3_log_entry, f).offset
        assert ENTRY_DTYPE.fields[f][0].itemsize == C.sizeof(t)
        assert ENTRY_DTYPE.fields[f][0].kind == ("f" if t is C.c_double else "i")


def test_enable_checks_come_in_the_documented_order(lib):
    for cap, every, field in ((0, 0, b"capacity"), (-1, 1, b"capacity"), ((1 << 20) + 1, 1, b"capacity"),
                              (8, 0, b"every"), (8, -3, b"every"), (1 << 20, (1 << 20) + 1, b"every"),
                              (1, 1, b"null handle"), (1 << 20, 1 << 20, b"null handle")):
        assert lib.td3_log_enable(None, cap, every) == -1
        err = lib.td3_last_error()
        assert field in err, (cap, every, err)
        if field != b"capacity":
            assert b"capacity" not in err


def test_read_checks_come_in_the_documented_order(lib):
    from td3_amd import _lib
    out = (_lib.td3_log_entry * 4)()
    f, n = C.c_int64(), C.c_int64()
    call = lib.td3_log_read
    assert call(None, -1, -1, None, None, None) == -1
    assert b"first must be >= 0" in lib.td3_last_error()
    assert call(None, 0, -1, None, None, None) == -1
    assert b"n must be >= 0" in lib.td3_last_error()
    assert call(None, 0, 4, None, None, None) == -1
    assert b"out is null" in lib.td3_last_error() and b"first_out" not in lib.td3_last_error()
    assert call(None, 0, 4, out, None, None) == -1
    assert b"first_out is null" in lib.td3_last_error()
    assert call(None, 0, 0, None, C.byref(f), None) == -1         # n == 0 needs no out
    assert b"n_out is null" in lib.td3_last_error()
    assert call(None, 0, 4, out, C.byref(f), C.byref(n)) == -1
    assert b"null handle" in lib.td3_last_error()


def test_set_and_info_checks_come_in_the_documented_order(lib):
    from td3_amd import _lib
    ent = (_lib.td3_log_entry * 4)()
    call = lib.td3_log_set
    assert call(None, None, -1, -5) == -1
    assert b"n must be >= 0" in lib.td3_last_error()
    assert call(None, None, 4, 2) == -1
    assert b"entries is null" in lib.td3_last_error()
    assert call(None, ent, 4, 3) == -1
    assert b"count must be >= n" in lib.td3_last_error()
    assert call(None, None, 0, -1) == -1                          # n == 0 needs no entries
    assert b"count must be >= n" in lib.td3_last_error()
    assert call(None, ent, 4, 4) == -1
    assert b"null handle" in lib.td3_last_error()
    assert call(None, None, 0, 0) == -1
    assert b"null handle" in lib.td3_last_error()
    assert lib.td3_log_info(None, None) == -1
    assert b"null info" in lib.td3_last_error()
    assert lib.td3_log_info(None, C.byref(_lib.td3_log_info_t())) == -1
    assert b"null handle" in lib.td3_last_error()


def test_python_surface_imports_without_gpu():
    import inspect
    from td3_amd import TD3_featured, TD3_particles, train_log
    for mod in (TD3_featured, TD3_particles):
        p = inspect.signature(mod.TD3.enable_train_log).parameters
        assert p["capacity"].default == 4096 and p["every"].default == 1
        assert isinstance(inspect.getattr_static(mod.TD3, "train_log"), property)
    for m in ("entries", "info", "summary", "state_dict", "load_state_dict", "save", "load"):
        assert callable(getattr(train_log.TrainLog, m)), m
    assert isinstance(inspect.getattr_static(train_log.TrainLog, "count"), property)
    e = __import__("numpy").zeros(0, train_log.ENTRY_DTYPE)
    s = train_log.summarize(e)
    assert s["steps"] == 0 and s["nonfinite"] == 0 and s["first_step"] is None
