"""CPU checks of prioritized replay at the C-ABI boundary (include/td3.h: rb_enable_priorities,
rb_set_priorities, rb_update_priorities, rb_sample_prioritized, rb_get_priorities, rb_priority_info,
td3_train_step_prioritized): exported, bound with the argument types of ``SIGNATURES``, the ctypes
structs laid out as the header's, and every argument check that precedes the handle made -- in the
header's order -- before the handle is looked at, so a null handle reaches them without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_enable_priorities", "rb_set_priorities", "rb_update_priorities", "rb_sample_prioritized",
           "rb_get_priorities", "rb_priority_info", "td3_train_step_prioritized")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_priority_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    sig = _lib.SIGNATURES
    assert sig["rb_enable_priorities"][1] == [C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    for s in ("rb_set_priorities", "rb_update_priorities"):      # handle, idx, values, n, stream
        assert len(sig[s][1]) == 5 and sig[s][1][3] is C.c_int64
    args = sig["rb_sample_prioritized"][1]                       # handle, batch, beta, u, idx, w, stream
    assert len(args) == 7 and args[1] is C.c_int and args[2] is C.c_double
    args = sig["td3_train_step_prioritized"][1]
    assert len(args) == 9 and args[3] is C.c_double
    assert args[7] == C.POINTER(_lib.td3_step_stats) and args[8] == C.POINTER(_lib.td3_per_stats)


def _decls(name):
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [d.strip() for d in body.split(";") if d.strip()]


def test_priority_structs_match_header():
    from td3_amd import _lib
    assert _decls("rb_priority_info_t") == ["int enabled", "double alpha, eps", "int levels", "double total",
                                            "float max_priority"]
    I = _lib.rb_priority_info_t
    assert [n for n, _ in I._fields_] == ["enabled", "alpha", "eps", "levels", "total", "max_priority"]
    assert (I.enabled.offset, I.alpha.offset, I.eps.offset, I.levels.offset, I.total.offset,
            I.max_priority.offset) == (0, 8, 16, 24, 32, 40)
    assert C.sizeof(I) == 48
    assert _decls("td3_per_stats") == ["float* weight", "float* td_abs"]
    assert _lib.td3_per_stats._fields_ == [("weight", C.c_void_p), ("td_abs", C.c_void_p)]
    assert C.sizeof(_lib.td3_per_stats) == 16
    # the step's other structs are the ones test_cabi.py pins: unchanged by this entry point
    assert C.sizeof(_lib.td3_step_stats) == 64


def test_priority_stream_id_is_documented():
    """The draw's Philox stream id (5) is its own, next to the target noise (2) and exploration (4)."""
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    assert re.search(r"stream id 5", txt) and re.search(r"target noise \(2\)", txt)
    common = open(os.path.join(ROOT, "td3_amd", "csrc", "common.h")).read()
    ids = dict(re.findall(r"(kStream\w+) = (\d+)u", common))
    assert ids["kStreamPriority"] == "5" and len(set(ids.values())) == len(ids)


@pytest.mark.parametrize("alpha,eps,field", [
    (-0.1, 1e-6, b"alpha"), (1.5, 1e-6, b"alpha"), (float("nan"), 1e-6, b"alpha"),
    (0.6, 0.0, b"eps"), (0.6, -1.0, b"eps"), (0.6, float("nan"), b"eps")])
def test_enable_errors_name_the_field(lib, alpha, eps, field):
    assert lib.rb_enable_priorities(None, alpha, eps, None) == -1
    err = lib.td3_last_error()
    assert field in err and b"null handle" not in err, err


def test_enable_checks_come_in_the_documented_order(lib):
    assert lib.rb_enable_priorities(None, 2.0, 0.0, None) == -1       # alpha before eps
    assert b"alpha" in lib.td3_last_error()
    for alpha in (0.0, 0.6, 1.0):                                     # both ends accepted: the handle is next
        assert lib.rb_enable_priorities(None, alpha, 1e-6, None) == -1
        assert b"null handle" in lib.td3_last_error()


def test_store_checks_come_in_the_documented_order(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for call in (lib.rb_set_priorities, lib.rb_update_priorities):
        assert call(None, None, None, -1, None) == -1                 # n first
        assert b"n must be >= 0" in lib.td3_last_error()
        assert call(None, None, p, 3, None) == -1                     # then the arrays
        assert b"null idx" in lib.td3_last_error()
        assert call(None, p, None, 3, None) == -1
        assert b"null idx" in lib.td3_last_error()
        assert call(None, p, p, 3, None) == -1                        # then the handle
        assert b"null handle" in lib.td3_last_error()
        assert call(None, None, None, 0, None) == -1                  # n == 0 returns 0 only on a real ring
        assert b"null handle" in lib.td3_last_error()


def test_sample_checks_come_in_the_documented_order(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    call = lib.rb_sample_prioritized
    for batch in (0, -3):
        assert call(None, batch, 2.0, None, None, None, None) == -1   # batch first
        assert b"batch must be positive" in lib.td3_last_error()
    for beta in (-0.1, 1.5, float("nan")):
        assert call(None, 8, beta, None, None, None, None) == -1      # then beta
        assert b"beta" in lib.td3_last_error()
    for idx, w in ((None, p), (p, None), (None, None)):
        assert call(None, 8, 0.4, None, idx, w, None) == -1           # then the outputs
        assert b"idx_out" in lib.td3_last_error() and b"null handle" not in lib.td3_last_error()
    for beta in (0.0, 0.4, 1.0):                                      # inject_u is nullable; the handle is next
        assert call(None, 8, beta, None, p, p, None) == -1
        assert b"null handle" in lib.td3_last_error()


def test_host_queries_refuse_null(lib):
    from td3_amd import _lib
    out = (C.c_float * 4)()
    assert lib.rb_get_priorities(None, 0, 4, out) == -1
    assert b"null" in lib.td3_last_error()
    info = _lib.rb_priority_info_t()
    assert lib.rb_priority_info(None, C.byref(info)) == -1
    assert b"null" in lib.td3_last_error()
    assert lib.td3_train_step_prioritized(None, None, 8, 0.4, None, None, None, None, None) == -1
    assert b"null handle" in lib.td3_last_error()
