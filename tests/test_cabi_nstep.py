"""CPU checks of the n-step adds at the C-ABI boundary (include/td3.h: rb_nstep, rb_add_device_nstep,
rb_add_particles_device_nstep): exported, bound with the argument types of ``SIGNATURES``, the ctypes
struct laid out as the header's, and the argument checks that need no ring made -- in the header's
order -- before the handle is looked at, so a null handle reaches them without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEP_SYMBOLS = ("rb_add_device_nstep", "rb_add_particles_device_nstep")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_nstep_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    for s in NSTEP_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    # handle, five / seven device arrays, the row count, the lane parameters by pointer, the stream
    for s, arrays in zip(NSTEP_SYMBOLS, (5, 7)):
        args = _lib.SIGNATURES[s][1]
        assert len(args) == 1 + arrays + 3
        assert args[1 + arrays] is C.c_int64 and args[2 + arrays] == C.POINTER(_lib.rb_nstep)


def test_nstep_struct_matches_header():
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    body = re.search(r"typedef struct rb_nstep \{(.*?)\} rb_nstep;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["int n", "double gamma", "const uint8_t* ended"]
    assert _lib.rb_nstep._fields_ == [("n", C.c_int), ("gamma", C.c_double), ("ended", C.c_void_p)]
    assert (_lib.rb_nstep.n.offset, _lib.rb_nstep.gamma.offset, _lib.rb_nstep.ended.offset) == (0, 8, 16)
    assert C.sizeof(_lib.rb_nstep) == 24


def _ns(n=3, gamma=0.9, ended=True):
    from td3_amd import _lib
    buf = (C.c_ubyte * 64)()
    ns = _lib.rb_nstep()
    ns.n, ns.gamma = n, gamma
    ns.ended = C.cast(buf, C.c_void_p) if ended else None
    ns._keep = buf
    return ns


def _calls(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    return ((lambda rows, ns: lib.rb_add_device_nstep(None, p, p, p, p, p, rows, ns, None)),
            (lambda rows, ns: lib.rb_add_particles_device_nstep(None, p, p, p, p, p, p, p, rows, ns, None)))


@pytest.mark.parametrize("bad,field", [
    (dict(n=0), b"ns->n"), (dict(n=9), b"ns->n"), (dict(n=-1), b"ns->n"),
    (dict(gamma=0.0), b"ns->gamma"), (dict(gamma=1.5), b"ns->gamma"), (dict(gamma=-0.5), b"ns->gamma"),
    (dict(gamma=float("nan")), b"ns->gamma"), (dict(ended=False), b"ns->ended")])
def test_nstep_struct_errors_name_the_field(lib, bad, field):
    """Each is refused with a null handle: the lane parameters are checked before the handle is touched."""
    for call in _calls(lib):
        assert call(1, _ns(**bad)) == -1
        err = lib.td3_last_error()
        assert field in err and b"null handle" not in err, err


def test_nstep_checks_come_in_the_documented_order(lib):
    for call in _calls(lib):
        assert call(1, None) == -1
        assert b"null ns" in lib.td3_last_error()
        assert call(1, _ns()) == -1                      # self-consistent parameters: the handle is next
        assert b"null handle" in lib.td3_last_error()
        assert call(1, _ns(n=8, gamma=1.0)) == -1        # both ends of the ranges are accepted
        assert b"null handle" in lib.td3_last_error()
        assert call(1, _ns(n=1)) == -1
        assert b"null handle" in lib.td3_last_error()
        assert call(0, _ns()) == -1                      # rows == 0 returns 0 only on a real ring
        assert b"null handle" in lib.td3_last_error()
        assert call(-1, _ns()) == -1
        assert b"rows must be >= 0" in lib.td3_last_error()
        assert call(-1, _ns(n=0)) == -1                  # rows is checked first
        assert b"rows must be >= 0" in lib.td3_last_error()
        assert call(-1, None) == -1
        assert b"rows must be >= 0" in lib.td3_last_error()
        assert call(1, _ns(n=0, gamma=0.0, ended=False)) == -1    # n before gamma before ended
        assert b"ns->n" in lib.td3_last_error()
        assert call(1, _ns(gamma=0.0, ended=False)) == -1
        assert b"ns->gamma" in lib.td3_last_error()
