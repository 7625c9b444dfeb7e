"""CPU checks of the TD3+BC calls at the C-ABI boundary (include/td3.h: td3_set_bc, td3_bc_info):
exported, bound with the argument types of ``SIGNATURES``, the ctypes struct laid out as the header's, and
the refusals that need no GPU made before any GPU work (a null handle reaches them without one)."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_cabi_train_log import _c_layout, _header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC_SYMBOLS = ("td3_set_bc", "td3_bc_info")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_bc_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    for s in BC_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
        assert re.search(r"^int %s\(td3_handle\* h, " % s, txt, flags=re.M), f"{s} not declared in include/td3.h"
    assert _lib.SIGNATURES["td3_set_bc"][1] == [C.c_void_p, C.c_double]
    assert re.search(r"^int td3_set_bc\(td3_handle\* h, double alpha\);", txt, flags=re.M)
    assert _lib.SIGNATURES["td3_bc_info"][1] == [C.c_void_p, C.POINTER(_lib.td3_bc_info_t)]
    assert re.search(r"^int td3_bc_info\(td3_handle\* h, td3_bc_info_t\* info\);", txt, flags=re.M)


def test_bc_info_struct_matches_header(lib):
    from td3_amd import _lib
    st = _lib.td3_bc_info_t
    fields = _header_struct("td3_bc_info_t")
    assert [f[0] for f in st._fields_] == [f[0] for f in fields]
    assert [f[0] for f in fields] == ["enabled", "alpha", "step", "lambda", "q_abs_mean", "bc_loss"]
    offsets, total = _c_layout(fields)
    for f, _ in st._fields_:
        assert getattr(st, f).offset == offsets[f], f
    assert C.sizeof(st) == total == 48


def test_the_config_struct_is_untouched(lib):
    """A setter, not a td3_config field: the struct and its size guard stay as they are."""
    from td3_amd import _lib
    assert "bc_alpha" not in [f[0] for f in _lib.td3_config._fields_]
    assert C.sizeof(_lib.td3_config) == lib.td3_config_size()
    for name in ("td3_step_stats", "td3_log_entry"):
        assert not any("bc" in f[0] for f in getattr(_lib, name)._fields_), name


@pytest.mark.parametrize("alpha", [-1.0, -1e-30, float("nan"), float("inf"), float("-inf")])
def test_bad_alpha_is_refused_before_the_handle(lib, alpha):
    assert lib.td3_set_bc(None, alpha) == -1
    err = lib.td3_last_error()
    assert b"alpha" in err and b"null handle" not in err, err


def test_null_arguments(lib):
    from td3_amd import _lib
    for alpha in (0.0, 2.5):
        assert lib.td3_set_bc(None, alpha) == -1
        assert b"null handle" in lib.td3_last_error()
    assert lib.td3_bc_info(None, None) == -1
    assert b"null info" in lib.td3_last_error()
    assert lib.td3_bc_info(None, C.byref(_lib.td3_bc_info_t())) == -1
    assert b"null handle" in lib.td3_last_error()


def test_python_surface_imports_without_gpu():
    from td3_amd import TD3_featured, TD3_particles
    p = inspect.signature(TD3_featured.TD3.__init__).parameters
    assert p["bc_alpha"].default is None
    assert "bc_alpha" not in inspect.signature(TD3_particles.TD3.__init__).parameters
    assert isinstance(inspect.getattr_static(TD3_featured.TD3, "bc_alpha"), property)
    assert callable(TD3_featured.TD3.bc_info)
