"""CPU checks of the BC row-mask calls at the C-ABI boundary (include/td3.h: td3_set_bc_filter,
td3_bc_filter_info, td3_bc_filter_keep): exported, bound with the argument types of ``SIGNATURES``, the
ctypes struct laid out as the header's, the existing structs untouched, and the refusals that need no GPU
made before any GPU work (a null handle reaches them without one)."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_cabi_train_log import _c_layout, _header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("td3_set_bc_filter", "td3_bc_filter_info", "td3_bc_filter_keep")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
        assert re.search(r"^int %s\(td3_handle\* h, " % s, txt, flags=re.M), f"{s} not declared in include/td3.h"
    assert _lib.SIGNATURES["td3_set_bc_filter"][1] == [C.c_void_p, C.c_int, C.c_int]
    assert re.search(r"^int td3_set_bc_filter\(td3_handle\* h, int demo_rows, int q_filter\);", txt, flags=re.M)
    assert _lib.SIGNATURES["td3_bc_filter_info"][1] == [C.c_void_p, C.POINTER(_lib.td3_bc_filter_info_t)]
    assert re.search(r"^int td3_bc_filter_info\(td3_handle\* h, td3_bc_filter_info_t\* info\);", txt, flags=re.M)
    assert _lib.SIGNATURES["td3_bc_filter_keep"][1] == [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    # the section follows "Demonstration replay" and precedes "gradient clipping"
    at = [txt.index(s) for s in ("--- Demonstration replay (two rings) */", "--- BC on the demonstration rows, Q-filter */",
                                 "--- gradient clipping */")]
    assert at == sorted(at)


def test_filter_info_struct_matches_header(lib):
    from td3_amd import _lib
    st = _lib.td3_bc_filter_info_t
    fields = _header_struct("td3_bc_filter_info_t")
    assert [f[0] for f in st._fields_] == [f[0] for f in fields]
    assert [f[0] for f in fields] == ["demo_rows", "q_filter", "step", "n_demo", "kept", "bc_loss"]
    offsets, total = _c_layout(fields)
    for f, _ in st._fields_:
        assert getattr(st, f).offset == offsets[f], f
    assert C.sizeof(st) == total == 40


def test_the_existing_structs_are_untouched(lib):
    """Setters and a struct of their own: td3_config and td3_bc_info_t keep their layout and size."""
    from td3_amd import _lib
    assert not any("bc" in f[0] for f in _lib.td3_config._fields_)
    assert C.sizeof(_lib.td3_config) == lib.td3_config_size()
    assert [f[0] for f in _lib.td3_bc_info_t._fields_] == ["enabled", "alpha", "step", "lambda", "q_abs_mean", "bc_loss"]
    assert [f[0] for f in _header_struct("td3_bc_info_t")] == [f[0] for f in _lib.td3_bc_info_t._fields_]
    assert C.sizeof(_lib.td3_bc_info_t) == 48
    for name in ("td3_step_stats", "td3_log_entry"):
        assert not any("bc" in f[0] for f in getattr(_lib, name)._fields_), name


@pytest.mark.parametrize("switches", [(2, 0), (0, 2), (-1, 1), (1, -1)])
def test_a_bad_switch_is_refused_before_the_handle(lib, switches):
    assert lib.td3_set_bc_filter(None, *switches) == -1
    err = lib.td3_last_error()
    assert b"0 or 1" in err and b"null handle" not in err, err


def test_null_arguments(lib):
    from td3_amd import _lib
    for switches in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert lib.td3_set_bc_filter(None, *switches) == -1
        assert b"null handle" in lib.td3_last_error()
    assert lib.td3_bc_filter_info(None, None) == -1
    assert b"null info" in lib.td3_last_error()
    assert lib.td3_bc_filter_info(None, C.byref(_lib.td3_bc_filter_info_t())) == -1
    assert b"null handle" in lib.td3_last_error()
    assert lib.td3_bc_filter_keep(None, None, 0) == -1
    assert b"null keep" in lib.td3_last_error()
    assert lib.td3_bc_filter_keep(None, (C.c_float * 4)(), 4) == -1
    assert b"null handle" in lib.td3_last_error()


def test_the_kernel_has_a_translation_unit_of_its_own():
    from td3_amd import build
    assert "csrc/bcf.hip" in build.SOURCES and "csrc/bc.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "td3_amd", "csrc", "bcf.hip")).read()
    assert "row_bcf_kernel" in src and "launch_rows_bcf" in src
    for other in ("kernels.hip", "bc.hip"):
        assert "row_bcf_kernel" not in open(os.path.join(ROOT, "td3_amd", "csrc", other)).read(), other


def test_python_surface_imports_without_gpu():
    from td3_amd import TD3_featured, TD3_particles
    p = inspect.signature(TD3_featured.TD3.__init__).parameters
    assert p["bc_rows"].default == "all" and p["bc_q_filter"].default is False
    pp = inspect.signature(TD3_particles.TD3.__init__).parameters
    assert "bc_rows" not in pp and "bc_q_filter" not in pp
    for name in ("bc_rows", "bc_q_filter"):
        assert isinstance(inspect.getattr_static(TD3_featured.TD3, name), property)
    assert callable(TD3_featured.TD3.bc_filter_info)
