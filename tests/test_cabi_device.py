"""CPU checks of the device-resident entry points' C-ABI boundary (include/td3.h: rb_add_device,
td3_select_action_device, td3_eval_q_device): exported, bound, and refusing bad arguments with a
message before anything touches a GPU."""
import ctypes as C

import pytest

DEVICE_SYMBOLS = ("rb_add_device", "td3_select_action_device", "td3_eval_q_device")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_device_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    for s in DEVICE_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]


def test_explore_struct_layout():
    """td3_explore as include/td3.h declares it on LP64: three pointers and two uint64 at 8-byte
    alignment, the three floats packed behind the first pointer."""
    from td3_amd import _lib
    E = _lib.td3_explore
    assert [f[0] for f in E._fields_] == ["x", "mu", "theta", "sigma", "reset", "seed", "step", "inject_z",
                                          "z_out"]
    assert (E.x.offset, E.mu.offset, E.theta.offset, E.sigma.offset) == (0, 8, 12, 16)
    assert (E.reset.offset, E.seed.offset, E.step.offset) == (24, 32, 40)
    assert (E.inject_z.offset, E.z_out.offset, C.sizeof(E)) == (48, 56, 64)


def test_device_argument_errors_are_reported(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rb_add_device(None, p, p, p, p, p, 1, None) == -1
    assert b"null handle" in lib.td3_last_error()
    assert lib.rb_add_device(None, p, p, p, p, p, -1, None) == -1
    assert b"n must be >= 0" in lib.td3_last_error()
    assert lib.td3_select_action_device(None, p, 0, None, p, None) == -1
    assert b"n must be positive" in lib.td3_last_error()
    assert lib.td3_select_action_device(None, p, 1, None, p, None) == -1
    assert b"null argument" in lib.td3_last_error()
    assert lib.td3_eval_q_device(None, p, p, 0, p, None) == -1
    assert b"n must be positive" in lib.td3_last_error()
    assert lib.td3_eval_q_device(None, p, p, 1, p, None) == -1
    assert b"null argument" in lib.td3_last_error()
