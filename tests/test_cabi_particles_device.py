"""CPU checks of the particle learner's device-resident entry points at the C-ABI boundary
(include/td3.h: rb_add_particles_device, td3_select_action_particles_device,
td3_eval_q_particles_device): exported, bound with the argument types of ``SIGNATURES``, and refusing
bad arguments with a message before anything touches a GPU."""
import ctypes as C

import pytest

PARTICLE_DEVICE_SYMBOLS = ("rb_add_particles_device", "td3_select_action_particles_device",
                           "td3_eval_q_particles_device")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_particle_device_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    for s in PARTICLE_DEVICE_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0]
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    # seven device arrays, the row count, the stream / the explore struct by pointer
    assert len(_lib.SIGNATURES["rb_add_particles_device"][1]) == 10
    assert _lib.SIGNATURES["td3_select_action_particles_device"][1][4] == C.POINTER(_lib.td3_explore)
    assert len(_lib.SIGNATURES["td3_eval_q_particles_device"][1]) == 7


def test_particle_device_argument_errors_are_reported(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rb_add_particles_device(None, p, p, p, p, p, p, p, 1, None) == -1
    assert b"null handle" in lib.td3_last_error()
    assert lib.rb_add_particles_device(None, p, p, p, p, p, p, p, -1, None) == -1
    assert b"n must be >= 0" in lib.td3_last_error()
    for n in (0, -3):
        assert lib.td3_select_action_particles_device(None, p, p, n, None, p, None) == -1
        assert b"n must be positive" in lib.td3_last_error()
        assert lib.td3_eval_q_particles_device(None, p, p, p, n, p, None) == -1
        assert b"n must be positive" in lib.td3_last_error()
    assert lib.td3_select_action_particles_device(None, p, p, 1, None, p, None) == -1
    assert b"null argument" in lib.td3_last_error()
    assert lib.td3_eval_q_particles_device(None, p, p, p, 1, p, None) == -1
    assert b"null argument" in lib.td3_last_error()
