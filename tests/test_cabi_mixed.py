"""CPU checks of the demonstration-replay calls at the C-ABI boundary (include/td3.h "Demonstration
replay": td3_train_step_mixed, td3_debug_mixed_input): exported, bound with the argument types of
``SIGNATURES``, declared with the issue's prototypes, the refusals that need no GPU made before any GPU
work (null handles reach them without one), and ``MixedReplay``'s batch split."""
import ctypes as C
import inspect
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED_SYMBOLS = ("td3_train_step_mixed", "td3_debug_mixed_input")
PROTOTYPES = (
    "int td3_train_step_mixed(td3_handle* h, rb_handle* rb, rb_handle* demo, int batch, int n_demo, void* stream,\n"
    "                         const int64_t* inject_idx, const float* inject_noise, td3_step_stats* stats);",
    "int td3_debug_mixed_input(td3_handle* h, rb_handle* rb, rb_handle* demo, void* stream);",
)


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_mixed_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    for s, proto in zip(MIXED_SYMBOLS, PROTOTYPES):
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
        assert re.search(r"^" + re.escape(proto), txt, flags=re.M), f"{s} not declared as specified"
    # the step's tail is td3_train_step's: indices, noise, stats
    assert _lib.SIGNATURES["td3_train_step_mixed"][1] == (
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + _lib.SIGNATURES["td3_train_step"][1][4:])
    assert _lib.SIGNATURES["td3_debug_mixed_input"][1] == [C.c_void_p] * 4
    assert "td3_train_step_mixed" in txt.split("#ifndef TD3_HIP_H")[0], "not in the header's opening table"


@pytest.mark.parametrize("batch,n_demo,field", [(0, 0, b"batch"), (-3, 0, b"batch"), (4, -1, b"n_demo"),
                                                (4, 5, b"n_demo"), (1, 2, b"n_demo")])
def test_bad_sizes_are_refused_before_the_handles(lib, batch, n_demo, field):
    assert lib.td3_train_step_mixed(None, None, None, batch, n_demo, None, None, None, None) == -1
    err = lib.td3_last_error()
    assert field in err and b"null handle" not in err, err


def test_null_handles_are_refused_next(lib):
    for n_demo in (0, 2, 4):
        assert lib.td3_train_step_mixed(None, None, None, 4, n_demo, None, None, None, None) == -1
        assert b"null handle" in lib.td3_last_error()
    assert lib.td3_debug_mixed_input(None, None, None, None) == -1
    assert b"null handle" in lib.td3_last_error()


def test_no_struct_changes_its_layout(lib):
    from td3_amd import _lib
    assert C.sizeof(_lib.td3_config) == lib.td3_config_size()
    assert [f[0] for f in _lib.td3_step_stats._fields_] == ["critic_loss", "actor_loss", "actor_step", "y", "q1",
                                                            "q2", "idx", "noise"]
    assert C.sizeof(_lib.td3_step_stats) == 64
    for name in ("td3_step_stats", "td3_config"):
        assert not any("demo" in f[0] or "mixed" in f[0] for f in getattr(_lib, name)._fields_), name


def test_python_surface_imports_without_gpu():
    from td3_amd import TD3_featured, TD3_particles
    from td3_amd.my_replay_buffer import MixedReplay
    p = inspect.signature(MixedReplay.__init__).parameters
    assert list(p) == ["self", "online", "demo", "demo_fraction"] and p["demo_fraction"].default == 0.5
    assert MixedReplay.prioritized is False
    for name in ("add", "add_batch", "add_batch_hindsight", "add_batch_nstep", "flush", "save", "sample", "n_demo"):
        assert callable(getattr(MixedReplay, name)), name
    for name in ("size", "ptr"):
        assert isinstance(inspect.getattr_static(MixedReplay, name), property), name
    for mod in (TD3_featured, TD3_particles):
        assert mod.MixedReplay is MixedReplay
        assert list(inspect.signature(mod.TD3.train_step).parameters) == [
            "self", "replay_buffer", "batch_size", "indices", "noise", "stats", "u"]


def _standin(online_size, demo_size, fraction):
    from td3_amd.my_replay_buffer import MixedReplay
    m = MixedReplay.__new__(MixedReplay)      # the split needs two sizes and the fraction, no ring
    m.online = types.SimpleNamespace(size=online_size)
    m.demo = types.SimpleNamespace(size=demo_size)
    m.demo_fraction = fraction
    return m


@pytest.mark.parametrize("batch,fraction,want", [
    (33, 0.0, 0), (33, 0.5, 17), (33, 1.0, 33), (33, 1.0 / 3.0, 11),
    (256, 0.0, 0), (256, 0.5, 128), (256, 1.0, 256), (256, 1.0 / 3.0, 85)])
def test_n_demo_rounding_rule(batch, fraction, want):
    # floor(batch * f + 0.5): 16.5 + 0.5 -> 17, 11.0 + 0.5 -> 11, 85.33 + 0.5 -> 85
    assert _standin(10, 10, fraction).n_demo(batch) == want


def test_n_demo_empty_ring_rules():
    for batch in (33, 256):
        for f in (0.0, 0.5, 1.0):
            assert _standin(10, 0, f).n_demo(batch) == 0          # no demonstrations: all online
            assert _standin(0, 10, f).n_demo(batch) == batch      # tick 0 on loaded demonstrations
        with pytest.raises(ValueError):
            _standin(0, 0, 0.5).n_demo(batch)
    m = _standin(10, 10, 0.5)
    m.demo_fraction = 0.25                                         # a plain attribute: annealed between steps
    assert m.n_demo(256) == 64
    for bad in (-0.1, 1.5):
        m.demo_fraction = bad
        with pytest.raises(ValueError):
            m.n_demo(256)
