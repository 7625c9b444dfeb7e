"""CPU checks of the dataset-normalisation calls at the C-ABI boundary (include/td3.h: rb_state_moments,
rb_normalize_states, rb_norm_info): exported, bound with the argument types of ``SIGNATURES``, the ctypes
struct laid out as the header's, the existing structs unchanged, and the argument checks that need no
handle -- in the header's order -- made before any GPU work, so they are reached without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_cabi_rollout_stats import _header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_state_moments", "rb_normalize_states", "rb_norm_info")


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
        assert re.search(r"^int %s\(" % s, txt, flags=re.M), f"{s} not declared in include/td3.h"
    assert "dataset normalisation */" in txt


def test_kernels_have_a_translation_unit_of_their_own():
    from td3_amd.build import SOURCES
    assert "csrc/ringnorm.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "td3_amd", "csrc", "ringnorm.hip"))
    replay = open(os.path.join(ROOT, "td3_amd", "csrc", "replay.hip")).read()
    rollout = open(os.path.join(ROOT, "td3_amd", "csrc", "rollout.hip")).read()
    unit = open(os.path.join(ROOT, "td3_amd", "csrc", "ringnorm.hip")).read()
    assert "nm_sweep_kernel" in unit and "nm_apply_kernel" in unit
    for k in ("nm_sweep_kernel", "nm_merge_kernel", "nm_apply_kernel"):
        assert k in unit and k not in replay and k not in rollout
    shared = open(os.path.join(ROOT, "td3_amd", "csrc", "rollout.h")).read()
    assert "norm_elem" in shared and "norm_elem" in rollout and "norm_elem" in unit   # one element expression


def test_norm_info_struct_matches_header():
    from td3_amd import _lib
    st = _lib.rb_norm_info_t
    assert [f[0] for f in st._fields_] == _header_struct("rb_norm_info_t") == ["normalized", "obs_dim", "rows"]
    assert C.sizeof(st) == 16 and st.rows.offset == 8


@pytest.mark.parametrize("name,size", [("rb_info_t", 64), ("rb_priority_info_t", 48), ("rs_config", 48),
                                       ("rs_tick_t", 64), ("rs_episode", 24), ("rs_info_t", 64), ("rs_state", 112)])
def test_existing_structs_are_unchanged(lib, name, size):
    from td3_amd import _lib
    assert C.sizeof(getattr(_lib, name)) == size
    assert C.sizeof(_lib.td3_config) == lib.td3_config_size()


def test_refusals_without_a_handle_in_the_headers_order(lib):
    one = C.c_void_p(1)                                  # never dereferenced: an earlier check fails
    for merge in (0, 1, 2, -1):
        assert lib.rb_state_moments(None, None, merge, None) == -1
        assert b"null rb" in lib.td3_last_error(), lib.td3_last_error()
        assert lib.rb_state_moments(None, one, merge, None) == -1
        assert b"null rb" in lib.td3_last_error()
        assert lib.rb_state_moments(one, None, merge, None) == -1
        assert b"null rs" in lib.td3_last_error(), lib.td3_last_error()
    for merge in (2, -1, 1 << 20):
        assert lib.rb_state_moments(one, one, merge, None) == -1
        assert b"merge must be 0 or 1" in lib.td3_last_error(), lib.td3_last_error()
    assert lib.rb_normalize_states(None, None, None) == -1
    assert b"null rb" in lib.td3_last_error()
    assert lib.rb_normalize_states(one, None, None) == -1
    assert b"null rs" in lib.td3_last_error()
    assert lib.rb_norm_info(None, None) == -1
    assert b"null info" in lib.td3_last_error()
    assert lib.rb_norm_info(one, None) == -1
    assert b"null info" in lib.td3_last_error()
    from td3_amd import _lib
    assert lib.rb_norm_info(None, C.byref(_lib.rb_norm_info_t())) == -1
    assert b"null handle" in lib.td3_last_error()


def test_python_surface_imports_without_gpu():
    from td3_amd import my_replay_buffer as rb, rollout_stats as rs
    for cls in (rb.ReplayBuffer_featured, rb.ReplayBuffer_particles):
        p = inspect.signature(cls.state_moments).parameters
        assert list(p)[1:] == ["stats", "merge", "gamma", "obs_clip", "eps", "col_mask"]
        assert p["stats"].default is None and p["merge"].default is False
        assert (p["gamma"].default, p["obs_clip"].default, p["eps"].default) == (0.99, 10.0, 1e-8)
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
        assert list(inspect.signature(cls.normalize_states).parameters)[1:] == ["stats"]
        assert isinstance(cls.normalized, property)
    assert "normalize_states" in rb.MixedReplay.__doc__
    assert callable(rs.RolloutStats.host_normalizer)


def test_host_normalizer_agrees_with_the_reference():
    """``host_normalizer`` on given moments (the handle replaced by its ``state_dict``: no GPU) against
    the restatement, within 1 fp32 ulp; masked columns and count == 0 bit for bit."""
    from ring_moments_reference import moments, normalise
    from td3_amd.rollout_stats import RolloutStats
    rs = np.random.RandomState(3)
    x = (rs.uniform(-5, 5, (500, 6)) + 5.0 * np.sin(np.arange(6))).astype(np.float32)
    x[:, 2] = 1e3 + 1e-2 * rs.standard_normal(500)
    x[0, 0] = 1e6                                        # clipped
    count, mean, m2 = moments(x)
    mask = np.array([1, 1, 1, 0, 1, 1], np.uint8)

    def handle(cnt):
        h = RolloutStats.__new__(RolloutStats)
        h._h, h.obs_clip, h.eps, h.col_mask = None, 10.0, 1e-8, mask
        h.state_dict = lambda: {"count": np.float64(cnt), "mean": mean, "m2": m2}
        return h
    got = handle(count).host_normalizer()(x)
    want = normalise(x, count, mean, m2, 1e-8, 10.0, mask)
    assert got.dtype == np.float32 and got.shape == x.shape
    step = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= step).all()
    assert got[:, 3].tobytes() == x[:, 3].tobytes() and got[0, 0] == 10.0
    one = handle(count).host_normalizer()(x[7])          # a single state, as a host loop passes it
    assert one.shape == (6,) and one.tobytes() == got[7].tobytes()
    assert handle(0.0).host_normalizer()(x).tobytes() == x.tobytes()
