"""CPU checks of the hindsight fan-out adds at the C-ABI boundary (include/td3.h: rb_hindsight,
rb_add_device_hindsight, rb_add_particles_device_hindsight): exported, bound with the argument types
of ``SIGNATURES``, the ctypes struct laid out as the header's, and the argument checks that need no
ring made -- in the header's order -- before the handle is looked at, so a null handle reaches them
without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINDSIGHT_SYMBOLS = ("rb_add_device_hindsight", "rb_add_particles_device_hindsight")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_hindsight_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    for s in HINDSIGHT_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    # handle, five / seven device arrays, the row count, the relabels by pointer, the stream
    for s, arrays in zip(HINDSIGHT_SYMBOLS, (5, 7)):
        args = _lib.SIGNATURES[s][1]
        assert len(args) == 1 + arrays + 3
        assert args[1 + arrays] is C.c_int64 and args[2 + arrays] == C.POINTER(_lib.rb_hindsight)


def test_hindsight_struct_matches_header():
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    body = re.search(r"typedef struct rb_hindsight \{(.*?)\} rb_hindsight;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["int k", "int g", "int cols[8]", "const float* goals", "const float* rewards"]
    assert _lib.rb_hindsight._fields_ == [("k", C.c_int), ("g", C.c_int), ("cols", C.c_int * 8),
                                          ("goals", C.c_void_p), ("rewards", C.c_void_p)]
    assert C.sizeof(_lib.rb_hindsight) == 2 * 4 + 8 * 4 + 2 * C.sizeof(C.c_void_p)


def _hs(k=3, g=2, cols=(2, 0), goals=True, rewards=True):
    from td3_amd import _lib
    buf = (C.c_float * 64)()
    hs = _lib.rb_hindsight()
    hs.k, hs.g = k, g
    for j, c in enumerate(cols):
        hs.cols[j] = c
    hs.goals = C.cast(buf, C.c_void_p) if goals else None
    hs.rewards = C.cast(buf, C.c_void_p) if rewards else None
    hs._keep = buf
    return hs


def _calls(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    return ((lambda n, hs: lib.rb_add_device_hindsight(None, p, p, p, p, p, n, hs, None)),
            (lambda n, hs: lib.rb_add_particles_device_hindsight(None, p, p, p, p, p, p, p, n, hs, None)))


@pytest.mark.parametrize("bad,field", [
    (dict(k=0), b"hs->k"), (dict(k=65), b"hs->k"), (dict(g=9), b"hs->g"), (dict(g=0), b"hs->g"),
    (dict(g=3, cols=(1, 4, 1)), b"hs->cols must be distinct"), (dict(cols=(2, -1)), b"hs->cols must be non-negative"),
    (dict(goals=False), b"hs->goals"), (dict(rewards=False), b"hs->rewards")])
def test_hindsight_struct_errors_name_the_field(lib, bad, field):
    """Each is refused with a null handle: the relabels are checked before the handle is touched."""
    for call in _calls(lib):
        assert call(1, _hs(**bad)) == -1
        err = lib.td3_last_error()
        assert field in err and b"null handle" not in err, err


def test_hindsight_null_struct_null_handle_and_negative_n(lib):
    for call in _calls(lib):
        assert call(1, None) == -1
        assert b"null hs" in lib.td3_last_error()
        assert call(1, _hs()) == -1                      # self-consistent relabels: the handle is next
        assert b"null handle" in lib.td3_last_error()
        assert call(0, _hs()) == -1                      # n == 0 returns 0 only on a real ring
        assert b"null handle" in lib.td3_last_error()
        assert call(-1, _hs()) == -1
        assert b"n must be >= 0" in lib.td3_last_error()
        assert call(-1, _hs(k=0)) == -1                  # n is checked first
        assert b"n must be >= 0" in lib.td3_last_error()


def test_python_shape_checks_need_no_library_call():
    """_hindsight_dims / _hindsight_expand: the shape rules of add_batch_hindsight and the expanded
    order of main.py:70-91 (transition, then its K relabels), in float64."""
    import numpy as np
    from td3_amd.my_replay_buffer import _hindsight_dims, _hindsight_expand
    n, K, sd = 3, 2, 5
    r, g1, g2 = np.zeros((n, K)), np.zeros((n, K)), np.zeros((n, K, 2))
    assert _hindsight_dims([4], g1, r, n) == ([4], K, 1)
    assert _hindsight_dims([4], g1[:, :, None], r, n) == ([4], K, 1)
    assert _hindsight_dims(np.array([3, 1]), g2, r, n) == ([3, 1], K, 2)
    for cols, goals, rewards in (([3, 1], g1, r), ([4], g2, r), ([3, 1], g2, r[:2]), ([3, 1], g2[:2], r),
                                 ([3, 1], g2, r.reshape(-1)), ([], g2, r), (list(range(9)), g2, r)):
        with pytest.raises(ValueError):
            _hindsight_dims(cols, goals, rewards, n)
    rs = np.random.RandomState(0)
    s, s2, a = rs.standard_normal((n, sd)), rs.standard_normal((n, sd)), rs.standard_normal((n, 2))
    rew, d = rs.standard_normal(n), np.array([0., 1., 0.])
    goals, rewards = rs.standard_normal((n, K, 2)), rs.standard_normal((n, K))
    es, ea, es2, er, ed = _hindsight_expand([s, a, s2, rew, d], (0, 2), 3, [3, 1], K, goals, rewards)
    assert es.dtype == np.float64 and es.shape == (n * (1 + K), sd)
    for i in range(n):
        for j in range(1 + K):
            e = i * (1 + K) + j
            ws, ws2 = s[i].copy(), s2[i].copy()
            if j:
                ws[[3, 1]] = ws2[[3, 1]] = goals[i, j - 1]
            np.testing.assert_array_equal(es[e], ws)
            np.testing.assert_array_equal(es2[e], ws2)
            np.testing.assert_array_equal(ea[e], a[i])
            assert er[e] == (rewards[i, j - 1] if j else rew[i]) and ed[e] == d[i]
    for cols in ([3, 3], [5, 1], [-1, 2]):
        with pytest.raises(ValueError):
            _hindsight_expand([s, a, s2, rew, d], (0, 2), 3, cols, K, goals, rewards)
