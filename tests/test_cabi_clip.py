"""CPU checks of the gradient-clipping calls at the C-ABI boundary (include/td3.h: td3_set_grad_clip,
td3_clip_info): exported, bound with the argument types of ``SIGNATURES``, the ctypes struct laid out as the
header's, and the refusals that need no GPU made before any GPU work, in the header's order (a null handle
reaches them without one)."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_cabi_train_log import C_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_SYMBOLS = ("td3_set_grad_clip", "td3_clip_info")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_clip_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    for s in CLIP_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    assert _lib.SIGNATURES["td3_set_grad_clip"][1] == [C.c_void_p, C.c_int, C.c_double]
    assert re.search(r"^int td3_set_grad_clip\(td3_handle\* h, int group, double max_norm\);", txt, flags=re.M)
    assert _lib.SIGNATURES["td3_clip_info"][1] == [C.c_void_p, C.POINTER(_lib.td3_clip_info_t)]
    assert re.search(r"^int td3_clip_info\(td3_handle\* h, td3_clip_info_t\* info\);", txt, flags=re.M)


def _header_arrays(name):
    """[(field, C type, length)] of a struct of scalar arrays in include/td3.h, in order."""
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for d in (d.strip() for d in body.split(";")):
        if d:
            ctype, field, n = re.fullmatch(r"(\w+)\s+(\w+)\[(\d+)\]", d).groups()
            out.append((field, ctype, int(n)))
    return out


def test_clip_info_struct_matches_header(lib):
    from td3_amd import _lib
    st = _lib.td3_clip_info_t
    fields = _header_arrays("td3_clip_info_t")
    assert [f[0] for f in st._fields_] == [f[0] for f in fields] == ["enabled", "max_norm", "step", "grad_norm", "coef"]
    off = 0
    for name, ctype, n in fields:                        # the C rules for naturally aligned scalar arrays
        sz = C_SIZES[ctype]
        off = (off + sz - 1) // sz * sz
        assert getattr(st, name).offset == off and getattr(st, name).size == sz * n == sz * 2, name
        off += sz * n
    assert C.sizeof(st) == (off + 7) // 8 * 8 == 72


def test_the_other_structs_are_untouched(lib):
    """A setter and a query, not fields: td3_config and its size guard, td3_step_stats and td3_log_entry stay."""
    from td3_amd import _lib
    assert C.sizeof(_lib.td3_config) == lib.td3_config_size()
    assert C.sizeof(_lib.td3_log_entry) == lib.td3_log_entry_size() == 136
    for name in ("td3_config", "td3_step_stats", "td3_log_entry"):
        assert not any("grad" in f[0] or "max_norm" in f[0] or "coef" in f[0]
                       for f in getattr(_lib, name)._fields_), name      # (td3_config.noise_clip is TD3's own)
    assert [f[0] for f in _lib.td3_step_stats._fields_] == ["critic_loss", "actor_loss", "actor_step", "y", "q1", "q2",
                                                            "idx", "noise"]


@pytest.mark.parametrize("max_norm", [-1.0, -1e-30, float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("group", [0, 1, 2, -1])
def test_bad_max_norm_is_refused_before_the_group(lib, max_norm, group):
    assert lib.td3_set_grad_clip(None, group, max_norm) == -1
    err = lib.td3_last_error()
    assert b"max_norm" in err and b"group must" not in err and b"null handle" not in err, err


@pytest.mark.parametrize("group", [2, -1, 7])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_bad_group_is_refused_before_the_handle(lib, group, max_norm):
    assert lib.td3_set_grad_clip(None, group, max_norm) == -1
    err = lib.td3_last_error()
    assert b"group" in err and b"null handle" not in err, err


def test_null_arguments(lib):
    from td3_amd import _lib
    for group in (0, 1):
        for max_norm in (0.0, 1.0):
            assert lib.td3_set_grad_clip(None, group, max_norm) == -1
            assert b"null handle" in lib.td3_last_error()
    assert lib.td3_clip_info(None, None) == -1
    assert b"null info" in lib.td3_last_error()
    assert lib.td3_clip_info(None, C.byref(_lib.td3_clip_info_t())) == -1
    assert b"null handle" in lib.td3_last_error()


def test_python_surface_imports_without_gpu():
    from td3_amd import TD3_featured, TD3_particles
    for mod in (TD3_featured, TD3_particles):
        p = inspect.signature(mod.TD3.__init__).parameters
        assert p["max_grad_norm"].default is None
        assert isinstance(inspect.getattr_static(mod.TD3, "max_grad_norm"), property)
        assert callable(mod.TD3.clip_info)
    # the particle class's earlier parameters keep their places
    names = list(inspect.signature(TD3_particles.TD3.__init__).parameters)
    assert names[:11] == ["self", "obs_space", "action_space", "lr", "norm", "CDQ", "device", "seed", "use_graph",
                          "init", "per_beta"]


def test_weight_normalization_is_refused_before_a_handle_exists(lib):
    from td3_amd.TD3_featured import TD3

    class Box:
        def __init__(self, shape):
            self.shape = tuple(shape)

    for v in (1.0, (None, 0.5)):
        with pytest.raises(ValueError, match="weight_normalization"):
            TD3(Box((3,)), Box((1,)), norm="weight_normalization", max_grad_norm=v)
    with pytest.raises(ValueError, match="actor, critic"):
        TD3(Box((3,)), Box((1,)), norm="weight_normalization", max_grad_norm=(1.0, 2.0, 3.0))


def test_the_kernels_have_a_translation_unit_of_their_own():
    from td3_amd import build
    assert "csrc/clip.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "td3_amd", "csrc", "clip.hip")).read()
    assert "grad_sqsum_kernel" in src and "adam_flat_clip_kernel" in src
    for other in ("kernels.hip", "kernels_optim.h", "bc.hip"):
        txt = open(os.path.join(ROOT, "td3_amd", "csrc", other)).read()
        assert "grad_sqsum" not in txt and "adam_flat_clip" not in txt and "ClipDev" not in txt, other
