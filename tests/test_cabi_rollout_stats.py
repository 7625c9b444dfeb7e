"""CPU checks of the rollout-statistics calls at the C-ABI boundary (include/td3.h: rs_*): exported,
bound with the argument types of ``SIGNATURES``, the ctypes structs laid out as the header's, and
every documented argument check -- in the header's order -- made before the handle is looked at and
before any GPU work, so a null handle reaches them without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_SYMBOLS = ("rs_create", "rs_destroy", "rs_tick", "rs_info", "rs_get_state", "rs_set_state", "rs_read_episodes")


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def test_rs_symbols_exported_and_bound(lib):
    from td3_amd import _lib
    for s in RS_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound in td3_amd/_lib.py"
        assert getattr(lib, s).restype is _lib.SIGNATURES[s][0] is C.c_int
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    for s in RS_SYMBOLS:
        assert re.search(r"^int %s\(" % s, txt, flags=re.M), f"{s} not declared in include/td3.h"
    assert "csrc/rollout.hip" in __import__("td3_amd.build", fromlist=["SOURCES"]).SOURCES


def _header_struct(name):
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for d in (d.strip() for d in body.split(";")):
        if d:                                            # "type a, b" or "const type* a"
            parts = d.split(",")
            names.append(parts[0].split()[-1].lstrip("*"))
            names += [p.strip().lstrip("*") for p in parts[1:]]
    return names


@pytest.mark.parametrize("name,size", [("rs_config", 48), ("rs_tick_t", 64), ("rs_episode", 24),
                                       ("rs_info_t", 64), ("rs_state", 112)])
def test_rs_structs_match_header(name, size):
    from td3_amd import _lib
    st = getattr(_lib, name)
    assert [f[0] for f in st._fields_] == _header_struct(name)
    assert C.sizeof(st) == size


def test_episode_dtype_is_the_struct():
    from td3_amd import _lib
    from td3_amd.rollout_stats import EPISODE_DTYPE
    assert EPISODE_DTYPE.itemsize == C.sizeof(_lib.rs_episode) == 24
    for f, _ in _lib.rs_episode._fields_:
        assert EPISODE_DTYPE.fields[f][1] == getattr(_lib.rs_episode, f).offset


def _cfg(**kw):
    from td3_amd import _lib
    cfg = _lib.rs_config()
    cfg.obs_eps, cfg.obs_clip, cfg.rew_eps, cfg.rew_clip, cfg.gamma = 1e-8, 10.0, 1e-8, 10.0, 0.99
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("args,cfg,field", [
    ((0, 3, 8), {}, b"rows"), ((-1, 3, 8), {}, b"rows"), (((1 << 24) + 1, 3, 8), {}, b"rows"),
    ((4, 0, 8), {}, b"obs_dim"), ((4, (1 << 20) + 1, 8), {}, b"obs_dim"),
    ((4, 3, 0), {}, b"log_cap"), ((4, 3, (1 << 24) + 1), {}, b"log_cap"),
    ((4, 3, 8), None, b"null cfg"),
    ((4, 3, 8), dict(obs_eps=-1.0), b"cfg->obs_eps"), ((4, 3, 8), dict(obs_eps=NAN), b"cfg->obs_eps"),
    ((4, 3, 8), dict(obs_clip=0.0), b"cfg->obs_clip"), ((4, 3, 8), dict(obs_clip=INF), b"cfg->obs_clip"),
    ((4, 3, 8), dict(rew_eps=-1e-9), b"cfg->rew_eps"),
    ((4, 3, 8), dict(rew_clip=-1.0), b"cfg->rew_clip"), ((4, 3, 8), dict(rew_clip=NAN), b"cfg->rew_clip"),
    ((4, 3, 8), dict(gamma=1.5), b"cfg->gamma"), ((4, 3, 8), dict(gamma=-0.1), b"cfg->gamma"),
    ((4, 3, 8), dict(gamma=NAN), b"cfg->gamma")])
def test_rs_create_errors_name_the_field(lib, args, cfg, field):
    h = C.c_void_p()
    c = None if cfg is None else C.byref(_cfg(**cfg))
    assert lib.rs_create(*args, 0, c, C.byref(h)) == -1
    assert field in lib.td3_last_error(), lib.td3_last_error()
    assert not h.value


def test_rs_create_checks_come_in_the_documented_order(lib):
    h = C.c_void_p()
    bad = _cfg(obs_eps=-1.0, obs_clip=0.0, rew_eps=-1.0, rew_clip=0.0, gamma=2.0)
    order = [((0, 0, 0), None, b"out is null", None), ((0, 0, 0), None, b"rows", h), ((4, 0, 0), None, b"obs_dim", h),
             ((4, 3, 0), None, b"log_cap", h), ((4, 3, 8), None, b"null cfg", h), ((4, 3, 8), bad, b"cfg->obs_eps", h)]
    for args, cfg, field, out in order:
        assert lib.rs_create(*args, 0, None if cfg is None else C.byref(cfg), None if out is None else C.byref(out)) == -1
        assert field in lib.td3_last_error(), (field, lib.td3_last_error())
    for fix, field in (("obs_eps", b"cfg->obs_clip"), ("obs_clip", b"cfg->rew_eps"), ("rew_eps", b"cfg->rew_clip"),
                       ("rew_clip", b"cfg->gamma")):
        setattr(bad, fix, 1.0)
        assert lib.rs_create(4, 3, 8, 0, C.byref(bad), C.byref(h)) == -1
        assert field in lib.td3_last_error(), (field, lib.td3_last_error())


def _tick(**kw):
    from td3_amd import _lib
    buf = (C.c_float * 64)()
    a = _lib.rs_tick_t()
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, C.cast(buf, C.c_void_p) if v is True else v)
    return a


def test_rs_tick_checks_come_in_the_documented_order(lib):
    def err(a):
        assert lib.rs_tick(None, None if a is None else C.byref(a), None) == -1
        return lib.td3_last_error()
    assert b"null a" in err(None)
    assert b"a->update" in err(_tick(update=2, obs_out=True, ended=True))
    assert b"a->update" in err(_tick(update=-1))
    assert b"a->obs_out" in err(_tick(obs_out=True, next_obs_out=True, reward_out=True, ended=True))
    assert b"a->next_obs_out" in err(_tick(obs=True, obs_out=True, next_obs_out=True, reward_out=True, ended=True))
    assert b"a->reward_out" in err(_tick(next_obs=True, next_obs_out=True, reward_out=True, ended=True))
    assert b"a->ended" in err(_tick(ended=True))
    for ok in (_tick(), _tick(update=1, obs=True, next_obs=True, reward=True, ended=True, obs_out=True,
                              next_obs_out=True, reward_out=True), _tick(obs=True), _tick(reward=True, update=1)):
        e = err(ok)                                      # self-consistent arguments: the handle is next
        assert b"null handle" in e and b"a->" not in e, e


def _state(**kw):
    from td3_amd import _lib
    buf = (C.c_double * 64)()
    st = _lib.rs_state()
    st._keep = buf
    for k in ("mean", "m2", "G", "ep_return", "ep_len", "log"):
        setattr(st, k, C.cast(buf, C.c_void_p))
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def test_rs_state_checks_come_in_the_documented_order(lib):
    ptrs = ("mean", "m2", "G", "ep_return", "ep_len", "log")
    for call in (lib.rs_get_state, lib.rs_set_state):
        assert call(None, None) == -1
        assert b"null st" in lib.td3_last_error()
        for j, k in enumerate(ptrs):                     # the first null pointer is the one named
            assert call(None, C.byref(_state(**{q: None for q in ptrs[j:]}))) == -1
            assert b"st->%s is null" % k.encode() in lib.td3_last_error(), lib.td3_last_error()
        assert call(None, C.byref(_state())) == -1
        assert b"null handle" in lib.td3_last_error()
    scal = (("count", -1.0), ("ret_count", NAN), ("ep_count", -1), ("ep_len_sum", -1), ("tick", -1))
    for j, (k, _) in enumerate(scal):
        assert lib.rs_set_state(None, C.byref(_state(**dict(scal[j:])))) == -1
        assert b"st->%s must be" % k.encode() in lib.td3_last_error(), lib.td3_last_error()
    assert lib.rs_set_state(None, C.byref(_state(count=-1.0, mean=None))) == -1      # pointers before scalars
    assert b"st->mean is null" in lib.td3_last_error()
    assert lib.rs_get_state(None, C.byref(_state(count=-1.0))) == -1                 # get does not read them
    assert b"null handle" in lib.td3_last_error()


def test_rs_read_episodes_and_info_checks(lib):
    from td3_amd import _lib
    out = (_lib.rs_episode * 4)()
    f, n = C.c_int64(), C.c_int64()
    call = lib.rs_read_episodes
    assert call(None, -1, -1, None, None, None) == -1
    assert b"first must be >= 0" in lib.td3_last_error()
    assert call(None, 0, -1, None, None, None) == -1
    assert b"n must be >= 0" in lib.td3_last_error()
    assert call(None, 0, 4, None, None, None) == -1
    assert b"out is null" in lib.td3_last_error() and b"first_out" not in lib.td3_last_error()
    assert call(None, 0, 4, out, None, None) == -1
    assert b"first_out is null" in lib.td3_last_error()
    assert call(None, 0, 0, None, C.byref(f), None) == -1         # n == 0 needs no out
    assert b"n_out is null" in lib.td3_last_error()
    assert call(None, 0, 4, out, C.byref(f), C.byref(n)) == -1
    assert b"null handle" in lib.td3_last_error()
    assert lib.rs_info(None, None) == -1
    assert b"null info" in lib.td3_last_error()
    assert lib.rs_info(None, C.byref(_lib.rs_info_t())) == -1
    assert b"null handle" in lib.td3_last_error()
    assert lib.rs_destroy(None) == 0


def test_python_surface_imports_without_gpu():
    import inspect
    from td3_amd import loop, rollout_stats as rs
    assert list(inspect.signature(rs.RolloutStats.__init__).parameters)[1:] == [
        "n_envs", "obs_dim", "gamma", "obs_clip", "rew_clip", "eps", "col_mask", "log_cap", "device"]
    assert list(inspect.signature(rs.NormalizedVecEnv.__init__).parameters)[1:] == [
        "env", "stats", "norm_obs", "norm_reward", "update"]
    assert list(inspect.signature(rs.evaluate_device).parameters)[:4] == ["policy", "env", "stats", "episodes"]
    p = inspect.signature(loop.DeviceTrainLoop.__init__).parameters
    assert p["log_every"].default == 0 and p["on_log"].default is None
