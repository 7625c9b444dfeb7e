"""ctypes binding of libtd3hip.so (the C-ABI declared in include/td3.h).

The library is built in-tree by ``td3_amd.build`` (hipcc, gfx950).  There is no
fallback: if the shared object is missing or fails to load, importing the
product modules raises -- the HIP path is the only compute path.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtd3hip.so")


class rb_info_t(C.Structure):
    _fields_ = [("state_dim", C.c_int), ("action_dim", C.c_int), ("record_floats", C.c_int),
                ("max_size", C.c_int64), ("ptr", C.c_int64), ("size", C.c_int64),
                ("data", C.c_void_p), ("device", C.c_int),
                ("n_particles", C.c_int), ("particle_dim", C.c_int)]


class td3_config(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("state_dim", C.c_int), ("action_dim", C.c_int),
                ("actor_hidden", C.c_int * 3), ("critic_hidden", C.c_int * 3),
                ("norm", C.c_int), ("max_action", C.c_float),
                ("discount", C.c_double), ("tau", C.c_double), ("policy_noise", C.c_double),
                ("noise_clip", C.c_double), ("policy_freq", C.c_int),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("seed", C.c_uint64), ("device", C.c_int),
                ("use_graph", C.c_int), ("particles", C.c_int), ("n_particles", C.c_int),
                ("particle_dim", C.c_int), ("cdq", C.c_int)]


class td3_step_stats(C.Structure):
    _fields_ = [("critic_loss", C.c_double), ("actor_loss", C.c_double), ("actor_step", C.c_int),
                ("y", C.c_void_p), ("q1", C.c_void_p), ("q2", C.c_void_p), ("idx", C.c_void_p),
                ("noise", C.c_void_p)]


class td3_explore(C.Structure):
    _fields_ = [("x", C.c_void_p), ("mu", C.c_float), ("theta", C.c_float), ("sigma", C.c_float),
                ("reset", C.c_void_p), ("seed", C.c_uint64), ("step", C.c_uint64),
                ("inject_z", C.c_void_p), ("z_out", C.c_void_p)]


class rb_hindsight(C.Structure):
    _fields_ = [("k", C.c_int), ("g", C.c_int), ("cols", C.c_int * 8), ("goals", C.c_void_p),
                ("rewards", C.c_void_p)]


class rb_nstep(C.Structure):
    _fields_ = [("n", C.c_int), ("gamma", C.c_double), ("ended", C.c_void_p)]


class rb_priority_info_t(C.Structure):
    _fields_ = [("enabled", C.c_int), ("alpha", C.c_double), ("eps", C.c_double), ("levels", C.c_int),
                ("total", C.c_double), ("max_priority", C.c_float)]


class td3_per_stats(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("td_abs", C.c_void_p)]


class rs_config(C.Structure):
    _fields_ = [("obs_eps", C.c_double), ("obs_clip", C.c_double), ("rew_eps", C.c_double),
                ("rew_clip", C.c_double), ("gamma", C.c_double), ("col_mask", C.c_void_p)]


class rs_tick_t(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("next_obs", C.c_void_p), ("reward", C.c_void_p), ("ended", C.c_void_p),
                ("obs_out", C.c_void_p), ("next_obs_out", C.c_void_p), ("reward_out", C.c_void_p),
                ("update", C.c_int)]


class rs_episode(C.Structure):
    _fields_ = [("ret", C.c_float), ("len", C.c_int32), ("row", C.c_int32), ("reserved", C.c_int32),
                ("tick", C.c_int64)]


class rs_info_t(C.Structure):
    _fields_ = [("rows", C.c_int), ("obs_dim", C.c_int), ("log_cap", C.c_int), ("device", C.c_int),
                ("ep_count", C.c_int64), ("ep_len_sum", C.c_int64), ("tick", C.c_int64),
                ("ep_return_sum", C.c_double), ("count", C.c_double), ("ret_count", C.c_double)]


class rs_state(C.Structure):
    _fields_ = [("count", C.c_double), ("mean", C.c_void_p), ("m2", C.c_void_p),
                ("ret_count", C.c_double), ("ret_mean", C.c_double), ("ret_m2", C.c_double),
                ("G", C.c_void_p), ("ep_return", C.c_void_p), ("ep_len", C.c_void_p), ("log", C.c_void_p),
                ("ep_count", C.c_int64), ("ep_len_sum", C.c_int64), ("tick", C.c_int64),
                ("ep_return_sum", C.c_double)]


class rb_norm_info_t(C.Structure):
    _fields_ = [("normalized", C.c_int), ("obs_dim", C.c_int), ("rows", C.c_int64)]


class td3_log_entry(C.Structure):
    _fields_ = [("step", C.c_int64), ("batch", C.c_int32), ("actor_step", C.c_int32), ("prioritized", C.c_int32),
                ("nonfinite", C.c_int32), ("critic_loss", C.c_double), ("actor_loss", C.c_double),
                ("q1_mean", C.c_double), ("q2_mean", C.c_double), ("y_mean", C.c_double),
                ("q_min", C.c_double), ("q_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double),
                ("q_gap_mean", C.c_double), ("td_abs_mean", C.c_double), ("td_abs_max", C.c_double),
                ("w_mean", C.c_double), ("w_min", C.c_double)]


class td3_bc_info_t(C.Structure):
    _fields_ = [("enabled", C.c_int), ("alpha", C.c_double), ("step", C.c_int64), ("lambda", C.c_double),
                ("q_abs_mean", C.c_double), ("bc_loss", C.c_double)]


class td3_bc_filter_info_t(C.Structure):
    _fields_ = [("demo_rows", C.c_int), ("q_filter", C.c_int), ("step", C.c_int64), ("n_demo", C.c_int64),
                ("kept", C.c_int64), ("bc_loss", C.c_double)]


class td3_clip_info_t(C.Structure):
    _fields_ = [("enabled", C.c_int * 2), ("max_norm", C.c_double * 2), ("step", C.c_int64 * 2),
                ("grad_norm", C.c_double * 2), ("coef", C.c_double * 2)]


class td3_log_info_t(C.Structure):
    _fields_ = [("enabled", C.c_int), ("capacity", C.c_int), ("every", C.c_int), ("count", C.c_int64)]


_P = C.c_void_p
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes); every symbol of include/td3.h.
SIGNATURES = {
    "rb_create": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "rb_destroy": (C.c_int, [_P]),
    "rb_info": (C.c_int, [_P, C.POINTER(rb_info_t)]),
    "rb_stream": (_P, [_P]),
    "rb_add": (C.c_int, [_P, _D, _D, _D, _D, _D, C.c_int64, _P]),
    "rb_add_records": (C.c_int, [_P, _F, C.c_int64, _P]),
    "rb_add_device": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rb_add_particles_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rb_add_device_hindsight": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(rb_hindsight), _P]),
    "rb_add_particles_device_hindsight": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64,
                                                    C.POINTER(rb_hindsight), _P]),
    "rb_add_device_nstep": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(rb_nstep), _P]),
    "rb_add_particles_device_nstep": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64,
                                                C.POINTER(rb_nstep), _P]),
    "rb_fill_synthetic": (C.c_int, [_P, C.c_int64, C.c_float, C.c_uint64, _P]),
    "rb_sample": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rb_enable_priorities": (C.c_int, [_P, C.c_double, C.c_double, _P]),
    "rb_set_priorities": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rb_update_priorities": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rb_sample_prioritized": (C.c_int, [_P, C.c_int, C.c_double, _P, _P, _P, _P]),
    "rb_get_priorities": (C.c_int, [_P, C.c_int64, C.c_int64, _F]),
    "rb_priority_info": (C.c_int, [_P, C.POINTER(rb_priority_info_t)]),
    "rs_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(rs_config), C.POINTER(_P)]),
    "rs_destroy": (C.c_int, [_P]),
    "rs_tick": (C.c_int, [_P, C.POINTER(rs_tick_t), _P]),
    "rs_info": (C.c_int, [_P, C.POINTER(rs_info_t)]),
    "rs_get_state": (C.c_int, [_P, C.POINTER(rs_state)]),
    "rs_set_state": (C.c_int, [_P, C.POINTER(rs_state)]),
    "rs_read_episodes": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(rs_episode), _I64, _I64]),
    "rb_state_moments": (C.c_int, [_P, _P, C.c_int, _P]),
    "rb_normalize_states": (C.c_int, [_P, _P, _P]),
    "rb_norm_info": (C.c_int, [_P, C.POINTER(rb_norm_info_t)]),
    "rb_read_records": (C.c_int, [_P, C.c_int64, C.c_int64, _F]),
    "rb_write_records": (C.c_int, [_P, C.c_int64, C.c_int64, _F, C.c_int64, C.c_int64]),
    "rb_sync": (C.c_int, [_P]),
    "rb_create_particles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_uint64,
                                      C.POINTER(_P)]),
    "rb_add_particles": (C.c_int, [_P, _D, _D, _D, _D, _D, _D, _D, C.c_int64, _P]),
    "rb_sample_particles": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "td3_config_size": (C.c_size_t, []),
    "td3_default_config": (C.c_int, [C.POINTER(td3_config), C.c_size_t]),
    "td3_create": (C.c_int, [C.POINTER(td3_config), C.POINTER(_P)]),
    "td3_destroy": (C.c_int, [_P]),
    "td3_tensor_count": (C.c_int, [_P, C.c_int]),
    "td3_tensor_info": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, C.c_int, _I64, _I64]),
    "td3_num_params": (C.c_int64, [_P, C.c_int]),
    "td3_get_params": (C.c_int, [_P, C.c_int, _F, C.c_int64]),
    "td3_set_params": (C.c_int, [_P, C.c_int, _F, C.c_int64]),
    "td3_get_counters": (C.c_int, [_P, _I64, _I64, _I64]),
    "td3_set_counters": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64]),
    "td3_set_adam": (C.c_int, [_P, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "td3_get_adam": (C.c_int, [_P, C.c_int, _D]),
    "td3_train_step": (C.c_int, [_P, _P, C.c_int, _P, _I64, _F, C.POINTER(td3_step_stats)]),
    "td3_train_step_prioritized": (C.c_int, [_P, _P, C.c_int, C.c_double, _P, _F, _F,
                                             C.POINTER(td3_step_stats), C.POINTER(td3_per_stats)]),
    "td3_train_step_prioritized_particles": (C.c_int, [_P, _P, C.c_int, C.c_double, _P, _F, _F,
                                                       C.POINTER(td3_step_stats), C.POINTER(td3_per_stats)]),
    "td3_train_step_batch": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _P, _F,
                                       C.POINTER(td3_step_stats)]),
    "td3_select_action": (C.c_int, [_P, _F, _F, C.c_int]),
    "td3_eval_q": (C.c_int, [_P, _F, _F, _F, C.c_int]),
    "td3_select_action_device": (C.c_int, [_P, _P, C.c_int, C.POINTER(td3_explore), _P, _P]),
    "td3_eval_q_device": (C.c_int, [_P, _P, _P, C.c_int, _P, _P]),
    "td3_select_action_particles_device": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(td3_explore), _P, _P]),
    "td3_eval_q_particles_device": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P]),
    "td3_train_step_batch_particles": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _F,
                                                 C.POINTER(td3_step_stats)]),
    "td3_actor_learn_particles": (C.c_int, [_P, _P, _P, C.c_int, _P, _D]),
    "td3_select_action_particles": (C.c_int, [_P, _F, _F, _F, C.c_int]),
    "td3_eval_q_particles": (C.c_int, [_P, _F, _F, _F, _F, C.c_int]),
    "td3_log_entry_size": (C.c_size_t, []),
    "td3_log_enable": (C.c_int, [_P, C.c_int, C.c_int]),
    "td3_log_info": (C.c_int, [_P, C.POINTER(td3_log_info_t)]),
    "td3_log_read": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(td3_log_entry), _I64, _I64]),
    "td3_log_set": (C.c_int, [_P, C.POINTER(td3_log_entry), C.c_int64, C.c_int64]),
    "td3_set_bc": (C.c_int, [_P, C.c_double]),
    "td3_bc_info": (C.c_int, [_P, C.POINTER(td3_bc_info_t)]),
    "td3_set_bc_filter": (C.c_int, [_P, C.c_int, C.c_int]),
    "td3_bc_filter_info": (C.c_int, [_P, C.POINTER(td3_bc_filter_info_t)]),
    "td3_bc_filter_keep": (C.c_int, [_P, _F, C.c_int]),
    "td3_set_grad_clip": (C.c_int, [_P, C.c_int, C.c_double]),
    "td3_clip_info": (C.c_int, [_P, C.POINTER(td3_clip_info_t)]),
    "td3_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "td3_comm_init": (C.c_int, [_P, C.POINTER(C.c_ubyte), C.c_int, C.c_int]),
    "td3_comm_init_local": (C.c_int, [C.POINTER(_P), C.c_int]),
    "td3_dp_gather_optimizer_state": (C.c_int, [_P]),
    "td3_train_step_local": (C.c_int, [C.POINTER(_P), C.POINTER(_P), C.c_int, C.c_int, _I64, _F,
                                       C.POINTER(td3_step_stats)]),
    "td3_sync": (C.c_int, [_P]),
    "td3_stream": (_P, [_P]),
    "td3_profile_stages": (C.c_int, [_P, _P, C.c_int, C.c_int, _F, C.c_int, C.POINTER(C.c_int)]),
    "td3_stage_name": (C.c_char_p, [_P, C.c_int]),
    "td3_stage_kernel": (C.c_char_p, [_P, C.c_int]),
    "td3_debug_last_stage": (C.c_char_p, [_P, C.c_int, C.c_int]),
    "td3_time_stage": (C.c_int, [_P, C.c_int, C.c_int, _F]),
    "td3_probe_kernel": (C.c_int, [_P, _P, C.c_int, C.c_char_p, C.c_int, _F, C.POINTER(C.c_int)]),
    "td3_stage_flops": (C.c_double, [_P, C.c_int]),
    "td3_stage_bytes": (C.c_double, [_P, C.c_int]),
    "td3_debug_activation": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int]),
    "td3_debug_plan_flags": (C.c_int, [_P, _P]),
    "td3_debug_per_stage": (C.c_int, [_P, _P, C.c_int, _P]),
    "td3_train_step_mixed": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _I64, _F,
                                       C.POINTER(td3_step_stats)]),
    "td3_debug_mixed_input": (C.c_int, [_P, _P, _P, _P]),
    "td3_debug_log_launch": (C.c_int, [_P, _P]),
    "td3_debug_row_lds": (C.c_int, []),
    "td3_debug_act_fail": (C.c_int, [_P, C.c_int]),
    "td3_debug_query_route": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "td3_last_error": (C.c_char_p, []),
}

TD3_ACTOR, TD3_ACTOR_TARGET, TD3_CRITIC, TD3_CRITIC_TARGET = 0, 1, 2, 3
TD3_ACTOR_ADAM_M, TD3_ACTOR_ADAM_V, TD3_CRITIC_ADAM_M, TD3_CRITIC_ADAM_V = 4, 5, 6, 7
TD3_ACTOR_GRAD, TD3_CRITIC_GRAD = 8, 9

_lib = None
_shutting_down = False


def _mark_shutdown():
    global _shutting_down
    _shutting_down = True


atexit.register(_mark_shutdown)


def alive() -> bool:
    """False once interpreter shutdown started (destructors must not call into HIP then)."""
    return _lib is not None and not _shutting_down


def load(path: str = LIB_PATH):
    """Load libtd3hip.so and declare every exported signature (raises if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own ROCm runtime (torch/lib/libamdhip64.so, soname
    # libamdhip64.so.7).  Loading torch first makes our DT_NEEDED libamdhip64.so.7 /
    # libhsa-runtime64.so.1 / librccl.so.1 resolve to those already-loaded copies, so the
    # process has ONE HIP runtime and torch streams / pointers are valid in our calls.
    import torch  # noqa: F401
    path = os.environ.get("TD3_LIB", path)       # kernel-variant experiments (tools/)
    if not os.path.exists(path):
        raise ImportError(
            f"libtd3hip.so not found at {path}: build it with `python -m td3_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class TD3Error(RuntimeError):
    pass


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = _lib.td3_last_error().decode(errors="replace") if _lib is not None else ""
        raise TD3Error(f"{what} failed ({rc}): {msg}")


def default_config():
    """A td3_config filled with the library's defaults (TD3_base / TD3_featured hyper-parameters);
    raises when this binding's struct layout differs from the library's include/td3.h."""
    lib = load()
    if C.sizeof(td3_config) != lib.td3_config_size():
        raise TD3Error(f"td3_config binding is {C.sizeof(td3_config)} bytes, libtd3hip's "
                       f"{lib.td3_config_size()}: td3_amd/_lib.py is out of date with include/td3.h")
    cfg = td3_config()
    check(lib.td3_default_config(C.byref(cfg), C.sizeof(cfg)), "td3_default_config")
    return cfg


def fptr(a):
    """float* of a C-contiguous float32 numpy array."""
    return a.ctypes.data_as(_F)


def i64ptr(a):
    return a.ctypes.data_as(_I64)


def dptr(a):
    return a.ctypes.data_as(_D)
