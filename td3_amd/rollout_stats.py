"""Rollout statistics of a GPU-resident vector environment (include/td3.h, "rollout statistics").

``RolloutStats`` keeps running observation moments, running moments of the discounted return and a
log of finished episodes in device memory; ``tick`` is one kernel launch on torch's current stream
and reads nothing back.  ``NormalizedVecEnv`` wraps a vector environment of ``td3_amd.loop`` (what
gym's ``NormalizeObservation`` / ``NormalizeReward`` wrappers do on the host) so that
``DeviceTrainLoop`` runs on it unchanged: the rows it stores are the normalised ones, and the train
step, the fused gather, n-step and prioritized replay work on them as they are.  ``evaluate_device``
is ``main.py``'s ``eval_policy`` for such an environment.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

__all__ = ["RolloutStats", "NormalizedVecEnv", "evaluate_device", "EPISODE_DTYPE"]

# rs_episode of include/td3.h
EPISODE_DTYPE = np.dtype([("ret", "<f4"), ("len", "<i4"), ("row", "<i4"), ("reserved", "<i4"), ("tick", "<i8")])
_STATE_ARRAYS = ("mean", "m2", "G", "ep_return", "ep_len", "log")
_STATE_SCALARS = ("count", "ret_count", "ret_mean", "ret_m2", "ep_count", "ep_len_sum", "tick", "ep_return_sum")
_CONFIG = ("n_envs", "obs_dim", "log_cap", "gamma", "obs_clip", "rew_clip", "eps")


def _torch():
    import torch
    return torch


class RolloutStats:
    """Running normalisation and the episode log for ``n_envs`` rows of ``obs_dim`` columns.

    ``col_mask`` (``[obs_dim]``, optional): a zero takes the column out of normalisation (copied
    through bit for bit, no moments kept), e.g. the goal columns a hindsight relabel overwrites."""

    def __init__(self, n_envs, obs_dim, *, gamma, obs_clip=10.0, rew_clip=10.0, eps=1e-8, col_mask=None,
                 log_cap=4096, device=None):
        from .my_replay_buffer import default_device_index
        self._lib = _lib.load()
        self._h = None
        self.n_envs, self.obs_dim, self.log_cap = int(n_envs), int(obs_dim), int(log_cap)
        self.gamma, self.obs_clip, self.rew_clip, self.eps = float(gamma), float(obs_clip), float(rew_clip), float(eps)
        if col_mask is None:
            self.col_mask = np.ones(max(self.obs_dim, 0), np.uint8)
        else:
            self.col_mask = (np.asarray(col_mask).reshape(-1) != 0).astype(np.uint8)
            if self.col_mask.shape[0] != self.obs_dim:
                raise ValueError(f"col_mask must have obs_dim = {self.obs_dim} entries, got {self.col_mask.shape[0]}")
        self._dev = default_device_index() if device is None else int(getattr(device, "index", device) or 0)
        self.device = _torch().device("cuda", self._dev)
        cfg = _lib.rs_config()
        cfg.obs_eps = cfg.rew_eps = self.eps
        cfg.obs_clip, cfg.rew_clip, cfg.gamma = self.obs_clip, self.rew_clip, self.gamma
        cfg.col_mask = self.col_mask.ctypes.data
        h = C.c_void_p()
        check(self._lib.rs_create(self.n_envs, self.obs_dim, self.log_cap, self._dev, C.byref(cfg), C.byref(h)),
              "rs_create")
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and _lib.alive():
                self._lib.rs_destroy(self._h)
        except Exception:
            pass
        self._h = None

    # ------------------------------------------------------------------ the tick
    def _rows(self, x, width, name, inplace):
        """``x`` as a contiguous fp32 tensor ``[n_envs][width]`` (``[n_envs]`` for width 0) on the device."""
        torch = _torch()
        if not getattr(x, "is_cuda", False):
            raise TypeError(f"tick: {name} must be a CUDA tensor (the statistics live on the device)")
        shape = (self.n_envs, width) if width else (self.n_envs,)
        if x.dtype is torch.float32 and x.device == self.device and tuple(x.shape) == shape and x.is_contiguous():
            return x                           # the loop's case: no torch op in front of the launch
        t = x.to(self.device, torch.float32).reshape(shape).contiguous()
        if inplace and t.data_ptr() != x.data_ptr():
            raise ValueError(f"tick: inplace needs {name} to be a contiguous float32 tensor on {self.device}")
        return t

    def tick(self, obs=None, next_obs=None, reward=None, ended=None, *, update=True, norm_obs=True,
             norm_reward=True, inplace=False):
        """One environment tick (``rs_tick``: one launch on torch's current stream, nothing read back).

        ``obs`` ``[n_envs][obs_dim]`` are the rows the next actions are chosen from (after
        auto-reset), ``next_obs`` the transition's own next state, ``reward`` ``[n_envs]``, ``ended``
        ``[n_envs]`` bool / uint8; each may be None.  With ``update`` the moments take in ``obs`` and
        the discounted returns; ``update=False`` freezes them (evaluation) while episodes are still
        logged.  Returns ``(obs, next_obs, reward)`` normalised with the moments as they stand after
        the update (None where the input is None or its ``norm_*`` is off), in fresh tensors, or
        written over the inputs with ``inplace``."""
        torch = _torch()
        a = _lib.rs_tick_t()
        a.update = 1 if update else 0
        keep, outs = [], [None, None, None]
        for j, (x, w, name, want) in enumerate(((obs, self.obs_dim, "obs", norm_obs),
                                                (next_obs, self.obs_dim, "next_obs", norm_obs),
                                                (reward, 0, "reward", norm_reward))):
            if x is None:
                continue
            t = self._rows(x, w, name, inplace and want)
            keep.append(t)
            setattr(a, name, t.data_ptr())
            if want:
                outs[j] = t if inplace else torch.empty_like(t)
                setattr(a, name + "_out", outs[j].data_ptr())
        if ended is not None:
            if reward is None:
                raise ValueError("tick: ended needs reward")
            if not getattr(ended, "is_cuda", False) or ended.dtype not in (torch.bool, torch.uint8):
                raise TypeError("tick: ended must be a bool or uint8 CUDA tensor")
            e = ended                          # a contiguous bool [n_envs] is read as it is: one byte per row
            if e.device != self.device or e.dim() != 1 or not e.is_contiguous():
                e = ended.to(self.device).reshape(-1).contiguous()
            if e.shape[0] != self.n_envs:
                raise ValueError(f"tick: ended must have one entry per row ({self.n_envs}), got {e.shape[0]}")
            keep.append(e)
            a.ended = e.data_ptr()
        # inputs and outputs belong to torch's current stream, and so does the launch: stream order
        # alone puts it behind the ops that made the inputs, and the allocator may reuse `keep` after it
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.rs_tick(self._h, C.byref(a), C.c_void_p(stream)), "rs_tick")
        del keep
        return tuple(outs)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """Every moment, accumulator, counter and the log ring as numpy values (synchronises)."""
        arrs = {"mean": np.empty(self.obs_dim, np.float64), "m2": np.empty(self.obs_dim, np.float64),
                "G": np.empty(self.n_envs, np.float64), "ep_return": np.empty(self.n_envs, np.float64),
                "ep_len": np.empty(self.n_envs, np.int32), "log": np.zeros(self.log_cap, EPISODE_DTYPE)}
        st = _lib.rs_state()
        for k in _STATE_ARRAYS:
            setattr(st, k, arrs[k].ctypes.data)
        check(self._lib.rs_get_state(self._h, C.byref(st)), "rs_get_state")
        sd = dict(arrs)
        for k in _STATE_SCALARS:
            v = getattr(st, k)
            sd[k] = np.float64(v) if isinstance(v, float) else np.int64(v)
        for k in _CONFIG:
            sd[k] = np.asarray(getattr(self, k))
        sd["col_mask"] = self.col_mask.copy()
        return sd

    def load_state_dict(self, sd, moments_only=False):
        """Adopt a ``state_dict`` (same ``n_envs`` / ``obs_dim`` / ``log_cap``; synchronises).  With
        ``moments_only`` only the observation and return moments are taken -- the row count may
        differ, accumulators and the log are cleared: the frozen copy an evaluation runs on."""
        if int(sd["obs_dim"]) != self.obs_dim:
            raise ValueError(f"state has obs_dim {int(sd['obs_dim'])}, this handle {self.obs_dim}")
        if not np.array_equal(np.asarray(sd["col_mask"]).reshape(-1) != 0, self.col_mask != 0):
            raise ValueError("state was made with another col_mask")
        if not moments_only and (int(sd["n_envs"]), int(sd["log_cap"])) != (self.n_envs, self.log_cap):
            raise ValueError(f"state has n_envs / log_cap {int(sd['n_envs'])} / {int(sd['log_cap'])}, "
                             f"this handle {self.n_envs} / {self.log_cap}")
        arrs = {"mean": np.ascontiguousarray(sd["mean"], np.float64), "m2": np.ascontiguousarray(sd["m2"], np.float64)}
        if moments_only:
            arrs.update(G=np.zeros(self.n_envs, np.float64), ep_return=np.zeros(self.n_envs, np.float64),
                        ep_len=np.zeros(self.n_envs, np.int32), log=np.zeros(self.log_cap, EPISODE_DTYPE))
        else:
            arrs.update(G=np.ascontiguousarray(sd["G"], np.float64),
                        ep_return=np.ascontiguousarray(sd["ep_return"], np.float64),
                        ep_len=np.ascontiguousarray(sd["ep_len"], np.int32),
                        log=np.ascontiguousarray(sd["log"], EPISODE_DTYPE))
        want = {"mean": self.obs_dim, "m2": self.obs_dim, "G": self.n_envs, "ep_return": self.n_envs,
                "ep_len": self.n_envs, "log": self.log_cap}
        for k, n in want.items():
            if arrs[k].shape != (n,):
                raise ValueError(f"state entry {k} has shape {arrs[k].shape}, expected ({n},)")
        st = _lib.rs_state()
        for k in _STATE_ARRAYS:
            setattr(st, k, arrs[k].ctypes.data)
        for k in _STATE_SCALARS:
            keep = k in ("count", "ret_count", "ret_mean", "ret_m2") or not moments_only
            v = sd[k] if keep else 0
            setattr(st, k, float(v) if isinstance(getattr(st, k), float) else int(v))
        check(self._lib.rs_set_state(self._h, C.byref(st)), "rs_set_state")

    def save(self, path):
        """The ``state_dict`` as one ``.npz``."""
        np.savez(path, **self.state_dict())

    def load(self, path):
        with np.load(path) as z:
            self.load_state_dict({k: z[k] for k in z.files})

    def frozen_copy(self, n_envs=None):
        """A new handle for ``n_envs`` rows with this one's configuration and moments and empty
        accumulators and log: what an evaluation ticks with ``update=False``."""
        other = RolloutStats(self.n_envs if n_envs is None else n_envs, self.obs_dim, gamma=self.gamma,
                             obs_clip=self.obs_clip, rew_clip=self.rew_clip, eps=self.eps, col_mask=self.col_mask,
                             log_cap=self.log_cap, device=self._dev)
        other.load_state_dict(self.state_dict(), moments_only=True)
        return other

    def host_normalizer(self):
        """``f(x) -> float32`` with the observation moments read once (synchronises now, never again):
        ``rs_tick`` step 2 in numpy -- fp64, one rounding, masked columns and ``count == 0`` passed
        through -- for host loops in ``main.py``'s style (``state = f(state)`` before ``select_action``
        and ``add``) on a ring normalised with these moments."""
        sd = self.state_dict()
        count, mean, clip = float(sd["count"]), sd["mean"].copy(), self.obs_clip
        on = self.col_mask != 0
        den = np.sqrt(sd["m2"] / count + self.eps) if count > 0 else np.ones_like(mean)

        def f(x):
            x = np.asarray(x, np.float32)
            if count == 0:
                return x.copy()
            y = np.clip((x.astype(np.float64) - mean) / den, -clip, clip).astype(np.float32)
            return np.where(on, y, x)
        return f

    # ------------------------------------------------------------------ the log
    def info(self):
        inf = _lib.rs_info_t()
        check(self._lib.rs_info(self._h, C.byref(inf)), "rs_info")
        return inf

    def episodes(self, first=0):
        """The logged episodes with sequence numbers >= ``first`` that are still in the ring (the
        last ``log_cap``), oldest first: a structured array with fields ``seq``, ``ret``, ``len``,
        ``row``, ``tick`` (synchronises)."""
        raw = np.zeros(self.log_cap, EPISODE_DTYPE)
        f0, n = C.c_int64(), C.c_int64()
        check(self._lib.rs_read_episodes(self._h, int(first), 1 << 62,
                                         raw.ctypes.data_as(C.POINTER(_lib.rs_episode)), C.byref(f0), C.byref(n)),
              "rs_read_episodes")
        out = np.zeros(n.value, np.dtype([("seq", "<i8"), ("ret", "<f4"), ("len", "<i4"), ("row", "<i4"),
                                          ("tick", "<i8")]))
        out["seq"] = f0.value + np.arange(n.value)
        for k in ("ret", "len", "row", "tick"):
            out[k] = raw[k][:n.value]
        return out

    def summary(self):
        """Counters of the run so far (synchronises): episodes, their mean return and length, ticks."""
        i = self.info()
        n = max(int(i.ep_count), 1)
        return {"episodes": int(i.ep_count), "mean_return": i.ep_return_sum / n, "mean_length": i.ep_len_sum / n,
                "tick": int(i.tick), "count": float(i.count), "ret_count": float(i.ret_count)}


class NormalizedVecEnv:
    """A vector environment of ``td3_amd.loop`` seen through a ``RolloutStats``: ``state`` and the
    ``next_state`` / ``reward`` that ``step`` returns are normalised, by one ``stats.tick`` per step
    (``reset`` ticks with the observations only).  The inner environment keeps its raw state.  Tuple
    states (``SyntheticParticleVecEnv``) normalise the features and pass the particles through.
    ``update=False`` freezes the moments.  Everything else (``goal_cols``, ``sample_goals``, ...) is
    the inner environment's."""

    def __init__(self, env, stats, *, norm_obs=True, norm_reward=True, update=True):
        if stats.n_envs != env.n_envs:
            raise ValueError(f"stats has {stats.n_envs} rows, the environment {env.n_envs}")
        self.env, self.stats = env, stats
        self.norm_obs, self.norm_reward, self.update = bool(norm_obs), bool(norm_reward), bool(update)
        self.n_envs = env.n_envs
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self._max_episode_steps = env._max_episode_steps
        self.state = None
        self._last_next = (None, None)         # (normalised, raw) next_state of the last step

    def __getattr__(self, name):               # only what this class does not define itself
        if "env" not in self.__dict__:
            raise AttributeError(name)
        return getattr(self.__dict__["env"], name)

    @staticmethod
    def _feat(state):
        return state[0] if isinstance(state, tuple) else state

    @staticmethod
    def _with_feat(state, feat):
        return (feat, *state[1:]) if isinstance(state, tuple) else feat

    def reset(self):
        raw = self.env.reset()
        obs, _, _ = self.stats.tick(obs=self._feat(raw), update=self.update, norm_obs=self.norm_obs)
        self.state = self._with_feat(raw, obs) if self.norm_obs else raw
        return self.state

    def step(self, action):
        nxt, reward, done, time_limit = self.env.step(action)
        raw = self.env.state
        obs, nobs, rew = self.stats.tick(obs=self._feat(raw), next_obs=self._feat(nxt), reward=reward, ended=done,
                                         update=self.update, norm_obs=self.norm_obs, norm_reward=self.norm_reward)
        self.state = self._with_feat(raw, obs) if self.norm_obs else raw
        out = self._with_feat(nxt, nobs) if self.norm_obs else nxt
        self._last_next = (out, nxt)
        return out, (rew if self.norm_reward else reward), done, time_limit

    def imagine_reward(self, next_state, goals):
        """The inner environment's hook on the RAW next state: the loop hands back the normalised
        ``next_state`` this wrapper returned from ``step``.  A relabelled reward cannot be scaled as the
        stored one is without reading the scale back, so hindsight needs ``norm_reward=False``."""
        if self.norm_reward:
            raise ValueError("hindsight relabels need norm_reward=False: a relabelled reward would not be scaled")
        norm, raw = self._last_next
        return self.env.imagine_reward(raw if next_state is norm else next_state, goals)


def evaluate_device(policy, env, stats, episodes, *, poll_every=8, max_ticks=None):
    """``main.py``'s ``eval_policy`` on a GPU-resident vector environment: the noise-free policy on
    ``env`` (a raw evaluation environment) seen through a frozen copy of ``stats`` -- its moments,
    ``update=False``, its own accumulators and log, so ``stats`` itself is not touched -- until
    ``episodes`` episodes are logged.  The counters are read back every ``poll_every`` ticks, not every
    tick.  Returns the mean return and length of the first ``episodes`` episodes logged (row order
    within a tick)."""
    episodes = int(episodes)
    if episodes < 1:
        raise ValueError("episodes must be >= 1")
    ev = stats.frozen_copy(env.n_envs)
    if episodes + int(poll_every) * env.n_envs > ev.log_cap:
        raise ValueError(f"log_cap {ev.log_cap} cannot hold {episodes} episodes between two polls")
    wenv = NormalizedVecEnv(env, ev, norm_reward=False, update=False)
    state = wenv.reset()
    t = 0
    while True:
        wenv.step(policy.select_action_device(state))
        state = wenv.state
        t += 1
        if t % int(poll_every) == 0 and ev.info().ep_count >= episodes:
            break
        if max_ticks is not None and t >= int(max_ticks):
            raise RuntimeError(f"evaluate_device: {int(ev.info().ep_count)} of {episodes} episodes after {t} ticks")
    eps = ev.episodes()[:episodes]
    return float(eps["ret"].astype(np.float64).mean()), float(eps["len"].astype(np.float64).mean())
