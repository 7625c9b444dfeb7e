"""The acting / training loop around the learner.

``TrainLoop.run`` keeps the order of the reference's main loop (``main.py:240-289``): act
(uniform random before ``start_policy``, else ``select_action`` + OU noise, clipped), ``env.step``,
``add_to_replay_buffer`` (the transition and its hindsight relabels), then one ``policy.train``
per environment step once ``t >= start_training``; episode ends reset the env and the noise.

What runs where on MI355X:

* ``policy.train`` only enqueues the captured step graph (no host sync), so ``env.step`` of the
  next iteration runs on the host while the GPU trains;
* ``select_action`` runs behind a queued step that changes the online actor in that step's own
  stream (``td3_handle::actor_stream``: stream order, no event), and otherwise on the learner's
  acting stream.  After critic-only steps (``total_it % policy_freq != 0``) it therefore overlaps
  the training step, and its result is still exactly the sequential one: the actor it reads is the
  same;
* ``add_to_replay_buffer`` hands the transition and all its relabels to the ring in one batched
  ``rb_add`` (pinned staging, async copy on the ring's stream; ``train`` waits on its event), the
  env-specific reward / state hooks staying on the host (``main.py:70-91``).

The gym / MuJoCo / SPlisHSPlasH environments are not part of this build (not installed here);
``SyntheticEnv`` is a gym-shaped stand-in with a configurable host cost per step, used by
``bench.py --loop`` and the tests.

``DeviceTrainLoop`` is the same order for environments that live on the GPU (``SyntheticVecEnv``:
the stand-in as torch ops on ``[n_envs]`` device rows): ``select_action_device`` applies policy,
OU noise and clip on the device, ``add_batch`` on CUDA tensors assembles the ring records from
device memory, and no transition crosses the host (``tools/bench_rollout.py``).  With
``SyntheticParticleVecEnv`` (states are ``(features, particles)`` tuples) and the particle learner
and ring it is the same loop: ``rb_add_particles_device`` builds the wide records in the ring and the
query's encoder reads the simulator's particle tensor in place.  With ``relabel=`` (hindsight,
``SyntheticGoalVecEnv``) each tick's transitions and their K relabels are stored by one fan-out add
(``add_batch_hindsight``): the relabelled rows are never built outside the ring.  With ``n_step=n``
each tick is stored by ``add_batch_nstep``: the rows of the previous n - 1 ticks mature in the ring into
multi-step transitions (include/td3.h), the train step unchanged.  ``rollout_stats.NormalizedVecEnv``
around any of these environments adds running observation / reward normalisation and an episode log
kept on the device (one launch per tick); ``log_every`` / ``on_log`` are where the loop reads it.
"""
from __future__ import annotations

import time

import numpy as np

from .exploration import OrnsteinUhlenbeckActionNoise

__all__ = ["add_to_replay_buffer", "TrainLoop", "SyntheticEnv", "Box", "SyntheticVecEnv",
           "SyntheticParticleVecEnv", "SyntheticGoalVecEnv", "hindsight_relabel", "DeviceTrainLoop"]


def add_to_replay_buffer(replay_buffer, state, action, reward, next_state, done_bool, relabels=()):
    """``main.py:70-91``: store the transition, then every hindsight relabel
    ``(manip_state, manip_next_state, manip_reward)`` computed by the env hooks, as one batch."""
    relabels = list(relabels)
    if not relabels:
        replay_buffer.add(state, action, next_state, reward, done_bool)
        return
    n = 1 + len(relabels)
    s = np.stack([np.asarray(state, np.float64)] + [np.asarray(m[0], np.float64) for m in relabels])
    s2 = np.stack([np.asarray(next_state, np.float64)] + [np.asarray(m[1], np.float64) for m in relabels])
    r = np.array([float(reward)] + [float(m[2]) for m in relabels], np.float64)
    a = np.repeat(np.asarray(action, np.float64).reshape(1, -1), n, axis=0)
    d = np.full(n, float(done_bool), np.float64)
    replay_buffer.add_batch(s, a, s2, r, d)


class Box:
    """The part of ``gym.spaces.Box`` the loop and the learners use: ``shape``, ``low``/``high``
    and ``sample()`` (uniform, numpy's global RNG)."""

    def __init__(self, low, high, shape):
        self.shape = tuple(shape)
        self.low = np.full(self.shape, low, np.float64)
        self.high = np.full(self.shape, high, np.float64)

    def sample(self):
        return np.random.uniform(self.low, self.high)


class SyntheticEnv:
    """Gym-shaped stand-in: s' = tanh(W s + U a), r = -|s'|^2 / sd, episodes of fixed length.
    ``step_cost_us`` busy-waits to model a simulator's host time per step."""

    def __init__(self, state_dim, action_dim, max_action=1.0, max_episode_steps=1000, step_cost_us=0.0,
                 seed=0):
        rs = np.random.RandomState(seed)
        self.observation_space = Box(-np.inf, np.inf, (state_dim,))
        self.action_space = Box(-max_action, max_action, (action_dim,))
        self._W = rs.standard_normal((state_dim, state_dim)) / np.sqrt(state_dim)
        self._U = rs.standard_normal((state_dim, action_dim)) / np.sqrt(action_dim)
        self._max_episode_steps = int(max_episode_steps)
        self._cost = float(step_cost_us) * 1e-6
        self._rs = rs
        self._t = 0
        self._s = None

    def reset(self):
        self._t = 0
        self._s = self._rs.standard_normal(self.observation_space.shape[0]) * 0.1
        return self._s.copy()

    def step(self, action):
        t0 = time.perf_counter()
        a = np.asarray(action, np.float64).reshape(-1)
        self._s = np.tanh(self._W @ self._s + self._U @ a)
        self._t += 1
        r = -float(self._s @ self._s) / len(self._s)
        done = self._t >= self._max_episode_steps
        while self._cost and time.perf_counter() - t0 < self._cost:
            pass
        return self._s.copy(), r, done, {}


class TrainLoop:
    """``main.py:240-289`` without evaluation, checkpoints and the RTPT progress bar (out of
    scope); ``relabel(env, state, action, reward, next_state, done_bool)`` may return hindsight
    relabels for ``add_to_replay_buffer``; ``on_episode_end(info)`` is called at episode ends."""

    def __init__(self, env, policy, replay_buffer, *, max_action, start_policy=0, start_training=0,
                 batch_size=256, expl_noise=0.1, done_swap=True, relabel=None, on_episode_end=None):
        self.env, self.policy, self.replay_buffer = env, policy, replay_buffer
        self.max_action = max_action
        self.start_policy, self.start_training = int(start_policy), int(start_training)
        self.batch_size = int(batch_size)
        self.noise = OrnsteinUhlenbeckActionNoise(env.action_space.shape[0], sigma=expl_noise)
        self.done_swap = done_swap
        self.relabel = relabel
        self.on_episode_end = on_episode_end

    def run(self, max_timesteps):
        env, policy, rb = self.env, self.policy, self.replay_buffer
        state, done = env.reset(), False
        episode_reward, episode_timesteps, episode_num, grad_steps = 0.0, 0, 0, 0
        t0 = time.perf_counter()
        for t in range(int(max_timesteps)):
            episode_timesteps += 1
            if t < self.start_policy:
                action = env.action_space.sample()
            else:
                action = (policy.select_action(state) + self.noise.sample()).clip(-self.max_action,
                                                                                  self.max_action)
            next_state, reward, done, _ = env.step(action)
            if self.done_swap:
                done_bool = float(done) if episode_timesteps < env._max_episode_steps else 0.0
            else:
                done_bool = float(done)
            relabels = self.relabel(env, state, action, reward, next_state, done_bool) if self.relabel else ()
            add_to_replay_buffer(rb, state, action, reward, next_state, done_bool, relabels)
            state = next_state
            episode_reward += reward
            if t >= self.start_training:
                policy.train(rb, self.batch_size)
                grad_steps += 1
            if done:
                if self.on_episode_end:
                    self.on_episode_end({"t": t, "episode": episode_num, "reward": episode_reward,
                                         "length": episode_timesteps})
                state, done = env.reset(), False
                self.noise.reset()
                episode_reward, episode_timesteps = 0.0, 0
                episode_num += 1
        if hasattr(policy, "sync"):
            policy.sync()
        dt = time.perf_counter() - t0
        return {"env_steps": int(max_timesteps), "grad_steps": grad_steps, "episodes": episode_num,
                "seconds": dt, "env_steps_per_s": int(max_timesteps) / dt if dt > 0 else 0.0}


class SyntheticVecEnv:
    """``n_envs`` copies of ``SyntheticEnv``'s dynamics as torch ops on device rows (a stand-in for a
    batched GPU simulator): s' = tanh(s W^T + a U^T), r = -|s'|^2 / sd, episodes of fixed length,
    fp32.  Finished rows reset themselves: ``step`` returns the transition's own
    ``(next_state, reward, done, time_limit)`` (``time_limit``: the episode ended at
    ``max_episode_steps``, main.py:256's done swap) while ``state`` already holds the observation
    the next action is chosen from, i.e. the fresh one on the rows that ended."""

    def __init__(self, n_envs, state_dim, action_dim, max_action=1.0, max_episode_steps=1000, seed=0,
                 device=None):
        import torch
        rs = np.random.RandomState(seed)
        self.n_envs = int(n_envs)
        self.observation_space = Box(-np.inf, np.inf, (state_dim,))
        self.action_space = Box(-max_action, max_action, (action_dim,))
        self.device = torch.device("cuda") if device is None else torch.device(device)
        W = rs.standard_normal((state_dim, state_dim)) / np.sqrt(state_dim)
        U = rs.standard_normal((state_dim, action_dim)) / np.sqrt(action_dim)
        self._Wt = torch.as_tensor(W.T.copy(), dtype=torch.float32, device=self.device)
        self._Ut = torch.as_tensor(U.T.copy(), dtype=torch.float32, device=self.device)
        self._max_episode_steps = int(max_episode_steps)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self._t = torch.zeros(self.n_envs, dtype=torch.int64, device=self.device)
        self.state = None

    def _fresh(self):
        import torch
        return 0.1 * torch.randn((self.n_envs, self._Wt.shape[0]), generator=self._gen, device=self.device,
                                 dtype=torch.float32)

    def reset(self):
        self._t.zero_()
        self.state = self._fresh()
        return self.state

    def step(self, action):
        import torch
        nxt = torch.tanh(self.state @ self._Wt + action.to(torch.float32) @ self._Ut)
        reward = -(nxt * nxt).sum(dim=1) / nxt.shape[1]
        self._t += 1
        done = self._t >= self._max_episode_steps
        self.state = torch.where(done[:, None], self._fresh(), nxt)
        self._t.masked_fill_(done, 0)
        return nxt, reward, done, done.clone()


class SyntheticParticleVecEnv:
    """The particle-observation stand-in (the water-pouring environment's shapes): ``state`` is the
    tuple (features ``[n_envs][F]``, particles ``[n_envs][N][D]``) of fp32 device tensors,
    p' = tanh(p P^T + a V^T) per particle, f' = tanh(f W^T + a U^T + mean_N(p) M^T),
    r = -|f'|^2 / F, episodes of fixed length.  Auto-reset and the ``step`` return as
    ``SyntheticVecEnv``, with ``next_state`` a tuple too."""

    def __init__(self, n_envs, feat_dim, n_particles, particle_dim, action_dim, max_action=1.0,
                 max_episode_steps=1000, seed=0, device=None):
        import torch
        rs = np.random.RandomState(seed)
        F, N, D, A = int(feat_dim), int(n_particles), int(particle_dim), int(action_dim)
        self.n_envs = int(n_envs)
        self.observation_space = (Box(-np.inf, np.inf, (F,)), Box(-np.inf, np.inf, (N, D)))
        self.action_space = Box(-max_action, max_action, (A,))
        self.device = torch.device("cuda") if device is None else torch.device(device)

        def mat(rows, cols):                   # x [.., rows] @ mat -> [.., cols], unit-variance rows in
            m = rs.standard_normal((rows, cols)) / np.sqrt(rows)
            return torch.as_tensor(m, dtype=torch.float32, device=self.device)

        self._Wt, self._Ut, self._Mt = mat(F, F), mat(A, F), mat(D, F)
        self._Pt, self._Vt = mat(D, D), mat(A, D)
        self._dims = (F, N, D)
        self._max_episode_steps = int(max_episode_steps)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self._t = torch.zeros(self.n_envs, dtype=torch.int64, device=self.device)
        self.state = None

    def _fresh(self):
        import torch
        F, N, D = self._dims
        kw = dict(generator=self._gen, device=self.device, dtype=torch.float32)
        return 0.1 * torch.randn((self.n_envs, F), **kw), torch.randn((self.n_envs, N, D), **kw)

    def reset(self):
        self._t.zero_()
        self.state = self._fresh()
        return self.state

    def step(self, action):
        import torch
        f, p = self.state
        a = action.to(torch.float32)
        p2 = torch.tanh(p @ self._Pt + (a @ self._Vt)[:, None, :])
        f2 = torch.tanh(f @ self._Wt + a @ self._Ut + p.mean(dim=1) @ self._Mt)
        reward = -(f2 * f2).sum(dim=1) / f2.shape[1]
        self._t += 1
        done = self._t >= self._max_episode_steps
        ff, fp = self._fresh()
        self.state = (torch.where(done[:, None], ff, f2), torch.where(done[:, None, None], fp, p2))
        self._t.masked_fill_(done, 0)
        return (f2, p2), reward, done, done.clone()


class SyntheticGoalVecEnv(SyntheticVecEnv):
    """A goal-conditioned ``SyntheticVecEnv`` (the shape of the reference's own environment, whose
    observation carries the goal parameters ``manip_state`` overwrites): the leading
    ``state_dim - goal_dim`` columns are the physical state with ``SyntheticVecEnv``'s dynamics, the
    last ``goal_dim`` columns are goal weights, drawn per row at reset (uniform in [0, 1)), held
    through the episode and copied into ``next_state``.  The reward is
    r = -|p'|^2 / P + sum_g w_g p'_g over the physical next state p' and the goal weights w.
    ``sample_goals`` and ``imagine_reward`` are the two hooks of a hindsight ``relabel``
    (``env._imagine_reward`` / ``env.manip_state``, main.py:70-91); ``goal_cols`` are the columns."""

    def __init__(self, n_envs, state_dim, action_dim, goal_dim, max_action=1.0, max_episode_steps=1000, seed=0,
                 device=None):
        self.goal_dim = int(goal_dim)
        self.phys_dim = int(state_dim) - self.goal_dim
        if not 1 <= self.goal_dim <= self.phys_dim:
            raise ValueError("goal_dim must be in 1..state_dim / 2 (the reward weighs goal_dim physical columns)")
        super().__init__(n_envs, self.phys_dim, action_dim, max_action=max_action,
                         max_episode_steps=max_episode_steps, seed=seed, device=device)
        self.observation_space = Box(-np.inf, np.inf, (int(state_dim),))
        self.goal_cols = list(range(self.phys_dim, int(state_dim)))

    def _fresh(self):
        import torch
        w = torch.rand((self.n_envs, self.goal_dim), generator=self._gen, device=self.device, dtype=torch.float32)
        return torch.cat([super()._fresh(), w], dim=1)

    def sample_goals(self, k):
        """``[n_envs][k][goal_dim]`` fresh goal weights, from the distribution of ``reset``."""
        import torch
        return torch.rand((self.n_envs, int(k), self.goal_dim), generator=self._gen, device=self.device,
                          dtype=torch.float32)

    def imagine_reward(self, next_state, goals):
        """The reward of reaching ``next_state`` (``[n][state_dim]``; its own goal columns are not
        read) under ``goals``: ``[n][goal_dim]`` -> ``[n]``, ``[n][k][goal_dim]`` -> ``[n][k]``."""
        P, G = self.phys_dim, self.goal_dim
        p = next_state[:, :P]
        base = -(p * p).sum(dim=1) / P
        if goals.dim() == 2:
            return base + (goals * p[:, :G]).sum(dim=1)
        return base[:, None] + (goals * p[:, None, :G]).sum(dim=2)

    def step(self, action):
        import torch
        P = self.phys_dim
        w = self.state[:, P:]
        nxt = torch.cat([torch.tanh(self.state[:, :P] @ self._Wt + action.to(torch.float32) @ self._Ut), w], dim=1)
        reward = self.imagine_reward(nxt, w)
        self._t += 1
        done = self._t >= self._max_episode_steps
        self.state = torch.where(done[:, None], self._fresh(), nxt)
        self._t.masked_fill_(done, 0)
        return nxt, reward, done, done.clone()


def hindsight_relabel(k):
    """A ``relabel`` for ``DeviceTrainLoop`` (``--hindsight_number k``, main.py:70-91) over an
    environment with ``goal_cols``, ``sample_goals`` and ``imagine_reward``: k fresh goals per row
    and the reward the transition would have earned under each."""
    def relabel(env, state, action, reward, next_state, done_bool):
        goals = env.sample_goals(k)
        return env.goal_cols, goals, env.imagine_reward(next_state, goals)
    return relabel


class DeviceTrainLoop:
    """``main.py:240-289``'s order per tick over all rows of a GPU-resident vector environment
    (``state`` attribute, ``reset()``, ``step(actions) -> (next_state, reward, done, time_limit)``
    on device tensors, auto-reset as ``SyntheticVecEnv``): act (uniform before ``start_policy``
    ticks, else the policy with device OU noise), ``env.step``, ``add_batch`` of the n transitions,
    ``train_steps_per_tick`` gradient steps from tick ``start_training`` on; rows whose episode
    ended have their noise reset at the next query.  Every piece only queues GPU work
    (``select_action_device``, ``rb_add_device``, ``train``): the host reads nothing back and
    keeps only the tick counter.  A state may be one tensor (featured learner and ring) or the
    tuple ``(features, particles)`` of ``SyntheticParticleVecEnv`` (particle learner and ring).

    ``relabel(env, state, action, reward, next_state, done_bool)``, when given, returns the tick's
    hindsight relabels ``(goal_cols, goals [n][K][G], rewards [n][K])`` (main.py:70-91; goals and
    rewards device tensors, made by the environment's own torch ops); the tick then stores each
    transition and its K relabels through ``add_batch_hindsight``, still without a host copy.

    ``n_step`` > 1 stores each tick through ``add_batch_nstep(..., ended=done, n=n_step,
    gamma=policy.discount)``: the rows of the previous ``n_step - 1`` ticks mature in the ring into
    multi-step transitions, with no read-back of ``done``.  The stored ``done`` is still ``done_bool``,
    so a time-limit end under ``done_swap`` bootstraps and stops maturing.  Not with ``relabel=``.

    ``on_log(t, loop)``, when given with ``log_every`` > 0, is called after every ``log_every``-th tick
    (``t`` counts the ticks done): the place to read ``rollout_stats.RolloutStats.summary()`` of a
    ``NormalizedVecEnv`` or to evaluate.  What it reads back is its own cost; off by default."""

    def __init__(self, env, policy, replay_buffer, *, start_policy, start_training, batch_size, expl_noise,
                 done_swap=True, train_steps_per_tick=1, seed=0, relabel=None, n_step=1, log_every=0, on_log=None):
        from .exploration import DeviceOUNoise
        self.n_step = int(n_step)
        if self.n_step < 1:
            raise ValueError(f"n_step must be >= 1, got {n_step}")
        if self.n_step > 1 and relabel is not None:
            raise ValueError("n_step > 1 cannot be combined with relabel= (n-step hindsight rows are not supported)")
        self.env, self.policy, self.replay_buffer = env, policy, replay_buffer
        self.start_policy, self.start_training = int(start_policy), int(start_training)
        self.batch_size = int(batch_size)
        self.done_swap = done_swap
        self.train_steps_per_tick = int(train_steps_per_tick)
        self.relabel = relabel
        self.log_every, self.on_log = int(log_every), on_log
        self.max_action = float(policy.max_action)
        self.noise = DeviceOUNoise(env.n_envs, policy.action_dim, sigma=expl_noise, device=policy.device,
                                   seed=seed)

    def run(self, max_ticks):
        import torch
        env, policy, rb = self.env, self.policy, self.replay_buffer
        n, ad, ma = env.n_envs, policy.action_dim, self.max_action
        state = env.reset()
        ended = None                          # rows whose episode ended at the previous tick
        grad_steps = 0
        t0 = time.perf_counter()
        for t in range(int(max_ticks)):
            if t < self.start_policy:
                action = (torch.rand((n, ad), device=policy.device, dtype=torch.float32) * 2 - 1) * ma
                if ended is not None:
                    self.noise.reset(ended)
            else:
                action = policy.select_action_device(state, noise=self.noise, reset=ended)
            next_state, reward, done, time_limit = env.step(action)
            done_bool = (done & ~time_limit) if self.done_swap else done
            rows = (*state, action, *next_state) if isinstance(state, tuple) else (state, action, next_state)
            if self.n_step > 1:
                rb.add_batch_nstep(*rows, reward, done_bool, ended=done, n=self.n_step, gamma=policy.discount)
            elif self.relabel is None:
                rb.add_batch(*rows, reward, done_bool)
            else:
                cols, goals, rewards = self.relabel(env, state, action, reward, next_state, done_bool)
                rb.add_batch_hindsight(*rows, reward, done_bool, goal_cols=cols, goals=goals, rewards=rewards)
            state, ended = env.state, done
            if t >= self.start_training:
                for _ in range(self.train_steps_per_tick):
                    policy.train(rb, self.batch_size)
                    grad_steps += 1
            if self.on_log is not None and self.log_every > 0 and (t + 1) % self.log_every == 0:
                self.on_log(t + 1, self)
        policy.sync()
        torch.cuda.synchronize(policy.device)
        dt = time.perf_counter() - t0
        steps = int(max_ticks) * n
        return {"ticks": int(max_ticks), "env_steps": steps, "grad_steps": grad_steps, "seconds": dt,
                "env_steps_per_s": steps / dt if dt > 0 else 0.0}
