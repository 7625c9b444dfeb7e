#!/usr/bin/env python3
"""Env-steps/s of a rollout on a GPU-resident vector environment: host-vector path vs device path.

    python tools/bench_rollout.py [--config featured|particles] [--ticks K] [--warmup W] [--train-steps T]
                                  [--hindsight K | --nstep N [--n-envs E] [--repeats R]] [--out FILE]

Both paths act on the same ``SyntheticVecEnv`` (HalfCheetah dims: 17 / 6, torch ops on device rows)
with the same learner and replay ring, act -> env.step -> add per tick over ``n_envs`` rows:

* ``host``: what the API offered before the device entry points: states copied to the host,
  ``select_action_batch`` + numpy Ornstein-Uhlenbeck noise + clip, actions copied to the device for
  ``env.step``, the transition copied back to the host for the numpy ``add_batch``;
* ``device``: ``select_action_device`` (policy + OU noise + clip in HIP kernels) and ``add_batch`` on
  the CUDA tensors (``rb_add_device``): no copy, no synchronisation, the host keeps the tick counter.

``--train-steps T`` adds T ``train(256)`` calls per tick to both (default 0: the rollout alone).
One JSON line per ``n_envs`` in {1, 16, 256}, with the host time per call of the device path's two
entry points (they only queue work, so this is their whole host cost).  Not the BASELINE metric.

``--config particles`` is the same comparison for the particle learner on ``SyntheticParticleVecEnv``
at the water-pouring dims (features 7, particles 350 x 9, actions 3; a transition is a 6,320-float
record): ``select_action_batch`` on host tuples and the float64 ``add_batch`` against
``select_action_device`` on the simulator's tensors and ``rb_add_particles_device``.  Each line also
gives the device add's achieved GB/s at that ``n_envs``: bytes read from the seven source arrays plus
bytes written to the ring, over the add kernel's device time between two events on the ring's stream
(median of 20 adds).  ``--add-rows R`` appends one line with that figure alone for an add of R rows
(a streaming size: whether the kernel or the launch bounds the small adds).

``--hindsight K`` (either config; ``--n-envs``, default 256) measures the device path with K hindsight
relabels per transition (main.py:70-91) instead, two forms of the store in the same run:

* ``fanout``: ``add_batch_hindsight`` (``rb_add_device_hindsight`` / ``rb_add_particles_device_hindsight``:
  each source row read once, written 1 + K times with the goal columns and the reward patched);
* ``expand``: what the API offered before it: the n * (1 + K) rows built with torch
  (``repeat_interleave`` + index assignments) and handed to ``add_batch``.

One JSON line: for each form the add's effective GB/s (ring bytes written + source bytes read, the same
numerator for both, over the device time of one call) and the env-steps/s of ``DeviceTrainLoop`` with a
``relabel`` (median of ``--repeats`` alternated runs), the two ratios, and the fan-out kernel's own time
between two events on the ring's stream (the method of the plain add's ``device_add_gb_per_s``).

``--nstep N`` (either config; ``--n-envs``, default 256) measures the n-step add
(``rb_add_device_nstep`` / ``rb_add_particles_device_nstep``) instead.  One JSON line: the device time
of one n-step add in steady state (no episode ends: every row matures its N - 1 predecessors) next to
the plain device add's at the same shapes, both between two events on the ring's stream (median of 20
after a warm-up); the algorithmic bytes written by each (the records, plus per maturing copy the
next-state block and the two scalars) and the n-step add's time predicted from them at the plain add's
achieved bytes per second; and the env-steps/s of ``DeviceTrainLoop`` with ``n_step=N`` against
``n_step=1`` (median of ``--repeats`` alternated runs).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SD, AD, MA = 17, 6, 1.0
PF, PN, PD, PA = 7, 350, 9, 3            # the particle configuration (water-pouring dims)


def host_rollout_particles(env, pol, rb, ticks, train_steps, batch, sigma=0.1, theta=0.1):
    import torch
    n = env.n_envs
    X = np.zeros((n, PA))
    env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        f, p = (x.cpu().numpy() for x in env.state)
        X = X + (theta * (0.0 - X) + sigma * np.random.randn(n, PA))
        a = (pol.select_action_batch((f, p)) + X).clip(-MA, MA)
        (f2, p2), r, d, tl = env.step(torch.as_tensor(a, dtype=torch.float32).to(env.device))
        d_h = d.cpu().numpy()
        rb.add_batch(f, p, a, f2.cpu().numpy(), p2.cpu().numpy(), r.cpu().numpy(), (d & ~tl).cpu().numpy())
        X[d_h] = 0.0
        for _ in range(train_steps):
            pol.train(rb, batch)
    pol.sync()
    torch.cuda.synchronize()
    return ticks * n / (time.perf_counter() - t0)


def device_add_gbps(env, rb, reps=20):
    """Achieved GB/s of rb_add_particles_device at the env's n_envs: (bytes read + bytes written) over
    the kernel's device time between two events on the ring's stream, median of `reps` adds."""
    import torch
    n = env.n_envs
    (f, p), a = env.reset(), torch.zeros((n, PA), device=env.device)
    (f2, p2), r, d, _ = env.step(a)
    ts = [t.to(torch.float32).reshape(n, -1).contiguous() for t in (f, p, a, f2, p2, r, d)]
    stream = torch.cuda.ExternalStream(int(rb._lib.rb_stream(rb.handle)), device=env.device)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = rb._lib.rb_add_particles_device(rb.handle, *[t.data_ptr() for t in ts], n, None)
        e1.record(stream)
        assert rc == 0, rb._lib.td3_last_error()
        stream.synchronize()
        ms.append(e0.elapsed_time(e1))
    nbytes = 4 * n * (sum(t.shape[1] for t in ts) + rb.record_floats)
    t = float(np.median(ms)) * 1e-3
    return nbytes / t / 1e9, 1e6 * t


def host_rollout(env, pol, rb, ticks, train_steps, batch, sigma=0.1, theta=0.1):
    import torch
    n = env.n_envs
    X = np.zeros((n, AD))
    env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        s = env.state.cpu().numpy()
        X = X + (theta * (0.0 - X) + sigma * np.random.randn(n, AD))
        a = (pol.select_action_batch(s) + X).clip(-MA, MA)
        s2, r, d, tl = env.step(torch.as_tensor(a, dtype=torch.float32).to(env.device))
        d_h = d.cpu().numpy()
        rb.add_batch(s, a, s2.cpu().numpy(), r.cpu().numpy(), (d & ~tl).cpu().numpy())
        X[d_h] = 0.0
        for _ in range(train_steps):
            pol.train(rb, batch)
    pol.sync()
    torch.cuda.synchronize()
    return ticks * n / (time.perf_counter() - t0)


def device_rollout(env, pol, rb, ticks, train_steps, batch, sigma=0.1):
    import torch
    from td3_amd.exploration import DeviceOUNoise
    n = env.n_envs
    particles = isinstance(env.observation_space, tuple)
    noise = DeviceOUNoise(n, pol.action_dim, sigma=sigma, device=pol.device)
    state, ended = env.reset(), None
    t_sel = t_add = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        c0 = time.perf_counter()
        a = pol.select_action_device(state, noise=noise, reset=ended)
        c1 = time.perf_counter()
        s2, r, d, tl = env.step(a)
        c2 = time.perf_counter()
        if particles:
            rb.add_batch(*state, a, *s2, r, d & ~tl)
        else:
            rb.add_batch(state, a, s2, r, d & ~tl)
        t_add += time.perf_counter() - c2
        t_sel += c1 - c0
        state, ended = env.state, d
        for _ in range(train_steps):
            pol.train(rb, batch)
    pol.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return ticks * n / dt, 1e6 * t_sel / ticks, 1e6 * t_add / ticks


HG = 3                                   # goal columns of the hindsight runs (tsp, spill_punish, target_fill)


def torch_expand(rows, state_slots, reward_slot, cols_t, goals, rewards):
    """What a user of the device path had to write before the fan-out add: the n * (1 + K) expanded
    rows of main.py:70-91 as torch tensors (every array repeated 1 + K times, the goal columns and
    the rewards of the relabel rows assigned), ready for ``add_batch``."""
    import torch
    n, K = rewards.shape
    out = []
    for k, x in enumerate(rows):
        e = x.to(torch.float32).reshape(n, -1).repeat_interleave(1 + K, dim=0)
        if k in state_slots:
            e.view(n, 1 + K, -1)[:, 1:, cols_t] = goals
        elif k == reward_slot:
            e.view(n, 1 + K)[:, 1:] = rewards
        out.append(e)
    return out


def use_torch_expansion(rb, particles):
    """Make ``rb.add_batch_hindsight`` the baseline form: ``torch_expand`` + ``add_batch``."""
    import torch
    slots = ((0, 3), 5) if particles else ((0, 2), 3)
    cols_t = {}

    def add_batch_hindsight(*rows, goal_cols, goals, rewards):
        key = tuple(goal_cols)
        if key not in cols_t:
            cols_t[key] = torch.as_tensor(key, device=rb.device)
        rb.add_batch(*torch_expand(rows, *slots, cols_t[key], goals, rewards))

    rb.add_batch_hindsight = add_batch_hindsight
    return rb


def particle_relabel(K):
    """A relabel over ``SyntheticParticleVecEnv`` with the cost profile of the reference's: K draws of
    HG goal values for the last HG feature columns, rewards recomputed from next_feat (torch ops)."""
    import torch
    cols = list(range(PF - HG, PF))

    def relabel(env, state, action, reward, next_state, done_bool):
        f2 = next_state[0]
        goals = torch.rand((f2.shape[0], K, HG), device=f2.device, dtype=torch.float32)
        return cols, goals, -(f2 * f2).sum(dim=1, keepdim=True) / PF + (goals * f2[:, None, :HG]).sum(dim=2)

    return relabel


def hindsight_add_gbps(env, rb, relabel, particles, reps=20, warm=3):
    """Effective GB/s of one hindsight add of env.n_envs transitions through ``rb.add_batch_hindsight``
    (either form): the bytes the add has to move -- the n * (1 + K) ring records written plus the source
    arrays, goals and rewards read once -- over the form's device time, median of `reps`.  The time is
    taken between two events on torch's current stream around the call, twice.  For the GB/s torch's
    current stream is the ring's own (no hand-off between two streams inside the interval) and a ~1 ms
    matrix product is queued first, so every launch of the form is queued by the time the first event
    fires: the interval is the GPU's work alone.  For the latency of one call as the loop makes it, the
    call runs from torch's default stream on an idle GPU: the interval then also holds the host's time
    to issue the launches and the two stream hand-offs of ``_TorchOrder``.
    Returns (GB/s, device us, idle-GPU call us)."""
    import torch
    n = env.n_envs
    busy = torch.randn((4096, 4096), device=env.device)
    sink = torch.empty_like(busy)
    state = env.reset()
    action = torch.zeros((n, env.action_space.shape[0]), device=env.device)
    next_state, reward, done, _ = env.step(action)
    cols, goals, rewards = relabel(env, state, action, reward, next_state, done)
    rows = (*state, action, *next_state) if particles else (state, action, next_state)
    K = rewards.shape[1]
    ring_stream = torch.cuda.ExternalStream(int(rb._lib.rb_stream(rb.handle)), device=env.device)
    ms = {True: [], False: []}
    for queued in (True, False):
        for k in range(warm + reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(ring_stream) if queued else contextlib.nullcontext():
                if queued:
                    torch.mm(busy, busy, out=sink)
                e0.record()
                rb.add_batch_hindsight(*rows, reward, done, goal_cols=cols, goals=goals, rewards=rewards)
                e1.record()
            torch.cuda.synchronize()
            if k >= warm:
                ms[queued].append(e0.elapsed_time(e1))
    src = sum(x.numel() // n for x in rows) + 2 + K * (len(cols) + 1)
    nbytes = 4 * n * ((1 + K) * rb.record_floats + src)
    t = float(np.median(ms[True])) * 1e-3
    return nbytes / t / 1e9, 1e6 * t, 1e3 * float(np.median(ms[False]))


def fanout_kernel_gbps(env, rb, relabel, particles, reps=20):
    """The fan-out kernel alone, as ``device_add_gbps`` measures the plain add: the same bytes over the
    device time between two events on the ring's stream around the C call, median of `reps`."""
    import torch
    from td3_amd.my_replay_buffer import _hindsight_device
    n = env.n_envs
    state = env.reset()
    action = torch.zeros((n, env.action_space.shape[0]), device=env.device)
    next_state, reward, done, _ = env.step(action)
    cols, goals, rewards = relabel(env, state, action, reward, next_state, done)
    rows = (*state, action, *next_state, reward, done) if particles else (state, action, next_state, reward, done)
    ts = [t.to(torch.float32).reshape(n, -1).contiguous() for t in rows]
    K = rewards.shape[1]
    hs, keep = _hindsight_device(env.device, cols, goals, rewards, n)
    call = rb._lib.rb_add_particles_device_hindsight if particles else rb._lib.rb_add_device_hindsight
    stream = torch.cuda.ExternalStream(int(rb._lib.rb_stream(rb.handle)), device=env.device)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = call(rb.handle, *[t.data_ptr() for t in ts], n, hs, None)
        e1.record(stream)
        assert rc == 0, rb._lib.td3_last_error()
        stream.synchronize()
        ms.append(e0.elapsed_time(e1))
    nbytes = 4 * n * ((1 + K) * rb.record_floats + sum(t.shape[1] for t in ts) + K * (len(cols) + 1))
    t = float(np.median(ms)) * 1e-3
    return nbytes / t / 1e9, 1e6 * t


def hindsight_main(args, emit):
    """``--hindsight K``: the fan-out add against the torch expansion + ``add_batch``, in one run."""
    import torch
    from td3_amd.loop import (DeviceTrainLoop, SyntheticGoalVecEnv, SyntheticParticleVecEnv, hindsight_relabel)
    particles, K, n_envs = args.config == "particles", args.hindsight, args.n_envs
    if particles:
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as Ring
        ring_rows, prefill, what = 100_000, 20_000, "SyntheticParticleVecEnv (7 / 350 x 9 / 3)"
        make_env = lambda: SyntheticParticleVecEnv(n_envs, PF, PN, PD, PA, max_action=MA, max_episode_steps=1000)
        relabel = particle_relabel(K)
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as Ring
        ring_rows, prefill, what = 1_000_000, 100_000, "SyntheticGoalVecEnv (HalfCheetah dims)"
        make_env = lambda: SyntheticGoalVecEnv(n_envs, SD, AD, HG, max_action=MA, max_episode_steps=1000)
        relabel = hindsight_relabel(K)
    np.random.seed(0)
    torch.manual_seed(0)
    env = make_env()
    pol = TD3(env.observation_space, env.action_space, max_action=MA, norm="layer", device=env.device.index)
    rings = {}
    for form in ("fanout", "expand"):
        rb = Ring(env.observation_space, env.action_space, max_size=ring_rows, device=env.device.index)
        rb.fill_synthetic(prefill, max_action=MA, seed=1)
        rings[form] = use_torch_expansion(rb, particles) if form == "expand" else rb
    add = {form: hindsight_add_gbps(env, rings[form], relabel, particles) for form in rings}
    kern = fanout_kernel_gbps(env, rings["fanout"], relabel, particles)
    sps = {form: [] for form in rings}
    for rep in range(1 + args.repeats):              # the forms alternate; the first pass is the warm-up
        for form, rb in rings.items():
            loop = DeviceTrainLoop(env, pol, rb, start_policy=0, start_training=0, batch_size=args.batch,
                                   expl_noise=0.1, train_steps_per_tick=args.train_steps, relabel=relabel)
            r = loop.run(args.warmup if rep == 0 else args.ticks)
            if rep:
                sps[form].append(r["env_steps_per_s"])
    fan, exp = float(np.median(sps["fanout"])), float(np.median(sps["expand"]))
    emit(json.dumps({
        "metric": f"hindsight K={K} on {what}: act -> env.step -> relabel -> add of each transition and its K "
                  f"relabels, {args.train_steps} train({args.batch}) per tick; fan-out add vs torch expansion + "
                  "add_batch",
        "n_envs": n_envs, "hindsight": K, "goal_cols": HG, "record_floats": int(rings["fanout"].record_floats),
        "fanout_add_gb_per_s": round(add["fanout"][0], 1), "fanout_add_device_us": round(add["fanout"][1], 2),
        "fanout_add_idle_call_us": round(add["fanout"][2], 2),
        "expand_add_gb_per_s": round(add["expand"][0], 1), "expand_add_device_us": round(add["expand"][1], 2),
        "expand_add_idle_call_us": round(add["expand"][2], 2),
        "add_fanout_over_expand": round(add["fanout"][0] / add["expand"][0], 3),
        "fanout_kernel_gb_per_s": round(kern[0], 1), "fanout_kernel_us": round(kern[1], 2),
        "fanout_steps_per_s": round(fan, 1), "expand_steps_per_s": round(exp, 1),
        "steps_fanout_over_expand": round(fan / exp, 3),
        "fanout_steps_per_s_runs": [round(x, 1) for x in sps["fanout"]],
        "expand_steps_per_s_runs": [round(x, 1) for x in sps["expand"]],
        "unit": "GB/s (add), env-steps/s (loop)", "higher_is_better": True,
        "ticks": args.ticks, "warmup": args.warmup, "train_steps_per_tick": args.train_steps, "n_gpus": 1}))


def nstep_add_us(env, rb, particles, n_step, reps=20):
    """Device time (us) of one add of env.n_envs rows, event-timed as ``device_add_gbps`` /
    ``fanout_kernel_gbps`` (two events on the ring's stream around the C call, median of `reps`, after
    a warm-up): ``n_step`` 0 is the plain device add, otherwise the n-step add in steady state -- no
    episode ends, so after n_step - 1 warm-up ticks every row matures its n_step - 1 predecessors."""
    import torch
    from td3_amd import _lib
    n = env.n_envs
    state = env.reset()
    action = torch.zeros((n, env.action_space.shape[0]), device=env.device)
    next_state, reward, done, _ = env.step(action)
    rows = (*state, action, *next_state, reward, done) if particles else (state, action, next_state, reward, done)
    ts = [t.to(torch.float32).reshape(n, -1).contiguous() for t in rows]
    ts[-1].zero_()                                   # done = 0: nothing stops maturing
    ended = torch.zeros(n, dtype=torch.uint8, device=env.device)
    ns = _lib.rb_nstep()
    ns.n, ns.gamma, ns.ended = max(n_step, 1), 0.99, ended.data_ptr()
    kind = "particles_device" if particles else "device"
    if n_step:
        fn = getattr(rb._lib, f"rb_add_{kind}_nstep")
        call = lambda: fn(rb.handle, *[t.data_ptr() for t in ts], n, ns, None)
    else:
        fn = getattr(rb._lib, f"rb_add_{kind}")
        call = lambda: fn(rb.handle, *[t.data_ptr() for t in ts], n, None)
    stream = torch.cuda.ExternalStream(int(rb._lib.rb_stream(rb.handle)), device=env.device)
    torch.cuda.synchronize()
    ms = []
    warm = max(3, n_step)
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = call()
        e1.record(stream)
        assert rc == 0, rb._lib.td3_last_error()
        stream.synchronize()
        if k >= warm:
            ms.append(e0.elapsed_time(e1))
    return 1e3 * float(np.median(ms))


def nstep_main(args, emit):
    """``--nstep N``: the n-step add next to the plain device add at the same shapes, and the loop."""
    import torch
    from td3_amd.loop import DeviceTrainLoop, SyntheticParticleVecEnv, SyntheticVecEnv
    particles, N, n_envs = args.config == "particles", args.nstep, args.n_envs
    if particles:
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as Ring
        ring_rows, prefill, what = 100_000, 20_000, "SyntheticParticleVecEnv (7 / 350 x 9 / 3)"
        make_env = lambda: SyntheticParticleVecEnv(n_envs, PF, PN, PD, PA, max_action=MA, max_episode_steps=1000)
        next_block = PF + PN * PD
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as Ring
        ring_rows, prefill, what = 1_000_000, 100_000, "SyntheticVecEnv (HalfCheetah dims)"
        make_env = lambda: SyntheticVecEnv(n_envs, SD, AD, max_action=MA, max_episode_steps=1000)
        next_block = SD
    np.random.seed(0)
    torch.manual_seed(0)
    env = make_env()
    pol = TD3(env.observation_space, env.action_space, max_action=MA, norm="layer", device=env.device.index)
    rings = {}
    for form in ("nstep", "plain"):
        rings[form] = Ring(env.observation_space, env.action_space, max_size=ring_rows, device=env.device.index)
        rings[form].fill_synthetic(prefill, max_action=MA, seed=1)
    rec = int(rings["nstep"].record_floats)
    plain_us = nstep_add_us(env, rings["plain"], particles, 0)
    nstep_us = nstep_add_us(env, rings["nstep"], particles, N)
    # algorithmic bytes written: the new records, plus per maturing copy the next-state block and the two scalars
    plain_bytes = 4 * n_envs * rec
    nstep_bytes = plain_bytes + 4 * n_envs * (N - 1) * (next_block + 2)
    predicted_us = plain_us * nstep_bytes / plain_bytes        # at the plain add's achieved bytes per second
    sps = {form: [] for form in rings}
    for rep in range(1 + args.repeats):              # the forms alternate; the first pass is the warm-up
        for form, rb in rings.items():
            loop = DeviceTrainLoop(env, pol, rb, start_policy=0, start_training=0, batch_size=args.batch,
                                   expl_noise=0.1, train_steps_per_tick=args.train_steps,
                                   n_step=N if form == "nstep" else 1)
            r = loop.run(args.warmup if rep == 0 else args.ticks)
            if rep:
                sps[form].append(r["env_steps_per_s"])
    ns_sps, one_sps = float(np.median(sps["nstep"])), float(np.median(sps["plain"]))
    emit(json.dumps({
        "metric": f"n-step add, n = {N}, on {what}: one add of {n_envs} rows in steady state (every row matures "
                  f"its {N - 1} predecessors) next to the plain device add; act -> env.step -> add loop with "
                  f"{args.train_steps} train({args.batch}) per tick, n_step = {N} against n_step = 1",
        "n_envs": n_envs, "n_step": N, "record_floats": rec, "next_state_floats": next_block,
        "plain_add_device_us": round(plain_us, 2), "nstep_add_device_us": round(nstep_us, 2),
        "nstep_over_plain_time": round(nstep_us / plain_us, 3),
        "plain_add_bytes_written": plain_bytes, "nstep_add_bytes_written": nstep_bytes,
        "nstep_over_plain_bytes": round(nstep_bytes / plain_bytes, 3),
        "nstep_add_us_at_plain_bandwidth": round(predicted_us, 2),
        "nstep_measured_over_predicted": round(nstep_us / predicted_us, 3),
        "nstep_steps_per_s": round(ns_sps, 1), "one_step_steps_per_s": round(one_sps, 1),
        "steps_nstep_over_one_step": round(ns_sps / one_sps, 3),
        "nstep_steps_per_s_runs": [round(x, 1) for x in sps["nstep"]],
        "one_step_steps_per_s_runs": [round(x, 1) for x in sps["plain"]],
        "unit": "us (add, lower is better), env-steps/s (loop, higher is better)",
        "ticks": args.ticks, "warmup": args.warmup, "train_steps_per_tick": args.train_steps, "n_gpus": 1}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("featured", "particles"), default="featured")
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--add-rows", type=int, default=0,
                    help="--config particles: one more line, the device add's GB/s for this many rows")
    ap.add_argument("--hindsight", type=int, default=0,
                    help="K > 0: compare the fan-out hindsight add with the torch expansion + add_batch instead")
    ap.add_argument("--nstep", type=int, default=0,
                    help="N in 2..8: measure the n-step add against the plain device add, and the loop, instead")
    ap.add_argument("--n-envs", type=int, default=256, help="--hindsight / --nstep: environments (default 256)")
    ap.add_argument("--repeats", type=int, default=3,
                    help="--hindsight / --nstep: timed loop runs per form (median)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.hindsight > 0 or args.nstep > 0:
        def emit_line(line):
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        if args.hindsight > 0 and args.nstep > 0:
            ap.error("--hindsight and --nstep are separate measurements")
        if args.nstep > 0 and not 2 <= args.nstep <= 8:
            ap.error("--nstep takes a horizon in 2..8")
        (hindsight_main if args.hindsight > 0 else nstep_main)(args, emit_line)
        return
    import torch
    from td3_amd.loop import SyntheticParticleVecEnv, SyntheticVecEnv
    particles = args.config == "particles"
    if particles:
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as Ring
        rows, prefill, host_run = 100_000, 20_000, host_rollout_particles      # 25 KB a record
        what = "SyntheticParticleVecEnv (7 / 350 x 9 / 3)"
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as Ring
        rows, prefill, host_run = 1_000_000, 100_000, host_rollout
        what = "SyntheticVecEnv (HalfCheetah dims)"

    def emit(line):
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for n_envs in (1, 16, 256):
        np.random.seed(0)
        torch.manual_seed(0)
        if particles:
            env = SyntheticParticleVecEnv(n_envs, PF, PN, PD, PA, max_action=MA, max_episode_steps=1000)
        else:
            env = SyntheticVecEnv(n_envs, SD, AD, max_action=MA, max_episode_steps=1000)
        pol = TD3(env.observation_space, env.action_space, max_action=MA, norm="layer", device=env.device.index)
        res = {}
        extra = {}
        for path in ("host", "device"):
            rb = Ring(env.observation_space, env.action_space, max_size=rows, device=env.device.index)
            rb.fill_synthetic(prefill, max_action=MA, seed=1)
            run = host_run if path == "host" else device_rollout
            run(env, pol, rb, args.warmup, args.train_steps, args.batch)
            res[path] = run(env, pol, rb, args.ticks, args.train_steps, args.batch)
            if particles and path == "device":
                gbps, us = device_add_gbps(env, rb)
                extra = {"device_add_gb_per_s": round(gbps, 1), "device_add_kernel_us": round(us, 2)}
            del rb
        dev_sps, sel_us, add_us = res["device"]
        line = json.dumps({
            "metric": f"env-steps/s of act -> env.step -> add on {what}, "
                      f"{args.train_steps} train({args.batch}) per tick",
            "n_envs": n_envs, "unit": "env-steps/s", "higher_is_better": True,
            "device_steps_per_s": round(dev_sps, 1), "host_steps_per_s": round(res["host"], 1),
            "device_over_host": round(dev_sps / res["host"], 3),
            "device_select_host_us_per_call": round(sel_us, 1), "device_add_host_us_per_call": round(add_us, 1),
            **extra,
            "ticks": args.ticks, "warmup": args.warmup, "train_steps_per_tick": args.train_steps, "n_gpus": 1})
        emit(line)
        del pol, env
    if particles and args.add_rows > 0:
        env = SyntheticParticleVecEnv(args.add_rows, PF, PN, PD, PA, max_action=MA)
        rb = Ring(env.observation_space, env.action_space, max_size=max(rows, args.add_rows),
                  device=env.device.index)
        gbps, us = device_add_gbps(env, rb)
        emit(json.dumps({"metric": f"rb_add_particles_device of {args.add_rows} rows (7 / 350 x 9 / 3): bytes read + "
                                   "written over the kernel's device time", "rows": args.add_rows, "unit": "GB/s",
                         "higher_is_better": True, "device_add_gb_per_s": round(gbps, 1),
                         "device_add_kernel_us": round(us, 2), "n_gpus": 1}))


if __name__ == "__main__":
    main()
