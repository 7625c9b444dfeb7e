#!/usr/bin/env python3
"""Env-steps/s of a rollout on a GPU-resident vector environment: host-vector path vs device path.

    python tools/bench_rollout.py [--config featured|particles] [--ticks K] [--warmup W] [--train-steps T]
                                  [--out FILE]

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
"""
from __future__ import annotations

import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("featured", "particles"), default="featured")
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--add-rows", type=int, default=0,
                    help="--config particles: one more line, the device add's GB/s for this many rows")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
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
