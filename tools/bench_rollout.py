#!/usr/bin/env python3
"""Env-steps/s of a rollout on a GPU-resident vector environment: host-vector path vs device path.

    python tools/bench_rollout.py [--ticks K] [--warmup W] [--train-steps T] [--out FILE]

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
    noise = DeviceOUNoise(n, AD, sigma=sigma, device=pol.device)
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
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from td3_amd.TD3_featured import TD3
    from td3_amd.loop import SyntheticVecEnv
    from td3_amd.my_replay_buffer import ReplayBuffer_featured

    for n_envs in (1, 16, 256):
        np.random.seed(0)
        torch.manual_seed(0)
        env = SyntheticVecEnv(n_envs, SD, AD, max_action=MA, max_episode_steps=1000)
        pol = TD3(env.observation_space, env.action_space, max_action=MA, norm="layer", device=env.device.index)
        res = {}
        for path in ("host", "device"):
            rb = ReplayBuffer_featured(env.observation_space, env.action_space, max_size=1_000_000,
                                       device=env.device.index)
            rb.fill_synthetic(100_000, max_action=MA, seed=1)
            run = host_rollout if path == "host" else device_rollout
            run(env, pol, rb, args.warmup, args.train_steps, args.batch)
            res[path] = run(env, pol, rb, args.ticks, args.train_steps, args.batch)
            del rb
        dev_sps, sel_us, add_us = res["device"]
        line = json.dumps({
            "metric": "env-steps/s of act -> env.step -> add on SyntheticVecEnv (HalfCheetah dims), "
                      f"{args.train_steps} train({args.batch}) per tick",
            "n_envs": n_envs, "unit": "env-steps/s", "higher_is_better": True,
            "device_steps_per_s": round(dev_sps, 1), "host_steps_per_s": round(res["host"], 1),
            "device_over_host": round(dev_sps / res["host"], 3),
            "device_select_host_us_per_call": round(sel_us, 1), "device_add_host_us_per_call": round(add_us, 1),
            "ticks": args.ticks, "warmup": args.warmup, "train_steps_per_tick": args.train_steps, "n_gpus": 1})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del pol, env


if __name__ == "__main__":
    main()
