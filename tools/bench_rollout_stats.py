"""Cost of the rollout statistics (include/td3.h: rs_tick; td3_amd/rollout_stats.py) next to the torch-op
restatement of the same tick -- what a user of the device loop has to write without it, so the baseline.

Reports, as one JSON line and a file (default profiles/rollout_stats.json):
  (a) device microseconds per tick of ``RolloutStats.tick`` (one launch) and of ``TorchTick.tick`` (the
      restatement below: fp64 torch ops, nothing read back) at (rows, obs_dim) = (256, 17), (256, 376),
      (4096, 17), every input given, ``update`` on, a row ending every 1000 ticks as in the loop.  Each
      figure is the time between two HIP events around ``--launches`` ticks, divided by their number;
      the ticks are queued while the stream is still busy with a filler kernel, so the events bracket
      back-to-back device work and not the host's submit rate.  The two forms alternate; median and
      spread (max - min) over ``--reps`` windows each.  ``fused_faster_beyond_spread`` says whether the
      fused median is below the torch median by more than the larger of the two spreads;
  (b) env-steps/s of ``DeviceTrainLoop`` (SyntheticVecEnv at HalfCheetah dims, 256 environments, no train
      step: the acting / stepping / adding path the statistics sit in) three ways: bare, under
      ``NormalizedVecEnv``, and under the same wrapper with the torch restatement.  The three alternate;
      the first pass is the warm-up; median and every run of ``--repeats`` passes of ``--ticks`` ticks.
No pass/fail: the numbers are reported.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SD, AD, MA = 17, 6, 1.0                    # bench.py CONFIGS["halfcheetah"]
SHAPES = ((256, 17), (256, 376), (4096, 17))
GAMMA, EPS, CLIP, LOG_CAP = 0.99, 1e-8, 10.0, 4096


class TorchTick:
    """The tick of include/td3.h ("rollout statistics") as torch ops on fp64 device tensors, nothing read
    back: the moment merges, both normalisations, the reward scaling and the episode log (row-ordered
    slots from a cumulative sum over ``ended``; rows that did not end write a spare slot)."""

    def __init__(self, rows, dim, device):
        import torch
        kw = dict(dtype=torch.float64, device=device)
        self.rows = rows
        self.count, self.mean, self.m2 = torch.zeros((), **kw), torch.zeros(dim, **kw), torch.zeros(dim, **kw)
        self.ret_count, self.ret_mean, self.ret_m2 = (torch.zeros((), **kw) for _ in range(3))
        self.G, self.ep_return = torch.zeros(rows, **kw), torch.zeros(rows, **kw)
        self.ep_len = torch.zeros(rows, dtype=torch.int32, device=device)
        self.log_ret = torch.zeros(LOG_CAP + 1, dtype=torch.float32, device=device)
        self.log_len = torch.zeros(LOG_CAP + 1, dtype=torch.int32, device=device)
        self.log_row = torch.zeros(LOG_CAP + 1, dtype=torch.int32, device=device)
        self.log_tick = torch.zeros(LOG_CAP + 1, dtype=torch.int64, device=device)
        self.ep_count = torch.zeros((), dtype=torch.int64, device=device)
        self.ep_len_sum = torch.zeros((), dtype=torch.int64, device=device)
        self.ep_return_sum = torch.zeros((), **kw)
        self.tick_no = torch.zeros((), dtype=torch.int64, device=device)
        self.row_ids = torch.arange(rows, dtype=torch.int32, device=device)

    @staticmethod
    def _merge(count, mean, m2, x):
        n = x.shape[0]
        mb = x.mean(dim=0)
        m2b = ((x - mb) ** 2).sum(dim=0)
        delta, tot = mb - mean, count + n
        return tot, mean + delta * n / tot, m2 + m2b + delta * delta * count * n / tot

    def tick(self, obs=None, next_obs=None, reward=None, ended=None, update=True, **_):
        import torch
        out = [None, None, None]
        if update and obs is not None:
            self.count, self.mean, self.m2 = self._merge(self.count, self.mean, self.m2, obs.double())
        rstd = torch.rsqrt(self.m2 / self.count + EPS)
        for j, x in enumerate((obs, next_obs)):
            if x is not None:
                out[j] = ((x.double() - self.mean) * rstd).clamp_(-CLIP, CLIP).float()
        if reward is not None:
            r = reward.double()
            self.G = GAMMA * self.G + r
            if update:
                self.ret_count, self.ret_mean, self.ret_m2 = self._merge(self.ret_count, self.ret_mean, self.ret_m2,
                                                                         self.G)
            out[2] = (r * torch.rsqrt(self.ret_m2 / self.ret_count + EPS)).clamp_(-CLIP, CLIP).float()
            self.ep_return += r
            self.ep_len += 1
            if ended is not None:
                e = ended.bool()
                self.G = torch.where(e, 0.0, self.G)
                k = torch.cumsum(e, dim=0) - 1
                slot = torch.where(e, (self.ep_count + k) % LOG_CAP, LOG_CAP)
                self.log_ret[slot] = self.ep_return.float()
                self.log_len[slot] = self.ep_len
                self.log_row[slot] = self.row_ids
                self.log_tick[slot] = self.tick_no
                self.ep_count += e.sum()
                self.ep_return_sum += torch.where(e, self.ep_return, 0.0).sum()
                self.ep_len_sum += torch.where(e, self.ep_len, 0).sum()
                self.ep_return = torch.where(e, 0.0, self.ep_return)
                self.ep_len = torch.where(e, 0, self.ep_len)
            self.tick_no += 1
        return tuple(out)


def tick_device_us(rows, dim, launches, reps):
    """(a): the fused tick and the torch restatement at one shape, alternating windows."""
    import torch
    from td3_amd.rollout_stats import RolloutStats
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    filler = torch.randn(4096, 4096, device=dev)
    obs = torch.randn(rows, dim, device=dev) * 3 + 1
    nxt = torch.randn(rows, dim, device=dev) * 3 + 1
    rew = torch.randn(rows, device=dev)
    ends = [(torch.arange(rows, device=dev) % 1000) == (t % 1000) for t in range(launches)]
    forms = {"fused": RolloutStats(rows, dim, gamma=GAMMA, log_cap=LOG_CAP, device=0), "torch": TorchTick(rows, dim, dev)}
    res = {k: [] for k in forms}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for form in forms.values():                        # warm: code objects, the allocator's blocks
            for t in range(20):
                form.tick(obs, nxt, rew, ends[t])
        for _ in range(reps):
            for name, form in forms.items():
                stream.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(32):                        # tens of ms of device work: the ticks queue behind it
                    filler @ filler
                e0.record(stream)
                for t in range(launches):
                    form.tick(obs, nxt, rew, ends[t])
                e1.record(stream)
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) * 1000.0 / launches)
    stream.synchronize()
    out = {"rows": rows, "obs_dim": dim}
    for name, v in res.items():
        out[name] = {"median_us": round(float(np.median(v)), 3), "spread_us": round(float(max(v) - min(v)), 3),
                     "windows_us": [round(x, 3) for x in v]}
    spread = max(out["fused"]["spread_us"], out["torch"]["spread_us"])
    out["torch_over_fused"] = round(out["torch"]["median_us"] / out["fused"]["median_us"], 2)
    out["fused_faster_beyond_spread"] = bool(out["torch"]["median_us"] - out["fused"]["median_us"] > spread)
    return out


def loop_steps_per_s(n_envs, ticks, warmup, repeats):
    """(b): the device loop bare, under NormalizedVecEnv, and under it with the torch restatement."""
    import torch
    from td3_amd.TD3_featured import TD3
    from td3_amd.loop import DeviceTrainLoop, SyntheticVecEnv
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    from td3_amd.rollout_stats import NormalizedVecEnv, RolloutStats

    def torch_stats():
        st = TorchTick(n_envs, SD, torch.device("cuda", 0))
        st.n_envs = n_envs                             # all NormalizedVecEnv asks of its stats besides tick()
        return st

    np.random.seed(0)
    torch.manual_seed(0)
    make_env = lambda: SyntheticVecEnv(n_envs, SD, AD, max_action=MA, max_episode_steps=1000)
    envs = {"bare": make_env(),
            "normalized": NormalizedVecEnv(make_env(), RolloutStats(n_envs, SD, gamma=GAMMA, device=0)),
            "torch_restatement": NormalizedVecEnv(make_env(), torch_stats())}
    pol = TD3(envs["bare"].observation_space, envs["bare"].action_space, max_action=MA, norm="layer", device=0)
    rb = ReplayBuffer_featured(envs["bare"].observation_space, envs["bare"].action_space, max_size=1_000_000, device=0)
    rb.fill_synthetic(100_000, max_action=MA, seed=1)
    sps = {k: [] for k in envs}
    for rep in range(1 + repeats):
        for name, env in envs.items():
            loop = DeviceTrainLoop(env, pol, rb, start_policy=0, start_training=10 ** 9, batch_size=256, expl_noise=0.1)
            r = loop.run(warmup if rep == 0 else ticks)
            if rep:
                sps[name].append(r["env_steps_per_s"])
    out = {"n_envs": n_envs, "ticks": ticks, "warmup": warmup, "train_steps_per_tick": 0}
    for name, v in sps.items():
        out[name] = {"median_env_steps_per_s": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v]}
    for name in ("normalized", "torch_restatement"):
        out[name]["over_bare"] = round(out[name]["median_env_steps_per_s"] / out["bare"]["median_env_steps_per_s"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_stats.json"))
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_stats: no GPU (torch.cuda.is_available() is False); nothing is measured "
                         "without one")
    from bench import pin_host_thread
    pin_host_thread(0)
    res = {"config": dict(gamma=GAMMA, eps=EPS, clip=CLIP, log_cap=LOG_CAP, launches=args.launches, reps=args.reps,
                          loop_dims=(SD, AD)),
           "device": torch.cuda.get_device_name(0),
           "a_tick_device_us": [tick_device_us(r, d, args.launches, args.reps) for r, d in SHAPES],
           "b_loop_env_steps_per_s": loop_steps_per_s(args.n_envs, args.ticks, args.warmup, args.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
