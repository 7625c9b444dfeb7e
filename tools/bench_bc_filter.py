"""Cost of the BC term's row mask (include/td3.h "BC on the demonstration rows, Q-filter": td3_set_bc_filter)
on the demonstration-replay step, at the HalfCheetah dims (batch 256) and the Humanoid dims (batch 1024): a
10^6-row online ring, a 10^5-row demo ring, demo_fraction 0.5, rings from fill_synthetic, LayerNorm,
bc_alpha 2.5.

Reports, as one JSON line and a file (default profiles/bc_filter.json), per shape:
  (a) steps/s of ``TD3.train`` on the ``MixedReplay`` with BC over all rows (``all``: the stage list and
      kernels of the parent commit's mixed step with BC on -- the yardstick, measured in the same run), with
      ``bc_rows="demo"`` (``demo``) and with the Q-filter added (``demo_qf``): three learners that share the
      two rings, warmed up, then ``--runs`` rounds in which each runs one timed region that ends in a
      synchronise -- the regions ALTERNATE round after round; the median, every run, each variant's spread
      (max - min over its runs, as a share of its median) and its us per step over ``all``;
  (b) device microseconds of the actor phase's actor_head_bwd stage of each of the three, and of a learner
      with BC off (td3_profile_stages, then td3_time_stage: ``--iters`` launches replayed from a graph,
      median of ``--reps``).  The profiled step draws from one ring, so the masked kernels run with
      n_d = B there; what a row does not keep saves it no instruction (the mask is a select);
  (c) td3_bc_filter_info of the last timed actor step of ``demo`` and ``demo_qf``.
With ``--parent DIR`` (a built checkout of the parent commit) it also runs ``bench.py --gpus 1`` of this
tree and of that one as child processes, in ABBA order (this, parent, parent, this, ...),
``--bench-runs`` times each, for C2 and C3: the spread of each build's own runs is the yardstick for "the
step with the switches off is unchanged".
No pass/fail: the numbers are reported.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_bc import stage_us  # noqa: E402
from bench_mixed import bench_pair  # noqa: E402
from bench_per import Box, timed_region, write_result  # noqa: E402

SHAPES = {"halfcheetah": "C2", "humanoid": "C3"}
ONLINE_ROWS, DEMO_ROWS, ALPHA = 1_000_000, 100_000, 2.5
# variant -> (bc_alpha, bc_rows, bc_q_filter)
VARIANTS = {"all": (ALPHA, "all", False), "demo": (ALPHA, "demo", False), "demo_qf": (ALPHA, "demo", True)}


def make(cfg):
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import MixedReplay, ReplayBuffer_featured as RB
    obs, act = Box((cfg["sd"],)), Box((cfg["ad"],))
    online = RB(obs, act, max_size=ONLINE_ROWS, device=0, seed=101)
    online.fill_synthetic(ONLINE_ROWS, cfg["ma"], seed=7)
    demo = RB(obs, act, max_size=DEMO_ROWS, device=0, seed=202)
    demo.fill_synthetic(DEMO_ROWS, cfg["ma"], seed=9)
    pols = {k: TD3(obs, act, max_action=cfg["ma"], device=0, seed=17, use_graph="auto", norm="layer", bc_alpha=a,
                   bc_rows=rows, bc_q_filter=qf) for k, (a, rows, qf) in VARIANTS.items()}
    off = TD3(obs, act, max_action=cfg["ma"], device=0, seed=17, use_graph="auto", norm="layer")
    return pols, off, MixedReplay(online, demo, 0.5), online


def measure(name, args):
    import torch
    from bench import CONFIGS
    cfg = CONFIGS[name]
    Bc = cfg["batch"]
    steps, warmup = args.steps or (2000 if Bc <= 256 else 1000), args.warmup or 100
    torch.manual_seed(1000)
    pols, off, mix, online = make(cfg)
    gc.collect()
    gc.disable()
    for pol in pols.values():
        for _ in range(warmup):
            pol.train(mix, Bc)
    runs = {k: [] for k in pols}
    for _ in range(args.runs):
        for k, pol in pols.items():
            runs[k].append(timed_region(pol, mix, steps, Bc))
    gc.enable()
    sps = {k: {"median": float(np.median(v)), "runs": [round(x, 2) for x in v],
               "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in runs.items()}
    res = {"shape": SHAPES[name], "batch": Bc, "online_rows": ONLINE_ROWS, "demo_rows": DEMO_ROWS, "demo_fraction": 0.5,
           "n_demo": mix.n_demo(Bc), "bc_alpha": ALPHA, "steps": steps, "warmup": warmup, "order": "alternated",
           "steps_per_s": sps}
    base = sps["all"]["median"]
    res["us_per_step_over_all"] = {k: round(1e6 / sps[k]["median"] - 1e6 / base, 3) for k in pols if k != "all"}
    res["relative_to_all"] = {k: round(sps[k]["median"] / base - 1.0, 4) for k in pols if k != "all"}
    res["bc_filter_info"] = {k: pols[k].bc_filter_info() for k in ("demo", "demo_qf")}
    res["stage_device_us"] = {k: stage_us(pol, online, Bc, args.iters, args.reps) for k, pol in (*pols.items(), ("off", off))}
    for pol in (*pols.values(), off):
        pol.sync()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=(*SHAPES, "all"), default="all")
    ap.add_argument("--steps", type=int, default=None, help="default 2000 (halfcheetah) / 1000 (humanoid)")
    ap.add_argument("--warmup", type=int, default=None, help="default 100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py A/B")
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_filter.json"))
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bc_filter: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    res = {"config": dict(runs=args.runs, iters=args.iters, reps=args.reps, norm="layer", demo_fraction=0.5)}
    if args.parent:                       # first: child processes, while this one has not opened the GPU
        res["bench_py"] = {c: bench_pair(args, c) for c in ("halfcheetah", "humanoid")}
    from bench import pin_host_thread
    pin_host_thread(0)
    res["device"] = torch.cuda.get_device_name(0)
    for name in (tuple(SHAPES) if args.config == "all" else (args.config,)):
        res[name] = measure(name, args)
        gc.collect()
    return write_result(res, args.out)


if __name__ == "__main__":
    sys.exit(main())
