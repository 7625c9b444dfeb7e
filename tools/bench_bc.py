"""Cost of the TD3+BC actor phase (include/td3.h "TD3+BC": td3_set_bc) at bench.py's two featured shapes:
C2, HalfCheetah dims at batch 256 (a 10^6-row ring), and C3, Humanoid dims at batch 1024 (a 2*10^6-row
ring), both LayerNorm, rings from fill_synthetic.

Reports, as one JSON line and a file (default profiles/bc.json), per shape:
  (a) steps/s of ``TD3.train`` with BC off and on: two learners that live side by side, warmed up, then
      ``--runs`` rounds in which each runs one timed region of ``--steps`` steps that ends in a
      synchronise -- the regions ALTERNATE round after round; the median and every run;
  (b) device microseconds of the actor phase's actor_head_bwd stage, plain and in its BC form, by
      td3_time_stage: ``--iters`` launches replayed from a graph between two events, median of ``--reps``.
With ``--parent DIR`` (a built checkout of the parent commit) it also runs ``bench.py --gpus 1`` of this
tree and of that one as child processes, in ABBA order (this, parent, parent, this, ...),
``--bench-runs`` times each, per ``--bench-config``:
the spread of each build's own runs is the yardstick for "the BC-off step is unchanged".
No pass/fail: the numbers are reported.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_per import Box, timed_region, write_result  # noqa: E402

VARIANTS = (("off", None), ("on", 2.5))       # name -> bc_alpha


def make(cfg, alpha, batch):
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured as RB
    obs = Box((cfg["sd"],))
    pol = TD3(obs, Box((cfg["ad"],)), max_action=cfg["ma"], device=0, seed=17, use_graph="auto", norm="layer",
              bc_alpha=alpha)
    rb = RB(obs, Box((cfg["ad"],)), max_size=cfg["replay"], device=0, seed=101)
    rb.fill_synthetic(cfg["replay"], cfg["ma"], seed=7)
    return pol, rb


def stage_us(pol, rb, batch, iters, reps):
    """{stage: median device us} of the actor phase's actor_head_bwd stage."""
    from td3_amd._lib import check
    ms = (C.c_float * 128)()
    n = C.c_int()
    check(pol._lib.td3_profile_stages(pol._h, rb.handle, batch, 1, ms, 128, C.byref(n)), "td3_profile_stages")
    out = {}
    for i in range(n.value):
        name = pol._lib.td3_stage_name(pol._h, i).decode()
        if name != "actor_head_bwd":
            continue
        t = []
        for _ in range(reps):
            v = C.c_float()
            check(pol._lib.td3_time_stage(pol._h, i, iters, C.byref(v)), "td3_time_stage")
            t.append(v.value * 1000.0)
        out[name] = {"kernel": pol._lib.td3_stage_kernel(pol._h, i).decode(), "median_us": round(float(np.median(t)), 3),
                     "reps_us": [round(x, 3) for x in t]}
    return out


def measure(name, args):
    import torch
    from bench import CONFIGS
    cfg = CONFIGS[name]
    Bc = cfg["batch"]
    steps, warmup = args.steps or (2000 if Bc <= 256 else 1000), args.warmup or 100
    torch.manual_seed(1000)
    trio = {k: make(cfg, alpha, Bc) for k, alpha in VARIANTS}
    gc.collect()
    gc.disable()
    for pol, rb in trio.values():
        for _ in range(warmup):
            pol.train(rb, Bc)
    runs = {k: [] for k in trio}
    for _ in range(args.runs):
        for k, (pol, rb) in trio.items():
            runs[k].append(timed_region(pol, rb, steps, Bc))
    gc.enable()
    res = {"batch": Bc, "ring_rows": cfg["replay"], "steps": steps, "warmup": warmup, "order": "alternated",
           "steps_per_s": {k: {"median": float(np.median(v)), "runs": [round(x, 2) for x in v]} for k, v in runs.items()}}
    off = res["steps_per_s"]["off"]["median"]
    res["us_per_step_over_off"] = {k: round(1e6 / res["steps_per_s"][k]["median"] - 1e6 / off, 3)
                                   for k in trio if k != "off"}
    res["stage_device_us"] = {k: stage_us(pol, rb, Bc, args.iters, args.reps) for k, (pol, rb) in trio.items()}
    res["bc_info"] = {k: trio[k][0].bc_info() for k in trio if k != "off"}
    for pol, _ in trio.values():
        pol.sync()
    return res


def bench_pair(args, config):
    """bench.py of this tree and of the parent's, alternated child processes; every steps/s figure."""
    out = {"this": [], "parent": [], "order": "ABBA: this, parent, parent, this, this, parent, ...",
           "argv": ["--gpus", "1", "--config", config, "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]}
    trees = (("this", ROOT), ("parent", os.path.abspath(args.parent)))
    for i in range(args.bench_runs):
        for key, tree in (trees if i % 2 == 0 else trees[::-1]):
            r = subprocess.run([sys.executable, "bench.py", *out["argv"]], cwd=tree, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench_bc: bench.py failed in {tree} ({r.returncode}):\n{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            out[key].append({"value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"]})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("halfcheetah", "humanoid", "both"), default="both")
    ap.add_argument("--steps", type=int, default=None, help="default 2000 (halfcheetah) / 1000 (humanoid)")
    ap.add_argument("--warmup", type=int, default=None, help="default 100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py A/B")
    ap.add_argument("--bench-config", choices=("halfcheetah", "humanoid", "both"), default="halfcheetah")
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc.json"))
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bc: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    both = ("halfcheetah", "humanoid")
    res = {"config": dict(runs=args.runs, iters=args.iters, reps=args.reps, alpha=2.5, norm="layer")}
    if args.parent:                       # first: child processes, while this one has not opened the GPU
        res["bench_py"] = {c: bench_pair(args, c) for c in (both if args.bench_config == "both" else (args.bench_config,))}
    from bench import pin_host_thread
    pin_host_thread(0)
    res["device"] = torch.cuda.get_device_name(0)
    for name in (both if args.config == "both" else (args.config,)):
        res[name] = measure(name, args)
        gc.collect()
    return write_result(res, args.out)


if __name__ == "__main__":
    sys.exit(main())
