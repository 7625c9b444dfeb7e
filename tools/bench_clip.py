"""Cost of global-norm gradient clipping (include/td3.h "gradient clipping": td3_set_grad_clip) at bench.py's
shapes: C2, HalfCheetah dims at batch 256; C3, Humanoid dims at batch 1024; C4, the particle learner at batch
4096 -- all LayerNorm, rings from fill_synthetic.

Reports, as one JSON line and a file (default profiles/clip.json), per shape:
  (a) steps/s of ``TD3.train`` with clipping off, on for the critic only, and on for both groups: three
      learners that live side by side, warmed up, then ``--runs`` rounds in which each runs one timed region
      of ``--steps`` steps that ends in a synchronise -- the regions ALTERNATE round after round; the median,
      the range and every run;
  (b) device microseconds of the stages a clipping group runs (<tag>_dw gradient-only, <tag>_enc_adam,
      <tag>_gnorm, <tag>_adam) against the fused <tag>_dw (+ <tag>_enc_adam) they replace, by
      td3_time_stage: ``--iters`` launches replayed from a graph between two events, median of ``--reps``.
With ``--parent DIR`` (a built checkout of the parent commit) it also runs ``bench.py --gpus 1`` of this tree
(clipping off: bench.py never turns it on) and of that one as child processes, in ABBA order, ``--bench-runs``
times each, per ``--bench-config``: the spread of the parent's own runs is the yardstick for "the step with
clipping off is unchanged".  The thresholds are far below the gradients' norms, so every step really scales.
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

MAX_NORM = 1e-3
VARIANTS = (("off", None), ("critic", (None, MAX_NORM)), ("both", (MAX_NORM, MAX_NORM)))   # name -> max_grad_norm
TAIL = ("_dw", "_enc_adam", "_gnorm", "_adam")


def make(cfg, max_grad_norm):
    if cfg["kind"] == "particles":
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as RB
        obs = (Box((cfg["F"],)), Box((cfg["N"], cfg["D"])))
        pol = TD3(obs, Box((cfg["ad"],)), norm="layer", device=0, seed=17, use_graph="auto", max_grad_norm=max_grad_norm)
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as RB
        obs = Box((cfg["sd"],))
        pol = TD3(obs, Box((cfg["ad"],)), max_action=cfg["ma"], device=0, seed=17, use_graph="auto", norm="layer",
                  max_grad_norm=max_grad_norm)
    rb = RB(obs, Box((cfg["ad"],)), max_size=cfg["replay"], device=0, seed=101)
    rb.fill_synthetic(cfg["replay"], cfg["ma"], seed=7)
    return pol, rb


def stage_us(pol, rb, batch, iters, reps):
    """{stage: median device us} of the actor phase's optimizer tails (C_* and A_*)."""
    from td3_amd._lib import check
    ms = (C.c_float * 128)()
    n = C.c_int()
    check(pol._lib.td3_profile_stages(pol._h, rb.handle, batch, 1, ms, 128, C.byref(n)), "td3_profile_stages")
    out = {}
    for i in range(n.value):
        name = pol._lib.td3_stage_name(pol._h, i).decode()
        if not (name[:1] in "CA" and name[1:] in TAIL):
            continue
        t = []
        for _ in range(reps):
            v = C.c_float()
            check(pol._lib.td3_time_stage(pol._h, i, iters, C.byref(v)), "td3_time_stage")
            t.append(v.value * 1000.0)
        out[name] = {"kernel": pol._lib.td3_stage_kernel(pol._h, i).decode(), "median_us": round(float(np.median(t)), 3),
                     "reps_us": [round(x, 3) for x in t]}
    for tag in "CA":
        out[f"{tag}_total_us"] = round(sum(v["median_us"] for k, v in out.items() if k[:1] == tag and k[1:] in TAIL), 3)
    return out


def measure(name, args):
    import torch
    from bench import CONFIGS
    cfg = CONFIGS[name]
    Bc = cfg["batch"]
    part = cfg["kind"] == "particles"
    steps = args.steps or (200 if part else 2000 if Bc <= 256 else 1000)
    warmup = args.warmup or (10 if part else 100)
    iters = 3 if part else args.iters
    torch.manual_seed(1000)
    trio = {k: make(cfg, mn) for k, mn in VARIANTS}
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
           "steps_per_s": {k: {"median": float(np.median(v)), "range": [round(min(v), 2), round(max(v), 2)],
                               "runs": [round(x, 2) for x in v]} for k, v in runs.items()}}
    off = res["steps_per_s"]["off"]["median"]
    res["us_per_step_over_off"] = {k: round(1e6 / res["steps_per_s"][k]["median"] - 1e6 / off, 3)
                                   for k in trio if k != "off"}
    res["stage_device_us"] = {k: stage_us(pol, rb, Bc, iters, args.reps) for k, (pol, rb) in trio.items()}
    res["clip_info"] = {k: trio[k][0].clip_info() for k in trio if k != "off"}
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
                raise SystemExit(f"bench_clip: bench.py failed in {tree} ({r.returncode}):\n{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            out[key].append({"value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"]})
            print(f"bench_clip: bench.py {config} {key}: {line['value']} {line['unit']}", file=sys.stderr, flush=True)
    for key in ("this", "parent"):
        v = [x["value"] for x in out[key]]
        out[f"{key}_median"], out[f"{key}_range"] = float(np.median(v)), [min(v), max(v)]
    lo = max(out["this_range"][0], out["parent_range"][0])
    hi = min(out["this_range"][1], out["parent_range"][1])
    spread = out["parent_range"][1] - out["parent_range"][0]
    out["ranges_overlap"] = lo <= hi
    out["median_gap_within_parent_spread"] = abs(out["this_median"] - out["parent_median"]) < spread
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("halfcheetah", "humanoid", "particles", "all"), default="all")
    ap.add_argument("--steps", type=int, default=None, help="default 2000 (halfcheetah) / 1000 (humanoid) / 200 (particles)")
    ap.add_argument("--warmup", type=int, default=None, help="default 100 / 100 / 10")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py A/B")
    ap.add_argument("--bench-config", choices=("halfcheetah", "humanoid", "both"), default="both")
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip.json"))
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    every = ("halfcheetah", "humanoid", "particles")
    res = {"config": dict(runs=args.runs, iters=args.iters, reps=args.reps, max_norm=MAX_NORM, norm="layer")}
    if args.parent:                       # first: child processes, while this one has not opened the GPU
        both = ("halfcheetah", "humanoid")
        res["bench_py"] = {c: bench_pair(args, c) for c in (both if args.bench_config == "both" else (args.bench_config,))}
    from bench import pin_host_thread
    pin_host_thread(0)
    res["device"] = torch.cuda.get_device_name(0)
    for name in (every if args.config == "all" else (args.config,)):
        res[name] = measure(name, args)
        print(f"bench_clip: {name}: {json.dumps(res[name]['steps_per_s'])}", file=sys.stderr, flush=True)
        gc.collect()
    return write_result(res, args.out)


if __name__ == "__main__":
    sys.exit(main())
