"""Cost of the training log (include/td3.h "training log": td3_log_enable, train_log_kernel) at bench.py's
two learner shapes: HalfCheetah dims at batch 256 (a 10^6-row ring) and the particle learner at batch 4096
(features 7, 350 particles x 9, 3 actions, CDQ, a 10^5-row ring), both LayerNorm, rings from fill_synthetic.

Reports, as one JSON line and a file (default profiles/train_log.json), per shape:
  (a) steps/s of ``TD3.train`` with the log off, with ``every=1`` and with ``every=16``: three learners that
      live side by side, warmed up, then ``--runs`` rounds in which each runs one timed region of ``--steps``
      steps that ends in a synchronise -- the regions ALTERNATE, off / every=1 / every=16, round after
      round; the median of each and every run;
  (b) device microseconds per launch of train_log_kernel at that shape: the time between two HIP events
      around ``--launches`` launches (td3_debug_log_launch: the last logged step's launch again, same
      buffers, same slot), queued while the stream is still busy with a filler kernel so the events
      bracket back-to-back device work and not the host's submit rate; median of ``--reps`` windows.
With ``--parent DIR`` (a built checkout of the parent commit) it also runs ``bench.py --gpus 1`` of this
tree and of that one as child processes, ALTERNATED, ``--bench-runs`` times each, and reports every
steps/s figure: the spread of the parent's own runs is the yardstick for "the log-off step is unchanged".
No pass/fail: the numbers are reported.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
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

from bench_per import Box, device_us, timed_region, write_result  # noqa: E402

VARIANTS = (("off", None), ("every_1", 1), ("every_16", 16))


def make(cfg, every):
    if cfg["kind"] == "particles":
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as RB
        obs = (Box((cfg["F"],)), Box((cfg["N"], cfg["D"])))
        pol = TD3(obs, Box((cfg["ad"],)), norm="layer", device=0, seed=17, use_graph="auto")
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as RB
        obs = Box((cfg["sd"],))
        pol = TD3(obs, Box((cfg["ad"],)), max_action=cfg["ma"], device=0, seed=17, use_graph="auto", norm="layer")
    rb = RB(obs, Box((cfg["ad"],)), max_size=cfg["replay"], device=0, seed=101)
    rb.fill_synthetic(cfg["replay"], cfg["ma"], seed=7)
    if every is not None:
        pol.enable_train_log(capacity=4096, every=every)
    return pol, rb


def measure(name, args):
    import torch
    from bench import CONFIGS
    from td3_amd._lib import check
    cfg = CONFIGS[name]
    Bc = cfg["batch"]
    part = cfg["kind"] == "particles"
    steps, warmup = (args.steps or (200 if part else 2000)), (args.warmup or (10 if part else 100))
    torch.manual_seed(1000)
    trio = {k: make(cfg, every) for k, every in VARIANTS}
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
                                   for k in ("every_1", "every_16")}
    pol, rb = trio["every_1"]
    pol.train(rb, Bc)                                      # the last step is a logged one
    pol.sync()
    stream = torch.cuda.Stream(device=0)
    sp = stream.cuda_stream
    res["kernel_device_us"] = device_us(lambda: check(pol._lib.td3_debug_log_launch(pol._h, sp), "log launch"),
                                        stream, args.launches, args.reps)
    stream.synchronize()
    pol.sync()
    last = pol.train_log.entries()[-1]
    res["last_entry"] = {k: (int(last[k]) if last[k].dtype.kind == "i" else float(last[k])) for k in last.dtype.names}
    for pol, rb in trio.values():
        pol.sync()
    return res


def bench_pair(args):
    """bench.py of this tree and of the parent's, alternated child processes; every steps/s figure."""
    out = {"this": [], "parent": [], "order": "alternated: this, parent, this, ...",
           "argv": ["--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]}
    trees = (("this", ROOT), ("parent", os.path.abspath(args.parent)))
    for _ in range(args.bench_runs):
        for key, tree in trees:
            r = subprocess.run([sys.executable, "bench.py", *out["argv"]], cwd=tree, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench_train_log: bench.py failed in {tree} ({r.returncode}):\n{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            out[key].append(line)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("halfcheetah", "particles", "both"), default="both")
    ap.add_argument("--steps", type=int, default=None, help="default 2000 (halfcheetah) / 200 (particles)")
    ap.add_argument("--warmup", type=int, default=None, help="default 100 / 10")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py A/B")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_log.json"))
    args = ap.parse_args(argv)
    if args.launches < 200:
        ap.error("--launches must be at least 200")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_log: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    res = {"config": dict(runs=args.runs, launches=args.launches, reps=args.reps, capacity=4096, norm="layer")}
    if args.parent:                       # first: child processes, while this one has not opened the GPU
        res["bench_py"] = bench_pair(args)
    from bench import pin_host_thread
    pin_host_thread(0)
    res["device"] = torch.cuda.get_device_name(0)
    for name in (("halfcheetah", "particles") if args.config == "both" else (args.config,)):
        res[name] = measure(name, args)
        gc.collect()
    return write_result(res, args.out)


if __name__ == "__main__":
    sys.exit(main())
