"""Cost of prioritized replay on the device ring (include/td3.h: rb_sample_prioritized,
rb_update_priorities, td3_train_step_prioritized) at bench.py's flagship shape: HalfCheetah dims,
batch 256, LayerNorm, a 10^6-row ring from fill_synthetic.

Reports, as one JSON line and a file (default profiles/per_c2.json):
  (a) steps/s of ``TD3.train`` on a ring without priorities: the production path, whose first layer
      draws the rows (what bench.py times), and
  (b) steps/s of ``TD3.train`` on a prioritized ring (draw, gather, weighted step, write-back),
      each as bench.py measures it: warm-up, then ``--runs`` timed regions of ``--steps`` steps that end
      in a synchronise; the median and every run;
  (c) device microseconds per call of the draw (two launches), the stand-alone gather of the drawn rows
      and the priority update (clear, store, one repair launch per tree level above the leaves), for
      the 10^6-row ring (4 levels) and a 4096-row ring (2 levels).  Each figure is the time between two
      HIP events around ``--launches`` calls, divided by their number; the calls are queued while the
      stream is still busy with a filler kernel, so the events bracket back-to-back device work and
      not the host's submit rate.  Median of ``--reps`` such windows.
``--config particles`` measures the particle learner's step (td3_train_step_prioritized_particles) at
bench.py's C4 shape instead: features 7, 350 particles x 9, 3 actions, batch 4096, LayerNorm, CDQ, a
10^5-row ring (default file profiles/per_c4.json).  Its (a) and (b) regions ALTERNATE, uniform then
prioritized, run after run, on two learners that live side by side; its (c) is the device time of the
prioritized step's own extra stages at that batch, by the same event method: the draw, the gather of
the drawn rows' small fields (the step's own launch, td3_debug_per_stage 0), the combine of the critics'
|TD error| rows (td3_debug_per_stage 1) and the priority update.
No pass/fail: the numbers are reported.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SD, AD, MA, B = 17, 6, 1.0, 256            # bench.py CONFIGS["halfcheetah"]


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def timed_region(pol, rb, steps, batch):
    import torch
    pol.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pol.train(rb, batch)
    pol.sync()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def steps_per_s(pol, rb, steps, warmup, runs):
    for _ in range(warmup):
        pol.train(rb, B)
    out = [timed_region(pol, rb, steps, B) for _ in range(runs)]
    return {"median": float(np.median(out)), "runs": [round(x, 1) for x in out]}


def device_us(call, stream, launches, reps):
    """Median over ``reps`` windows of (HIP-event time around ``launches`` calls) / launches, in us."""
    import torch
    filler = torch.randn(4096, 4096, device="cuda")
    res = []
    with torch.cuda.stream(stream):
        for _ in range(20):                              # warm: code objects, the ring's stream ordering
            call()
        for _ in range(reps):
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(8):                           # a few ms of device work: the calls queue behind it
                filler @ filler
            e0.record(stream)
            for _ in range(launches):
                call()
            e1.record(stream)
            e1.synchronize()
            res.append(e0.elapsed_time(e1) * 1000.0 / launches)
    return {"median_us": round(float(np.median(res)), 3), "windows_us": [round(x, 3) for x in res]}


def ring_costs(rows, launches, reps):
    import torch
    from td3_amd import _lib
    from td3_amd._lib import check
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    rb = ReplayBuffer_featured(Box((SD,)), Box((AD,)), max_size=rows, seed=101)
    rb.fill_synthetic(rows, MA, seed=7)
    rb.enable_priorities()
    lib, h = rb._lib, rb.handle
    dev = rb.device
    # priorities spread like |TD errors|, so the draws walk different paths of the tree
    rb.set_priorities(torch.arange(rows, device=dev), torch.randn(rows, device=dev).abs() + 1e-3)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    w = torch.empty(B, dtype=torch.float32, device=dev)
    td = torch.rand(B, device=dev)
    outs = [torch.empty((B, n), device=dev) for n in (SD, AD, SD, 1, 1)]
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {
        "draw": lambda: check(lib.rb_sample_prioritized(h, B, 0.4, None, idx.data_ptr(), w.data_ptr(), sp), "draw"),
        "gather": lambda: check(lib.rb_sample(h, B, *[t.data_ptr() for t in outs], idx.data_ptr(), None, sp), "gather"),
        "update": lambda: check(lib.rb_update_priorities(h, idx.data_ptr(), td.data_ptr(), B, sp), "update"),
    }
    res = {"rows": rows, "levels": rb.priority_info()["levels"]}
    for name, call in calls.items():
        res[name] = device_us(call, stream, launches, reps)
    stream.synchronize()
    check(lib.rb_sync(h), "rb_sync")
    return res


def particles_main(args):
    """--config particles: see the module docstring."""
    import torch
    from bench import CONFIGS, pin_host_thread
    from td3_amd._lib import check
    from td3_amd.TD3_particles import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    pin_host_thread(0)
    cfg = CONFIGS["particles"]
    F, N, D, A, Bc = cfg["F"], cfg["N"], cfg["D"], cfg["ad"], cfg["batch"]
    rows = args.rows or cfg["replay"]
    obs = (Box((F,)), Box((N, D)))
    torch.manual_seed(1000)
    res = {"config": dict(features=F, particles=N, particle_dim=D, action_dim=A, batch=Bc, norm="layer", cdq=True,
                          ring_rows=rows, steps=args.steps, warmup=args.warmup, runs=args.runs,
                          launches=args.launches, reps=args.reps, per_beta=0.4, alpha=0.6, order="alternated"),
           "device": torch.cuda.get_device_name(0)}
    pair = {}
    for key, prioritized in (("a_uniform_steps_per_s", False), ("b_prioritized_steps_per_s", True)):
        pol = TD3(obs, Box((A,)), norm="layer", device=0, seed=17, use_graph="auto",
                  per_beta=0.4 if prioritized else None)
        rb = ReplayBuffer_particles(obs, Box((A,)), max_size=rows, device=0, seed=101)
        rb.fill_synthetic(rows, cfg["ma"], seed=7)
        if prioritized:
            rb.enable_priorities()
        pair[key] = (pol, rb)
    gc.collect()
    gc.disable()
    for pol, rb in pair.values():
        for _ in range(args.warmup):
            pol.train(rb, Bc)
    runs = {k: [] for k in pair}
    for _ in range(args.runs):
        for k, (pol, rb) in pair.items():
            runs[k].append(timed_region(pol, rb, args.steps, Bc))
    gc.enable()
    for k, v in runs.items():
        res[k] = {"median": float(np.median(v)), "runs": [round(x, 2) for x in v]}
    pol, rb = pair["b_prioritized_steps_per_s"]
    pol.sync()
    lib, h, dev = rb._lib, rb.handle, rb.device
    idx = torch.empty(Bc, dtype=torch.int64, device=dev)
    w = torch.empty(Bc, dtype=torch.float32, device=dev)
    td = torch.rand(Bc, device=dev)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {
        "draw": lambda: check(lib.rb_sample_prioritized(h, Bc, 0.4, None, idx.data_ptr(), w.data_ptr(), sp), "draw"),
        "gather": lambda: check(lib.td3_debug_per_stage(pol._h, h, 0, sp), "gather"),
        "combine": lambda: check(lib.td3_debug_per_stage(pol._h, h, 1, sp), "combine"),
        "update": lambda: check(lib.rb_update_priorities(h, idx.data_ptr(), td.data_ptr(), Bc, sp), "update"),
    }
    check(lib.rb_sample_prioritized(h, Bc, 0.4, None, idx.data_ptr(), w.data_ptr(), sp), "draw")   # rows for `update`
    cost = {"rows": rows, "batch": Bc, "levels": rb.priority_info()["levels"]}
    for name, call in calls.items():
        cost[name] = device_us(call, stream, args.launches, args.reps)
    cost["sum_of_medians_us"] = round(sum(cost[k]["median_us"] for k in calls), 3)
    stream.synchronize()
    check(lib.rb_sync(h), "rb_sync")
    res["c_device_us_per_call"] = cost
    return res


def write_result(res, out):
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(line, flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("halfcheetah", "particles"), default="halfcheetah")
    ap.add_argument("--steps", type=int, default=None, help="default 2000 (halfcheetah) / 200 (particles)")
    ap.add_argument("--warmup", type=int, default=None, help="default 100 / 10")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=None, help="default 10^6 / bench.py's particle ring")
    ap.add_argument("--out", default=None, help="default profiles/per_c2.json / profiles/per_c4.json")
    args = ap.parse_args(argv)
    if args.launches < 200:
        ap.error("--launches must be at least 200")
    part = args.config == "particles"
    args.steps = args.steps or (200 if part else 2000)
    args.warmup = args.warmup or (10 if part else 100)
    args.out = args.out or os.path.join(ROOT, "profiles", "per_c4.json" if part else "per_c2.json")
    if not part:
        args.rows = args.rows or 1_000_000

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_per: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    if part:
        return write_result(particles_main(args), args.out)
    from bench import pin_host_thread
    pin_host_thread(0)
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured

    torch.manual_seed(1000)
    res = {"config": dict(state_dim=SD, action_dim=AD, batch=B, norm="layer", ring_rows=args.rows, steps=args.steps,
                          warmup=args.warmup, runs=args.runs, launches=args.launches, reps=args.reps, per_beta=0.4,
                          alpha=0.6),
           "device": torch.cuda.get_device_name(0)}
    gc.collect()
    gc.disable()
    for key, prioritized in (("a_uniform_steps_per_s", False), ("b_prioritized_steps_per_s", True)):
        pol = TD3(Box((SD,)), Box((AD,)), max_action=MA, device=0, seed=17, use_graph="auto", norm="layer")
        rb = ReplayBuffer_featured(Box((SD,)), Box((AD,)), max_size=args.rows, device=0, seed=101)
        rb.fill_synthetic(args.rows, MA, seed=7)
        if prioritized:
            rb.enable_priorities()
        res[key] = steps_per_s(pol, rb, args.steps, args.warmup, args.runs)
        del pol, rb
    gc.enable()
    res["c_device_us_per_call"] = [ring_costs(args.rows, args.launches, args.reps),
                                   ring_costs(4096, args.launches, args.reps)]
    return write_result(res, args.out)


if __name__ == "__main__":
    sys.exit(main())
