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


def steps_per_s(pol, rb, steps, warmup, runs):
    import torch
    for _ in range(warmup):
        pol.train(rb, B)
    out = []
    for _ in range(runs):
        pol.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pol.train(rb, B)
        pol.sync()
        torch.cuda.synchronize()
        out.append(steps / (time.perf_counter() - t0))
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_c2.json"))
    args = ap.parse_args(argv)
    if args.launches < 200:
        ap.error("--launches must be at least 200")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_per: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
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
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
