"""Cost of the demonstration-replay step (include/td3.h "Demonstration replay": td3_train_step_mixed) at
bench.py's shapes: C2, HalfCheetah dims at batch 256 (a 10^6-row online ring), C3, Humanoid dims at batch
1024 (a 2*10^6-row online ring), and C4, the particle learner at batch 4096 (a 10^5-row online ring).  The
demo ring holds 10^5 rows (10^4 at C4), demo_fraction is 0.5, rings from fill_synthetic, LayerNorm.

Reports, as one JSON line and a file (default profiles/mixed.json), per shape:
  (a) steps/s of ``TD3.train`` on the online ring alone (plain), on the ``MixedReplay`` (mixed) and of the
      host composition the mixed step replaces (``sample`` on both rings, ``torch.cat`` per field,
      ``train`` on that foreign batch): three learners that share the two rings, warmed up, then ``--runs``
      rounds in which each runs one timed region that ends in a synchronise -- the regions ALTERNATE round
      after round; the median and every run;
  (b) device microseconds of the mixed input launch (td3_debug_mixed_input: ``--launches`` calls queued
      behind a few ms of device work between two events, median of ``--reps`` windows; and ``--iters`` of
      them replayed from one graph) next to the stand-alone gather_kernel at the same batch
      (td3_time_stage stage 0: ``--iters`` launches replayed from a graph, median of ``--reps``); the
      launch's achieved GB/s (from the direct-launch figure) with
      bytes = live rows x (record floats read + floats written) x 4, and its fraction of the 5.5 TB/s at
      which whole random rows gather on this part.
With ``--parent DIR`` (a built checkout of the parent commit) it also runs ``bench.py --gpus 1`` of this
tree and of that one as child processes, in ABBA order (this, parent, parent, this, ...),
``--bench-runs`` times each, for C2 and C3: the spread of each build's own runs is the yardstick for "the
plain step is unchanged".
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

from bench_per import Box, device_us, timed_region, write_result  # noqa: E402

SHAPES = {"halfcheetah": "C2", "humanoid": "C3", "particles": "C4"}
DEMO_ROWS = {"halfcheetah": 100_000, "humanoid": 100_000, "particles": 10_000}
STEPS = {"halfcheetah": 2000, "humanoid": 1000, "particles": 60}
RANDOM_ROW_GBS = 5500.0          # whole random rows of a buffer far larger than the caches, gathered once


class HostMix:
    """The composition without the feature: a foreign buffer whose ``sample`` concatenates the two rings'."""

    def __init__(self, mix):
        self.mix = mix

    def sample(self, batch_size):
        return self.mix.sample(batch_size)


def make(cfg, demo_rows):
    from td3_amd.my_replay_buffer import MixedReplay
    if cfg["kind"] == "particles":
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as RB
        obs = (Box((cfg["F"],)), Box((cfg["N"], cfg["D"])))
        kw = {}
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as RB
        obs = Box((cfg["sd"],))
        kw = dict(max_action=cfg["ma"])
    act = Box((cfg["ad"],))
    online = RB(obs, act, max_size=cfg["replay"], device=0, seed=101)
    online.fill_synthetic(cfg["replay"], cfg["ma"], seed=7)
    demo = RB(obs, act, max_size=demo_rows, device=0, seed=202)
    demo.fill_synthetic(demo_rows, cfg["ma"], seed=9)
    mix = MixedReplay(online, demo, 0.5)
    pols = {k: TD3(obs, act, device=0, seed=17, use_graph="auto", norm="layer", **kw) for k in ("plain", "mixed", "host")}
    return pols, {"plain": online, "mixed": mix, "host": HostMix(mix)}, online, demo


def moved_floats(cfg, online):
    """(record floats read, floats written) per live row of the mixed input launch."""
    if cfg["kind"] != "particles":
        sd, ad = cfg["sd"], cfg["ad"]
        return online.record_floats, 3 * sd + ad + 2              # X_SA [s | a], X_SP s, X_S2A s', R, ND
    F, A, np_ = cfg["F"], cfg["ad"], cfg["N"] * cfg["D"]
    return online.record_floats, 7 * F + 2 * A + 2 + 2 * np_      # 3 + 2 J small segments (CDQ: J = 2), the blocks


def graph_us(call, device, iters, reps):
    """Median over ``reps`` replays of (HIP-event time around one graph of ``iters`` calls) / iters, in us."""
    import torch
    stream = torch.cuda.Stream(device=device)
    sp = stream.cuda_stream
    try:
        with torch.cuda.stream(stream):
            for _ in range(20):                          # warm: the rings' ordering moves to this stream
                call(sp)
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                for _ in range(iters):
                    call(sp)
            g.replay()                                   # warm (graph upload)
            t = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                g.replay()
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1) * 1000.0 / iters)
        stream.synchronize()
    except Exception as e:                               # reported, not fatal: the direct-launch figure stands
        return {"error": f"{type(e).__name__}: {e}"}
    return {"median_us": round(float(np.median(t)), 3), "reps_us": [round(x, 3) for x in t],
            "method": "td3_debug_mixed_input, graph replay"}


def input_costs(cfg, pol, online, demo, batch, args):
    import torch
    from td3_amd._lib import check
    lib = pol._lib
    out = {}
    # the stand-alone gather_kernel of the online ring at this batch (for the particle learner: its small fields)
    ms = (C.c_float * 128)()
    n = C.c_int()
    check(lib.td3_profile_stages(pol._h, online.handle, batch, 0, ms, 128, C.byref(n)), "td3_profile_stages")
    t = []
    for _ in range(args.reps):
        v = C.c_float()
        check(lib.td3_time_stage(pol._h, 0, args.iters, C.byref(v)), "td3_time_stage")
        t.append(v.value * 1000.0)
    out["gather_kernel"] = {"median_us": round(float(np.median(t)), 3), "reps_us": [round(x, 3) for x in t],
                            "method": "td3_time_stage stage 0, graph replay"}
    mix_pol = pol
    from td3_amd.my_replay_buffer import MixedReplay
    mix_pol.train(MixedReplay(online, demo, 0.5), batch)          # the step whose input launch is re-queued
    mix_pol.sync()
    stream = torch.cuda.Stream(device=online.device)
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    out["mixed_input"] = device_us(lambda: check(lib.td3_debug_mixed_input(mix_pol._h, online.handle, demo.handle, sp),
                                                 "td3_debug_mixed_input"), stream, args.launches, args.reps)
    out["mixed_input"]["method"] = "td3_debug_mixed_input, direct launches behind queued device work"
    stream.synchronize()
    # the same launch timed as gather_kernel is: `iters` of them replayed from one graph between two events
    out["mixed_input_graph"] = graph_us(lambda sp: check(lib.td3_debug_mixed_input(mix_pol._h, online.handle, demo.handle, sp),
                                                         "td3_debug_mixed_input"), online.device, args.iters, args.reps)
    rd, wr = moved_floats(cfg, online)
    by = batch * (rd + wr) * 4
    gbs = by / (out["mixed_input"]["median_us"] * 1e-6) / 1e9
    out["mixed_input"].update(bytes=by, record_floats_read=rd, floats_written=wr, gb_per_s=round(gbs, 1))
    if cfg["kind"] == "particles":
        out["mixed_input"]["fraction_of_random_row_rate"] = round(gbs / RANDOM_ROW_GBS, 3)
    return out


def measure(name, args):
    import torch
    from bench import CONFIGS
    cfg = CONFIGS[name]
    Bc = cfg["batch"]
    steps, warmup = args.steps or STEPS[name], args.warmup or (100 if name != "particles" else 6)
    torch.manual_seed(1000)
    pols, bufs, online, demo = make(cfg, DEMO_ROWS[name])
    gc.collect()
    gc.disable()
    for k, pol in pols.items():
        for _ in range(warmup):
            pol.train(bufs[k], Bc)
    runs = {k: [] for k in pols}
    for _ in range(args.runs):
        for k, pol in pols.items():
            runs[k].append(timed_region(pol, bufs[k], steps, Bc))
    gc.enable()
    res = {"shape": SHAPES[name], "batch": Bc, "online_rows": cfg["replay"], "demo_rows": DEMO_ROWS[name],
           "demo_fraction": 0.5, "n_demo": bufs["mixed"].n_demo(Bc), "steps": steps, "warmup": warmup,
           "order": "alternated",
           "steps_per_s": {k: {"median": float(np.median(v)), "runs": [round(x, 2) for x in v]} for k, v in runs.items()}}
    med = {k: res["steps_per_s"][k]["median"] for k in pols}
    res["us_per_step_mixed_over_plain"] = round(1e6 / med["mixed"] - 1e6 / med["plain"], 3)
    res["mixed_over_host"] = round(med["mixed"] / med["host"], 3)
    res["input_device_us"] = input_costs(cfg, pols["mixed"], online, demo, Bc, args)
    for pol in pols.values():
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
                raise SystemExit(f"bench_mixed: bench.py failed in {tree} ({r.returncode}):\n{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            out[key].append({"value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"]})
    for key in ("this", "parent"):
        v = [x["value"] for x in out[key]]
        out[key + "_median"], out[key + "_min"], out[key + "_max"] = float(np.median(v)), min(v), max(v)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=(*SHAPES, "all"), default="all")
    ap.add_argument("--steps", type=int, default=None, help="default 2000 (halfcheetah) / 1000 (humanoid) / 60 (particles)")
    ap.add_argument("--warmup", type=int, default=None, help="default 100 / 100 / 6")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py A/B")
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed.json"))
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    res = {"config": dict(runs=args.runs, launches=args.launches, iters=args.iters, reps=args.reps, norm="layer",
                          demo_fraction=0.5)}
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
