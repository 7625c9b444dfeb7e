#!/usr/bin/env python3
"""TD3 gradient-steps/s on MI355X (BASELINE.json metric), HalfCheetah-v4 shapes, batch 256/GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full] [--config C]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

``--gpus N`` without an external launcher starts the N rank processes itself (``launch_workers``,
before any GPU call); under ``torch.distributed.run`` it must equal WORLD_SIZE.

One "step" = one ``TD3.train(replay_buffer, 256)`` call (TD3_featured.py:123-171): Philox
index draw + HBM gather from a 1e6-row replay ring pre-filled with synthetic transitions
(SURVEY.md §8d), the twin-critic update and, every policy_freq=2 steps, the actor update +
Polyak.  N GPUs = data parallel: every rank owns a replay shard and samples its own 256
rows; gradients are all-reduced over RCCL (xGMI) before Adam, so one step is one optimizer step
on a global batch of 256·N rows.  ``value`` = optimizer steps/s over the K timed steps,
``ms_per_step`` = the milliseconds one of them took, ``samples_per_s`` = rows consumed per second
over all ranks (weak scaling).

A plain run sets up, takes the W warm-up steps, times the K steps (one timed region), writes the
learner's state after the last timed step with ``--dump-outputs DIR`` (``dump_outputs``) and prints
ONE JSON line on rank 0 (the driver contract).  Everything else is behind ``--full``: the timed
region is repeated (``--runs``, 5 there unless given; ``value`` = the median run)
and the line gains a ``roofline`` object for the
dominant kernel (HIP-event timed live; ``step_frac`` = the step's algorithmic FLOP / measured
step time / fp32 MFMA peak), a ``gather`` object for the replay-ring sample kernel (bytes / HIP
event time vs the 8 TB/s HBM peak) and a ``cpu_baseline`` (the torch-CPU restatement of the
reference step, oracle/td3_torch_cpu.py, on the host cores of this box: rank 0, N=1 only, in a
child process); ``--no-roofline`` / ``--no-cpu-baseline`` leave those parts out of a ``--full``
run.  Each rank pins its host thread to 8 CPUs of its GPU's NUMA node before touching
the GPU (``pin_host_thread``; ``BENCH_PIN=0`` turns it off) and reports them in ``host_pin``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


# BASELINE.json configs besides the headline one (``--config``): C1 Pendulum-v1 (the reference's
# CPU-runnable case) B=256 replay 1e5, C3 Humanoid-v4 TD3_featured
# B=1024 replay 2e6, C4 water-pouring particles TD3_particles B=4096 (F=7, N=350, D=9, A=3 as
# assumed in SURVEY.md §8d) replay 1e5.
CONFIGS = {
    "pendulum": dict(kind="featured", sd=3, ad=1, ma=2.0, batch=256, replay=100_000,
                     workload="TD3_base/TD3_featured.train(replay_buffer, 256) on Pendulum-v1 shapes "
                              "(state 3, action 1, max_action 2, actor 500-400-300, critic 2x 500-400-200, "
                              "LayerNorm, policy_freq 2), replay 1e5 per GPU (BASELINE config 1)"),
    "halfcheetah": dict(kind="featured", sd=17, ad=6, ma=1.0, batch=256, replay=1_000_000,
                        workload="TD3_featured.train(replay_buffer, 256) on HalfCheetah-v4 shapes "
                                 "(state 17, action 6, actor 500-400-300, critic 2x 500-400-200, "
                                 "LayerNorm, policy_freq 2), replay 1e6 per GPU"),
    "humanoid": dict(kind="featured", sd=376, ad=17, ma=0.4, batch=1024, replay=2_000_000,
                     workload="TD3_featured.train(replay_buffer, 1024) on Humanoid-v4 shapes "
                              "(state 376, action 17, actor 500-400-300, critic 2x 500-400-200, "
                              "LayerNorm, policy_freq 2), replay 2e6 per GPU"),
    "particles": dict(kind="particles", F=7, N=350, D=9, ad=3, ma=1.0, batch=4096, replay=100_000,
                      workload="TD3_particles.train(replay_buffer, 4096): features 7, 350 particles x 9, "
                               "action 3, encoders conv1 256 / conv2 128, MLP 500-400-300 with lnorm1 + "
                               "LayerNorm, CDQ, policy_freq 2, replay 1e5 per GPU"),
}
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8 TB/s spec
# per-config rocprofv3 PMC summaries (tools/pmc_summary.py output): HBM bytes per launch per kernel
PMC_FILES = {"halfcheetah": "pmc_traffic.json", "humanoid": "pmc_traffic_humanoid.json",
             "pendulum": "pmc_traffic_pendulum.json",
             "particles": "pmc_traffic_particles.json"}
FP32_PEAK_TFLOPS = 157.3         # MI355X_MICROARCH.md: f32 MFMA / vector peak


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _parse_cpulist(s):
    out = set()
    for part in s.strip().split(","):
        if part:
            a, _, b = part.partition("-")
            out.update(range(int(a), int(b or a) + 1))
    return out


# Run in a child process: this one must not initialise the GPU before it has pinned itself (the
# HIP runtime's own threads inherit the affinity of the thread that creates them).
_BUS_QUERY = ("import ctypes, sys\n"
              "for n in ('libamdhip64.so', '/opt/rocm/lib/libamdhip64.so'):\n"
              "    try:\n        h = ctypes.CDLL(n); break\n    except OSError:\n        h = None\n"
              "b = ctypes.create_string_buffer(64)\n"
              "print(b.value.decode() if h and h.hipDeviceGetPCIBusId(b, 64, int(sys.argv[1])) == 0 else '')\n")


def pin_host_thread(local_rank):
    """Pin this rank's host thread (and the HIP-runtime threads it will create) to a few CPUs of the
    GPU's own NUMA node, as RCCL does for its proxy threads.  Measured in the driver's form
    (`tools/gpu_r6_numa.sh`, `profiles/r06_host_pinning.txt`): unpinned, whole invocations drop
    into a slow mode (9.65-10.2 k steps/s) when the scheduler moves the launching thread across a
    shared 256-CPU host; pinned to 8 CPUs every invocation ran 10.37-10.44 k.  BENCH_PIN: "0" off,
    "node" the whole local node, n (default 8) n CPUs of it, offset by the local rank.  Returns the
    previous CPU set (restored for the CPU baseline) and a description for the JSON line."""
    mode = os.environ.get("BENCH_PIN", "8").strip().lower()
    if mode in ("0", "off", "") or not hasattr(os, "sched_setaffinity"):
        return None, None
    import subprocess
    allowed = sorted(os.sched_getaffinity(0))
    node, local = None, set()
    try:
        q = subprocess.run([sys.executable, "-c", _BUS_QUERY, str(local_rank)], capture_output=True,
                           text=True, timeout=120)
        bus = q.stdout.strip().lower()
        if bus:
            dev = os.path.join("/sys/bus/pci/devices", bus)
            local = _parse_cpulist(open(os.path.join(dev, "local_cpulist")).read())
            node = int(open(os.path.join(dev, "numa_node")).read())
    except (OSError, ValueError, subprocess.SubprocessError):
        pass
    pool = sorted(local.intersection(allowed)) or allowed
    if mode == "node":
        cpus = pool
    else:
        n = max(1, min(int(mode) if mode.isdigit() else 8, len(pool)))
        start = (local_rank * n) % len(pool)
        cpus = (pool[start:] + pool[:start])[:n]
    os.sched_setaffinity(0, cpus)
    return allowed, {"cpus": cpus if len(cpus) <= 16 else f"{len(cpus)} CPUs", "numa_node": node,
                     "gpu_local": bool(local), "env": "BENCH_PIN"}


def stage_table(pol, rb, batch, iters=50, reps=5):
    """Per-stage device time (HIP events, handle stream) for an odd and an even step: the median
    over `reps` runs of the mean of iters/reps back-to-back launches (a host or clock hiccup in
    one run does not move the figure)."""
    lib, h = pol._lib, pol._h
    rows = []
    ms = (C.c_float * 128)()
    n = C.c_int()
    for phase in (0, 1):
        rc = lib.td3_profile_stages(h, rb.handle, batch, phase, ms, 128, C.byref(n))
        if rc:
            raise RuntimeError(lib.td3_last_error().decode())
        names = [lib.td3_stage_name(h, i).decode() for i in range(n.value)]
        kernels = [lib.td3_stage_kernel(h, i).decode() for i in range(n.value)]
        flops = [lib.td3_stage_flops(h, i) for i in range(n.value)]
        nbytes = [lib.td3_stage_bytes(h, i) for i in range(n.value)]
        for i in range(1, n.value):
            if names[i].endswith("_allreduce") or names[i].endswith("_join"):
                continue          # a collective (or the comm-stream join) cannot be re-launched on its own
            t = C.c_float()
            runs = []
            for _ in range(reps):
                rc = lib.td3_time_stage(h, i, max(1, iters // reps), C.byref(t))
                if rc:
                    raise RuntimeError(lib.td3_last_error().decode())
                runs.append(float(t.value))
            rows.append(dict(phase=phase, stage=names[i], kernel=kernels[i],
                             ms=float(np.median(runs)), flops=float(flops[i]), bytes=float(nbytes[i])))
    return rows


def step_flops(cfg):
    """Algorithmic FLOP of one gradient step, the mean of a critic-only and a policy step (SURVEY.md
    §8d): per sample, critic phase = target actor fwd + target twin fwd + twin fwd + twin dW + twin
    dX (no input layer), actor phase = actor fwd + dW + dX (no input layer) + Q1 fwd + dX; MACs of a
    network = sum of in*out over its Linears.  Particles add the per-particle encoder (conv1 1xD,
    conv2 1x1 over N particles: fwd E, bwd E + N*256*128 for dh1; no encoder grad for Q1 in the
    actor phase).  C2 1.753 GFLOP, C3 10.416 GFLOP, C4 1126 GFLOP."""
    B, ad = cfg["batch"], cfg["ad"]
    def mlp(inp, arch, out):
        dims = [inp] + list(arch) + [out]
        return sum(a * b for a, b in zip(dims[:-1], dims[1:])), dims[0] * dims[1]
    if cfg["kind"] == "particles":
        F, N, D = cfg["F"], cfg["N"], cfg["D"]
        Af, _ = mlp(128 + F, (500, 400, 300), ad)
        Qf, _ = mlp(128 + F + ad, (500, 400, 300), ad)
        E = N * (256 * D + 128 * 256)
        Eb = E + N * 256 * 128
        critic = (E + Af) + 4 * (E + Qf) + 4 * Qf + 2 * Eb
        actor = (E + Af) + (E + Qf) + Qf + 2 * Af + Eb
    else:
        sd = cfg["sd"]
        Af, Ain = mlp(sd, (500, 400, 300), ad)
        Qf, Qin = mlp(sd + ad, (500, 400, 200), 1)
        critic = Af + 6 * Qf + 2 * (Qf - Qin)
        actor = 3 * Af - Ain + 2 * Qf
    return 2.0 * B * (critic + actor / 2.0)


def gather_line(pol, rb, cfg, reps=5, iters=40):
    """The replay-ring sample (gather_kernel: Philox draw, record reads, batch-row writes) timed on
    its own from a captured graph (td3_time_stage stage 0), against the HBM peak.  Bytes: the
    sampled records read whole (featured: rec = pad4(2 sd + ad + 2) floats; particle rings read only
    the small fields, the encoders read the particle blocks in place) and the batch rows written
    (td3.hip input_from_ring*: featured [s | a], s, s', r, not_done; padded rows are written too)."""
    lib, h = pol._lib, pol._h
    B = cfg["batch"]
    Bp = (B + 31) // 32 * 32
    ad = cfg["ad"]
    if cfg["kind"] == "particles":
        F = cfg["F"]
        per_row = 3 * F + 2 * (2 * F + ad) + 2          # XA, XAQ, XTA, XQ_j [f | a], XTQ_j, r, nd (CDQ)
        read, written = B * per_row * 4, Bp * per_row * 4
        # what this kernel has to move: the record's small fields (f, a, f', r, nd) once each way;
        # the particle blocks are not copied (the encoders read them from the ring in place)
        algorithmic = B * 4 * (2 * F + ad + 2)
    else:
        sd = cfg["sd"]
        rec = (2 * sd + ad + 2 + 3) // 4 * 4
        read, written = B * rec * 4, Bp * (3 * sd + ad + 2) * 4
        algorithmic = B * 4 * (2 * sd + ad + 2)
    t = C.c_float()
    runs = []
    for _ in range(reps):
        rc = lib.td3_time_stage(h, 0, iters, C.byref(t))
        if rc:
            raise RuntimeError(lib.td3_last_error().decode())
        runs.append(float(t.value))
    us = float(np.median(runs)) * 1e3
    moved = read + written
    return {"kernel": "td3::gather_kernel", "bound": "hbm", "us": round(us, 3),
            "bytes_read": int(read), "bytes_written": int(written),
            "achieved": round(moved / us * 1e-3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(moved / us * 1e-3 / HBM_PEAK_GBS, 4),
            "algorithmic_bytes": int(2 * algorithmic),
            "algorithmic_TBps": round(2 * algorithmic / us * 1e-6, 3),
            "in_step": "separate launch" if cfg["kind"] == "particles" or cfg["sd"] * 2 + ad + 2 > 128
                       else "fused into F_fwd01 (kProL0G); this line is the stand-alone kernel"}


def kernel_families(rows):
    """Stage rows of one odd + one even step grouped by the HIP kernel they launch."""
    fam = {}
    for r in rows:
        f = fam.setdefault(r["kernel"], {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
        f["ms"] += r["ms"]
        f["flops"] += r["flops"]
        f["bytes"] += r.get("bytes", 0.0)
        f["launches"] += 1
    return fam


def dominant_kernel(rows):
    fam = kernel_families(rows)
    return max((k for k in fam if k != "rccl"), key=lambda k: fam[k]["ms"])


def probe_kernel(pol, rb, batch, kernel, steps):
    """The kernel's in-step device time: `steps` production steps (after the timed region) with HIP
    events around each of its launches on the step stream (td3_probe_kernel)."""
    lib, h = pol._lib, pol._h
    ms, n = C.c_float(), C.c_int()
    if lib.td3_probe_kernel(h, rb.handle, batch, kernel.encode(), steps, C.byref(ms), C.byref(n)):
        raise RuntimeError(lib.td3_last_error().decode())
    return {"steps": steps, "launches": n.value, "ms_total": float(ms.value)}


def roofline_from_stages(rows, pmc, probe=None):
    """Dominant kernel over one odd + one even step; achieved = algorithmic FLOP per launch / its
    mean launch time in back-to-back stage replays (HIP events, handle stream: within a few % of
    the rocprofv3 average of the same bench command).  `probe` adds the in-step figure: HIP events
    around each launch inside production steps, which also counts the event records and the
    launch's dispatch behind the previous stage (an upper bound on the kernel's duration)."""
    fam = kernel_families(rows)
    dom = dominant_kernel(rows)
    f = fam[dom]
    per_launch_flops = f["flops"] / f["launches"]
    per_launch_bytes = f["bytes"] / f["launches"]
    per_launch_s = f["ms"] / f["launches"] * 1e-3
    # t_roof = max(FLOP / 157.3 TFLOP/s, algorithmic bytes / 8 TB/s); the kernel's bound
    # is the side that sets t_roof, and achieved / peak / unit are that side's
    t_mfma = per_launch_flops / (FP32_PEAK_TFLOPS * 1e12)
    t_hbm = per_launch_bytes / (HBM_PEAK_GBS * 1e9)
    traffic = None
    if pmc and dom in pmc.get("kernels", {}):
        traffic = pmc["kernels"][dom].get("hbm_bytes_per_launch")
    if t_hbm > t_mfma:
        achieved = per_launch_bytes / per_launch_s / 1e9
        out = {"kernel": dom, "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
               "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4)}
    else:
        achieved = per_launch_flops / per_launch_s / 1e12 if f["flops"] > 0 else 0.0
        out = {"kernel": dom, "bound": "mfma", "achieved": round(achieved, 3), "peak": FP32_PEAK_TFLOPS,
               "unit": "TFLOP/s", "frac": round(achieved / FP32_PEAK_TFLOPS, 4)}
    out.update({"traffic": traffic, "launches_per_2_steps": f["launches"],
                "avg_launch_us": round(per_launch_s * 1e6, 3),
                "flops_per_launch": per_launch_flops, "algorithmic_bytes_per_launch": per_launch_bytes,
                "t_roof_us": {"mfma": round(t_mfma * 1e6, 3), "hbm": round(t_hbm * 1e6, 3)},
                "roofline_frac": round(max(t_mfma, t_hbm) / per_launch_s, 4),
                "timing": "back-to-back replays of the stage (td3_time_stage, HIP events on the handle stream)"})
    if dom.startswith("td3::dwsk_kernel"):
        out["stage_kernels"] = [dom, "td3::dwsk_combine_kernel"]
        out["timing"] += ("; the split-K dW stage is two launches (partial tiles, then the fixed-order "
                          "combine with Adam), timed together and charged with the stage's FLOPs")
        kern = (pmc or {}).get("kernels", {})
        if all(k in kern for k in out["stage_kernels"]):      # the stage's traffic: both launches
            out["traffic"] = sum(kern[k].get("hbm_bytes_per_launch", 0) for k in out["stage_kernels"])
    if probe and probe["launches"] > 0:
        in_step_s = probe["ms_total"] / probe["launches"] * 1e-3
        out["in_step_launch_us"] = round(in_step_s * 1e6, 3)
        out["in_step_frac"] = round(max(t_mfma, t_hbm) / in_step_s, 4)
        out["in_step_timing"] = (f"HIP events around each of the stage's {probe['launches']} launches in "
                                 f"{probe['steps']} production steps right after the timed region "
                                 "(td3_probe_kernel); includes the event records and the dispatch gap")
    return out, fam


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, seconds=12.0):
    """The reference's CPU path restated in torch (oracle/td3_torch_cpu.py: F.linear / F.layer_norm
    forward, autograd, torch.optim.Adam, pinned to the reference's goldens by
    tests/test_torch_cpu_restatement.py) on this host's cores: same shapes and batch as the GPU
    line.  Threads: every CPU this process may run on (os.sched_getaffinity), capped by
    OMP_NUM_THREADS when set (the GPU box gives a job 16 CPUs of a larger machine)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen
    from oracle import td3_oracle as orc
    from oracle.td3_torch_cpu import FeaturedTorch, ParticleTorch
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        cores = min(cores, int(os.environ["OMP_NUM_THREADS"]))
    prev = torch.get_num_threads()
    torch.set_num_threads(cores)
    B, ad = cfg["batch"], cfg["ad"]
    rs = np.random.RandomState(0)
    rows = 2048 if cfg["kind"] == "particles" else 20000
    if cfg["kind"] == "particles":
        F, N, D = cfg["F"], cfg["N"], cfg["D"]
        a0 = gen.init_params(gen.particle_actor_shapes(F, D, ad, "layer"), 1)
        c0 = gen.init_params(gen.particle_critic_shapes(F, D, ad, "layer"), 2)
        L = ParticleTorch(a0, c0, norm="layer")
        buf = orc.ParticleBuffer(F, N, D, ad, rows)
        buf.state_features[:] = rs.standard_normal(buf.state_features.shape)
        buf.state_particles[:] = rs.standard_normal(buf.state_particles.shape)
        buf.next_state_features[:] = rs.standard_normal(buf.next_state_features.shape)
        buf.next_state_particles[:] = rs.standard_normal(buf.next_state_particles.shape)
        what = "particles F7 N350 D9 A3"
    else:
        sd = cfg["sd"]
        a0 = gen.init_params(gen.featured_actor_shapes(sd, ad, "layer"), 1)
        c0 = gen.init_params(gen.featured_critic_shapes(sd, ad, "layer"), 2)
        L = FeaturedTorch(a0, c0, max_action=cfg["ma"], norm="layer")
        buf = orc.FeaturedBuffer(sd, ad, rows)
        buf.state[:] = rs.standard_normal((rows, sd))
        buf.next_state[:] = rs.standard_normal((rows, sd))
        what = f"state {sd} action {ad}"
    buf.action[:] = rs.uniform(-cfg["ma"], cfg["ma"], buf.action.shape)
    buf.reward[:] = rs.standard_normal((rows, 1))
    buf.not_done[:] = (rs.uniform(size=(rows, 1)) > 0.01)
    buf.size = rows
    if cfg["kind"] != "particles":          # one untimed step (allocator / thread-pool warm-up)
        L.train_step(buf.gather(rs.randint(0, rows, B)), rs.standard_normal((B, ad)).astype(np.float32))
    steps = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds or steps < 2:
        idx = rs.randint(0, rows, B)
        noise = rs.standard_normal((B, ad)).astype(np.float32)
        L.train_step(buf.gather(idx), noise)
        steps += 1
    dt = time.perf_counter() - t0
    torch.set_num_threads(prev)
    return {"value": round(steps / dt, 4), "unit": "grad-steps/s", "cores": int(cores),
            "kind": "port", "cpu_model": _cpu_model(),
            "implementation": "oracle/td3_torch_cpu.py (torch-CPU restatement of TD3.train, "
                              f"torch {torch.__version__}, {cores} threads)",
            "sample": f"{steps} torch-CPU train steps ({what}, B={B}, norm=layer, warm) in {dt:.1f} s"}


def cpu_baseline_child(config, timeout_s=300):
    """cpu_baseline in a child process (``--cpu-baseline-only``) that has not initialised the GPU and
    runs on every CPU the job may use: in the bench process the torch-CPU threads would share the
    host with the HIP runtime's threads and inherit the launching thread's pinning."""
    import subprocess
    q = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--config", config],
                       capture_output=True, text=True, timeout=timeout_s)
    if q.returncode != 0:
        raise RuntimeError(f"cpu baseline child failed ({q.returncode}): {q.stderr.strip()[-400:]}")
    return json.loads(q.stdout.strip().splitlines()[-1])


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs of this node, one rank each (default 1; under an external launcher "
                         "it must equal WORLD_SIZE)")
    ap.add_argument("--steps", type=int, default=2000, help="timed steps (one timed region)")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--runs", type=int, default=None,
                    help="repeat the timed region of --steps steps; value = the median run "
                         "(SURVEY.md §8d).  Default 1, with --full 5")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: 5 timed runs, the "
                         "per-stage roofline, the gather line and the torch-CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the learner's state (parameters, targets, Adam "
                         "moments: what the last timed step left its caller) as DIR/<name>.npy")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="halfcheetah")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dp-self", action="store_true",
                    help="diagnostic: run the data-parallel stage lists (grad-only dW, RCCL all-reduce, "
                         "flat Adam) on a one-rank communicator, to price the DP path without peers")
    ap.add_argument("--no-roofline", action="store_true",
                    help="with --full: skip the stage table, the roofline and the gather line")
    ap.add_argument("--launch", choices=["auto", "graph", "eager"], default="auto",
                    help="step launch mode: hipGraph replay, direct launches, or auto (replay while the "
                         "GPU has caught up with the host, direct launches while steps are queued)")
    ap.add_argument("--eager", action="store_true", help="same as --launch eager")
    ap.add_argument("--norm", choices=["layer", "none", "weight_normalization"], default="layer",
                    help="network normalisation (SURVEY §8d measures norm=layer; featured configs only)")
    args = ap.parse_args(argv)
    if args.runs is None:
        args.runs = 5 if args.full else 1
    return args


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_workers(argv, n, worker=None, grace_s=20.0):
    """``bench.py --gpus N`` without an external launcher: start N rank processes of this script
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, rendezvous on 127.0.0.1)
    before this process touches the GPU -- it never imports torch -- and forward rank 0's
    stdout (the one JSON line).  Other ranks' stdout goes to stderr.  When a rank fails, the
    others are terminated (they would wait in a collective) and the launcher returns that rank's
    exit status; 0 only when every rank succeeded.  ``worker`` replaces the child command
    (CPU tests)."""
    import signal
    import subprocess
    import threading
    port = _free_port()
    cmd = list(worker) if worker is not None else [sys.executable, os.path.abspath(__file__), *argv]
    procs, out0 = [], []
    for rank in range(n):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL peer buffers)
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if rank == 0 else sys.stderr,
                                      start_new_session=True))
    reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    failed = None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad and failed is None:
            failed = bad[0]
            print(f"bench: rank {failed[0]} exited with {failed[1]}; stopping the other ranks",
                  file=sys.stderr, flush=True)
            for p in procs:
                if p.poll() is None:
                    os.killpg(p.pid, signal.SIGTERM)
            deadline = time.time() + grace_s
            for p in procs:
                try:
                    p.wait(timeout=max(0.1, deadline - time.time()))
                except subprocess.TimeoutExpired:
                    os.killpg(p.pid, signal.SIGKILL)
                    p.wait()
            break
        if all(c is not None for c in codes):
            break
        time.sleep(0.05)
    reader.join(timeout=10)
    text = out0[0].decode(errors="replace") if out0 and out0[0] else ""
    if text:
        sys.stdout.write(text)
        sys.stdout.flush()
    if failed is not None:
        return failed[1] if failed[1] > 0 else 1
    return 0


def main(argv=None):
    args = parse_args(argv)
    if args.cpu_baseline_only:                    # cpu_baseline_child's process: no GPU
        print(json.dumps(cpu_baseline(CONFIGS[args.config])), flush=True)
        return 0
    if "WORLD_SIZE" not in os.environ:
        if (args.gpus or 1) > 1:
            return launch_workers(sys.argv[1:] if argv is None else list(argv), args.gpus)
        args.gpus = 1
    else:
        world = int(os.environ["WORLD_SIZE"])
        if args.gpus is None:
            args.gpus = world
        if args.gpus != world:
            print(f"bench: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks",
                  file=sys.stderr)
            return 2
    run_rank(args)
    return 0


def run_rank(args):
    cfg = CONFIGS[args.config]
    if args.eager:
        args.launch = "eager"
    use_graph = {"auto": "auto", "graph": True, "eager": False}[args.launch]
    B, REPLAY_ROWS = cfg["batch"], cfg["replay"]
    prev_cpus, host_pin = pin_host_thread(int(os.environ.get("LOCAL_RANK", "0")))

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist = None
    if world > 1 or args.dp_self:
        import torch.distributed as dist
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    from td3_amd import _lib  # noqa: F401

    torch.manual_seed(1000)                         # same init on every rank
    if cfg["kind"] == "particles":
        from td3_amd.TD3_particles import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as RB
        obs = (Box((cfg["F"],)), Box((cfg["N"], cfg["D"])))
        pol = TD3(obs, Box((cfg["ad"],)), norm="layer", device=local, seed=17 + rank,
                  use_graph=use_graph)
    else:
        from td3_amd.TD3_featured import TD3
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as RB
        obs = Box((cfg["sd"],))
        pol = TD3(obs, Box((cfg["ad"],)), max_action=cfg["ma"], device=local, seed=17 + rank,
                  use_graph=use_graph, norm=None if args.norm == "none" else args.norm)
    rb = RB(obs, Box((cfg["ad"],)), max_size=REPLAY_ROWS, device=local, seed=101 + rank)
    rb.fill_synthetic(REPLAY_ROWS, cfg["ma"], seed=7 + rank)
    if world > 1 or args.dp_self:
        from td3_amd.data_parallel import init_rccl
        init_rccl(pol, dist)

    def barrier_sync():
        pol.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # the timed runs hold Python's cyclic garbage collector (a collection inside a 2 ms driver-form
    # run is a host stall the GPU waits behind); BENCH_GC=1 keeps it on.  The collection runs before
    # the warm-up steps: between them and the timed runs its tens of ms of GPU idle let the GPU's
    # clocks fall back (profiles/r06_gpu_ramp.txt), which the warm-up would then not have covered
    import gc
    hold_gc = os.environ.get("BENCH_GC", "0") != "1"
    gc_after = os.environ.get("BENCH_GC_AT", "before") == "after"     # round-5 order, for A/B runs
    if hold_gc and not gc_after:
        gc.collect()
        gc.disable()
    for _ in range(args.warmup):
        pol.train(rb, B)
    if hold_gc and gc_after:
        gc.collect()
        gc.disable()
    runs = []
    for _ in range(max(1, args.runs)):
        barrier_sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pol.train(rb, B)
        pol.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        dt = time.perf_counter() - t0
        if dist is not None:                       # the slowest rank's clock
            tt = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        runs.append(dt)
    if hold_gc:
        gc.enable()
    dt = float(np.median(runs))
    if args.dump_outputs:              # before anything below takes further steps
        dump_outputs(pol, args.dump_outputs, rank)

    rows, fam, roof, gat = None, None, None, None
    if args.full and not args.no_roofline:           # every rank runs it: profiled steps contain collectives
        rows = stage_table(pol, rb, B, iters=50 if cfg["kind"] != "particles" else 3,
                           reps=5 if cfg["kind"] != "particles" else 1)
        gat = gather_line(pol, rb, cfg)
        try:
            probe = probe_kernel(pol, rb, B, dominant_kernel(rows), 200 if cfg["kind"] != "particles" else 4)
        except RuntimeError as e:              # the in-step figure is a supplement: keep the line
            print(f"bench: in-step probe skipped: {e}", file=sys.stderr)
            probe = None
        if rank == 0:
            pmc = None
            pmc_path = os.path.join(ROOT, "profiles", PMC_FILES.get(args.config, ""))
            if os.path.isfile(pmc_path) and args.norm == "layer":
                with open(pmc_path) as f:
                    pmc = json.load(f)
            roof, fam = roofline_from_stages(rows, pmc, probe)
            if roof.get("traffic") is not None:
                roof["traffic_source"] = (f"profiles/{PMC_FILES[args.config]}: rocprofv3 --pmc FETCH_SIZE / "
                                          "WRITE_SIZE of this kernel in a separate profiling run of this "
                                          "configuration (committed; not measured inside this run)")

    cpu = None
    if prev_cpus is not None:            # the CPU baseline gets every CPU the job may use
        os.sched_setaffinity(0, prev_cpus)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline_child(args.config)

    if rank == 0:
        print(json.dumps(result_line(args, cfg, world, dt, runs, roof, gat, rows, cpu, host_pin)), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def dump_outputs(pol, path, rank=0):
    """What the last timed step left its caller, as ``path/<name>.npy`` (float32, flat, in
    ``state_dict()`` order): the four networks and the Adam moments of both optimizers, a few MB for
    every config.  ``train`` returns nothing; this state is its result.  Every rank makes the calls
    (a data-parallel optimizer ``state_dict()`` gathers its sharded moments), rank 0 writes.  The
    run's inputs are fixed by its arguments (``torch.manual_seed(1000)``, the learner / ring / fill
    seeds in ``run_rank``), so two builds given the same arguments can be compared array by array."""
    def flat(arrays):
        return np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in arrays])
    out = {name: flat(getattr(pol, name).numpy_dict().values())
           for name in ("actor", "critic", "actor_target", "critic_target")}
    for name in ("actor", "critic"):
        state = getattr(pol, name + "_optimizer").state_dict()["state"]
        for key in ("exp_avg", "exp_avg_sq"):
            out[f"{name}_adam_{key}"] = flat([state[i][key].numpy() for i in sorted(state)])
    if rank == 0:
        os.makedirs(path, exist_ok=True)
        for name, a in out.items():
            np.save(os.path.join(path, name + ".npy"), a)


def result_line(args, cfg, world, dt, runs, roof=None, gat=None, rows=None, cpu=None, host_pin=None):
    """The driver's JSON line.  ``value`` = optimizer steps/s of the job: every rank takes the same
    step at once (the replicas all-reduce one global batch of B·world rows per step), so this is
    the TD3 gradient-step rate (TD3_featured.py:123-171: one ``train`` = one step) at the global
    batch in ``config``; the rows consumed are ``samples_per_s``.  ``dt`` is the time of the timed
    run of ``args.steps`` steps, the median one when the region was repeated (the slowest rank's
    clock in each)."""
    B = cfg["batch"]
    steps_s = args.steps / dt
    metric = "TD3 gradient-steps/sec @ batch 256, HalfCheetah-v4, 1/2/4/8 GPU"
    if args.config != "halfcheetah":
        metric = f"TD3 gradient-steps/sec @ batch {B}, {args.config}, 1/2/4/8 GPU"
    out = {
        "metric": metric,
        "value": round(steps_s, 3),
        "unit": "grad-steps/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 5),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic (replay ring pre-filled on device: states / particles ~ N(0,1), "
                "a ~ U(-max_action, max_action), r ~ N(0,1), not_done ~ Bernoulli(0.99); "
                "torch-default random init)",
        "config": {"workload": cfg["workload"],
                   "global_batch": B * world, "per_gpu_batch": B, "replay_per_gpu": cfg["replay"],
                   "parallelism": f"dp{world}" if world > 1 else ("dp1-self" if args.dp_self else "single"),
                   "launch": args.launch, "norm": args.norm},
        "samples_per_s": round(steps_s * B * world, 1),
        # the same rate counted per rank-gradient: every rank computes one batch-B gradient per step
        # (N-GPU lines stay comparable with the per-GPU "@ batch 256" label)
        "batch_gradients_per_s": round(steps_s * world, 3),
        "runs": [round(args.steps / r, 3) for r in runs],
        "value_is": (f"median of {len(runs)} timed runs of {args.steps} steps each" if len(runs) > 1
                     else f"one timed run of {args.steps} steps") + "; one step = one "
                    f"optimizer step of every rank on a global batch of {B}x{world} rows",
    }
    if roof is not None:
        flops = step_flops(cfg)
        roof["step_flops"] = flops
        roof["step_frac"] = round(flops / (dt / args.steps) / (FP32_PEAK_TFLOPS * 1e12), 4)
        out["roofline"] = roof
    if gat is not None:
        out["gather"] = gat
    if rows is not None:
        out["stage_us"] = {f"{r['phase']}:{r['stage']}": round(r["ms"] * 1e3, 2) for r in rows}
    if cpu is not None:
        out["cpu_baseline"] = cpu
    if host_pin is not None:
        out["host_pin"] = host_pin
    return out


if __name__ == "__main__":
    sys.exit(main())
