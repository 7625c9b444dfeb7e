"""Cost of the dataset normalisation (include/td3.h "dataset normalisation": rb_state_moments,
rb_normalize_states) at three shapes: the HalfCheetah dims (C2) with 10^6 rows, the Humanoid dims (C3) with
10^6 rows and bench.py's particle dims with 10^5 rows, rings from fill_synthetic.

Reports, as one JSON line and a file (default profiles/normalize.json), per shape:
  (a) device microseconds of ``state_moments`` (its two launches together: the sweep and the merge of the
      chunk partials) and of ``normalize_states`` (one launch), from events around the call queued behind a
      few ms of other device work, the median of ``--reps`` (each rep of the normalise follows a
      ``fill_synthetic(0)``, which only clears the ring's ``normalized`` flag);
  (b) the bytes each moves, counted as the 128-byte lines of the ring it touches -- moments: once, the
      whole ring where the sweep stages whole records, else the lines of the state columns; normalise: the
      lines of the state and next-state columns, read and written -- and the TB/s that makes, next to the
      in-order HBM sweep of the part, 6.0-6.3 TB/s;
  (c) the wall time of the host path the two calls replace: ``rb_read_records``, the same expression in
      numpy (fp64, blocks of rows), ``rb_write_records``.
With ``--parent DIR`` (a built checkout of the parent commit) it also runs ``bench.py --gpus 1`` of this
tree and of that one as child processes, in ABBA order, ``--bench-runs`` times each, for C2 and C3: the
feature changes no step code, and the ranges of the two builds say so.
No pass/fail: the numbers are reported.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import gc
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_mixed import bench_pair  # noqa: E402
from bench_per import Box, write_result  # noqa: E402

SHAPES = {"halfcheetah": ("C2", 1_000_000), "humanoid": ("C3", 1_000_000), "particles": ("particles", 100_000)}
HBM_SWEEP_TBS = (6.0, 6.3)


def touched_lines(rec, ranges, rows):
    """128-byte lines of ``rows`` records of ``rec`` floats that hold a float of the column ``ranges``
    ([lo, hi) pairs): counted over one period of the layout (32 records are a whole number of lines)."""
    lines = set()
    for r in range(32):
        for lo, hi in ranges:
            b0, b1 = (r * rec + lo) * 4, (r * rec + hi) * 4 - 1
            lines.update(range(b0 // 128, b1 // 128 + 1))
    return len(lines) * rows / 32.0


def layout(rb):
    """(state width, record floats, column of the next state) of a ring of either kind."""
    dims = rb._dims()
    sd = dims[0]
    o_s2 = sum(w for _, w, _ in rb._fields[:rb.store_np.index("next_state" if "next_state" in rb.store_np
                                                              else "next_state_features")])
    return sd, rb.record_floats, o_s2


def device_us(call, reps, before=None):
    import torch
    filler = torch.randn(4096, 4096, device="cuda")
    out = []
    for _ in range(reps + 2):                               # two warm calls: code objects, scratch
        if before:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(4):
            filler @ filler
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    out = out[2:]
    return {"median": round(float(np.median(out)), 2), "runs": [round(x, 2) for x in out]}


def host_path(rb, stats, block=65536):
    """Wall seconds of read-back, numpy normalisation and write-back of the whole ring."""
    from td3_amd import _lib
    sd, rec, o_s2 = layout(rb)
    t0 = time.perf_counter()
    rows = rb._records()
    t1 = time.perf_counter()
    n = rb.size
    x = rows[:n, :sd].astype(np.float64)
    mean = x.mean(axis=0)
    m2 = ((x - mean) ** 2).sum(axis=0)
    den = np.sqrt(m2 / n + stats.eps)
    del x
    for lo in range(0, n, block):
        for o in (0, o_s2):
            v = rows[lo:lo + block, o:o + sd]
            v[...] = np.clip((v.astype(np.float64) - mean) / den, -stats.obs_clip, stats.obs_clip)
    t2 = time.perf_counter()
    _lib.check(rb._lib.rb_write_records(rb.handle, 0, rb.max_size, _lib.fptr(rows), rb.ptr % rb.max_size, n),
               "rb_write_records")
    t3 = time.perf_counter()
    return {"read_s": round(t1 - t0, 3), "numpy_s": round(t2 - t1, 3), "write_s": round(t3 - t2, 3),
            "total_s": round(t3 - t0, 3)}


def measure(name, args):
    import torch
    from bench import CONFIGS
    cfg = CONFIGS[name]
    shape, rows = SHAPES[name]
    rows = args.rows or rows
    if cfg["kind"] == "particles":
        from td3_amd.my_replay_buffer import ReplayBuffer_particles as RB
        rb = RB((Box((cfg["F"],)), Box((cfg["N"], cfg["D"]))), Box((cfg["ad"],)), max_size=rows, device=0, seed=1)
    else:
        from td3_amd.my_replay_buffer import ReplayBuffer_featured as RB
        rb = RB(Box((cfg["sd"],)), Box((cfg["ad"],)), max_size=rows, device=0, seed=1)
    rb.fill_synthetic(rows, cfg["ma"], seed=7)
    torch.cuda.synchronize()
    sd, rec, o_s2 = layout(rb)
    stats = rb.state_moments()
    mom = device_us(lambda: rb.state_moments(stats), args.reps)
    app = device_us(lambda: rb.normalize_states(stats), args.reps, before=lambda: rb.fill_synthetic(0))
    whole = sd <= 256 and rec - (sd + 3) // 4 * 4 < 32      # ringnorm.hip: whole records are staged
    mom_bytes = rows * rec * 4.0 if whole else 128.0 * touched_lines(rec, [(0, sd)], rows)
    app_bytes = 2 * 128.0 * touched_lines(rec, [(0, sd), (o_s2, o_s2 + sd)], rows)
    res = {"shape": shape, "rows": rows, "state_dim": sd, "record_floats": rec, "ring_bytes": rows * rec * 4,
           "moments": {"launches": 2, "device_us": mom, "bytes": mom_bytes, "counted": "whole ring once" if whole
                       else "the lines of the state columns, once",
                       "tb_per_s": round(mom_bytes / (mom["median"] * 1e-6) / 1e12, 3)},
           "normalize": {"launches": 1, "device_us": app, "bytes": app_bytes,
                         "counted": "the lines of the state and next-state columns, read + written",
                         "tb_per_s": round(app_bytes / (app["median"] * 1e-6) / 1e12, 3)},
           "hbm_sweep_tb_per_s": list(HBM_SWEEP_TBS)}
    if not args.no_host:
        rb.fill_synthetic(0)
        res["host_path"] = host_path(rb, stats)
    del rb, stats
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=(*SHAPES, "all"), default="all")
    ap.add_argument("--rows", type=int, default=None, help="default 10^6 / 10^6 / 10^5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host path (read, numpy, write)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py A/B")
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize.json"))
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_normalize: no GPU (torch.cuda.is_available() is False); nothing is measured without one")
    res = {"config": dict(reps=args.reps)}
    if args.parent:                       # first: child processes, while this one has not opened the GPU
        res["bench_py"] = {c: bench_pair(args, c) for c in ("halfcheetah", "humanoid")}
    res["device"] = torch.cuda.get_device_name(0)
    for name in (tuple(SHAPES) if args.config == "all" else (args.config,)):
        res[name] = measure(name, args)
    return write_result(res, args.out)


if __name__ == "__main__":
    sys.exit(main())
