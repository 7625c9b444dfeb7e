"""bench.py's accounting on CPU (no GPU): the roofline object of the dominant kernel, the in-step
probe fields, the split-K dW stage note, and the step FLOP model against SURVEY.md §8d."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _rows():
    # one odd + one even step: F_fwd01 twice (dominant), a row kernel, the dW stage
    return [
        dict(phase=0, stage="F_fwd01", kernel="td3::gemm_kernel<0, 2, 5>", ms=0.016, flops=3.5e8),
        dict(phase=0, stage="heads", kernel="td3::row_kernel2<0, 7, true>", ms=0.005, flops=0.0),
        dict(phase=1, stage="F_fwd01", kernel="td3::gemm_kernel<0, 2, 5>", ms=0.017, flops=4.0e8),
        dict(phase=1, stage="C_dw", kernel="td3::dw_kernel<true>", ms=0.011, flops=3.0e8),
    ]


def test_roofline_dominant_kernel_and_fraction():
    roof, fam = bench.roofline_from_stages(_rows(), None)
    assert roof["kernel"] == "td3::gemm_kernel<0, 2, 5>"
    assert roof["launches_per_2_steps"] == 2
    assert roof["avg_launch_us"] == pytest.approx(16.5)
    assert roof["flops_per_launch"] == pytest.approx(3.75e8)
    assert roof["achieved"] == pytest.approx(3.75e8 / 16.5e-6 / 1e12, rel=1e-3)
    assert roof["frac"] == pytest.approx(roof["achieved"] / bench.FP32_PEAK_TFLOPS, abs=1e-4)
    assert roof["traffic"] is None and "stage_kernels" not in roof
    assert set(fam) == {"td3::gemm_kernel<0, 2, 5>", "td3::row_kernel2<0, 7, true>", "td3::dw_kernel<true>"}


def test_roofline_in_step_probe_fields_and_traffic():
    pmc = {"kernels": {"td3::gemm_kernel<0, 2, 5>": {"hbm_bytes_per_launch": 9491019}}}
    probe = {"steps": 200, "launches": 200, "ms_total": 4.0}
    roof, _ = bench.roofline_from_stages(_rows(), pmc, probe)
    assert roof["traffic"] == 9491019
    assert roof["in_step_launch_us"] == pytest.approx(20.0)
    assert roof["in_step_frac"] == pytest.approx(3.75e8 / 20e-6 / 1e12 / bench.FP32_PEAK_TFLOPS, abs=1e-4)
    assert roof["avg_launch_us"] == pytest.approx(16.5)          # achieved stays on the replays


def test_split_k_dw_stage_is_named_as_two_launches():
    rows = [dict(phase=0, stage="C_dw", kernel="td3::dwsk_kernel<true, false>", ms=0.044, flops=1.95e9)]
    roof, _ = bench.roofline_from_stages(rows, None)
    assert roof["stage_kernels"] == ["td3::dwsk_kernel<true, false>", "td3::dwsk_combine_kernel"]


def test_roofline_bound_is_the_larger_of_flop_and_byte_time():
    """t_roof = max(FLOP / 157.3 TFLOP/s, bytes / 8 TB/s).  A dW stage whose Adam state
    outweighs its FLOPs (C2 C_dw: ~0.3 GFLOP, ~20 MB) is HBM-bound, and its achieved figure is
    GB/s against the 8 TB/s peak; a GEMM stage of the same rows stays MFMA-bound."""
    rows = [dict(phase=0, stage="C_dw", kernel="td3::dw_kernel<true>", ms=0.012, flops=2.985e8, bytes=2.0e7),
            dict(phase=0, stage="heads", kernel="td3::row_kernel2<0, 7, true>", ms=0.005, flops=0.0)]
    roof, _ = bench.roofline_from_stages(rows, None)
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == bench.HBM_PEAK_GBS
    assert roof["achieved"] == pytest.approx(2.0e7 / 12e-6 / 1e9, rel=1e-3)
    assert roof["frac"] == pytest.approx(roof["achieved"] / bench.HBM_PEAK_GBS, abs=1e-4)
    assert roof["t_roof_us"]["hbm"] == pytest.approx(2.5) and roof["roofline_frac"] == pytest.approx(2.5 / 12, abs=1e-3)
    rows[0]["bytes"] = 2.0e6
    roof, _ = bench.roofline_from_stages(rows, None)
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s"


def test_rccl_stage_is_never_the_dominant_kernel():
    rows = _rows() + [dict(phase=0, stage="C_allreduce", kernel="rccl", ms=1.0, flops=0.0)]
    assert bench.dominant_kernel(rows) == "td3::gemm_kernel<0, 2, 5>"


@pytest.mark.parametrize("name,gflop", [("halfcheetah", 1.753), ("humanoid", 10.416), ("particles", 1126.3)])
def test_step_flops_match_survey(name, gflop):
    assert bench.step_flops(bench.CONFIGS[name]) / 1e9 == pytest.approx(gflop, rel=1e-3)


def test_pin_host_thread_modes(monkeypatch):
    """bench.pin_host_thread: off, n CPUs offset by the local rank, restorable (no GPU here: the
    bus query finds no device and the pool is the allowed set)."""
    import os
    if not hasattr(os, "sched_setaffinity"):
        return
    before = os.sched_getaffinity(0)
    try:
        monkeypatch.setenv("BENCH_PIN", "0")
        assert bench.pin_host_thread(0) == (None, None)
        assert os.sched_getaffinity(0) == before
        monkeypatch.setenv("BENCH_PIN", "1")
        prev, info = bench.pin_host_thread(1)
        assert set(prev) == before and len(os.sched_getaffinity(0)) == 1
        pool = sorted(before)
        assert os.sched_getaffinity(0) == {pool[1 % len(pool)]} and info["cpus"] == [pool[1 % len(pool)]]
        os.sched_setaffinity(0, prev)
        monkeypatch.setenv("BENCH_PIN", "node")
        prev, info = bench.pin_host_thread(0)
        assert os.sched_getaffinity(0) == before
    finally:
        os.sched_setaffinity(0, before)
    assert bench._parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}


def test_plain_run_times_the_steps_once_and_full_repeats_them():
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (plain.full, plain.runs, plain.dump_outputs) == (False, 1, None)
    assert bench.parse_args(["--full"]).runs == 5
    assert bench.parse_args(["--runs", "3"]).runs == 3
    line = bench.result_line(plain, bench.CONFIGS["halfcheetah"], 1, 0.002, [0.002])
    assert line["steps"] == 20 and line["ms_per_step"] == pytest.approx(0.1)
    assert line["value"] == pytest.approx(1e4) and line["runs"] == [line["value"]]
    for k in ("roofline", "gather", "stage_us", "cpu_baseline"):
        assert k not in line


def test_dump_outputs_writes_float32_arrays_on_rank0_only(tmp_path):
    """bench.dump_outputs on a stand-in learner: the four networks and the Adam moments, flat, in
    state_dict order; every rank makes the calls, only rank 0 writes."""
    import numpy as np
    import torch

    class View:
        def __init__(self, base):
            self.base = base

        def numpy_dict(self):
            return {"w": np.full((2, 3), self.base, np.float64), "b": np.arange(2, dtype=np.float32)}

    class Opt:
        def state_dict(self):
            return {"state": {i: {"step": torch.tensor(1.0), "exp_avg": torch.full((2,), float(i)),
                                  "exp_avg_sq": torch.full((3,), 10.0 + i)} for i in (1, 0)}}

    class Pol:
        actor, critic, actor_target, critic_target = View(1), View(2), View(3), View(4)
        actor_optimizer = critic_optimizer = Opt()

    bench.dump_outputs(Pol(), str(tmp_path / "r1"), rank=1)
    assert not (tmp_path / "r1").exists()
    bench.dump_outputs(Pol(), str(tmp_path / "r0"), rank=0)
    names = ["actor", "critic", "actor_target", "critic_target", "actor_adam_exp_avg",
             "actor_adam_exp_avg_sq", "critic_adam_exp_avg", "critic_adam_exp_avg_sq"]
    assert sorted(os.listdir(tmp_path / "r0")) == sorted(n + ".npy" for n in names)
    got = {n: np.load(tmp_path / "r0" / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    assert got["critic"].tolist() == [2.0] * 6 + [0.0, 1.0]
    assert got["actor_adam_exp_avg"].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert got["critic_adam_exp_avg_sq"].tolist() == [10.0] * 3 + [11.0] * 3
