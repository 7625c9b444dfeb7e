"""The optimizer tail the planner emits behind each group's dW stage (stages.hip add_dw_stage, the
data-parallel schedules of dp.hip), pinned as literal (stage name, kernel) lists: from a group's
first `<tag>_dw*` stage to the last stage of that group's tail, critic-only step (phase 0) and policy
step (phase 1), for a learner without a communicator ("fused") and the same learner on a one-rank
RCCL communicator ("dp").  The shapes are the smallest at which each branch exists: B = 64 takes
dw_kernel, B = 512 is the smallest batch with 64 x 64 tiles and the split-K dW.

The lists were written down from this file's own dump (`python tests/test_gpu_dw_schedules.py`) of the
commit before the dW stage builder was split; a change that moves one of them is a change of schedule
and says so by editing the list."""
import ctypes as C
import os
import pprint

import pytest

from helpers import featured_setup_dims, particle_setup_dims, stage_kernels

pytestmark = pytest.mark.gpu

HALFCHEETAH, HUMANOID = (17, 6), (376, 17)
KNOBS = ("TD3_DP_BUCKETS", "TD3_DP_SHARD", "TD3_W4", "TD3_DWSK_T")       # read at every plan build

CASES = {
    # name: (kind, dims, B, norm, environment)
    "small_batch": ("featured", HALFCHEETAH, 64, "layer", {}),
    "split_k": ("featured", HUMANOID, 512, "layer", {}),
    "buckets": ("featured", HUMANOID, 512, "layer", {"TD3_DP_BUCKETS": "2"}),
    "sharded_b64": ("featured", HALFCHEETAH, 64, "layer", {"TD3_DP_SHARD": "2"}),
    "sharded_b512": ("featured", HUMANOID, 512, "layer", {"TD3_DP_SHARD": "2"}),
    "sharded_no_images_b64": ("featured", HALFCHEETAH, 64, "layer", {"TD3_DP_SHARD": "2", "TD3_W4": "0"}),
    "sharded_no_images_b512": ("featured", HUMANOID, 512, "layer", {"TD3_DP_SHARD": "2", "TD3_W4": "0"}),
    "weight_normalization": ("featured", HALFCHEETAH, 64, "weight_normalization", {}),
    "particles": ("particles", (7, 16, 9, 3), 32, "layer", {}),
}

_setups = {}


def _setup(kind, dims, B, norm):
    key = (kind, dims, B, norm)
    if key not in _setups:
        _setups[key] = (featured_setup_dims(*dims, norm=norm, B=B) if kind == "featured"
                        else particle_setup_dims(*dims, norm=norm, B=B))
    return _setups[key]


def _group_tails(stages):
    """The (name, kernel) pairs from each group's first `<tag>_dw*` stage through the run of `<tag>_*`
    stages behind it, critic then actor."""
    out = []
    for tag in ("C_", "A_"):
        first = next((i for i, (n, _) in enumerate(stages) if n.startswith(tag + "dw")), None)
        if first is None:
            continue
        i = first
        while i < len(stages) and stages[i][0].startswith(tag):
            out.append(stages[i])
            i += 1
    return out


def plan_tails(name):
    """{(mode, phase): tails} of one case; the case's environment must be in place."""
    from td3_amd import _lib
    from test_gpu_parity import _make as make_featured
    from test_gpu_particles import _make as make_particles
    kind, dims, B, norm, _ = CASES[name]
    S = _setup(kind, dims, B, norm)
    got = {}
    for mode in ("fused", "dp"):
        pol, rb = make_featured(S) if kind == "featured" else make_particles(S)
        if mode == "dp":
            uid = (C.c_ubyte * 128)()
            _lib.check(pol._lib.td3_comm_unique_id(uid), "td3_comm_unique_id")
            _lib.check(pol._lib.td3_comm_init(pol._h, uid, 1, 0), "td3_comm_init")
        for phase in (0, 1):
            got[(mode, phase)] = _group_tails(stage_kernels(pol, rb, B, phase))
    return got


def _fused(c_dw, a_dw):
    """Without a communicator the optimizer is the dW launch's epilogue: no tail."""
    return {("fused", 0): [("C_dw", c_dw)], ("fused", 1): [("C_dw", c_dw), ("A_dw", a_dw)]}


EXPECTED = {
    "small_batch": {
        **_fused("td3::dw_kernel<true>", "td3::dw_kernel<false>"),
        ("dp", 0): [("C_dw", "td3::dw_kernel<true>"), ("C_allreduce", "rccl"), ("C_adam", "td3::adam_flat_kernel")],
        ("dp", 1): [("C_dw", "td3::dw_kernel<true>"), ("C_allreduce", "rccl"), ("C_adam", "td3::adam_flat_kernel"),
                    ("A_dw", "td3::dw_kernel<false>"), ("A_allreduce", "rccl"), ("A_adam", "td3::adam_flat_kernel")],
    },
    "split_k": {
        **_fused("td3::dwsk_kernel<true, false>", "td3::dwsk_kernel<false, false>"),
        ("dp", 0): [("C_dw", "td3::dwsk_kernel<true, false>"), ("C_allreduce", "rccl"),
                    ("C_adam", "td3::adam_flat_kernel")],
        ("dp", 1): [("C_dw", "td3::dwsk_kernel<true, false>"), ("C_allreduce", "rccl"),
                    ("C_adam", "td3::adam_flat_kernel"),
                    ("A_dw", "td3::dwsk_kernel<false, false>"), ("A_allreduce", "rccl"),
                    ("A_adam", "td3::adam_flat_kernel")],
    },
    "buckets": {
        **_fused("td3::dwsk_kernel<true, false>", "td3::dwsk_kernel<false, false>"),
        ("dp", 0): [("C_dw_0", "td3::dwsk_kernel<true, false>"), ("C_dw_1", "td3::dwsk_kernel<true, false>"),
                    ("C_0_allreduce", "rccl"), ("C_1_allreduce", "rccl"), ("C_join", "(stream join)")],
        ("dp", 1): [("C_dw_0", "td3::dwsk_kernel<true, false>"), ("C_dw_1", "td3::dwsk_kernel<true, false>"),
                    ("C_0_allreduce", "rccl"), ("C_1_allreduce", "rccl"), ("C_join", "(stream join)"),
                    ("A_dw", "td3::dwsk_kernel<false, false>"), ("A_allreduce", "rccl"),
                    ("A_adam", "td3::adam_flat_kernel")],
    },
    "sharded_b64": {
        **_fused("td3::dw_kernel<true>", "td3::dw_kernel<false>"),
        ("dp", 0): [("C_dw", "td3::dw_kernel<true>"), ("C_rs_adam_ag", "rccl"), ("C_w4", "td3::w4_pack_kernel")],
        ("dp", 1): [("C_dw", "td3::dw_kernel<true>"), ("C_rs_adam_ag", "rccl"), ("C_polyak", "td3::polyak_w4_kernel"),
                    ("A_dw", "td3::dw_kernel<false>"), ("A_rs_adam_ag", "rccl"), ("A_polyak", "td3::polyak_w4_kernel")],
    },
    "sharded_b512": {
        **_fused("td3::dwsk_kernel<true, false>", "td3::dwsk_kernel<false, false>"),
        ("dp", 0): [("C_dw", "td3::dwsk_kernel<true, false>"), ("C_rs_adam_ag", "rccl"),
                    ("C_w4", "td3::w4_pack_kernel")],
        ("dp", 1): [("C_dw", "td3::dwsk_kernel<true, false>"), ("C_rs_adam_ag", "rccl"),
                    ("C_polyak", "td3::polyak_w4_kernel"),
                    ("A_dw", "td3::dwsk_kernel<false, false>"), ("A_rs_adam_ag", "rccl"),
                    ("A_polyak", "td3::polyak_w4_kernel")],
    },
    "sharded_no_images_b64": {
        **_fused("td3::dw_kernel<true>", "td3::dw_kernel<false>"),
        ("dp", 0): [("C_dw", "td3::dw_kernel<true>"), ("C_rs_adam_ag", "rccl")],
        ("dp", 1): [("C_dw", "td3::dw_kernel<true>"), ("C_rs_adam_ag", "rccl"), ("C_polyak", "td3::polyak_flat_kernel"),
                    ("A_dw", "td3::dw_kernel<false>"), ("A_rs_adam_ag", "rccl"),
                    ("A_polyak", "td3::polyak_flat_kernel")],
    },
    "sharded_no_images_b512": {
        **_fused("td3::dwsk_kernel<true, false>", "td3::dwsk_kernel<false, false>"),
        ("dp", 0): [("C_dw", "td3::dwsk_kernel<true, false>"), ("C_rs_adam_ag", "rccl")],
        ("dp", 1): [("C_dw", "td3::dwsk_kernel<true, false>"), ("C_rs_adam_ag", "rccl"),
                    ("C_polyak", "td3::polyak_flat_kernel"),
                    ("A_dw", "td3::dwsk_kernel<false, false>"), ("A_rs_adam_ag", "rccl"),
                    ("A_polyak", "td3::polyak_flat_kernel")],
    },
    "weight_normalization": {
        ("fused", 0): [("C_dw", "td3::dw_kernel<true>"), ("C_wn", "td3::wn_kernel")],
        ("fused", 1): [("C_dw", "td3::dw_kernel<true>"), ("C_wn", "td3::wn_kernel"),
                       ("A_dw", "td3::dw_kernel<false>"), ("A_wn", "td3::wn_kernel")],
        ("dp", 0): [("C_dw", "td3::dw_kernel<true>"), ("C_allreduce", "rccl"), ("C_wn", "td3::wn_kernel")],
        ("dp", 1): [("C_dw", "td3::dw_kernel<true>"), ("C_allreduce", "rccl"), ("C_wn", "td3::wn_kernel"),
                    ("A_dw", "td3::dw_kernel<false>"), ("A_allreduce", "rccl"), ("A_wn", "td3::wn_kernel")],
    },
    "particles": {
        ("fused", 0): [("C_dw", "td3::dw_kernel<false>"), ("C_enc_adam", "td3::enc_adam_kernel")],
        ("fused", 1): [("C_dw", "td3::dw_kernel<false>"), ("C_enc_adam", "td3::enc_adam_kernel"),
                       ("A_dw", "td3::dw_kernel<false>"), ("A_enc_adam", "td3::enc_adam_kernel")],
        ("dp", 0): [("C_dw", "td3::dw_kernel<false>"), ("C_enc_adam", "td3::enc_adam_kernel"),
                    ("C_allreduce", "rccl"), ("C_adam", "td3::adam_flat_kernel")],
        ("dp", 1): [("C_dw", "td3::dw_kernel<false>"), ("C_enc_adam", "td3::enc_adam_kernel"),
                    ("C_allreduce", "rccl"), ("C_adam", "td3::adam_flat_kernel"),
                    ("A_dw", "td3::dw_kernel<false>"), ("A_enc_adam", "td3::enc_adam_kernel"),
                    ("A_allreduce", "rccl"), ("A_adam", "td3::adam_flat_kernel")],
    },
}


@pytest.mark.parametrize("name", list(CASES))
def test_dw_stage_tail(name, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[name][4].items():
        monkeypatch.setenv(k, v)
    got = plan_tails(name)
    for key, want in EXPECTED[name].items():
        assert got[key] == want, (name, key, got[key])
    assert set(got) == set(EXPECTED[name])


if __name__ == "__main__":          # the dump the literal lists above come from
    dump = {}
    for case in CASES:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(CASES[case][4])
        dump[case] = plan_tails(case)
    print("EXPECTED = " + pprint.pformat(dump, width=118))
