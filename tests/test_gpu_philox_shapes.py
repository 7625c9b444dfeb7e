"""The production first layer (Philox rows drawn and read from the ring inside the first forward
launch, learner.h Plan::body_ring) against the oracle at the shapes where its kernels change.

Every case runs a critic-only and a policy step from the oracle's state with NO injected indices:
the rows and the noise the step drew are read back, the batch is taken from the host-side
``orc.FeaturedBuffer`` that holds the same rows (never from the GPU), and the oracle replays the
step.  y / Q1 / Q2, the losses, the four parameter groups and the counters are held to the
teacher-forced contracts of tests/test_gpu_edges.py; both Adam moments of every critic tensor (and
of every actor tensor on the policy step) to 2e-4 / 4e-4 of the tensor's max, the bounds of
``test_overlapped_allreduce_schedule_single_rank`` -- the parameters of a first Adam step show only
the gradient's sign, the moments show a wrong X_SA / X_SP row copy in the layer-0 dW.  A second
learner then runs the same step from the same state with those indices and that noise injected
(``gather_kernel`` + Plan::body), and the kernel the planner picked is asserted per phase
(``td3_profile_stages`` / ``td3_stage_kernel``; prologue numbers in the names: 0 = kProCopy,
3 = kProGather, 5 = kProL0G).

First-layer instantiations of the ring-sampled step (kernels_launch.h) and the cases that run them.
The planner (stages.hip gemm_wn, can_fuse_l0, l0r16_config) picks per phase: a policy step has a
fourth network (the online actor) in the launch, so hc_none / hc_wn / inj_noise (B = 256) run
l0r16 on the critic-only step and the 32-row GEMM on the policy step.

=============================  ======================================================================
instantiation                  cases
=============================  ======================================================================
l0r16_kernel<2, 4, true>       pend_b1 (31 padding rows), hc_b33, k0_24, k0_32_b64, odd_w_layer,
                               odd_w_none, part_ring
l0r16_kernel<6, 2, true>       hc_b128, wide_w; critic-only step of hc_none, hc_wn, inj_noise
l0r16_kernel<5, 2, true>       unreachable: taken only when b96 > 256 >= b80 (l0r16_config), and
                               ceil(N / 80) >= ceil(N / 96) makes b80 >= b96 (TD3_L0R16_N96 left on)
gemm_kernel<0, 2, kProL0G>     hc_b257, k0_32_b257; policy step of hc_none, hc_wn, inj_noise
gemm_kernel<0, 4, kProL0G>     hc_b512, hc_b544 (Bp % 64 = 32: dw64_kernel behind it)
gemm_kernel<0, 1, kProL0G>     l0g_wn1: B >= 512 with 129..255 32-column layer-1 tiles (narrow widths)
gemm_kernel<0, 0, kProL0G>     l0g_wn0: B >= 512 with <= 128 such tiles (narrow widths)
                               Below B = 512 neither is reachable: the stage leaves l0r16 only when
                               b96 = 2 t S96 > 256 (t = Bp / 32 <= 15, S96 = sum ceil(N / 96)), and
                               sum ceil(N / 32) >= 3 S96 - 2 nets gives t * that > 384 - 2 * 4 * 15 =
                               264 >= TD3_WN2_MIN 32-column tiles: gemm_wn returns 2 (or 4: K <= 128).
                               With the default (500, 400, .) widths neither is reachable at all.
gemm_kernel<0, 4, kProGather>  ant_b256, ant_b33, rec128 (stage F_fwd0: input wider than 32 columns)
gemm_kernel<0, {0,1,2},        unreachable: the sample is fused only for 2 sd + ad + 2 <= 128, so the
            kProGather>        stage's K = pad32(sd + ad) <= 128 and gemm_wn returns 4 first
gather_kernel + kProCopy       rec129 (2 sd + ad + 2 = 129: the first record the prologue leaves to
                               the separate kernel; Humanoid's 772 floats are the only other one)
=============================  ======================================================================

Fused against injected path: the two read the same floats and run the same GEMM / l0r16 body behind
another prologue.  Measured on an MI355X, EVERY case above (all 22, both steps) came out
bit-identical in y, Q1, Q2 and all four parameter groups, rec129 included (there both paths run
gather_kernel, with drawn against injected indices): ``assert_array_equal`` holds for every case
and none is left to the oracle bounds alone.  The oracle errors measured there: y / Q1 / Q2 at most
1.4e-6 of the max, the moments at most 5.1e-6 (exp_avg) and 9.4e-6 (exp_avg_sq) of the tensor max,
so no case needed another ring seed.
"""
import numpy as np
import pytest

from helpers import orc, stage_kernels
from test_gpu_edges import _setup
from test_gpu_parity import _load_oracle_state, _params_close, _rel_to_max

pytestmark = pytest.mark.gpu

R16_24 = "td3::l0r16_kernel<2, 4, true>"
R16_62 = "td3::l0r16_kernel<6, 2, true>"
L0G = "td3::gemm_kernel<0, %d, 5>"            # kProL0G
GATHER = "td3::gemm_kernel<0, 4, 3>"          # kProGather
COPY = "td3::gemm_kernel<0, 4, 0>"            # kProCopy behind the separate gather_kernel
FUSED = "(fused into F_fwd0)"

NARROW0 = dict(actor_arch=(256, 32, 32), q_arch=(256, 32, 32))
NARROW1 = dict(actor_arch=(256, 96, 32), q_arch=(256, 96, 32))
ODD = dict(actor_arch=(64, 48, 40), q_arch=(96, 72, 33))
WIDE = dict(actor_arch=(512, 512, 512), q_arch=(512, 512, 512))

# id: (sd, ad, B, setup keywords, first-layer kernel of the critic-only step, of the policy step)
CASES = {
    "pend_b1": (3, 1, 1, {}, R16_24, R16_24),                      # 31 padding rows
    "hc_b33": (17, 6, 33, {}, R16_24, R16_24),                     # ragged second row tile
    "hc_b128": (17, 6, 128, {}, R16_62, R16_62),
    "hc_b257": (17, 6, 257, {}, L0G % 2, L0G % 2),                 # ragged, 32-row tiles
    "k0_24": (24, 4, 64, {}, R16_24, R16_24),                      # actor K0 = 24 (12 MFMAs), critic 28
    "k0_32_b64": (29, 3, 64, {}, R16_24, R16_24),                  # 16-MFMA layout under the sample
    "k0_32_b257": (29, 3, 257, {}, L0G % 2, L0G % 2),
    "odd_w_layer": (11, 3, 96, dict(ODD), R16_24, R16_24),        # partly empty column tiles
    "odd_w_none": (11, 3, 96, dict(ODD, norm=None), R16_24, R16_24),
    "wide_w": (17, 6, 128, dict(WIDE), R16_62, R16_62),            # last tile 32 of 96 columns
    "ant_b256": (27, 8, 256, {}, GATHER, GATHER),                  # stand-alone sampled layer 0
    "ant_b33": (27, 8, 33, {}, GATHER, GATHER),
    "rec128": (55, 16, 64, {}, GATHER, GATHER),                    # widest fused record
    "rec129": (55, 17, 64, {}, COPY, COPY),                        # first unfused record
    "hc_b512": (17, 6, 512, {}, L0G % 4, L0G % 4),                 # + split-K dW
    "hc_b544": (17, 6, 544, {}, L0G % 4, L0G % 4),                 # Bp % 64 = 32, dw64_kernel
    "hc_none": (17, 6, 256, dict(norm=None), R16_62, L0G % 2),     # no kH0 store
    "hc_wn": (17, 6, 256, dict(norm="weight_normalization"), R16_62, L0G % 2),   # row-major kW0
    "part_ring": (17, 6, 64, dict(fill=37), R16_24, R16_24),       # the draw is over the 37 rows held
    "inj_noise": (17, 6, 256, {}, R16_62, L0G % 2),                # body_ring[.][1]
    "l0g_wn1": (17, 6, 512, dict(NARROW1), L0G % 1, L0G % 1),
    "l0g_wn0": (17, 6, 512, dict(NARROW0), L0G % 0, L0G % 0),
}


def _moments(pol, group):
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    m, v = ((_lib.TD3_ACTOR_ADAM_M, _lib.TD3_ACTOR_ADAM_V), (_lib.TD3_CRITIC_ADAM_M, _lib.TD3_CRITIC_ADAM_V))[group]
    return _ParamView(pol, m, group).numpy_dict(), _ParamView(pol, v, group).numpy_dict()


def _moment_errs(pol, group, ref_m, ref_v):
    """Worst exp_avg / exp_avg_sq error over the group's tensors, relative to each tensor's max."""
    m, v = _moments(pol, group)
    em = max((_rel_to_max(m[k], ref_m[k]), k) for k in ref_m)
    ev = max((_rel_to_max(v[k], ref_v[k]), k) for k in ref_v)
    return em, ev


def _groups(pol):
    return {"actor": pol.actor.flat(), "critic": pol.critic.flat(),
            "actor_target": pol.actor_target.flat(), "critic_target": pol.critic_target.flat()}


@pytest.mark.parametrize("case", list(CASES))
def test_philox_step_at_shape(case):
    sd, ad, B, kw, k_critic, k_policy = CASES[case]
    pol, rb, L, buf = _setup(sd, ad, **kw)
    inj, rbi, _, _ = _setup(sd, ad, **kw)                     # the injected path, from the same state
    rs = np.random.RandomState(B)
    draws = []
    for step in (1, 2):                                       # critic-only, then a policy step
        _load_oracle_state(pol, L)
        _load_oracle_state(inj, L)
        given = rs.standard_normal((B, ad)).astype(np.float32) if case == "inj_noise" else None
        out = pol.train_step(rb, B, noise=given, stats=True)
        idx, noise = out["idx"], out["noise"]
        assert idx.min() >= 0 and idx.max() < buf.size, (step, idx.min(), idx.max())
        assert np.isfinite(noise).all()
        if given is not None:
            np.testing.assert_array_equal(noise, given)
        draws.append(idx.tobytes())
        rec = orc.featured_train_step(L, buf.gather(idx), noise)
        fig = {"y": _rel_to_max(out["y"], rec["y"][:, 0]), "q1": _rel_to_max(out["q1"], rec["q1"][:, 0]),
               "q2": _rel_to_max(out["q2"], rec["q2"][:, 0]),
               "critic_m,v": _moment_errs(pol, 1, L.critic_m, L.critic_v)}
        if out["actor_step"]:
            fig["actor_m,v"] = _moment_errs(pol, 0, L.actor_m, L.actor_v)
        two = inj.train_step(rbi, B, indices=idx, noise=noise, stats=True)
        a, b = _groups(pol), _groups(inj)
        same = {k: bool(np.array_equal(out[k], two[k])) for k in ("y", "q1", "q2")}
        same.update({k: bool(np.array_equal(a[k], b[k])) for k in a})
        print(f"\n{case} step {step}: {fig} bit-identical to the injected path: {same}")

        assert fig["y"] <= 1e-5 and fig["q1"] <= 1e-5 and fig["q2"] <= 1e-5, (step, fig)
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        assert out["actor_step"] == ("actor_loss" in rec) == (step == 2)
        if out["actor_step"]:
            np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (step, "critic"))
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (step, "actor"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, L.lr, (step, "critic_target"))
        _params_close(pol.actor_target.numpy_dict(), L.actor_target, L.lr, (step, "actor_target"))
        assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
        for name in [k for k in fig if k.endswith("m,v")]:
            (em, km), (ev, kv) = fig[name]
            assert em <= 2e-4, (step, name, "exp_avg", km, em)
            assert ev <= 4e-4, (step, name, "exp_avg_sq", kv, ev)
        assert all(same.values()), (step, same)
    assert draws[0] != draws[1]                               # a fresh draw every step

    for phase, kernel in ((0, k_critic), (1, k_policy)):      # a real step each: last
        st = stage_kernels(pol, rb, B, phase)
        first = next(k for n, k in st[1:] if n.startswith("F_"))
        print(f"{case} phase {phase}: {st[0][1]} -> {st[1][0]} {first}")
        assert st[0][1] == ("td3::gather_kernel" if case == "rec129" else FUSED), st[:2]
        assert first == kernel, (phase, st[:2])


def test_ant_graph_equals_eager():
    """The ring-bound stand-alone layer 0 (gemm_kernel<0, 4, kProGather>) launched directly, replayed
    from the captured step graph, and under the default policy: the same Philox rows, the same
    kernels, bit-identical parameters after two critic-only and two policy steps."""
    outs = []
    for use_graph in (False, True, "auto"):
        pol, rb, _, _ = _setup(27, 8, use_graph=use_graph)
        for _ in range(4):
            pol.train_step(rb, 256)
        outs.append(_groups(pol))
    for other in outs[1:]:
        for k in outs[0]:
            np.testing.assert_array_equal(outs[0][k], other[k], err_msg=k)
