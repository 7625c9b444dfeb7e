"""The prioritized featured step (include/td3.h td3_train_step_prioritized) at the planner's edge shapes
(per_reference.EDGES) against the weighted oracle step, teacher-forced from the oracle's state; the
uniform step after a prioritized one at ragged batches; graph replay against direct launches.

Each case is there for one choice of the planner (stages.hip, step.hip): the sample fused or the separate
gather, layer 0 on row tiles or stand-alone, narrow or wide heads, dw_kernel / dw64_kernel / split-K
dwsk_kernel, with or without LayerNorm statistics, weight norm, ragged pad rows.  The importance weight
reaches the dW stage as the per-row gscale, so the check that sees a weight dropped, doubled or shifted by
a row there is the critic's Adam exp_avg: post-Adam parameters at step 1 are theta - lr sign(g).
tests/test_per_reference.py holds on the CPU that each case's weights spread and that a step without them
is more than 100x the moment tolerance away.

Tolerances are the project's (tests/test_gpu_parity.py, restated by tests/test_gpu_prioritized_step.py):
forward values / losses rtol 1e-5, post-Adam parameters within 1e-6 + 1e-5|x| on >= 99.9 % of the elements
and within 2*lr everywhere, Adam exp_avg within 2e-4 of its max."""
import numpy as np
import pytest

import bc_reference as bcr
import per_reference as per
from helpers import featured_setup_dims, gen, orc, stage_kernels
from test_gpu_bc import BC_KERNEL, _check_actor_step
from test_gpu_prioritized_step import (ALPHA, EPS, MOMENT_TOL, Box, _copy_state, _load_oracle_state, _params_close,
                                       _rel_to_max, _row_max, _views)
from test_gpu_train_log import _check as _check_log_entry

pytestmark = pytest.mark.gpu

GATHER = "td3::gather_kernel"
C_DW = {"dw64": "td3::dw64_kernel<true>", "dwsk": "td3::dwsk_kernel<true, false>"}
SEPARATE_GATHER = ("hum", "hum1024", "rec139", "in512")


def _make(S, use_graph=True, prioritized=True, bc_alpha=None):
    """test_gpu_prioritized_step._make for any widths and a partly filled ring: ``S["fill"]`` rows
    (default all) of the ring's data are written, ``S["actor_arch"]`` / ``S["q_arch"]`` size the networks."""
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    hp = dict(S["hp"])
    lr = hp.pop("lr", 1e-4)
    pol = TD3(Box((S["sd"],)), Box((S["ad"],)), max_action=S["ma"], norm=S["norm"], lr=lr, use_graph=use_graph,
              init="none", actor_arch=S.get("actor_arch", gen.ACTOR_ARCH), q_arch=S.get("q_arch", gen.Q_ARCH), **hp)
    pol.set_weights(S["actor"], S["critic"])
    if bc_alpha:
        pol.bc_alpha = bc_alpha
    fill = S.get("fill", gen.BUFFER_ROWS)
    rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS)
    rb.add_batch(*(x[:fill] for x in gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], gen.BUFFER_ROWS, gen.SEED)))
    assert rb.size == fill
    if prioritized:
        rb.enable_priorities(alpha=ALPHA, eps=EPS)
    return pol, rb


def _set_first(rb, p):
    import torch
    rb.set_priorities(torch.arange(p.size, device="cuda"), torch.as_tensor(p, device="cuda"))


def _moment_error(opt, ref_m):
    """The largest rel-to-max error of an optimizer's exp_avg over its tensors, and that tensor."""
    sd = opt.state_dict()
    errs = [(_rel_to_max(sd["state"][i]["exp_avg"].numpy(), ref_m[k]), k) for i, k in enumerate(ref_m)]
    return max(errs)


@pytest.mark.parametrize("case", per.EDGES, ids=[c["name"] for c in per.EDGES])
def test_prioritized_step_edge_shapes(case):
    """Two steps (critic-only, then the actor phase), each from the oracle's state: the draw and the
    weights, every output of the step, the parameters, the moments, the priorities written back, the
    training log's entry, and the kernel of the stage the case is there for."""
    name, alpha, beta = case["name"], case.get("bc_alpha"), case["beta"]
    S = per.edge_setup(case)
    pol, rb = _make(S, bc_alpha=alpha)
    pol.per_beta = beta
    log = pol.enable_train_log(capacity=4)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    lr, B, fill, size = S["kw"].get("lr", 1e-4), S["B"], S["fill"], gen.BUFFER_ROWS
    outs = []
    for step in (1, 2):
        p, u, noise = per.edge_step(case, S, step)
        _set_first(rb, p)
        idx = per.draw(p, u)
        w = per.weights(p, idx, fill, beta)
        _load_oracle_state(pol, L)
        batch = S["buf"].gather(idx)
        if alpha:
            rec = bcr.bc_featured_step(L, batch, noise, alpha, w=w)
        else:
            rec = per.weighted_featured_step(L, batch, noise, w)
        out = pol.train_step(rb, B, noise=noise, stats=True, u=u)
        outs.append(out)
        # the draw and the weights
        np.testing.assert_array_equal(out["idx"], idx)
        np.testing.assert_allclose(out["weight"], w, rtol=1e-5)
        if B == 1:
            assert out["weight"][0] == 1.0
        # forward values
        for k in ("y", "q1", "q2"):
            assert _rel_to_max(out[k], rec[k][:, 0]) <= 1e-5, (step, k)
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        np.testing.assert_allclose(out["td_abs"], rec["td_abs"], rtol=1e-5, atol=1e-6 * np.abs(rec["y"]).max())
        assert out["actor_step"] == (step == 2)
        assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
        cm = _moment_error(pol.critic_optimizer, L.critic_m)
        am = _moment_error(pol.actor_optimizer, L.actor_m) if step == 2 else (0.0, "")
        print(f"edge {name} step {step}: critic exp_avg {cm[0]:.3e} ({cm[1]}), actor exp_avg {am[0]:.3e} ({am[1]}), "
              f"bound {MOMENT_TOL:.0e}")
        if out["actor_step"]:
            np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
            if alpha:                       # the five BC scalars (and the actor's moments once more)
                _check_actor_step(out, rec, pol, L, lr, (name, step))
        else:
            assert "bc_loss" not in out
        # parameters and moments
        _params_close(pol.critic.numpy_dict(), L.critic, lr, (step, "critic"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, lr, (step, "critic_target"))
        _params_close(pol.actor.numpy_dict(), L.actor, lr, (step, "actor"))
        _params_close(pol.actor_target.numpy_dict(), L.actor_target, lr, (step, "actor_target"))
        assert cm[0] <= MOMENT_TOL, (step, "critic exp_avg") + cm
        assert am[0] <= MOMENT_TOL, (step, "actor exp_avg") + am
        # the write-back: the drawn rows hold (td_abs + eps)^alpha, every other leaf is untouched
        leaves = rb.priorities()
        assert leaves.shape == (size,)
        np.testing.assert_allclose(leaves[idx], per.priority(_row_max(idx, out["td_abs"]), ALPHA, EPS), rtol=1e-5)
        rest = np.ones(fill, bool)
        rest[idx] = False
        np.testing.assert_array_equal(leaves[:fill][rest], p[rest])
        np.testing.assert_array_equal(leaves[fill:], np.zeros(size - fill, np.float32))
        info = rb.priority_info()
        np.testing.assert_allclose(info["total"], leaves.astype(np.float64).sum(), rtol=1e-5)
        assert info["max_priority"] == max(p.max(), leaves[idx].max())
    # the log: y/Q-derived fields and w_mean / w_min bit for bit against train_log_reference.entry
    e = log.entries()
    assert len(e) == 2
    for t, out in enumerate(outs):
        _check_log_entry(e[t], out, B, 1, True, t + 1, prioritized=True)
    # the path the case is there for, on a plain ring of the same dims (a real step each: after the comparison)
    _, plain = _make(S, prioritized=False)
    st = [stage_kernels(pol, plain, B, phase) for phase in (0, 1)]
    print(f"edge {name} kernels: sample {st[0][0][1]}, C_dw {dict(st[0])['C_dw']} / {dict(st[1])['C_dw']}, "
          f"actor_head_bwd {dict(st[1])['actor_head_bwd']}")
    if name in C_DW:
        assert [dict(s)["C_dw"] for s in st] == [C_DW[name]] * 2, st
    if name in SEPARATE_GATHER:
        assert [s[0][1] for s in st] == [GATHER] * 2, st
    if alpha:
        assert dict(st[1])["actor_head_bwd"] == BC_KERNEL, st[1]


@pytest.mark.parametrize("B", [100, 544])
def test_uniform_step_after_prioritized_edge_batches(B):
    """test_gpu_prioritized_step.test_uniform_step_after_prioritized_is_bit_exact (injected rows, graph on)
    at ragged batches, Bp > B: the pad entries of the plan's weight buffer are part of what the next
    step of another kind refills with ones."""
    case = per.edge_case(f"uniform{B}", 17, 6, 1.0, "layer", B, 1.0, B)
    S = per.edge_setup(case)
    p, u, noise = per.edge_step(case, S, 1)
    a, rb = _make(S)
    b, plain = _make(S, prioritized=False)
    a.per_beta = 1.0
    _set_first(rb, p)
    out = a.train_step(rb, B, noise=noise, stats=True, u=u)
    assert out["weight"].min() <= 0.2                          # the buffer now holds non-unit weights
    _copy_state(a, a)                                          # both learners take their state the same way
    _copy_state(a, b)
    rs = np.random.RandomState(11)
    idx = rs.randint(0, gen.BUFFER_ROWS, size=B)
    nz = rs.standard_normal((B, S["ad"])).astype(np.float32)
    for step in range(2):                                      # the actor phase, then critic-only
        oa = a.train_step(rb, B, indices=idx, noise=nz, stats=True)
        ob = b.train_step(plain, B, indices=idx, noise=nz, stats=True)
        assert oa["actor_step"] == ob["actor_step"] == (step == 0)
        for k in ("idx", "y", "q1", "q2", "noise"):
            np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"step {step} {k}")
        assert oa["critic_loss"] == ob["critic_loss"]
        for va, vb in zip(_views(a), _views(b)):
            np.testing.assert_array_equal(va.flat(), vb.flat())


@pytest.mark.parametrize("sd,ad,B", [(17, 6, 256), (40, 17, 100), (60, 17, 64)])
def test_prioritized_graph_equals_eager(sd, ad, B):
    """Four free-running prioritized steps (the Philox draw, Philox noise) captured and launched directly:
    parameters, moments and leaves bit for bit.  The sample sits inside the fused layer-0/1 launch
    (sd = 17), inside the stand-alone layer 0 (sd = 40), and in the separate gather (sd = 60)."""
    case = per.edge_case(f"graph{sd}", sd, ad, 1.0, "layer", B, 0.4, B)
    S = featured_setup_dims(sd, ad, 1.0, "layer", B)
    p, _, _ = per.edge_step(case, dict(S, fill=gen.BUFFER_ROWS), 1)
    res = []
    for use_graph in (True, False):
        pol, rb = _make(S, use_graph=use_graph)
        _set_first(rb, p)
        for _ in range(4):
            pol.train(rb, B)
        pol.sync()
        assert pol._counters() == (4, 4, 2)
        res.append([v.flat() for v in _views(pol)] + [rb.priorities()])
    for i, (g, e) in enumerate(zip(*res)):
        np.testing.assert_array_equal(g, e, err_msg=f"view {i}")
    assert (res[0][-1] != p).sum() > B // 2
