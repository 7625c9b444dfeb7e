"""The particle learner's one-call prioritized step (include/td3.h td3_train_step_prioritized_particles)
against the weighted oracle step of per_particles_reference.py, and the rule that every other particle
step keeps unit weights bit for bit.

Shapes are the particle goldens' own (F = 7, N = 16, D = 9, A = 3, a ring of 1000 rows: a 2-level tree,
B = 32, and B = 20 for pad rows).  Tolerances are the project's (tests/test_gpu_parity.py,
tests/test_gpu_prioritized_step.py): forward values / losses rtol 1e-5, post-Adam parameters within
1e-6 + 1e-5|x| on >= 99.9 % of the elements and within 2*lr everywhere, the critic's Adam exp_avg within
2e-4 of its max."""
import numpy as np
import pytest

import per_particles_reference as ppr
import per_reference as per
from helpers import featured_setup, gen, orc
from test_gpu_parity import _load_oracle_state, _rel_to_max
from test_gpu_particles import _check_step
from test_gpu_prioritized_step import _copy_state, _row_max, _set_all, _views

pytestmark = pytest.mark.gpu

ALPHA, EPS = 0.6, 1e-6
ROWS = gen.BUFFER_ROWS


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _spaces(S):
    return (Box((S["F"],)), Box((S["N"], S["D"]))), Box((S["A"],))


def _policy(S, use_graph=True, per_beta=1.0):
    from td3_amd.TD3_particles import TD3
    obs, act = _spaces(S)
    pol = TD3(obs, act, norm=S["norm"], CDQ=S["cdq"], use_graph=use_graph, init="none", per_beta=per_beta)
    pol.set_weights(S["actor"], S["critic"])
    return pol


def _ring(S, prioritized=True, rows=ROWS):
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    obs, act = _spaces(S)
    rb = ReplayBuffer_particles(obs, act, max_size=rows)
    rb.add_batch(*gen.fill_particle_buffer(S["F"], S["N"], S["D"], S["A"], rows, gen.SEED))
    if prioritized:
        rb.enable_priorities(alpha=ALPHA, eps=EPS)
    return rb


def _critic_moments(pol):
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    return _ParamView(pol, _lib.TD3_CRITIC_ADAM_M, 1).numpy_dict()


@pytest.mark.parametrize("name", ppr.CASES)
def test_prioritized_particle_step_teacher_forced(name):
    """Two steps (critic-only, then the actor phase), each from the oracle's state: every output of the
    step, the parameters, the critic's moments and the priorities written back."""
    S = ppr.setup(name)
    pol, rb = _policy(S), _ring(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    B = S["B"]
    for step in (1, 2):
        _, p, u, noise = ppr.step_case(name, step)
        _set_all(rb, p)
        idx = per.draw(p, u)
        w = per.weights(p, idx, ROWS, pol.per_beta)
        assert w.min() <= 0.35                                  # a condition on the inputs
        _load_oracle_state(pol, L)
        rec = ppr.weighted_particle_step(L, S["buf"].gather(idx), noise, w)
        out = pol.train_step(rb, B, noise=noise, stats=True, u=u)
        np.testing.assert_array_equal(out["idx"], idx)
        np.testing.assert_allclose(out["weight"], w, rtol=1e-5)
        assert out["y"].shape == out["q1"].shape == out["q2"].shape == (B, S["A"])
        np.testing.assert_allclose(out["td_abs"], rec["td_abs"], rtol=1e-5, atol=1e-6 * np.abs(rec["y"]).max())
        assert out["actor_step"] == (step == 2)
        # y / q1 / q2 rel-to-max 1e-5, the weighted loss and the actor loss rtol 1e-5, the four parameter
        # groups, the counters
        _check_step(out, rec, pol, L, (name, step))
        if not S["cdq"]:
            np.testing.assert_array_equal(out["q2"], out["q1"])
        m = _critic_moments(pol)
        assert list(m) == list(L.critic_m)
        for k, v in L.critic_m.items():
            assert _rel_to_max(m[k].reshape(v.shape), v) <= per.MOMENT_TOL, (step, k)
        # the write-back: the drawn rows hold (row-max td_abs + eps)^alpha, every other leaf is untouched
        leaves = rb.priorities()
        np.testing.assert_allclose(leaves[idx], per.priority(_row_max(idx, out["td_abs"]), ALPHA, EPS), rtol=1e-5)
        rest = np.ones(ROWS, bool)
        rest[idx] = False
        np.testing.assert_array_equal(leaves[rest], p[rest])
        info = rb.priority_info()
        np.testing.assert_allclose(info["total"], leaves.astype(np.float64).sum(), rtol=1e-5)
        assert info["max_priority"] == max(p.max(), leaves[idx].max())


def test_prioritized_particle_graph_equals_eager():
    """Two prioritized steps captured and launched directly: parameters and leaves bit for bit."""
    outs = []
    for use_graph in (False, True):
        S = ppr.setup("part_layer")
        pol, rb = _policy(S, use_graph=use_graph), _ring(S)
        for step in (1, 2):
            _, p, u, noise = ppr.step_case("part_layer", step)
            if step == 1:
                _set_all(rb, p)
            pol.train_step(rb, S["B"], noise=noise, u=u)
        outs.append([v.flat() for v in _views(pol)] + [rb.priorities()])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    assert (outs[0][-1] != ppr.step_case("part_layer", 1)[1]).sum() > S["B"] // 2


def _after_prioritized(use_graph):
    """Learner a after one prioritized step with non-unit weights, learner b that never ran one, in
    the same state; their rings (a's prioritized, and a plain one each)."""
    S, p, u, noise = ppr.step_case("part_layer", 1)
    a, rb = _policy(S, use_graph=use_graph), _ring(S)
    b = _policy(S, use_graph=use_graph)
    _set_all(rb, p)
    out = a.train_step(rb, S["B"], noise=noise, stats=True, u=u)
    assert out["weight"].min() <= 0.35                          # the buffer now holds non-unit weights
    _copy_state(a, a)                                           # both learners take their state the same way
    _copy_state(a, b)
    return S, a, b, rb


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("path", ["injected", "philox"])
def test_uniform_particle_step_after_prioritized_is_bit_exact(use_graph, path):
    """The prioritized step leaves its weights in the plan's buffer; the next step of any other kind
    refills it with ones first.  That step -- the injected-index path, or the production path that
    draws its rows by the step counter -- equals bit for bit the same step of a learner that never ran
    a prioritized one, from the same state."""
    S, a, b, rb = _after_prioritized(use_graph)
    B = S["B"]
    plain_a, plain_b = _ring(S, prioritized=False), _ring(S, prioritized=False)
    rs = np.random.RandomState(11)
    idx = rs.randint(0, ROWS, size=B)
    nz = rs.standard_normal((B, S["A"])).astype(np.float32)
    for step in range(2):                                       # the actor phase, then critic-only
        if path == "injected":
            oa = a.train_step(rb, B, indices=idx, noise=nz, stats=True)
            ob = b.train_step(plain_b, B, indices=idx, noise=nz, stats=True)
        else:
            oa = a.train_step(plain_a, B, stats=True)
            ob = b.train_step(plain_b, B, stats=True)
        assert oa["actor_step"] == (step == 0)
        for k in ("idx", "y", "q1", "q2", "noise"):
            np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"step {step} {k}")
        assert oa["critic_loss"] == ob["critic_loss"]
        for va, vb in zip(_views(a), _views(b)):
            np.testing.assert_array_equal(va.flat(), vb.flat())


def test_actor_learn_after_prioritized_is_bit_exact():
    """_actor_learn right after a prioritized step: its actor phase reads no importance weights."""
    S, a, b, _ = _after_prioritized(True)
    f, p = gen.fill_particle_buffer(S["F"], S["N"], S["D"], S["A"], S["B"], gen.SEED + 2)[:2]
    la = a._actor_learn(f, p, stats=True)
    lb = b._actor_learn(f, p, stats=True)
    assert la == lb
    for va, vb in zip(_views(a), _views(b)):
        np.testing.assert_array_equal(va.flat(), vb.flat())


def test_particle_train_free_running_with_adds():
    """TD3.train on a prioritized particle ring: 20 steps without injection, rows added in between."""
    import torch
    S = ppr.setup("part_layer")
    pol, rb = _policy(S, per_beta=0.4), _ring(S)
    B = S["B"]
    before = rb.priorities()
    np.testing.assert_array_equal(before, np.ones(ROWS, np.float32))
    out = pol.train_step(rb, B, stats=True)                     # the first step tells which rows it drew
    leaves = rb.priorities()
    np.testing.assert_allclose(leaves[out["idx"]], per.priority(_row_max(out["idx"], out["td_abs"]), ALPHA, EPS),
                               rtol=1e-5)
    assert (leaves[out["idx"]] != 1.0).all()
    assert (np.diff(out["idx"]) >= 0).all() and out["idx"].max() < ROWS   # equal priorities: stratum k holds rows in order
    f, p, a, f2, p2, r, d = gen.fill_particle_buffer(S["F"], S["N"], S["D"], S["A"], 64, gen.SEED + 1)
    for it in range(19):
        if it % 3 == 0:
            rb.add((f[it], p[it]), a[it], (f2[it], p2[it]), r[it], d[it])   # host row: shipped in the step's stream order
        if it % 5 == 0:
            rb.add_batch(*[torch.as_tensor(x[:8], device="cuda") for x in (f, p, a, f2, p2, r, d)])
        pol.train(rb, B)
    pol.sync()
    assert pol._counters() == (20, 20, 10)
    leaves = rb.priorities()
    assert np.isfinite(leaves).all() and (leaves[:rb.size] > 0).all()
    assert (leaves != before).sum() > B // 2
    info = rb.priority_info()
    assert info["max_priority"] >= leaves.max() and info["max_priority"] >= 1.0
    np.testing.assert_allclose(info["total"], leaves.astype(np.float64).sum(), rtol=1e-5)
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()


def test_device_loop_on_a_prioritized_particle_ring():
    """DeviceTrainLoop over a particle environment, a prioritized particle ring and per_beta set."""
    from td3_amd.loop import DeviceTrainLoop, SyntheticParticleVecEnv
    S = ppr.setup("part_layer")
    F, N, D, A = S["F"], S["N"], S["D"], S["A"]
    pol = _policy(S, per_beta=0.4)
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    obs, act = _spaces(S)
    rb = ReplayBuffer_particles(obs, act, max_size=256)
    rb.enable_priorities(alpha=ALPHA, eps=EPS)
    env = SyntheticParticleVecEnv(8, F, N, D, A, max_episode_steps=25, device=pol.device)
    loop = DeviceTrainLoop(env, pol, rb, start_policy=2, start_training=4, batch_size=16, expl_noise=0.1)
    res = loop.run(12)
    assert res["env_steps"] == 96 and res["grad_steps"] == 8
    assert pol.total_it == 8 and rb.size == 96
    leaves = rb.priorities()
    assert np.isfinite(leaves).all() and (leaves[:96] > 0).all() and (leaves[96:] == 0).all()
    assert (leaves[:96] != 1.0).sum() > 8                       # the steps wrote their rows' priorities back
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()


def test_refusals():
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    from td3_amd.my_replay_buffer import ReplayBuffer_featured, ReplayBuffer_particles
    from td3_amd.TD3_featured import TD3 as TD3F
    S = ppr.setup("part_layer")
    pol, rb = _policy(S, per_beta=0.4), _ring(S, rows=64)
    lib = pol._lib

    def step(h, ring, beta=0.4):
        rc = lib.td3_train_step_prioritized_particles(h, ring.handle, 32, beta, None, None, None, None, None)
        return rc, lib.td3_last_error()

    for beta in (1.5, -0.1):
        rc, err = step(pol._h, rb, beta)
        assert rc == -1 and b"beta" in err
    pol.per_beta = 1.5
    with pytest.raises(TD3Error, match="beta"):
        pol.train(rb, 32)
    pol.per_beta = 0.4
    rc, err = step(pol._h, _ring(S, prioritized=False, rows=64))
    assert rc == -1 and b"not enabled" in err
    obs, act = _spaces(S)
    narrow = ReplayBuffer_particles((Box((S["F"] - 1,)), obs[1]), act, max_size=64)
    narrow.fill_synthetic(64)
    narrow.enable_priorities()
    rc, err = step(pol._h, narrow)
    assert rc == -1 and b"dims" in err
    empty = ReplayBuffer_particles(obs, act, max_size=64)
    empty.enable_priorities()
    rc, err = step(pol._h, empty)
    assert rc == -1 and b"empty" in err
    Fs = featured_setup("hc_layer")
    rbf = ReplayBuffer_featured(Box((Fs["sd"],)), Box((Fs["ad"],)), max_size=64)
    rbf.fill_synthetic(64)
    rbf.enable_priorities()
    rc, err = step(pol._h, rbf)                                 # kind mismatch, as td3_train_step
    assert rc == -1 and b"kind" in err
    polf = TD3F(Box((Fs["sd"],)), Box((Fs["ad"],)), max_action=Fs["ma"], norm=Fs["norm"], init="none")
    polf.set_weights(Fs["actor"], Fs["critic"])
    rc, err = step(polf._h, rbf)
    assert rc == -1 and b"featured learner" in err
    rc = lib.td3_train_step_prioritized(pol._h, rb.handle, 32, 0.4, None, None, None, None, None)
    err = lib.td3_last_error()                                  # the featured entry points here
    assert rc == -1 and b"particle learner" in err and b"td3_train_step_prioritized_particles" in err
    assert pol._counters() == (0, 0, 0) and polf._counters() == (0, 0, 0)   # nothing ran
    np.testing.assert_array_equal(rb.priorities(), np.ones(64, np.float32))
    pol.train(rb, 32)                                           # and the handle still steps
    assert pol._counters() == (1, 1, 0)
    default = _policy(S, per_beta=None)
    with pytest.raises(NotImplementedError, match="prioritized.*per_beta"):
        default.train(rb, 16)
    with pytest.raises(ValueError, match="u is the draw"):
        pol.train_step(_ring(S, prioritized=False, rows=64), 16, u=np.full(16, 0.5, np.float32))
    pols = [_policy(S, per_beta=0.4) for _ in range(2)]
    local_group(pols)
    rc, err = step(pols[0]._h, rb)
    assert rc == -1 and b"data-parallel" in err


def test_debug_per_stage_replays_the_steps_gather_and_combine():
    """The measurement entry (tools/bench_per.py): refused before a prioritized step of the plan on that
    ring; afterwards it queues the step's own gather and combine over the rows that step drew, which
    changes nothing the next step sees."""
    outs = []
    for replay in (False, True):
        S = ppr.setup("part_layer")
        pol, rb = _policy(S), _ring(S)
        lib = pol._lib
        if replay:
            assert lib.td3_debug_per_stage(pol._h, rb.handle, 0, None) == -1
            assert b"prioritized step" in lib.td3_last_error()
        for step in (1, 2):
            _, p, u, noise = ppr.step_case("part_layer", step)
            if step == 1:
                _set_all(rb, p)
            out = pol.train_step(rb, S["B"], noise=noise, stats=True, u=u)
            if replay:
                assert lib.td3_debug_per_stage(pol._h, rb.handle, 2, None) == -1
                for stage in (0, 1):
                    assert lib.td3_debug_per_stage(pol._h, rb.handle, stage, None) == 0, lib.td3_last_error()
                other = _ring(S, rows=64)
                assert lib.td3_debug_per_stage(pol._h, other.handle, 0, None) == -1   # not the step's ring
                pol.sync()
        outs.append([v.flat() for v in _views(pol)] + [rb.priorities(), out["td_abs"], out["y"]])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
