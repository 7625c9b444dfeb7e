"""The one-call prioritized TD3 step (include/td3.h td3_train_step_prioritized) against the weighted
oracle step of per_reference.py, and the rule that every other step keeps unit weights bit for bit.

Tolerances are the project's (tests/test_gpu_parity.py): forward values / losses rtol 1e-5, post-Adam
parameters within 1e-6 + 1e-5|x| on >= 99.9 % of the elements and within 2*lr everywhere, the critic's
Adam exp_avg within 2e-4 of its max."""
import numpy as np
import pytest

import per_reference as per
from helpers import featured_setup, gen, orc, particle_setup

pytestmark = pytest.mark.gpu

ALPHA, EPS = 0.6, 1e-6
MOMENT_TOL = per.MOMENT_TOL


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _rel_to_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.abs(b).max() + 1e-30))


def _make(S, use_graph=True, prioritized=True):
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    hp = dict(S["hp"])
    lr = hp.pop("lr", 1e-4)
    pol = TD3(Box((S["sd"],)), Box((S["ad"],)), max_action=S["ma"], norm=S["norm"], lr=lr,
              use_graph=use_graph, init="none", **hp)
    pol.set_weights(S["actor"], S["critic"])
    rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS)
    rb.add_batch(*gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], gen.BUFFER_ROWS, gen.SEED))
    if prioritized:
        rb.enable_priorities(alpha=ALPHA, eps=EPS)
    return pol, rb


def _params_close(gpu, ref, lr, what, frac=0.999):
    """SURVEY §8c post-Adam contract (restated from tests/test_gpu_parity.py): within 1e-6 + 1e-5|x| on
    >= `frac` of the elements, and within 2*lr everywhere -- the update of a near-zero gradient whose
    sign flips between two fp32 summation orders is +-lr, so two parameters differ by up to 2*lr."""
    for k in ref:
        g, o = np.asarray(gpu[k], np.float64), np.asarray(ref[k], np.float64)
        err = np.abs(g - o)
        tight = err <= 1e-6 + 1e-5 * np.abs(o)
        assert tight.mean() >= frac or (~tight).sum() <= 2, (what, k, (~tight).sum(), err.max())
        assert err.max() <= 2 * lr * 1.001, (what, k, err.max())


def _views(pol):
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    return [_ParamView(pol, w, g) for w, g in (
        (_lib.TD3_ACTOR, 0), (_lib.TD3_ACTOR_TARGET, 0), (_lib.TD3_CRITIC, 1), (_lib.TD3_CRITIC_TARGET, 1),
        (_lib.TD3_ACTOR_ADAM_M, 0), (_lib.TD3_ACTOR_ADAM_V, 0), (_lib.TD3_CRITIC_ADAM_M, 1),
        (_lib.TD3_CRITIC_ADAM_V, 1))]


def _load_oracle_state(pol, L):
    pol.set_weights(L.actor, L.critic, L.actor_target, L.critic_target)
    v = _views(pol)
    v[4].load_state_dict(L.actor_m)
    v[5].load_state_dict(L.actor_v)
    v[6].load_state_dict(L.critic_m)
    v[7].load_state_dict(L.critic_v)
    pol._set_counters(L.total_it, L.critic_step, L.actor_step)


def _row_max(idx, td_abs):
    """Per entry, the largest |TD error| of its row in the batch: a row drawn twice meets two target
    noises, and the write-back keeps the larger of its two values."""
    top = np.zeros(int(idx.max()) + 1, np.float32)
    np.maximum.at(top, idx, td_abs)
    return top[idx]


def _set_all(rb, p):
    import torch
    rb.set_priorities(torch.arange(p.size, device="cuda"), torch.as_tensor(p, device="cuda"))


@pytest.mark.parametrize("name", ["hc_layer", "hc_layer_b100"])
def test_prioritized_step_teacher_forced(name):
    """Two steps (critic-only, then the actor phase), each from the oracle's state: every output of the
    step, the parameters, the critic's moments and the priorities written back."""
    S = featured_setup(name)
    pol, rb = _make(S)
    pol.per_beta = 1.0
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    lr, B, size = S["kw"].get("lr", 1e-4), S["B"], gen.BUFFER_ROWS
    for step in (1, 2):
        _, p, u, noise = per.step_case(name, step)
        _set_all(rb, p)
        idx = per.draw(p, u)
        w = per.weights(p, idx, size, pol.per_beta)
        assert w.min() <= 0.2
        _load_oracle_state(pol, L)
        rec = per.weighted_featured_step(L, S["buf"].gather(idx), noise, w)
        out = pol.train_step(rb, B, noise=noise, stats=True, u=u)
        np.testing.assert_array_equal(out["idx"], idx)
        np.testing.assert_allclose(out["weight"], w, rtol=1e-5)
        for k in ("y", "q1", "q2"):
            assert _rel_to_max(out[k], rec[k][:, 0]) <= 1e-5, (step, k)
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        np.testing.assert_allclose(out["td_abs"], rec["td_abs"], rtol=1e-5, atol=1e-6 * np.abs(rec["y"]).max())
        assert out["actor_step"] == (step == 2)
        if out["actor_step"]:
            np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
        _params_close(pol.critic.numpy_dict(), L.critic, lr, (step, "critic"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, lr, (step, "critic_target"))
        _params_close(pol.actor.numpy_dict(), L.actor, lr, (step, "actor"))
        _params_close(pol.actor_target.numpy_dict(), L.actor_target, lr, (step, "actor_target"))
        assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
        sd = pol.critic_optimizer.state_dict()
        for i, k in enumerate(L.critic):
            assert _rel_to_max(sd["state"][i]["exp_avg"].numpy(), L.critic_m[k]) <= MOMENT_TOL, (step, k)
        # the write-back: the drawn rows hold (td_abs + eps)^alpha, every other leaf is untouched
        leaves = rb.priorities()
        np.testing.assert_allclose(leaves[idx], per.priority(_row_max(idx, out["td_abs"]), ALPHA, EPS), rtol=1e-5)
        rest = np.ones(size, bool)
        rest[idx] = False
        np.testing.assert_array_equal(leaves[rest], p[rest])
        info = rb.priority_info()
        np.testing.assert_allclose(info["total"], leaves.astype(np.float64).sum(), rtol=1e-5)
        assert info["max_priority"] == max(p.max(), leaves[idx].max())


def _copy_state(src, dst):
    for a, b in zip(_views(src), _views(dst)):
        b.set_flat(a.flat())
    dst._set_counters(*src._counters())


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("path", ["injected", "fused"])
def test_uniform_step_after_prioritized_is_bit_exact(use_graph, path):
    """The prioritized step leaves its weights in the plan's buffer; the next step of any other kind
    refills it with ones first.  That step -- the injected-index path, or the production path whose
    first layer draws the rows -- equals bit for bit the same step of a learner that never ran a
    prioritized one, from the same state."""
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    S, p, u, noise = per.step_case("hc_layer", 1)
    B = S["B"]
    a, rb = _make(S, use_graph=use_graph)
    b, plain = _make(S, use_graph=use_graph, prioritized=False)
    a.per_beta = 1.0
    _set_all(rb, p)
    out = a.train_step(rb, B, noise=noise, stats=True, u=u)
    assert out["weight"].min() <= 0.2                          # the buffer now holds non-unit weights
    _copy_state(a, a)                                          # both learners take their state the same way
    _copy_state(a, b)
    rs = np.random.RandomState(11)
    idx = rs.randint(0, gen.BUFFER_ROWS, size=B)
    nz = rs.standard_normal((B, S["ad"])).astype(np.float32)
    plain_a = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS)
    plain_a.add_batch(*gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], gen.BUFFER_ROWS, gen.SEED))
    for step in range(2):                                      # the actor phase, then critic-only
        if path == "injected":
            oa = a.train_step(rb, B, indices=idx, noise=nz, stats=True)
            ob = b.train_step(plain, B, indices=idx, noise=nz, stats=True)
        else:                                                  # a ring without priorities: the fused Philox draw
            oa = a.train_step(plain_a, B, stats=True)
            ob = b.train_step(plain, B, stats=True)
        for k in ("idx", "y", "q1", "q2", "noise"):
            np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"step {step} {k}")
        assert oa["critic_loss"] == ob["critic_loss"]
        for va, vb in zip(_views(a), _views(b)):
            np.testing.assert_array_equal(va.flat(), vb.flat())


def test_train_free_running_with_adds():
    """TD3.train on a prioritized ring: 20 steps without injection, rows added in between."""
    import torch
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    rows = gen.BUFFER_ROWS
    before = rb.priorities()
    np.testing.assert_array_equal(before, np.ones(rows, np.float32))
    out = pol.train_step(rb, S["B"], stats=True)               # the first step tells which rows it drew
    leaves = rb.priorities()
    np.testing.assert_allclose(leaves[out["idx"]], per.priority(_row_max(out["idx"], out["td_abs"]), ALPHA, EPS),
                               rtol=1e-5)
    assert (leaves[out["idx"]] != 1.0).all()
    assert (np.diff(out["idx"]) >= 0).all() and out["idx"].max() < rows   # equal priorities: stratum k holds rows in order
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], 64, gen.SEED + 1)
    for it in range(19):
        if it % 3 == 0:
            rb.add(s[it], a[it], s2[it], r[it], d[it])          # host row: shipped in the step's stream order
        if it % 5 == 0:
            rb.add_batch(*[torch.as_tensor(x[:8], device="cuda") for x in (s, a, s2, r, d)])
        pol.train(rb, S["B"])
    pol.sync()
    assert pol._counters() == (20, 20, 10)
    leaves = rb.priorities()
    assert np.isfinite(leaves).all() and (leaves[:rb.size] > 0).all()
    assert (leaves != before).sum() > S["B"] // 2
    info = rb.priority_info()
    assert info["max_priority"] >= leaves.max() and info["max_priority"] >= 1.0
    np.testing.assert_allclose(info["total"], leaves.astype(np.float64).sum(), rtol=1e-5)
    for k, v in pol.critic.numpy_dict().items():
        assert np.isfinite(v).all(), k


def test_refusals():
    from td3_amd import _lib
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    from td3_amd.TD3_particles import TD3 as TD3P
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    lib = pol._lib

    def step(h, ring, beta=0.4):
        rc = lib.td3_train_step_prioritized(h, ring.handle, 32, beta, None, None, None, None, None)
        return rc, lib.td3_last_error()

    for beta in (1.5, -0.1):
        rc, err = step(pol._h, rb, beta)
        assert rc == -1 and b"beta" in err
    pol.per_beta = 1.5
    with pytest.raises(TD3Error, match="beta"):
        pol.train(rb, 32)
    pol.per_beta = 0.4
    _, plain = _make(S, prioritized=False)
    rc, err = step(pol._h, plain)
    assert rc == -1 and b"not enabled" in err
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    narrow = ReplayBuffer_featured(Box((S["sd"] - 1,)), Box((S["ad"],)), max_size=64)
    narrow.fill_synthetic(64)
    narrow.enable_priorities()
    rc, err = step(pol._h, narrow)
    assert rc == -1 and b"dims" in err
    P = particle_setup("part_layer")
    obs = (Box((P["F"],)), Box((P["N"], P["D"])))
    polp = TD3P(obs, Box((P["A"],)), norm=P["norm"], CDQ=P["cdq"], init="none")
    polp.set_weights(P["actor"], P["critic"])
    rbp = ReplayBuffer_particles(obs, Box((P["A"],)), max_size=64)
    rbp.add_batch(*gen.fill_particle_buffer(P["F"], P["N"], P["D"], P["A"], 64, gen.SEED))
    rbp.enable_priorities()                                     # the ring of either kind has priorities ...
    assert rbp.priority_info()["total"] == 64.0
    rc, err = step(polp._h, rbp)                                # ... the particle learner's loss has no weights
    assert rc == -1 and b"particle learner" in err
    with pytest.raises(NotImplementedError, match="prioritized"):
        polp.train(rbp, 16)
    rc, err = step(pol._h, rbp)                                 # kind mismatch, as td3_train_step
    assert rc == -1 and b"kind" in err
    assert pol._counters() == (0, 0, 0)                         # nothing ran
    pol.train(rb, 32)                                           # and the handle still steps
    pols = [_make(S)[0] for _ in range(2)]
    local_group(pols)
    rc, err = step(pols[0]._h, rb)
    assert rc == -1 and b"data-parallel" in err
