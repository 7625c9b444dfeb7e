"""CPU checks of tests/clip_reference.py: with clipping off it is the oracle's step bit for bit, its rule is
clip_grad_norm_'s, and every (case, group) of a GPU parameter check is one clipping really moves.

Adam is almost invariant to a constant scale of the gradient, so a learner that ignored max_norm would pass
a parameter comparison under a constant coefficient: the share test below holds the schedule the GPU
parameter checks use to PARAM_SHARE, and shows the constant-coefficient schedule falling far short of it
(that one is checked on the GPU through gradients, norms, coefs and Adam moments only)."""
import copy

import numpy as np
import pytest

import clip_reference as cr
import per_particles_reference as ppr
from helpers import gen, orc


def _same_learner(a, b, what):
    for grp in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
        for k, v in getattr(b, grp).items():
            np.testing.assert_array_equal(getattr(a, grp)[k], v, err_msg=f"{what}: {grp} {k}")
    assert (a.total_it, a.critic_step, a.actor_step) == (b.total_it, b.critic_step, b.actor_step)


@pytest.mark.parametrize("name", ["hc_layer_b100", "hc_none"])
def test_off_reproduces_the_featured_oracle(name):
    S = cr.setup(name)
    a = orc.Learner(S["actor"], S["critic"], **S["kw"])
    b = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for idx, noise in cr.case_steps(name, 2):
        ra = cr.clipped_featured_step(a, S["buf"].gather(idx), noise, (None, 0.0))
        rb = orc.featured_train_step(b, S["buf"].gather(idx), noise)
        assert ra["clip"] == {} and ra["critic_loss"] == rb["critic_loss"]
    _same_learner(a, b, name)


@pytest.mark.parametrize("name", ["part_layer", "part_nocdq"])
def test_off_reproduces_the_particle_oracle(name):
    S = ppr.setup(name)
    a = orc.Learner(S["actor"], S["critic"], **S["kw"])
    b = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rs = np.random.RandomState(3)
    for _ in range(2):
        idx = rs.randint(0, gen.BUFFER_ROWS, size=S["B"])
        noise = rs.standard_normal((S["B"], S["A"])).astype(np.float32)
        ra = cr.clipped_particle_step(a, S["buf"].gather(idx), noise, (0.0, None))
        rb = orc.particle_train_step(b, S["buf"].gather(idx), noise)
        assert ra["clip"] == {} and ra["critic_loss"] == rb["critic_loss"]
    _same_learner(a, b, name)


def test_rule_is_clip_grad_norm():
    """Against torch.nn.utils.clip_grad_norm_ itself on one gradient dict, and the IEEE corners."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(0)
    grads = {"a": rs.standard_normal((7, 5)).astype(np.float32), "b": rs.standard_normal(11).astype(np.float32)}
    total = cr.grad_norm(grads)
    for mn in (0.3 * total, 3.0 * total):
        ps = [torch.nn.Parameter(torch.zeros(v.shape)) for v in grads.values()]
        for p, v in zip(ps, grads.values()):
            p.grad = torch.from_numpy(v.copy())
        got = float(torch.nn.utils.clip_grad_norm_(ps, mn))
        np.testing.assert_allclose(got, total, rtol=1e-6)
        coef = cr.clip_coef(total, mn)
        assert coef.dtype == np.float32 and (coef == 1.0) == (mn > total)
        for p, v in zip(ps, grads.values()):
            np.testing.assert_allclose(p.grad.numpy(), coef * v, rtol=2e-6)
    assert np.isnan(cr.clip_coef(np.nan, 1.0))          # no guard: a NaN total gives a NaN coef
    assert cr.clip_coef(np.inf, 1.0) == 0.0
    assert cr.clip_coef(0.0, 1.0) == 1.0


def test_teacher_forced_coef_is_used():
    S = cr.setup("hc_layer_b100")
    (idx, noise), = cr.case_steps("hc_layer_b100", 1)
    a = orc.Learner(S["actor"], S["critic"], **S["kw"])
    b = copy.deepcopy(a)
    ra = cr.clipped_featured_step(a, S["buf"].gather(idx), noise, (None, 1.0))
    rb = cr.clipped_featured_step(b, S["buf"].gather(idx), noise, (None, 1.0), coefs={"critic": np.float32(0.25)})
    assert rb["clip"]["critic"]["coef"] == 0.25 != ra["clip"]["critic"]["coef"]
    k = next(iter(a.critic_m))
    scale = np.float32(0.25) / np.float32(ra["clip"]["critic"]["coef"])
    np.testing.assert_allclose(b.critic_m[k], a.critic_m[k] * scale, rtol=1e-5, atol=1e-12)     # exp_avg ~ coef
    np.testing.assert_allclose(b.critic_v[k], a.critic_v[k] * scale ** 2, rtol=1e-5, atol=1e-18)  # exp_avg_sq ~ coef^2


def test_schedules():
    assert cr.factors("first") == [(None, 0.05), (0.05, None), (None, None), (None, None)]
    for name in cr.FEATURED_CASES:
        steps = cr.plan(name, "first")["steps"]
        assert [sorted(s["clip"]) for s in steps] == [["critic"], ["actor", "critic"]] * 2
        # 0.05 up to the rule's 1e-6 in the denominator (hc_none's actor norm is 0.02)
        np.testing.assert_allclose([steps[0]["clip"]["critic"]["coef"], steps[1]["clip"]["actor"]["coef"]], 0.05,
                                   rtol=1e-4)
        assert all(s["clip"]["critic"]["coef"] == 1.0 for s in steps[1:]) and steps[3]["clip"]["actor"]["coef"] == 1.0
        assert all(0.49 < v["coef"] < 0.51 for s in cr.plan(name, "half")["steps"] for v in s["clip"].values())


@pytest.mark.parametrize("name,schedule,group", cr.PARAM_CHECKS)
def test_clipping_moves_every_parameter_check(name, schedule, group):
    """The condition of a GPU parameter check: the clipped and the unclipped reference run differ on at least
    PARAM_SHARE of the group's elements by more than 10x the parameter tolerance."""
    assert cr.moved_share(name, schedule, group) >= cr.PARAM_SHARE


def test_constant_coefficient_would_not_show():
    """Why "half" is in no parameter check: Adam hides a constant coefficient."""
    assert ("hc_layer", "half", "critic") not in cr.PARAM_CHECKS
    assert max(cr.moved_share("hc_layer", "half", g) for g in ("critic", "actor")) < 0.2
