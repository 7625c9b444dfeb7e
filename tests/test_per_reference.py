"""CPU checks of the prioritized-replay references (tests/per_reference.py) that the GPU tests lean on."""
import copy

import numpy as np
import pytest

import per_reference as per
from helpers import featured_setup, gen, orc


def _rel_to_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("name", ["hc_layer", "hc_layer_b100"])
def test_unit_weights_reproduce_the_oracle_step(name):
    """weighted_featured_step with w = 1 is orc.featured_train_step exactly: two steps (the second with
    the actor phase), every recorded value and every piece of learner state bit for bit."""
    S = featured_setup(name)
    La = orc.Learner(S["actor"], S["critic"], **S["kw"])
    Lb = copy.deepcopy(La)
    rs = np.random.RandomState(3)
    for step in (1, 2):
        batch = S["buf"].gather(rs.randint(0, gen.BUFFER_ROWS, size=S["B"]))
        noise = rs.standard_normal((S["B"], S["ad"])).astype(np.float32)
        ra = per.weighted_featured_step(La, batch, noise, np.ones(S["B"], np.float32))
        rb = orc.featured_train_step(Lb, batch, noise)
        for k in ("y", "q1", "q2", "next_action"):
            np.testing.assert_array_equal(ra[k], rb[k])
        assert ra["critic_loss"] == rb["critic_loss"] and ("actor_loss" in ra) == ("actor_loss" in rb) == (step == 2)
        for grp in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
            for k, v in getattr(La, grp).items():
                np.testing.assert_array_equal(v, getattr(Lb, grp)[k], err_msg=f"{grp}/{k}")
        assert (La.total_it, La.critic_step, La.actor_step) == (Lb.total_it, Lb.critic_step, Lb.actor_step)


@pytest.mark.parametrize("name", ["hc_layer", "hc_layer_b100"])
def test_weighted_reference_separates_from_unweighted(name):
    """CPU side of the teacher-forced test: the unweighted oracle's critic exp_avg differs from the
    weighted one's by more than 100x the tolerance the GPU is held to, tensor by tensor -- a step that
    ignored the weights cannot pass.  """
    for step in (1, 2):
        S, p, u, noise = per.step_case(name, step)
        idx = per.draw(p, u)
        w = per.weights(p, idx, gen.BUFFER_ROWS, 1.0)
        assert w.min() <= 0.2 and w.max() == 1.0
        Lw = orc.Learner(S["actor"], S["critic"], **S["kw"])
        Lu = copy.deepcopy(Lw)
        batch = S["buf"].gather(idx)
        per.weighted_featured_step(Lw, batch, noise, w)
        orc.featured_train_step(Lu, batch, noise)
        for k in Lw.critic_m:
            assert _rel_to_max(Lu.critic_m[k], Lw.critic_m[k]) > 100 * per.MOMENT_TOL, k


@pytest.mark.parametrize("rows,batches,bound", [(1000, 160, 1222.0), (100, 40, 169.0)])
def test_reference_draw_meets_the_chi_square_bound(rows, batches, bound):
    """The stratified reference draw stays under dof + 5 sqrt(2 dof), the bound the GPU draw is held to,
    and a draw that ignores the priorities is far above it."""
    B = 256
    p = np.exp(np.random.RandomState(rows).standard_normal(rows)).astype(np.float32)
    dof = rows - 1
    assert abs(dof + 5 * np.sqrt(2 * dof) - bound) < 1.0
    for seed in range(3):
        rs = np.random.RandomState(seed)
        u = ((np.arange(B)[None, :] + rs.uniform(size=(batches, B))) / B).astype(np.float32)
        idx = np.minimum(per.draw(p, u.ravel()), rows - 1)
        chi2, d = per.chi_square(np.bincount(idx, minlength=rows).astype(np.float64), p)
        assert d == dof and chi2 < bound, (seed, chi2)
    uniform = np.random.RandomState(9).randint(0, rows, size=batches * B)
    assert per.chi_square(np.bincount(uniform, minlength=rows).astype(np.float64), p)[0] > 10 * bound
