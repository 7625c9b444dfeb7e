"""The numpy TD3+BC reference (tests/bc_reference.py) on the CPU: its actor gradients against torch
autograd of the loss written in torch ops, alpha = 0 against the oracle, and the share of each term of
dL/dpi in every case the GPU tests use."""
import copy

import numpy as np
import pytest

import bc_reference as bcr
from helpers import featured_setup, featured_setup_dims, load_golden, orc
from test_oracle_golden import _rel_to_max

from oracle.td3_torch_cpu import FeaturedTorch


def _first_batch(S, name):
    idx, noise = bcr.case_steps(S, name)[0]
    return S["buf"].gather(idx), noise


@pytest.mark.parametrize("alpha", [2.5, 0.5])
@pytest.mark.parametrize("name", ["hc_layer", "hc_none", "pend_layer"])
def test_actor_grads_match_torch_autograd(name, alpha):
    """loss = -lambda mean Q1(s, pi) + mse(pi, a), lambda = alpha / mean |Q1| detached, on the restatement's
    own actor and q: rel-to-max 2e-5, the tolerance tests/test_torch_cpu_restatement.py holds that
    restatement to."""
    import torch
    import torch.nn.functional as F
    S = featured_setup(name)
    (s, a, _, _, _), _ = _first_batch(S, name)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rec = {}
    grads = bcr.bc_actor_grads(L, s, a, alpha, rec)
    T = FeaturedTorch(S["actor"], S["critic"], **S["kw"])
    ts, ta = torch.from_numpy(s), torch.from_numpy(a)
    pi = T.actor(T.A, ts)
    q = T.q(T.C, "q1.", ts, pi)
    lam = alpha / q.abs().mean().detach()
    loss = -lam * q.mean() + F.mse_loss(pi, ta)
    loss.backward()
    np.testing.assert_allclose(rec["lambda"], float(lam), rtol=1e-5)
    np.testing.assert_allclose(rec["bc_actor_loss"], float(loss.detach()), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(rec["bc_loss"], float(F.mse_loss(pi, ta).detach()), rtol=1e-5)
    for k, g in grads.items():
        assert _rel_to_max(g, T.A[k].grad.numpy()) <= 2e-5, (name, alpha, k)


@pytest.mark.parametrize("name", ["hc_layer", "hc_wn", "pend_layer"])
def test_alpha_zero_is_the_oracle_step(name):
    S = featured_setup(name)
    G = load_golden("featured", name)
    La = orc.Learner(S["actor"], S["critic"], **S["kw"])
    Lb = copy.deepcopy(La)
    for step in (1, 2):
        batch, noise = S["buf"].gather(G[f"step{step}/idx"]), G[f"step{step}/noise"]
        ra = orc.featured_train_step(La, batch, noise)
        rb = bcr.bc_featured_step(Lb, batch, noise, 0.0)
        for k in ("y", "q1", "q2"):
            np.testing.assert_array_equal(ra[k], rb[k])
        assert ra["critic_loss"] == rb["critic_loss"]
    assert rb["actor_loss"] == ra["actor_loss"]
    for grp in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
        for k, v in getattr(La, grp).items():
            np.testing.assert_array_equal(v, getattr(Lb, grp)[k], err_msg=f"{grp} {k}")


def _shares_after_critic_step(S, alpha, name=None):
    """The term shares of the actor phase as the GPU tests reach it: one critic-only step, then step 2."""
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for idx, noise in bcr.case_steps(S, name):
        rec = bcr.bc_featured_step(L, S["buf"].gather(idx), noise, alpha)
    return bcr.term_shares(rec)


@pytest.mark.parametrize("name,alpha", bcr.CASES)
def test_neither_term_is_decoration_golden_cases(name, alpha):
    sq, sb = _shares_after_critic_step(featured_setup(name), alpha, name)
    print(f"{name} alpha={alpha}: Q term {sq:.3f}, BC term {sb:.3f} of |dL/dpi|")
    assert sq >= bcr.MIN_SHARE and sb >= bcr.MIN_SHARE, (name, alpha, sq, sb)


@pytest.mark.parametrize("case", bcr.EDGES)
def test_neither_term_is_decoration_edge_shapes(case):
    sd, ad, ma, norm, B, alpha = case
    sq, sb = _shares_after_critic_step(featured_setup_dims(sd, ad, ma, norm, B), alpha)
    print(f"{case}: Q term {sq:.3f}, BC term {sb:.3f} of |dL/dpi|")
    assert sq >= bcr.MIN_SHARE and sb >= bcr.MIN_SHARE, (case, sq, sb)
