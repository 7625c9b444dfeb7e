"""numpy references of prioritized replay (include/td3.h): the draw, the importance weights, the
priority of a TD error, and the weighted TD3 step rebuilt from the oracle's public pieces."""
from __future__ import annotations

import numpy as np

from helpers import featured_setup, gen, orc

f32 = np.float32
MOMENT_TOL = 2e-4          # rel-to-max of the critic's Adam exp_avg (test_gpu_parity.test_adam_moments_match_oracle)


def masses(u, total):
    """m = u * total as the device forms it: one fp32 multiply."""
    return (np.asarray(u, f32) * f32(total)).astype(f32)


def draw(p, u):
    """Rows of the mass fractions ``u`` over priorities ``p``: the first row whose inclusive prefix sum
    exceeds m.  The prefix sums are float64; with priorities whose partial sums are exact in fp32
    (small integers) every correct tree agrees with this bit for bit."""
    c = np.cumsum(np.asarray(p, np.float64))
    return np.searchsorted(c, masses(u, c[-1]).astype(np.float64), side="right").astype(np.int64)


def weights(p, idx, size, beta):
    """(size * p / total) ** -beta over the drawn rows, divided by the batch maximum; float64."""
    p = np.asarray(p, np.float64)
    w = (size * p[idx] / p.sum()) ** (-float(beta))
    return w / w.max()


def priority(td_abs, alpha, eps):
    return (np.asarray(td_abs, np.float64) + eps) ** alpha


def chi_square(counts, p):
    """Pearson chi-square of draw counts against the distribution p / sum(p), and its degrees of freedom."""
    p = np.asarray(p, np.float64)
    e = counts.sum() * p / p.sum()
    return float(((counts - e) ** 2 / e).sum()), p.size - 1


def weighted_featured_step(L, batch, noise, w, masks=None):
    """``orc.featured_train_step`` (TD3_featured.py:123-171) with per-row importance weights in the
    critic loss: critic_loss = sum_j mean(w (Q_j - y)^2), dL/dQ_j = 2/B w (Q_j - y).  The actor loss is
    not weighted.  ``w`` = 1 reproduces the oracle's step exactly."""
    masks = masks or {}
    rec = {}
    s, a, s2, r, nd = batch
    B = s.shape[0]
    w = np.asarray(w, f32).reshape(B, 1)
    L.total_it += 1
    eps = np.clip(noise.astype(f32) * f32(L.policy_noise), -f32(L.noise_clip), f32(L.noise_clip))
    ta, _ = orc.featured_actor(L.actor_target, L.norm, L.max_action, s2)
    next_a = np.clip(ta + eps, -f32(L.max_action), f32(L.max_action)).astype(f32)
    tq1, _ = orc.featured_q(L.critic_target, "q1", L.norm, s2, next_a)
    tq2, _ = orc.featured_q(L.critic_target, "q2", L.norm, s2, next_a)
    y = (r + (nd * f32(L.discount)) * np.minimum(tq1, tq2)).astype(f32)
    q1, c1 = orc.featured_q(L.critic, "q1", L.norm, s, a)
    q2, c2 = orc.featured_q(L.critic, "q2", L.norm, s, a)
    w64 = w.astype(np.float64)
    l1 = float(np.mean(w64 * (q1 - y).astype(np.float64) ** 2))
    l2 = float(np.mean(w64 * (q2 - y).astype(np.float64) ** 2))
    td_abs = 0.5 * (np.abs((q1 - y).astype(np.float64)) + np.abs((q2 - y).astype(np.float64)))
    rec.update(ta_out=ta, next_action=next_a, y=y, q1=q1, q2=q2, critic_loss=l1 + l2,
               critic_loss_parts=(l1, l2), td_abs=td_abs[:, 0])
    grads = {}
    for q, qv, (lin, ln, cache) in (("q1", q1, c1), ("q2", q2, c2)):
        if q in masks:
            cache["mask"] = masks[q]
        gq = ((f32(2.0 / B) * w) * (qv - y)).astype(f32)
        g, _ = orc.mlp_backward(lin, ln, cache, gq)
        grads.update(orc.pack_mlp_grads(f"{q}.", g, L.norm, P=L.critic))
    rec["critic_grads"] = grads
    L.adam_critic(grads)
    if L.total_it % L.policy_freq == 0:
        L.adam_actor(orc.featured_actor_grads(L, s, rec, masks))
        L.polyak()
    return rec


def step_case(name, step):
    """Integer priorities in [1, 15] (exact partial sums: the draw is reproducible bit for bit; with
    beta = 1 the weights are p_min / p and span [1/15, 1]), mass fractions and target noise of one step."""
    S = featured_setup(name)
    rs = np.random.RandomState(100 * step + S["B"])
    p = rs.randint(1, 16, size=gen.BUFFER_ROWS).astype(np.float32)
    u = rs.uniform(size=S["B"]).astype(np.float32)
    u = np.where((u * np.float32(p.sum())).astype(np.float32) >= p.sum(), np.float32(0.5), u)
    noise = rs.standard_normal((S["B"], S["ad"])).astype(np.float32)
    return S, p, u, noise
