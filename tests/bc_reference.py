"""numpy reference of the TD3+BC actor step (include/td3.h, "TD3+BC"; Fujimoto & Gu 2021) rebuilt from
the oracle's public pieces, and the cases the BC tests share.

    q_abs_mean = mean_r |Q1(s_r, pi_r)|           (no gradient)
    lambda     = alpha / q_abs_mean
    loss       = -lambda mean_r Q1(s_r, pi_r) + mean_{r,o} (pi_r,o - a_r,o)^2
    dL/dpi     = lambda dQ1/da (-1/B inside) + 2/(B A) (pi - a)
"""
from __future__ import annotations

import numpy as np

from helpers import gen, load_golden, orc

f32 = np.float32
MOMENT_TOL = 2e-4          # rel-to-max of an Adam exp_avg (test_gpu_parity.test_adam_moments_match_oracle)
MIN_SHARE = 0.10           # each term of dL/dpi carries at least this share of the total's L2 norm

# (golden configuration, alpha) of the teacher-forced GPU cases.  2.5 is the paper's default; it is used
# wherever both terms of dL/dpi then carry MIN_SHARE of the total (tests/test_bc_reference.py checks every
# pair on the CPU), else a value chosen there.
CASES = [("hc_layer", 2.5), ("hc_layer_b100", 2.5), ("hc_none", 2.5), ("hc_wn", 2.5), ("pend_layer", 2.5),
         ("hum_layer", 2.5)]
# (sd, ad, max_action, norm, B, alpha) of the edge shapes: every A in {1, 8, 9, 16, 17, 32} with a ragged
# B, every B in {33, 100, 257} with a wide A; max_action 2 in half; sd + ad <= 32 fuses layer 0 into the
# layer-1 launch, wider inputs keep the separate layer-0 stage (and its transposed W1 copy).  alpha is 2.5
# where that qualifies; at A = 16 and A = 32 with max_action 1 the BC term then carries 5-6 %, so 0.5.
# B = 1000 (ragged, > 512): the lambda reduction's second trip of eight rows per lane
EDGES = [(5, 1, 2.0, "layer", 33, 2.5), (11, 8, 1.0, "layer", 100, 2.5), (11, 9, 2.0, None, 257, 2.5),
         (14, 16, 1.0, "layer", 33, 0.5), (40, 17, 2.0, "layer", 100, 2.5), (40, 32, 1.0, None, 257, 0.5),
         (12, 17, 2.0, "layer", 257, 2.5), (40, 8, 2.0, "layer", 33, 2.5), (17, 6, 1.0, "layer", 1000, 2.5)]


def case_steps(S, name=None):
    """[(rows, N(0,1) target noise)] of the two steps of a case (critic-only, then the actor phase): the
    golden's recorded draws for a golden configuration, seeded draws for a setup of ``featured_setup_dims``.
    The CPU and the GPU tests run the same two steps, so the term shares checked on the CPU are the GPU's."""
    if name is not None:
        G = load_golden("featured", name)
        return [(G[f"step{k}/idx"], G[f"step{k}/noise"]) for k in (1, 2)]
    rs = np.random.RandomState(1000 * S["sd"] + 10 * S["ad"] + S["B"])
    return [(rs.randint(0, gen.BUFFER_ROWS, size=S["B"]), rs.standard_normal((S["B"], S["ad"])).astype(f32))
            for _ in range(2)]


def bc_actor_grads(L, s, a, alpha, record=None, masks=None):
    """``orc.featured_actor_grads`` with the TD3+BC loss; records pi, actor_q1, actor_loss (still
    -mean Q1), lambda, q_abs_mean, bc_loss, bc_actor_loss, actor_grads and the two terms of dL/dpi
    (gpi_q, gpi_bc).  ``alpha`` = 0 is the oracle's function itself."""
    if not alpha:
        return orc.featured_actor_grads(L, s, record, masks)
    rec = record if record is not None else {}
    B, A = a.shape
    masks = masks or {}
    pi, (alin, aln, acache, t) = orc.featured_actor(L.actor, L.norm, L.max_action, s)
    aq1, (qlin, qln, qcache) = orc.featured_q(L.critic, "q1", L.norm, s, pi)
    if "actor" in masks:
        acache["mask"] = masks["actor"]
    if "aq" in masks:
        qcache["mask"] = masks["aq"]
    qabs = f32(np.mean(np.abs(aq1), dtype=np.float64))
    with np.errstate(divide="ignore"):
        lam = f32(alpha) / qabs                                   # no guard: 0 gives inf
    d = (pi - a.astype(f32)).astype(f32)
    bc_loss = float(np.mean(d.astype(np.float64) ** 2))
    actor_loss = -float(np.mean(aq1, dtype=np.float64))
    gq = np.full((B, 1), -1.0 / B, dtype=f32)
    _, gx = orc.mlp_backward(qlin, qln, qcache, gq)
    gpi_q = (lam * gx[:, s.shape[1]:]).astype(f32)
    gpi_bc = (f32(2.0 / (B * A)) * d).astype(f32)
    gpi = (gpi_q + gpi_bc).astype(f32)
    gz = (gpi * f32(L.max_action)) * (f32(1) - t * t)
    ag, _ = orc.mlp_backward(alin, aln, acache, gz.astype(f32))
    agrads = orc.pack_mlp_grads("", ag, L.norm, P=L.actor)
    rec.update(pi=pi, actor_q1=aq1, actor_loss=actor_loss, q_abs_mean=float(qabs), bc_loss=bc_loss,
               bc_actor_loss=float(lam) * actor_loss + bc_loss, gpi_q=gpi_q, gpi_bc=gpi_bc, actor_grads=agrads)
    rec["lambda"] = float(lam)
    return agrads


def term_shares(rec):
    """(Q term, BC term) of dL/dpi as shares of the total's L2 norm."""
    tot = np.linalg.norm((rec["gpi_q"] + rec["gpi_bc"]).astype(np.float64))
    return (float(np.linalg.norm(rec["gpi_q"].astype(np.float64)) / tot),
            float(np.linalg.norm(rec["gpi_bc"].astype(np.float64)) / tot))


def bc_featured_step(L, batch, noise, alpha, w=None, masks=None):
    """``orc.featured_train_step`` (TD3_featured.py:123-171) with the TD3+BC actor loss and optional
    per-row importance weights in the critic loss (per_reference.weighted_featured_step; the actor loss
    is not weighted).  ``alpha`` = 0 and ``w`` = None reproduce the oracle's step exactly."""
    masks = masks or {}
    rec = {}
    s, a, s2, r, nd = batch
    B = s.shape[0]
    L.total_it += 1
    eps = np.clip(noise.astype(f32) * f32(L.policy_noise), -f32(L.noise_clip), f32(L.noise_clip))
    ta, _ = orc.featured_actor(L.actor_target, L.norm, L.max_action, s2)
    next_a = np.clip(ta + eps, -f32(L.max_action), f32(L.max_action)).astype(f32)
    tq1, _ = orc.featured_q(L.critic_target, "q1", L.norm, s2, next_a)
    tq2, _ = orc.featured_q(L.critic_target, "q2", L.norm, s2, next_a)
    y = (r + (nd * f32(L.discount)) * np.minimum(tq1, tq2)).astype(f32)
    q1, c1 = orc.featured_q(L.critic, "q1", L.norm, s, a)
    q2, c2 = orc.featured_q(L.critic, "q2", L.norm, s, a)
    w64 = np.ones((B, 1)) if w is None else np.asarray(w, np.float64).reshape(B, 1)
    l1 = float(np.mean(w64 * (q1 - y).astype(np.float64) ** 2))
    l2 = float(np.mean(w64 * (q2 - y).astype(np.float64) ** 2))
    td_abs = 0.5 * (np.abs((q1 - y).astype(np.float64)) + np.abs((q2 - y).astype(np.float64)))
    rec.update(ta_out=ta, next_action=next_a, y=y, q1=q1, q2=q2, critic_loss=l1 + l2,
               critic_loss_parts=(l1, l2), td_abs=td_abs[:, 0])
    grads = {}
    for q, qv, (lin, ln, cache) in (("q1", q1, c1), ("q2", q2, c2)):
        if q in masks:
            cache["mask"] = masks[q]
        if w is None:
            gq = (f32(2.0 / B) * (qv - y)).astype(f32)
        else:
            gq = ((f32(2.0 / B) * np.asarray(w, f32).reshape(B, 1)) * (qv - y)).astype(f32)
        g, _ = orc.mlp_backward(lin, ln, cache, gq)
        grads.update(orc.pack_mlp_grads(f"{q}.", g, L.norm, P=L.critic))
    rec["critic_grads"] = grads
    L.adam_critic(grads)
    if L.total_it % L.policy_freq == 0:
        L.adam_actor(bc_actor_grads(L, s, a, alpha, rec, masks))
        L.polyak()
    return rec
