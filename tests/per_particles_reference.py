"""numpy reference of the particle learner's prioritized step (include/td3.h
td3_train_step_prioritized_particles): the weighted TD3_particles step rebuilt from the oracle's public
pieces, and the inputs of one teacher-forced step."""
from __future__ import annotations

import functools

import numpy as np

from helpers import gen, orc, particle_setup, particle_setup_dims

f32 = np.float32
CASES = ("part_layer", "part_nocdq", "part_none", "b20")


@functools.lru_cache(maxsize=None)
def setup(name):
    """The particle goldens' configurations, and their dims at B = 20 (pad rows: 20 of 32).  Built once
    and shared: the tests read it and copy what they change."""
    if name == "b20":
        return particle_setup_dims(7, 16, 9, 3, B=20)
    return particle_setup(name)


def td_abs_rows(qs, y):
    """1/(J*A) sum_j sum_o |Q_j - y| per row, float64."""
    A = y.shape[1]
    t = sum(np.abs((q - y).astype(np.float64)).sum(axis=1) for q in qs)
    return t / (len(qs) * A)


def weighted_particle_step(L, batch, noise, w):
    """``orc.particle_train_step`` (TD3_particles.py:167-224) with per-row importance weights in the
    critic loss: critic_loss = sum_j 1/(B*A) sum_r w_r sum_o (Q_j - y)^2, dL/dQ_j = 2/(B*A) w_r (Q_j - y),
    one weight per transition shared by its A outputs.  The actor loss is not weighted.  ``w`` = 1
    reproduces the oracle's step exactly."""
    rec = {}
    f, p, a, f2, p2, r, nd = batch
    B = f.shape[0]
    w = np.asarray(w, f32).reshape(B, 1)
    L.total_it += 1
    eps = np.clip(noise.astype(f32) * f32(L.policy_noise), -f32(L.noise_clip), f32(L.noise_clip))
    ta, _ = orc.particle_net(L.actor_target, "", L.norm, f2, p2, actor=True)
    next_a = (ta + eps).astype(f32)
    qs = ("q1", "q2") if L.cdq else ("q1",)
    tqs = [orc.particle_net(L.critic_target, f"{q}.", L.norm, f2, p2, next_a)[0] for q in qs]
    tq = np.minimum(tqs[0], tqs[1]) if L.cdq else tqs[0]
    y = (r + (nd * f32(L.discount)) * tq).astype(f32)
    grads = {}
    cur = []
    for q in qs:
        qv, c = orc.particle_net(L.critic, f"{q}.", L.norm, f, p, a)
        cur.append(qv)
        gq = ((f32(2.0 / qv.size) * w) * (qv - y)).astype(f32)
        g, _ = orc.particle_net_backward(L.norm, f"{q}.", c, gq)
        grads.update(g)
    w64 = w.astype(np.float64)
    losses = [float(np.mean(w64 * (qv - y).astype(np.float64) ** 2)) for qv in cur]
    rec.update(ta_out=ta, next_action=next_a, y=y, critic_loss=sum(losses), td_abs=td_abs_rows(cur, y))
    for j, qv in enumerate(cur):
        rec[f"q{j + 1}"] = qv
    grads = {k: grads[k] for k in L.critic}
    rec["critic_grads"] = grads
    L.adam_critic(grads)
    if L.total_it % L.policy_freq == 0:
        orc.particle_actor_learn(L, f, p, rec)
    return rec


def step_case(name, step):
    """Integer priorities in [1, 15] (exact partial sums: the draw is reproducible bit for bit; with
    beta = 1 the weights are p_min / p over the batch), mass fractions and target noise of one step."""
    S = setup(name)
    rs = np.random.RandomState(100 * step + S["B"] + 7)
    p = rs.randint(1, 16, size=gen.BUFFER_ROWS).astype(np.float32)
    u = rs.uniform(size=S["B"]).astype(np.float32)
    u = np.where((u * np.float32(p.sum())).astype(np.float32) >= p.sum(), np.float32(0.5), u)
    noise = rs.standard_normal((S["B"], S["A"])).astype(np.float32)
    return S, p, u, noise
