"""numpy references of prioritized replay (include/td3.h): the draw, the importance weights, the
priority of a TD error, and the weighted TD3 step rebuilt from the oracle's public pieces."""
from __future__ import annotations

import numpy as np

from helpers import featured_setup, featured_setup_dims, gen, orc

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


def edge_case(name, sd, ad, ma, norm, B, beta, seed, **other):
    """One case of the prioritized step for edge_setup / edge_step; ``other``: fill, actor_arch, q_arch, bc_alpha."""
    return dict(name=name, sd=sd, ad=ad, max_action=ma, norm=norm, B=B, beta=beta, seed=seed, **other)


# The prioritized featured step at the shapes where the planner (stages.hip, step.hip) takes another
# path; each name says which.  Optional keys: fill (rows written to the ring of gen.BUFFER_ROWS; default
# all of them), actor_arch / q_arch, bc_alpha.  The seed is part of the case: tests/test_per_reference.py
# holds, on the CPU, that its two steps spread the weights, draw rows twice where the case is there for
# that, and separate a step that ignored the weights.
EDGES = [
    edge_case("b1", 17, 6, 1.0, "layer", 1, 1.0, 1),                    # one row: w == 1.0; 31 pad rows
    edge_case("b33", 17, 6, 1.0, "layer", 33, 1.0, 34),                 # ragged, two row tiles
    edge_case("b257", 17, 6, 1.0, "layer", 257, 0.4, 257),              # ragged; beta != 1 through powf
    # dw64: seed 544 replaced.  Its step 2 has Q1 layer-1 z[11, 79] = z[187, 79] = 1.25e-9 (one ring row drawn
    # twice; float64, max |z| 2.8): the fp32 oracle's sum came out negative, the GPU's positive as in float64
    # (td3_debug_activation), and q1.linears.1.weight moved by 2.8e-2 of its scale in row 79 alone; on the
    # GPU's masks the oracle agreed within 5e-7.  The relu' ambiguity of tests/test_gpu_gradients.py, not
    # the weights.  Seed 548: no critic or actor pre-activation of either step below 2.9e-7 of its layer's max
    edge_case("dw64", 17, 6, 1.0, "layer", 544, 1.0, 548),              # dw64_kernel reads the weighted gscale
    edge_case("dwsk", 17, 6, 1.0, "layer", 640, 1.0, 640),              # split-K dwsk_kernel + combine
    edge_case("none", 17, 6, 1.0, None, 256, 1.0, 2),                   # no LN statistics, no kH0 store
    edge_case("wn", 17, 6, 1.0, "weight_normalization", 256, 1.0, 3),   # row-major kW0, g/v gradients
    edge_case("hum", 376, 17, 0.4, "layer", 128, 1.0, 128),             # separate gather, wide heads
    # hum1024: seed 1024 replaced.  Its step 2 has Q2 layer-2 z[66, 46] = z[791, 46] = 1.26e-7 (one ring row
    # drawn twice; float64, max |z| 2.7): the fp32 oracle took it as negative, the GPU as positive as in
    # float64, q2.linears.2.weight moved by 3.1e-3 of its scale in row 46 alone, and on the GPU's masks the
    # oracle agreed within 7e-7.  Seed 1037: no pre-activation below 5.1e-7 of its layer's max
    edge_case("hum1024", 376, 17, 0.4, "layer", 1024, 0.4, 1037),       # the product's learner
    edge_case("rec139", 60, 17, 2.0, "layer", 100, 1.0, 139),           # record of 139 floats, max_action 2
    edge_case("a32", 9, 32, 0.5, "layer", 64, 1.0, 32),                 # widest head
    edge_case("a1", 3, 1, 2.0, "layer", 33, 1.0, 4),                    # narrowest record and head
    edge_case("in512", 480, 32, 0.4, "layer", 64, 1.0, 512, fill=300),  # widest network input
    edge_case("odd", 11, 3, 1.0, "layer", 96, 1.0, 96, actor_arch=(64, 48, 40), q_arch=(96, 72, 33)),
    edge_case("part", 17, 6, 1.0, "layer", 100, 1.0, 300, fill=300),    # leaves >= 300 stay 0, never drawn
    edge_case("bc17", 40, 17, 2.0, "layer", 100, 1.0, 17, bc_alpha=2.5),    # BC's wide head, weighted step
    edge_case("bc1000", 17, 6, 1.0, "layer", 1000, 1.0, 1000, bc_alpha=2.5),  # BC's 2nd lambda trip + dw64/split-K
]


def edge_fill(case):
    return case.get("fill", gen.BUFFER_ROWS)


def edge_setup(case):
    """The setup dict (helpers.featured_setup_dims) of one EDGES case, plus ``fill``, ``actor_arch`` and
    ``q_arch``: parameters of custom widths are drawn as tests/test_gpu_edges._setup draws them, and with
    ``fill`` the oracle buffer holds only the first ``fill`` rows of the ring's data."""
    sd, ad, ma, norm = case["sd"], case["ad"], case["max_action"], case["norm"]
    S = featured_setup_dims(sd, ad, ma, norm, case["B"])
    S["actor_arch"] = tuple(case.get("actor_arch", gen.ACTOR_ARCH))
    S["q_arch"] = tuple(case.get("q_arch", gen.Q_ARCH))
    if "actor_arch" in case or "q_arch" in case:
        S["actor"] = gen.init_params(gen._mlp_shapes("", sd, S["actor_arch"], ad, norm), gen.SEED)
        S["critic"] = gen.init_params(gen._mlp_shapes("q1.", sd + ad, S["q_arch"], 1, norm) +
                                      gen._mlp_shapes("q2.", sd + ad, S["q_arch"], 1, norm), gen.SEED + 100)
    S["fill"] = fill = edge_fill(case)
    if fill != gen.BUFFER_ROWS:
        buf = orc.FeaturedBuffer(sd, ad, gen.BUFFER_ROWS)
        s, a, s2, r, d = gen.fill_featured_buffer(sd, ad, ma, gen.BUFFER_ROWS, gen.SEED)
        for i in range(fill):
            buf.add(s[i], a[i], s2[i], r[i], d[i])
        S["buf"] = buf
    return S


def edge_step(case, S, step):
    """(p, u, noise) of one step of an EDGES case: ``fill`` integer priorities in [1, 15] (exact partial
    sums, as step_case), B mass fractions guarded against a mass that reaches the total, the N(0,1) target
    noise."""
    rs = np.random.RandomState(case["seed"] + 100 * step)
    p = rs.randint(1, 16, size=S["fill"]).astype(f32)
    u = rs.uniform(size=S["B"]).astype(f32)
    u = np.where((u * f32(p.sum())).astype(f32) >= p.sum(), f32(0.5), u)
    noise = rs.standard_normal((S["B"], S["ad"])).astype(f32)
    return p, u, noise


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
