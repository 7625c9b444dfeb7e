"""The data-parallel step (td3_comm_init_local groups, include/td3.h) at the planner's edge shapes: the
case table, each case's injected rows and noise, the arena sizes the sharded optimizer slices, and the
references of the CPU checks (tests/test_dp_reference.py).  The oracle side is helpers.oracle_dp_step /
oracle_dp_actor_phase and orc.featured_train_step on the global batch of n * b rows; nothing of the
step is restated here."""
from __future__ import annotations

import copy

import numpy as np

from helpers import dp_mean, featured_setup_dims, gen, oracle_dp_step, orc, particle_setup_dims

f32 = np.float32
MAX_REPLICAS = 8            # kMaxLocalReplicas


def edge_case(name, sd, ad, ma, norm, n, b, seed, **other):
    """One case for edge_setup / edge_step: ``n`` replicas of ``b`` rows each; ``other``: actor_arch, q_arch,
    env (the plan-build knobs of dp.hip), shards (the TD3_DP_SHARD values the case runs with)."""
    return dict(name=name, sd=sd, ad=ad, max_action=ma, norm=norm, n=n, b=b, seed=seed, **other)


# The data-parallel featured step at the shapes where the planner (stages.hip make_dw_work, dp.hip) takes
# another path; each name says which.  The seed is part of the case: tests/test_dp_reference.py holds, on
# the CPU, that a step which forgot the 1/n scale or the last shard is far outside the GPU tolerances and
# that no relu' of the fp32 oracle is ambiguous (its masks equal those of the float64 forward, and no
# pre-activation lies within RELU_MARGIN of zero).  A seed that had to change for that is recorded beside its case.
#
# Replica counts: the arenas at (17, 6) and (3, 1) hold 376512 and 666432 floats, both multiples of 12, so
# three (or six) slices of ceil(size / 4n) * 4 floats divide them exactly and no slice reaches the pad
# (test_dp_reference.test_odd_replica_counts_slice_into_the_pad).  The cases planned at n = 3 on those
# widths therefore run at n = 5 (8 floats past either arena) -- r5_b33, none, a1 -- or, where the case is
# there for its dW kernel and 5 x 576 rows would only cost time, at n = 2 (dwsk).  hum, a32 and part_r3
# keep n = 3: their arenas are no multiple of 12, and they carry the 1/3 scale.
EDGES = [
    edge_case("r2_b1", 17, 6, 1.0, "layer", 2, 1, 1),                     # one row per replica, 31 pad rows
    edge_case("r5_b33", 17, 6, 1.0, "layer", 5, 33, 33),                  # ragged, two row tiles; slice in the pad, 1/5
    # r7_b16: seed 16 replaced: its step 2 has a pre-activation at 1.3e-7 of its layer's max, inside RELU_MARGIN
    # (17: 1.2e-7; 18: 1.0e-7, and a dropped shard only 0.011 of scale away).  Seed 19: 9.7e-7
    edge_case("r7_b16", 17, 6, 1.0, "layer", 7, 16, 19),                  # most odd replicas; smallest row tile
    edge_case("dw64", 17, 6, 1.0, "layer", 2, 544, 544),                  # gradient-only dw64_kernel
    edge_case("dwsk", 17, 6, 1.0, "layer", 2, 576, 576),                  # gradient-only split-K + combine
    edge_case("none", 17, 6, 1.0, None, 5, 512, 512),                     # no LN problems in the split-K list, sharded
    edge_case("wn_sk", 17, 6, 1.0, "weight_normalization", 2, 512, 3, shards=("0",)),   # split-K dW -> sum -> wn_kernel
    edge_case("hum", 376, 17, 0.4, "layer", 3, 128, 128),                 # separate gather, wide heads
    edge_case("hum_buckets", 376, 17, 0.4, "layer", 2, 512, 1037, env={"TD3_DP_BUCKETS": "1"}, shards=("0",)),
    edge_case("rec139", 60, 17, 2.0, "layer", 2, 100, 139),               # record of 139 floats, max_action 2
    # a32: seed 32 replaced.  Its step 2 has the actor's layer-2 z[64, 84] = -2.4e-7 (replica 1's row 0; float64,
    # max |z| 2.36: 1.0e-7 of scale).  The fp32 oracle took it as negative, as float64 does, the GPU as positive,
    # and the actor's exp_avg of linears.2.weight stood 9.3e-3 of its scale from the oracle's while the actor
    # phase on the GPU's own masks agreed within 1e-4 (test_gpu_dp_edges.test_dp_step_edge_shapes[a32-*]).  The
    # relu' ambiguity of tests/test_gpu_gradients.py, which mask equality with float64 alone did not exclude:
    # RELU_MARGIN does (33: 2.1e-7).  Seed 34: no pre-activation below 3.9e-7 of its layer's max
    edge_case("a32", 9, 32, 0.5, "layer", 3, 64, 34),                     # widest head
    # a1: seed 4 replaced (a pre-activation of step 2 at 1.3e-7 of its layer's max).  Seed 5: 1.4e-6
    edge_case("a1", 3, 1, 2.0, "layer", 5, 33, 5),                        # narrowest record and head
    # in512: seed 512 replaced.  On its step 2 the TD errors of the last shard's 64 rows nearly cancel in
    # q2.linears.3.bias: a step that dropped that shard moved the tensor's exp_avg by 2.7e-4 of its scale,
    # next to the moment tolerance.  Seed 513: every tensor separates by more than 0.36
    edge_case("in512", 480, 32, 0.4, "layer", 2, 64, 513),                # widest network input
    edge_case("odd", 11, 3, 1.0, "layer", 5, 96, 96, actor_arch=(64, 48, 40), q_arch=(96, 72, 33)),
]

# The particle learner at the smallest shapes tests/test_gpu_dw_schedules.py uses (F, N, D, A)
PARTICLE_DIMS = (7, 16, 9, 3)
PARTICLE_EDGES = [
    dict(name="part_r3", dims=PARTICLE_DIMS, norm="layer", n=3, b=11, seed=311),     # ragged, slice in the pad, 1/3
    dict(name="part_r2", dims=PARTICLE_DIMS, norm="layer", n=2, b=32, seed=232),
]

BY_NAME = {c["name"]: c for c in EDGES + PARTICLE_EDGES}


def is_particles(case):
    return "dims" in case


def case_shards(case):
    """The TD3_DP_SHARD values a case runs with: sharded ("1") and all-reduce ("0") unless the case's
    schedule keeps the all-reduce whatever the knob says (weight normalization, the buckets)."""
    return tuple(case.get("shards", ("1", "0")))


def pad32(x):
    return (x + 31) // 32 * 32


def _mlp_floats(in_dim, arch, out_dim):
    """td3.hip layout_mlp for norm None / "layer": every Linear [pad32(out)][pad32(in)] + a bias of
    pad32(out), and three LayerNorm affine pairs (laid out whether or not the network has them)."""
    dims = (in_dim,) + tuple(arch) + (out_dim,)
    lin = sum(pad32(dims[i + 1]) * pad32(dims[i]) + pad32(dims[i + 1]) for i in range(4))
    return lin + sum(2 * pad32(d) for d in dims[1:4])


def arena_sizes(case):
    """(actor, critic) arena sizes in floats as td3_create lays them out (Group::size; td3.hip).  Weight
    normalization has another layout and no sharded step: not covered."""
    assert case["norm"] != "weight_normalization"
    if is_particles(case):
        F, _, D, A = case["dims"]
        enc = pad32(256 * D + 256 + 128 * 256 + 128)                   # encoder.h EncOff::size, padded to 32
        first = lambda in_dim: enc + 2 * pad32(in_dim)                 # noqa: E731  (+ lnorm1)
        actor = first(128 + F) + _mlp_floats(128 + F, gen.ACTOR_ARCH, A)
        critic = 2 * (first(128 + F + A) + _mlp_floats(128 + F + A, gen.QP_ARCH, A))
        return (actor + 63) // 64 * 64, (critic + 63) // 64 * 64
    sd, ad = case["sd"], case["ad"]
    return (_mlp_floats(sd, case.get("actor_arch", gen.ACTOR_ARCH), ad),
            2 * _mlp_floats(sd + ad, case.get("q_arch", gen.Q_ARCH), 1))


def shard_slice(size, n):
    """dp.hip shard_slice: the floats of one replica's slice of an arena of ``size``."""
    return (size + 4 * n - 1) // (4 * n) * 4


def edge_setup(case):
    """The setup dict of one case (helpers.featured_setup_dims / particle_setup_dims at B = n * b) plus
    ``actor_arch`` / ``q_arch``: parameters of custom widths are drawn as per_reference.edge_setup draws them."""
    n, b = case["n"], case["b"]
    if is_particles(case):
        return particle_setup_dims(*case["dims"], norm=case["norm"], B=n * b)
    sd, ad, ma, norm = case["sd"], case["ad"], case["max_action"], case["norm"]
    S = featured_setup_dims(sd, ad, ma, norm, n * b)
    S["actor_arch"] = tuple(case.get("actor_arch", gen.ACTOR_ARCH))
    S["q_arch"] = tuple(case.get("q_arch", gen.Q_ARCH))
    if "actor_arch" in case or "q_arch" in case:
        S["actor"] = gen.init_params(gen._mlp_shapes("", sd, S["actor_arch"], ad, norm), gen.SEED)
        S["critic"] = gen.init_params(gen._mlp_shapes("q1.", sd + ad, S["q_arch"], 1, norm) +
                                      gen._mlp_shapes("q2.", sd + ad, S["q_arch"], 1, norm), gen.SEED + 100)
    return S


def edge_step(case, S, step):
    """(idx [n, b], noise [n, b, ad]) of one step of a case: replica k's injected ring rows and its N(0,1)
    target noise; the global batch is their concatenation in replica order."""
    n, b = case["n"], case["b"]
    ad = S["A"] if is_particles(case) else S["ad"]
    rs = np.random.RandomState(case["seed"] + 100 * step)
    idx = rs.randint(0, gen.BUFFER_ROWS, size=(n, b))
    noise = rs.standard_normal((n, b, ad)).astype(f32)
    return idx, noise


# ---------------------------------------------------------------- deliberately wrong reductions
def sum_unscaled(grads, n):
    """A data-parallel step that sums but does not scale."""
    return dp_mean(grads, 1)


def drop_last(grads, n):
    """A step that drops the last replica's shard from the sum."""
    return dp_mean(grads[:n - 1], n)


VARIANTS = {"unscaled": sum_unscaled, "drop_last": drop_last}


def _adam_moment(m0, g):
    """exp_avg after one Adam step from m0 with gradient g (orc.adam_: m += (1 - beta1)(g - m))."""
    return {k: (m0[k] + f32(1 - 0.9) * (np.asarray(g[k], f32) - m0[k])).astype(f32) for k in m0}


def particle_variant_moments(L0, batch, noise, n, b, variant):
    """(critic exp_avg, actor exp_avg or None) of a wrong particle step from L0: the particle oracle has no
    gradient hook, and its losses are batch means, so the sum of the shard gradients is n times the
    global-batch gradient and the sum without the last shard (n - 1) / n times the gradient of the batch
    without its last b rows."""
    rows = n * b if variant == "unscaled" else (n - 1) * b
    scale = f32(n) if variant == "unscaled" else f32((n - 1) / n)
    Lv = copy.deepcopy(L0)
    rec = orc.particle_train_step(Lv, tuple(x[:rows] for x in batch), noise[:rows])
    cm = _adam_moment(L0.critic_m, {k: scale * v for k, v in rec["critic_grads"].items()})
    am = _adam_moment(L0.actor_m, {k: scale * v for k, v in rec["actor_grads"].items()}) \
        if "actor_grads" in rec else None
    return cm, am


# ---------------------------------------------------------------- relu' masks, fp32 and float64
class Float64Oracle:
    """The oracle's arithmetic in float64 while inside (it types every array through orc.f32)."""

    def __enter__(self):
        self.saved = orc.f32
        orc.f32 = np.float64
        return self

    def __exit__(self, *exc):
        orc.f32 = self.saved
        return False


def relu_preacts(L, critic_after, s, a, actor_step):
    """The pre-activations (one array per hidden layer) of the networks one step backpropagates through, in
    whatever precision orc.f32 is: Q1, Q2 on (s, a) with the pre-step critic; on a policy step the actor on s
    and Q1 on (s, pi(s)) with ``critic_after``, the critic the step has just updated.  Each is the oracle's
    own z = u W^T + b, formed again from the layer inputs its forward kept (the cache keeps max(z, 0))."""
    def z(lin, cache):
        return [(cache["u"][i] @ lin[i][0].T + lin[i][1][None, :]).astype(orc.f32) for i in range(3)]

    out = {}
    for q in ("q1", "q2"):
        _, (lin, _, cache) = orc.featured_q(L.critic, q, L.norm, s, a)
        out[q] = z(lin, cache)
    if actor_step:
        pi, (lin, _, cache, _) = orc.featured_actor(L.actor, L.norm, L.max_action, s)
        out["actor"] = z(lin, cache)
        _, (lin, _, cache) = orc.featured_q(critic_after, "q1", L.norm, s, pi)
        out["aq"] = z(lin, cache)
    return out


def _as64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


# A pre-activation this close to zero, relative to its layer's largest, may be decided either way by two
# correct fp32 implementations: 2 ulp of the layer's largest value.  The relu' flips met so far between the
# oracle and the GPU sat at 4e-10 and 5e-8 (per_reference.EDGES) and at 1.0e-7 (a32 below) of that scale.
RELU_MARGIN = 2.0 ** -22


def seed_sets_margin(case):
    """Whether a case's seed can move its smallest pre-activation away from zero: it picks the rows, so only
    while the global batch leaves most of the ring's gen.BUFFER_ROWS rows out.  The cases of 1024 rows and
    more draw nearly every ring row on every seed, and their smallest pre-activation belongs to the ring's
    data (dw64: 2e-8 ... 8e-8 of scale on seeds 544 ... 548; none: 1.8e-8 on each of 26 seeds): they hold
    mask equality with float64 only."""
    return 2 * case["n"] * case["b"] <= gen.BUFFER_ROWS


def relu_mask_flips(L0, critic_after, s, a, n, actor_step):
    """(flips, count, margin) of one step's relu' decisions, shard by shard (each replica's own forward):
    how many of the fp32 oracle's differ from the same forward in float64 from the same fp32 state, how
    many there are, and the smallest |z| of the float64 forward relative to its layer's largest."""
    b = s.shape[0] // n
    L64 = copy.copy(L0)
    L64.actor, L64.critic = _as64(L0.actor), _as64(L0.critic)
    after64 = _as64(critic_after)
    flips = total = 0
    margin = np.inf
    for k in range(n):
        sk, ak = s[k * b:(k + 1) * b], a[k * b:(k + 1) * b]
        z32 = relu_preacts(L0, critic_after, sk, ak, actor_step)
        with Float64Oracle():
            z64 = relu_preacts(L64, after64, sk.astype(np.float64), ak.astype(np.float64), actor_step)
        for name in z32:
            for x, y in zip(z32[name], z64[name]):
                flips += int(((x > 0) != (y > 0)).sum())
                total += x.size
                margin = min(margin, float(np.abs(y).min() / np.abs(y).max()))
    return flips, total, margin


# ---------------------------------------------------------------- one case's chain of reference steps
_last = {}


def edge_reference(case):
    """(S, steps) of a featured case: the setup and, for steps 1 and 2 (critic-only, policy), a dict of
    idx, noise, batch, L0 (the state before the step), Ldp (helpers.oracle_dp_step), L (the global-batch
    oracle after the step) and rec (its record).  The chain continues from the global-batch state, as
    the teacher-forced GPU tests do.  The last case asked for is kept: callers must leave it unchanged."""
    if _last.get("name") == case["name"]:
        return _last["value"]
    S = edge_setup(case)
    n = case["n"]
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    steps = []
    for step in (1, 2):
        idx, noise = edge_step(case, S, step)
        batch = S["buf"].gather(idx.reshape(-1))
        nz = noise.reshape(n * case["b"], -1)
        L0 = copy.deepcopy(L)
        Ldp = oracle_dp_step(L, batch, nz, n)
        rec = orc.featured_train_step(L, batch, nz)
        steps.append(dict(idx=idx, noise=noise, batch=batch, L0=L0, Ldp=Ldp, L=copy.deepcopy(L), rec=rec))
    _last.update(name=case["name"], value=(S, steps))
    return _last["value"]
