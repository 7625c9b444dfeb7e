"""Shared test helpers: golden loading, oracle driving, tolerance checks."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, GOLDEN):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen  # noqa: E402
from oracle import td3_oracle as orc  # noqa: E402

# Tolerances (fp32): forward values / losses rtol 1e-5 atol 1e-6,
# gradients rtol 1e-4 atol 1e-7, post-Adam params atol 2*lr on <=0.1% of elements.
FWD_RTOL, FWD_ATOL = 1e-5, 1e-6
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-7


def load_golden(kind, name):
    return dict(np.load(os.path.join(GOLDEN, f"{kind}_{name}.npz"), allow_pickle=False))


def featured_setup(name):
    sd, ad, ma, norm, B, steps, hp = gen.FEATURED_CONFIGS[name]
    return featured_setup_dims(sd, ad, ma, norm, B, steps, hp)


def featured_setup_dims(sd, ad, ma=1.0, norm="layer", B=256, steps=2, hp=None):
    """A featured setup of any state / action width (no golden fixture: oracle-only parity)."""
    hp = dict(hp or {})
    a0 = gen.init_params(gen.featured_actor_shapes(sd, ad, norm), gen.SEED)
    c0 = gen.init_params(gen.featured_critic_shapes(sd, ad, norm), gen.SEED + 100)
    buf = orc.FeaturedBuffer(sd, ad, gen.BUFFER_ROWS)
    s, a, s2, r, d = gen.fill_featured_buffer(sd, ad, ma, gen.BUFFER_ROWS, gen.SEED)
    for i in range(gen.BUFFER_ROWS):
        buf.add(s[i], a[i], s2[i], r[i], d[i])
    kw = dict(max_action=ma, norm=norm)
    kw.update(hp)
    return dict(sd=sd, ad=ad, ma=ma, norm=norm, B=B, steps=steps, hp=hp, actor=a0,
                critic=c0, buf=buf, kw=kw)


def particle_setup(name):
    Fd, N, D, A, norm, cdq, B, steps = gen.PARTICLE_CONFIGS[name]
    return particle_setup_dims(Fd, N, D, A, norm, cdq, B, steps)


def particle_setup_dims(Fd, N, D, A, norm="layer", cdq=True, B=32, steps=2, rows=gen.BUFFER_ROWS, data=None):
    """A particle setup of any shape (no golden fixture: oracle-only parity).  ``data`` (the seven
    arrays of ``gen.fill_particle_buffer``, ``rows`` of them) replaces the default ring rows; it is
    returned as ``S["data"]`` for the GPU ring (``test_gpu_particles._make(S, rows, data)``)."""
    a0 = gen.init_params(gen.particle_actor_shapes(Fd, D, A, norm), gen.SEED)
    c0 = gen.init_params(gen.particle_critic_shapes(Fd, D, A, norm, cdq), gen.SEED + 100)
    buf = orc.ParticleBuffer(Fd, N, D, A, rows)
    if data is None:
        data = gen.fill_particle_buffer(Fd, N, D, A, rows, gen.SEED)
    f, p, a, f2, p2, r, d = data
    for i in range(rows):
        buf.add((f[i], p[i]), a[i], (f2[i], p2[i]), r[i], d[i])
    return dict(F=Fd, N=N, D=D, A=A, norm=norm, cdq=cdq, B=B, steps=steps, actor=a0,
                critic=c0, buf=buf, kw=dict(norm=norm, cdq=cdq), rows=rows, data=data)


# The dyadic grid of tests/test_gpu_particle_edges.py: with particles on multiples of 1/8 in [-1, 1]
# and the encoder parameters below, every conv1 pre-activation is an odd multiple of 1/256
# (|z1| <= 8.5 at D <= 16) and every conv2 pre-activation an odd multiple of 1/8192 (|z2| < 545):
# every partial sum, in any order, is exact in fp32 (< 2^23 units) and no pre-activation is zero,
# so two correct fp32 implementations take the same relu' decisions in the encoder.
GRID_Z1_UNIT, GRID_Z2_UNIT = 1.0 / 256, 1.0 / 8192


def grid_particles(x):
    """Particle coordinates on multiples of 1/8 in [-1, 1]."""
    return np.round(np.clip(np.asarray(x, np.float64), -1.0, 1.0) * 8.0) / 8.0


def particle_grid_params(P, seed):
    """A copy of state dict ``P`` with every encoder's parameters redrawn on the dyadic grid:
    conv1.weight multiples of 1/16 in [-1/2, 1/2], conv1.bias odd multiples of 1/256 in (-1/2, 1/2),
    conv2.weight multiples of 1/16 in [-1/4, 1/4], conv2.bias odd multiples of 1/8192 in (-1/4, 1/4)."""
    rs = np.random.RandomState(seed)
    out = {k: v.copy() for k, v in P.items()}
    for k, v in out.items():
        if k.endswith("conv1.weight"):
            g = rs.randint(-8, 9, size=v.shape) / 16.0
        elif k.endswith("conv1.bias"):
            g = (2 * rs.randint(-64, 64, size=v.shape) + 1) / 256.0
        elif k.endswith("conv2.weight"):
            g = rs.randint(-4, 5, size=v.shape) / 16.0
        elif k.endswith("conv2.bias"):
            g = (2 * rs.randint(-1024, 1024, size=v.shape) + 1) / 8192.0
        else:
            continue
        out[k] = g.astype(np.float32)
    return out


def summary_close(arr, stats, samples, salt, rtol, atol, what=""):
    st, smp = gen.summarize(arr, salt=salt)
    np.testing.assert_allclose(smp, samples, rtol=rtol, atol=atol, err_msg=f"{what} samples")
    scale = max(1.0, abs(stats[0]))
    assert abs(st[0] - stats[0]) <= 1e-4 * scale + atol * np.asarray(arr).size ** 0.5, what
    np.testing.assert_allclose(st[1], stats[1], rtol=1e-4, atol=1e-10, err_msg=f"{what} sumsq")
    np.testing.assert_allclose(st[2], stats[2], rtol=1e-4, atol=atol, err_msg=f"{what} maxabs")


def params_close(P, golden, prefix, salt_base, atol, rtol=1e-5, frac_loose=1e-3, loose=2e-4):
    """Post-Adam parameter check: tight everywhere except a tiny loose fraction."""
    for i, (k, v) in enumerate(P.items()):
        st, smp = gen.summarize(v, salt=salt_base + i)
        ref = golden[f"{prefix}/{k}/samples"]
        err = np.abs(smp - ref)
        tol = atol + rtol * np.abs(ref)
        bad = err > tol
        assert bad.mean() <= frac_loose or bad.sum() <= 1, (prefix, k, bad.sum(), err.max())
        assert err.max() <= loose, (prefix, k, err.max())


def stage_kernels(pol, rb, B, actor_phase):
    """[(stage name, HIP kernel)] of the learner's plan for batch B and that phase, stage 0 the
    sample (td3_profile_stages: the production body, run once as a real step; GPU only)."""
    import ctypes as C
    from td3_amd import _lib
    ms = (C.c_float * 128)()
    n = C.c_int()
    _lib.check(pol._lib.td3_profile_stages(pol._h, rb.handle, B, actor_phase, ms, 128, C.byref(n)),
               "td3_profile_stages")
    return [(pol._lib.td3_stage_name(pol._h, i).decode(), pol._lib.td3_stage_kernel(pol._h, i).decode())
            for i in range(n.value)]


def dp_mean(grads, n):
    """The replicas' gradient dicts reduced as the product reduces them: summed in replica order
    (((g0 + g1) + g2) ..., as local_sum_kernel) and scaled by float32(1/n) (adam_flat_kernel's
    grad_scale)."""
    red = {}
    for name, g0 in grads[0].items():
        acc = np.asarray(g0, np.float32)
        for j in range(1, len(grads)):
            acc = (acc + np.asarray(grads[j][name], np.float32)).astype(np.float32)
        red[name] = (acc * np.float32(1.0 / n)).astype(np.float32)
    return red


def oracle_dp_step(L, batch, noise, n, step_fn=None, reduce=dp_mean):
    """The oracle's restatement of the product's data-parallel step: n Learner copies
    in lock-step (threads), replica k on rows [k*b, (k+1)*b) of the batch; each phase's gradients
    summed over replicas in replica order (((g0 + g1) + g2) ..., as local_sum_kernel) and scaled by
    float32(1/n) (adam_flat_kernel's grad_scale) before the oracle's own Adam + Polyak.  Returns
    replica 0's Learner (all replicas end identical).  Against this, the GPU data-parallel step
    differs only by the summation order inside each shard, as the single-device tests do.
    ``reduce`` (tests of the tests: a deliberately wrong reduction) replaces ``dp_mean``."""
    import copy
    import threading
    step_fn = step_fn or orc.featured_train_step
    B = batch[0].shape[0]
    b = B // n
    Ls = [copy.deepcopy(L) for _ in range(n)]
    bar = threading.Barrier(n)
    slots = [None] * n
    red = {}
    errs = []

    def hook_for(k):
        def hook(grads):
            slots[k] = grads
            bar.wait()
            if k == 0:
                red.clear()
                red.update(reduce(slots, n))
            bar.wait()
            return {name: v.copy() for name, v in red.items()}
        return hook

    def run(k):
        try:
            shard = tuple(x[k * b:(k + 1) * b] for x in batch)
            step_fn(Ls[k], shard, noise[k * b:(k + 1) * b], grad_hook=hook_for(k))
        except Exception as e:                      # pragma: no cover - surfaced below
            errs.append(e)
            bar.abort()

    ts = [threading.Thread(target=run, args=(k,)) for k in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    return Ls[0]


def oracle_dp_actor_phase(L0, s, n, critic, masks=None):
    """The actor phase of one data-parallel step restated by the oracle, TEACHER-FORCED from a given
    post-step critic (the GPU's): ``L0`` is the learner state before the step (its critic_target
    the pre-step target), ``critic`` the critic after the step's critic update.  Replica k's actor
    gradient on rows [k*b, (k+1)*b) of ``s`` (TD3_featured.py:159-161), summed in replica order and
    scaled by float32(1/n) as oracle_dp_step / adam_flat_kernel do, then the actor's Adam step and
    the Polyak update of both targets (:162-171).  Returns (learner, mean gradient): the actor phase
    no longer carries the critic's post-Adam rounding, so the actor is held to the single-device
    contracts (gradient 1e-4 of scale, parameters 99.9 %).  ``masks`` (per replica, nullable): the
    relu' masks {"actor": [...], "aq": [...]} of that replica's own forward (the GPU's, as
    tests/test_gpu_gradients.py uses them): at B = 8192 some pre-activation of the 4 M per layer lies
    within fp32 rounding of zero, and a flipped ReLU moves its row's whole gradient contribution."""
    import copy
    Lt = copy.deepcopy(L0)
    Lt.critic = {k: np.array(v, dtype=np.float32, copy=True) for k, v in critic.items()}
    b = s.shape[0] // n
    gs = [orc.featured_actor_grads(Lt, s[k * b:(k + 1) * b], masks=masks[k] if masks else None)
          for k in range(n)]
    red = dp_mean(gs, n)
    Lt.adam_actor({k: v.copy() for k, v in red.items()})
    Lt.polyak()
    return Lt, red


# ---------------------------------------------------------------- long-horizon drift
DRIFT_FLOOR = 1e-7            # absolute floor: a few fp32 ulps of the O(0.1) parameters


def drift_envelope(G):
    """Per-step envelope of the reference's own fp32 drift (tests/golden/make_drift.py): the max
    over every group and tensor of |theta_1thread - theta_t| (t = 2, 4, 8 threads, whole tensors),
    as a running max over the steps so far."""
    groups = ("actor", "critic", "actor_target", "critic_target")
    env = np.max([G[f"{g}/env"].max(axis=1) for g in groups], axis=0)
    return np.maximum.accumulate(env.astype(np.float64))


def drift_setup(name):
    """(kind, setup dict, batch, action width) of one drift configuration (gen.DRIFT_CONFIGS)."""
    kind, cfg = gen.DRIFT_CONFIGS[name]
    if kind == "featured":
        sd, ad, ma, norm, B = cfg
        return kind, featured_setup_dims(sd, ad, ma, norm, B), B, ad
    Fd, N, D, A, norm, cdq, B = cfg
    return kind, particle_setup_dims(Fd, N, D, A, norm, cdq, B), B, A


def drift_check(G, step, group, params, env):
    """max |theta - theta_ref| over the fixture's sampled positions of every tensor of `group`
    at `step`, and that value over the envelope (the contract is ratio <= 1)."""
    names = list(G[f"{group}/names"])
    assert names == list(params), (group, names[:3], list(params)[:3])
    if group.endswith("_target"):
        row = int(np.nonzero(G["target_steps"] == step)[0][0])
    else:
        row = step - 1
    worst = 0.0
    for i, k in enumerate(names):
        _, smp = gen.summarize_k(params[k], gen.DRIFT_SAMPLES, salt=i)
        ref = G[f"{group}/samples"][row, i, :smp.size]
        worst = max(worst, float(np.abs(smp.astype(np.float64) - ref).max()))
    return worst, worst / (env[step - 1] + DRIFT_FLOOR)
