"""numpy reference of global-norm gradient clipping in the TD3 step (include/td3.h, "gradient clipping";
torch.nn.utils.clip_grad_norm_ with its defaults), composed with the oracle's steps and with the BC /
prioritized references, and the cases and schedules the clipping tests share.

    total = sqrt(sum over every parameter element of g^2)       (fp64)
    coef  = float32(min(1, max_norm / (total + 1e-6)))          (fp64 until the one rounding)
    Adam sees coef * g                                           (fp32)

Every step function of the oracle and of the references hands its gradients to ``L.adam_critic`` /
``L.adam_actor``: ``clipping`` puts the rule in front of those two for the duration of one step, so the
clipped step is the unclipped one with nothing else touched.
"""
from __future__ import annotations

import functools

import numpy as np

import bc_reference as bcr
import per_particles_reference as ppr
from helpers import featured_setup, gen, load_golden, orc

f32 = np.float32
GROUPS = ("actor", "critic")            # td3_set_grad_clip's group index
OPEN = 1.0e6                            # a threshold no gradient of these cases reaches: clipping on, coef 1
MOMENT_TOL = 2e-4                       # rel-to-max of an Adam exp_avg (tests/test_gpu_parity.py)
MOMENT_SQ_TOL = 2 * MOMENT_TOL          # exp_avg_sq: quadratic in the same gradient
GRAD_TOL = {"critic": 2e-4, "actor": 1e-4}      # a gradient tensor against its own scale
# grad_norm on the device against the oracle's norm, relative: 4x the worst ratio measured over the 90
# comparisons of tests/test_gpu_clip.py on the MI355X (2.96e-7, the actor of pend_layer under "half" at
# step 2; the critic's worst 1.87e-7 at sd 5, ad 1, B 33), far below the gradient contract's
# 2e-4: the norm averages the tensors' rounding differences, it does not add them.
NORM_TOL = 1.2e-6
PARAM_SHARE = 0.5                       # the share of elements clipping has to move in a parameter check
FEATURED_CASES = ("hc_layer", "hc_none", "pend_layer", "hum_layer", "hc_layer_b100")
SCHEDULES = ("first", "half")
STEPS = 4


def grad_norm(grads):
    """The total L2 norm of a gradient dict, every element widened and squared in fp64."""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads.values())))


def clip_coef(total, max_norm):
    """float32(min(1, max_norm / (total + 1e-6))) in fp64; a NaN passes through (torch.clamp)."""
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(total) + 1e-6)
    return f32(1.0) if c > 1.0 else f32(c)


class clipping:
    """Within the block ``L.adam_critic`` / ``L.adam_actor`` clip first.  ``max_norms`` = (actor, critic),
    each None / 0 (off), a float, or a callable total -> float (a threshold relative to the step's own
    norm); ``coefs`` ({group: float32}) teacher-forces the factor.  ``info[group]``: grad_norm, max_norm,
    coef of the group's last step in the block."""

    def __init__(self, L, max_norms, coefs=None):
        self.L, self.max_norms, self.coefs, self.info = L, dict(zip(GROUPS, max_norms)), coefs or {}, {}

    def _wrap(self, group, step):
        def clipped(grads):
            mn = self.max_norms[group]
            total = grad_norm(grads)
            mn = mn(total) if callable(mn) else mn
            if not mn:
                return step(grads)
            coef = f32(self.coefs[group]) if group in self.coefs else clip_coef(total, mn)
            self.info[group] = dict(grad_norm=total, max_norm=float(mn), coef=float(coef))
            return step({k: (coef * np.asarray(g, f32)).astype(f32) for k, g in grads.items()})
        return clipped

    def __enter__(self):
        self.L.adam_critic = self._wrap("critic", self.L.adam_critic)
        self.L.adam_actor = self._wrap("actor", self.L.adam_actor)
        return self

    def __exit__(self, *exc):
        del self.L.adam_critic, self.L.adam_actor          # back to the class's methods


def clipped_featured_step(L, batch, noise, max_norms, coefs=None, alpha=0.0, w=None, masks=None):
    """``orc.featured_train_step`` with clipping; ``alpha`` (TD3+BC) and ``w`` (importance weights of a
    prioritized step) compose it with ``bc_reference.bc_featured_step``.  rec["clip"]: ``clipping.info``."""
    with clipping(L, max_norms, coefs) as c:
        if not alpha and w is None:
            rec = orc.featured_train_step(L, batch, noise, masks=masks)
        else:
            rec = bcr.bc_featured_step(L, batch, noise, alpha, w=w, masks=masks)
    rec["clip"] = c.info
    return rec


def clipped_particle_step(L, batch, noise, max_norms, coefs=None, w=None):
    """``orc.particle_train_step`` with clipping; ``w`` composes it with the weighted particle step."""
    with clipping(L, max_norms, coefs) as c:
        rec = orc.particle_train_step(L, batch, noise) if w is None else ppr.weighted_particle_step(L, batch, noise, w)
    rec["clip"] = c.info
    return rec


def clipped_actor_learn(L, f, p, max_norm, coef=None):
    """``orc.particle_actor_learn`` with the actor's clipping."""
    with clipping(L, (max_norm, None), {} if coef is None else {"actor": coef}) as c:
        rec = orc.particle_actor_learn(L, f, p)
    rec["clip"] = c.info
    return rec


# ---------------------------------------------------------------- cases and schedules
@functools.lru_cache(maxsize=None)
def setup(name):
    return featured_setup(name)


def case_steps(name, n=STEPS):
    """[(rows, N(0,1) target noise)] of a golden configuration's n steps: its recorded draws, then seeded
    draws as ``bc_reference.case_steps`` makes them."""
    S, G = setup(name), load_golden("featured", name)
    out = [(G[f"step{k}/idx"], G[f"step{k}/noise"]) for k in range(1, min(S["steps"], n) + 1)]
    rs = np.random.RandomState(1000 * S["sd"] + 10 * S["ad"] + S["B"])
    while len(out) < n:
        out.append((rs.randint(0, gen.BUFFER_ROWS, size=S["B"]), rs.standard_normal((S["B"], S["ad"])).astype(f32)))
    return out


def factors(schedule, n=STEPS, policy_freq=2):
    """[(actor, critic)] per step, each the threshold as a multiple of that step's own norm or None (open).
    "first": the first optimizer step of each group clipped to 0.05x its norm, the later ones open -- a
    coefficient that varies between steps, which Adam cannot hide; "half": every step at 0.5x."""
    if schedule == "half":
        return [(0.5, 0.5)] * n
    assert schedule == "first", schedule
    return [(0.05 if t == policy_freq else None, 0.05 if t == 1 else None) for t in range(1, n + 1)]


def relative(fac):
    """``factors`` entries as ``clipping`` thresholds: a multiple of the step's own norm, or OPEN."""
    return tuple(OPEN if x is None else (lambda total, x=x: x * total) for x in fac)


@functools.lru_cache(maxsize=None)
def plan(name, schedule):
    """The oracle's own run of a case under a schedule: per step the absolute thresholds (actor, critic) the
    GPU run is given, the recorded norms and coefs, and the learner it ends in.  Run once, shared, read only."""
    S = setup(name)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    steps = []
    for (idx, noise), fac in zip(case_steps(name), factors(schedule, policy_freq=L.policy_freq)):
        rec = clipped_featured_step(L, S["buf"].gather(idx), noise, relative(fac))
        info = rec["clip"]
        steps.append(dict(max_norms=tuple(info[g]["max_norm"] if g in info else OPEN for g in GROUPS), clip=info))
    return dict(steps=steps, L=L)


@functools.lru_cache(maxsize=None)
def unclipped(name):
    S = setup(name)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for idx, noise in case_steps(name):
        orc.featured_train_step(L, S["buf"].gather(idx), noise)
    return L


def moved_share(name, schedule, group):
    """The share of a group's elements that differ between the clipped and the unclipped reference run by more
    than 10x the parameter tolerance 1e-6 + 1e-5|x|: what a learner that ignored max_norm would fail by."""
    a, b = getattr(plan(name, schedule)["L"], group), getattr(unclipped(name), group)
    moved = total = 0
    for k in b:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        moved += int((np.abs(x - y) > 10 * (1e-6 + 1e-5 * np.abs(y))).sum())
        total += y.size
    return moved / total


# (case, schedule, group) of the GPU parameter checks: tests/test_clip_reference.py holds each to
# PARAM_SHARE on the CPU.  The constant-coefficient schedule and the groups whose share falls short are
# checked through their gradients, norms, coefs and Adam moments only.
PARAM_CHECKS = [(name, "first", g) for name in FEATURED_CASES for g in ("critic", "actor")]


def edge_steps(S, particles=False):
    """The two steps of an edge setup (two critic steps, the second with the actor phase): seeded rows and
    noise."""
    A = S["A"] if particles else S["ad"]
    key = (1000 * S["F"] + 10 * A + S["B"]) if particles else (1000 * S["sd"] + 10 * A + S["B"])
    rs = np.random.RandomState(key)
    return [(rs.randint(0, gen.BUFFER_ROWS, size=S["B"]), rs.standard_normal((S["B"], A)).astype(f32))
            for _ in range(2)]
