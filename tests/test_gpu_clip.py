"""Global-norm gradient clipping in the TD3 step (include/td3.h, "gradient clipping") against the numpy
reference of tests/clip_reference.py, teacher-forced from the oracle's state, and the rules around it: every
path gives the same bits, off is off, the other step entry points take it, a new threshold rebuilds nothing,
the refusals.

Tolerances are the project's (tests/test_gpu_parity.py): forward values and losses rtol 1e-5; a gradient
tensor within 2e-4 (critic) / 1e-4 (actor, teacher-forced on the GPU's post-step critic and relu' masks as
tests/test_gpu_data_parallel.py) of its scale; post-Adam parameters within 1e-6 + 1e-5|x| on >= 99.9 % of the
elements and within 2*lr everywhere; exp_avg within 2e-4 of its max and exp_avg_sq within 4e-4 (quadratic in
the same gradient).  The reported norm equals the fp64 norm of the read-back arena to 1e-12 (the same fp64
sum up to order), coef is float32(min(1, max_norm / (grad_norm + 1e-6))) exactly, and the norm is within
clip_reference.NORM_TOL of the oracle's.

Adam hides a constant scale of the gradient (tests/test_clip_reference.py), so a parameter check alone
would pass a learner that ignored max_norm: every clipped step is therefore also held through its Adam
moments (exp_avg scales with coef, exp_avg_sq with coef^2), whose reference runs on the GPU's reported coef.
The particle learner's actor phase is teacher-forced on the GPU's post-step critic too (without a mask hook)."""
import copy

import numpy as np
import pytest

import bc_reference as bcr
import clip_reference as cr
import per_particles_reference as ppr
import per_reference as per
from helpers import featured_setup, featured_setup_dims, gen, orc, particle_setup_dims, stage_kernels
from test_gpu_prioritized_step import (_copy_state, _load_oracle_state, _make as _make_featured, _params_close,
                                       _rel_to_max, _set_all, _views)

pytestmark = pytest.mark.gpu

GNORM, CLIP_ADAM = "td3::grad_sqsum_kernel", "td3::adam_flat_clip_kernel"


def _make(S, max_grad_norm, use_graph=True, prioritized=False):
    pol, rb = _make_featured(S, use_graph=use_graph, prioritized=prioritized)
    pol.max_grad_norm = max_grad_norm
    return pol, rb


def _make_particles(S, max_grad_norm, use_graph=True):
    from test_gpu_particles import _make as mk
    pol, rb = mk(S, use_graph=use_graph)
    pol.max_grad_norm = max_grad_norm
    return pol, rb


def _grads(pol, group):
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    which, g = (_lib.TD3_ACTOR_GRAD, 0) if group == "actor" else (_lib.TD3_CRITIC_GRAD, 1)
    return _ParamView(pol, which, g).numpy_dict()


def _check_clip_report(pol, out, group, max_norm, what):
    """clip_info against the read-back arena and the rule, and the stats keys against clip_info."""
    info = pol.clip_info()[group]
    assert info["enabled"] and info["max_norm"] == max_norm and info["step"] == pol._counters()[0], (what, info)
    host = cr.grad_norm(_grads(pol, group))
    np.testing.assert_allclose(info["grad_norm"], host, rtol=1e-12, err_msg=str(what))
    assert info["coef"] == float(cr.clip_coef(info["grad_norm"], max_norm)), (what, info)
    if out is not None:
        assert (out[f"{group}_grad_norm"], out[f"{group}_clip_coef"]) == (info["grad_norm"], info["coef"]), what
    return info


def _check_grads_and_norm(pol, group, ref, info, tol, what):
    got = _grads(pol, group)
    assert sorted(got) == sorted(ref)
    for k, v in ref.items():
        assert _rel_to_max(got[k].reshape(np.shape(v)), v) <= tol, (what, group, k)
    ratio = abs(info["grad_norm"] - cr.grad_norm(ref)) / cr.grad_norm(ref)
    print(f"clip norm ratio {what} {group}: {ratio:.3e}")
    assert ratio <= cr.NORM_TOL, (what, group, ratio)


def _check_moments(pol, L, groups, what):
    for group in groups:
        sd = getattr(pol, f"{group}_optimizer").state_dict()["state"]
        m, v = getattr(L, f"{group}_m"), getattr(L, f"{group}_v")
        for i, k in enumerate(m):
            assert _rel_to_max(sd[i]["exp_avg"].numpy().reshape(m[k].shape), m[k]) <= cr.MOMENT_TOL, (what, group, k)
            assert _rel_to_max(sd[i]["exp_avg_sq"].numpy().reshape(v[k].shape), v[k]) <= cr.MOMENT_SQ_TOL, (what, group, k)


def _check_params(pol, L, what, groups=("critic", "critic_target", "actor", "actor_target")):
    for g in groups:
        _params_close(getattr(pol, g).numpy_dict(), getattr(L, g), L.lr, (what, g))


def _featured_step(pol, rb, L, S, idx, noise, max_norms, what, alpha=0.0):
    """One teacher-forced step: the GPU step from the oracle's state, then the reference on the GPU's coefs."""
    from test_gpu_gradients import _gpu_masks
    B = S["B"]
    _load_oracle_state(pol, L)
    L0 = copy.deepcopy(L)
    pol.max_grad_norm = max_norms
    out = pol.train_step(rb, B, indices=idx, noise=noise, stats=True)
    groups = ["critic"] + (["actor"] if out["actor_step"] else [])
    infos = {g: _check_clip_report(pol, out, g, max_norms[cr.GROUPS.index(g)], (what, g)) for g in groups}
    if not out["actor_step"]:
        assert "actor_grad_norm" not in out
    batch = S["buf"].gather(idx)
    rec = cr.clipped_featured_step(L, batch, noise, max_norms, coefs={g: np.float32(i["coef"]) for g, i in infos.items()},
                                   alpha=alpha)
    assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
    for k in ("y", "q1", "q2"):
        assert _rel_to_max(out[k], rec[k][:, 0]) <= 1e-5, (what, k)
    np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
    _check_grads_and_norm(pol, "critic", rec["critic_grads"], infos["critic"], cr.GRAD_TOL["critic"], what)
    Lt = None
    if out["actor_step"]:
        # the actor phase runs through the critic the step has just updated: its reference is the oracle's
        # actor phase from the GPU's own post-step critic and relu' masks (helpers.oracle_dp_actor_phase's
        # form), on the GPU's coef -- gradient, moments and parameters alike
        np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
        Lt = copy.deepcopy(L0)
        Lt.critic = {k: np.array(v, np.float32) for k, v in pol.critic.numpy_dict().items()}
        masks = {k: v for k, v in _gpu_masks(pol, B, True).items() if k in ("actor", "aq")}
        ref = bcr.bc_actor_grads(Lt, batch[0], batch[1], alpha, masks=masks)
        _check_grads_and_norm(pol, "actor", ref, infos["actor"], cr.GRAD_TOL["actor"], what)
        coef = np.float32(infos["actor"]["coef"])
        Lt.adam_actor({k: (coef * v).astype(np.float32) for k, v in ref.items()})
        Lt.polyak()
        _check_moments(pol, Lt, ["actor"], what)
    _check_moments(pol, L, ["critic"], what)
    return out, rec, infos, Lt


def _check_featured_params(pol, L, Lt, what):
    """critic and its target against the reference run; on an actor step the actor and its target against the
    teacher-forced actor phase."""
    _check_params(pol, L, what, groups=("critic", "critic_target"))
    if Lt is not None:
        _check_params(pol, Lt, what, groups=("actor", "actor_target"))


@pytest.mark.parametrize("schedule", cr.SCHEDULES)
@pytest.mark.parametrize("name", cr.FEATURED_CASES)
def test_clipped_step_teacher_forced(name, schedule):
    S = cr.setup(name)
    plan = cr.plan(name, schedule)["steps"]
    pol, rb = _make(S, plan[0]["max_norms"])
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    flags = None
    for step, ((idx, noise), p) in enumerate(zip(cr.case_steps(name), plan), start=1):
        out, rec, infos, Lt = _featured_step(pol, rb, L, S, idx, noise, p["max_norms"], (name, schedule, step))
        for g, i in infos.items():                   # the schedule really clips where it says, and only there
            assert (i["coef"] < 1.0) == (p["clip"][g]["coef"] < 1.0), (step, g, i)
            np.testing.assert_allclose(i["coef"], p["clip"][g]["coef"], rtol=1e-3)
        if (name, schedule, "critic") in cr.PARAM_CHECKS:
            _check_featured_params(pol, L, Lt, (name, schedule, step))
        f = _plan_flags(pol)                         # the thresholds changed between steps: nothing was rebuilt
        assert flags in (None, f)
        flags = f
    assert pol.clip_info()["actor"]["step"] == pol.clip_info()["critic"]["step"] == 4


def _plan_flags(pol):
    import ctypes as C
    f = C.c_int()
    assert pol._lib.td3_debug_plan_flags(pol._h, C.byref(f)) == 0
    return f.value


# (sd, ad, max_action, norm, B): the smallest arenas with a ragged batch; no norm; the separate layer 0 and
# the wide head; a ragged batch past 512; Humanoid's dims at B = 1024 (the split-K dW in gradient-only mode)
EDGES = [(5, 1, 2.0, "layer", 33), (11, 9, 1.0, None, 257), (40, 17, 2.0, "layer", 100), (17, 6, 1.0, "layer", 1000),
         (376, 17, 0.4, "layer", 1024)]


@pytest.mark.parametrize("case", EDGES, ids=lambda c: "sd%d_ad%d_B%d" % (c[0], c[1], c[4]))
def test_clipped_step_edge_shapes(case):
    """Two critic steps and one actor step, the first of each group clipped to 0.05x its norm."""
    S = featured_setup_dims(*case)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    ref = copy.deepcopy(L)                           # the thresholds: the oracle's own norms, run once
    steps = cr.edge_steps(S)
    norms = []
    for (idx, noise), fac in zip(steps, cr.factors("first")):
        norms.append(cr.clipped_featured_step(ref, S["buf"].gather(idx), noise, cr.relative(fac))["clip"])
    pol, rb = _make(S, (cr.OPEN, norms[0]["critic"]["max_norm"]))
    for step, ((idx, noise), n) in enumerate(zip(steps, norms), start=1):
        mn = tuple(n[g]["max_norm"] if g in n else cr.OPEN for g in cr.GROUPS)
        out, rec, infos, Lt = _featured_step(pol, rb, L, S, idx, noise, mn, (case, step))
        assert infos["critic"]["coef"] < 1.0 if step == 1 else infos["actor"]["coef"] < 1.0
        _check_featured_params(pol, L, Lt, (case, step))
    if case[4] == 1024:
        st = dict(stage_kernels(pol, rb, S["B"], 1))
        assert st["C_dw"].startswith("td3::dwsk_kernel") and st["A_gnorm"] == GNORM and st["C_adam"] == CLIP_ADAM, st


def _particle_step(pol, rb, L, S, idx, noise, max_norms, what):
    from test_gpu_parity import _load_oracle_state as load
    load(pol, L)
    L0 = copy.deepcopy(L)
    pol.max_grad_norm = max_norms
    out = pol.train_step(rb, S["B"], indices=idx, noise=noise, stats=True)
    groups = ["critic"] + (["actor"] if out["actor_step"] else [])
    infos = {g: _check_clip_report(pol, out, g, max_norms[cr.GROUPS.index(g)], (what, g)) for g in groups}
    batch = S["buf"].gather(idx)
    rec = cr.clipped_particle_step(L, batch, noise, max_norms,
                                   coefs={g: np.float32(i["coef"]) for g, i in infos.items()})
    assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
    assert _rel_to_max(out["y"], rec["y"]) <= 1e-5 and _rel_to_max(out["q1"], rec["q1"]) <= 1e-5, what
    np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
    _check_grads_and_norm(pol, "critic", rec["critic_grads"], infos["critic"], cr.GRAD_TOL["critic"], what)
    if out["actor_step"]:
        # the actor phase as the featured test holds it: the oracle's _actor_learn from the pre-step state with
        # the GPU's own post-step critic, on the GPU's coef -- gradient, norm, moments and parameters
        np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
        Lt = copy.deepcopy(L0)
        gpu = pol.critic.numpy_dict()
        Lt.critic = {k: np.array(gpu[k], np.float32).reshape(v.shape) for k, v in L0.critic.items()}
        trec = cr.clipped_actor_learn(Lt, batch[0], batch[1], max_norms[0], coef=np.float32(infos["actor"]["coef"]))
        _check_grads_and_norm(pol, "actor", trec["actor_grads"], infos["actor"], cr.GRAD_TOL["actor"], what)
        _check_moments(pol, Lt, ["actor"], what)
        _check_params(pol, Lt, what, groups=("actor", "actor_target"))
    _check_moments(pol, L, ["critic"], what)
    return out, rec, infos


# (F, N, D, A, norm, cdq, B): the goldens' dims at B = 20 (pad rows), the same without CDQ, and D = 5 at
# N = 33 (a D that is no multiple of 4)
PARTICLE_EDGES = [(7, 16, 9, 3, "layer", True, 20), (7, 16, 9, 3, "layer", False, 20), (7, 33, 5, 1, "layer", True, 20)]


@pytest.mark.parametrize("case", PARTICLE_EDGES, ids=lambda c: "N%d_D%d_A%d_cdq%d" % (c[1], c[2], c[3], c[5]))
def test_clipped_particle_step_edge_shapes(case):
    S = particle_setup_dims(*case)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    ref = copy.deepcopy(L)
    steps = cr.edge_steps(S, particles=True)
    norms = []
    for (idx, noise), fac in zip(steps, cr.factors("first")):
        norms.append(cr.clipped_particle_step(ref, S["buf"].gather(idx), noise, cr.relative(fac))["clip"])
    pol, rb = _make_particles(S, (cr.OPEN, norms[0]["critic"]["max_norm"]))
    for step, ((idx, noise), n) in enumerate(zip(steps, norms), start=1):
        mn = tuple(n[g]["max_norm"] if g in n else cr.OPEN for g in cr.GROUPS)
        out, rec, infos = _particle_step(pol, rb, L, S, idx, noise, mn, (case, step))
        assert infos["critic"]["coef"] < 1.0 if step == 1 else infos["actor"]["coef"] < 1.0
    _check_params(pol, L, case, groups=("critic", "critic_target"))
    names = [n for n, _ in stage_kernels(pol, rb, S["B"], 1)]
    for tag in ("C", "A"):                           # the encoders' gradients reach the arena ahead of the norm
        i = names.index(f"{tag}_enc_adam")
        assert names[i - 1:i + 3] == [f"{tag}_dw", f"{tag}_enc_adam", f"{tag}_gnorm", f"{tag}_adam"], names


def test_actor_learn_particles_clips_the_actor():
    S = particle_setup_dims(7, 16, 9, 3, B=20)
    pol, rb = _make_particles(S, (1.0, None))
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    f, p = S["buf"].gather(np.arange(20))[:2]
    probe = cr.clipped_actor_learn(copy.deepcopy(L), f, p, lambda total: 0.05 * total)["clip"]["actor"]
    pol.max_grad_norm = (probe["max_norm"], None)
    pol._actor_learn(f, p)
    info = _check_clip_report(pol, None, "actor", probe["max_norm"], "actor_learn")
    assert 0.04 < info["coef"] < 0.06 and not pol.clip_info()["critic"]["enabled"]
    rec = cr.clipped_actor_learn(L, f, p, probe["max_norm"], coef=np.float32(info["coef"]))
    _check_grads_and_norm(pol, "actor", rec["actor_grads"], info, cr.GRAD_TOL["actor"], "actor_learn")
    _check_moments(pol, L, ["actor"], "actor_learn")
    _check_params(pol, L, "actor_learn", groups=("actor", "actor_target", "critic_target"))


# ---------------------------------------------------------------- every path gives the same bits
def _four_steps(S, max_grad_norm, use_graph=True, inject=None):
    """Parameters, moments, G arenas and clip_info after four steps; inject: [(idx, noise)]."""
    pol, rb = _make(S, max_grad_norm, use_graph=use_graph)
    drawn = []
    for t in range(4):
        if inject is None:
            out = pol.train_step(rb, S["B"], stats=True)
            drawn.append((out["idx"], out["noise"]))
        else:
            pol.train_step(rb, S["B"], indices=inject[t][0], noise=inject[t][1])
    pol.sync()
    arrays = [v.flat() for v in _views(pol)]
    arrays += [np.concatenate([g.ravel() for g in _grads(pol, grp).values()]) for grp in cr.GROUPS]
    return arrays, pol.clip_info(), drawn


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a[0], b[0])):
        np.testing.assert_array_equal(u, v, err_msg=f"{what}: array {i}")
    assert a[1] == b[1], (what, a[1], b[1])


@pytest.mark.parametrize("sd,ad,B", [(17, 6, 256), (40, 17, 100), (60, 17, 64)])
def test_graph_equals_eager_and_philox_equals_injected(sd, ad, B):
    S = featured_setup_dims(sd, ad, 1.0, "layer", B)
    mn = (0.05, 0.5)                                 # below the norms of LayerNorm setups: both groups really clip
    g = _four_steps(S, mn, use_graph=True)
    e = _four_steps(S, mn, use_graph=False)
    for grp in cr.GROUPS:
        assert g[1][grp]["step"] == 4 and 0.0 < g[1][grp]["coef"] < 1.0, g[1]
    _same(g, e, "graph vs eager")
    _same(g, _four_steps(S, mn, use_graph=True, inject=g[2]), "Philox vs injected")
    _same(g, _four_steps(S, mn, use_graph=True), "two runs")


# ---------------------------------------------------------------- off is off
@pytest.mark.parametrize("use_graph", [True, False])
def test_off_is_off(use_graph):
    S = featured_setup("hc_layer")
    B = S["B"]
    a, rba = _make_featured(S, use_graph=use_graph, prioritized=False)
    b, rbb = _make_featured(S, use_graph=use_graph, prioritized=False)
    a.max_grad_norm = 1.0
    a.train(rba, B)                                  # a plan built with clipping on, then rebuilt without
    a.train(rba, B)
    assert a.clip_info()["actor"]["step"] == 2
    a.max_grad_norm = None
    ci = a.clip_info()
    assert a.max_grad_norm is None and not ci["actor"]["enabled"] and not ci["critic"]["enabled"]
    assert ci["critic"]["step"] == 0 and ci["critic"]["grad_norm"] == 0.0
    _copy_state(b, a)
    for _ in range(4):
        a.train(rba, B)
        b.train(rbb, B)
    for va, vb in zip(_views(a), _views(b)):
        np.testing.assert_array_equal(va.flat(), vb.flat())
    lists = {}
    for phase in (0, 1):
        lists[phase] = stage_kernels(a, rba, B, phase)
        assert lists[phase] == stage_kernels(b, rbb, B, phase), phase
        assert not any(k in (GNORM, CLIP_ADAM) for _, k in lists[phase])
    # only the critic clipping: its fused stage becomes three, the actor phase's own stages stay as they are
    b.max_grad_norm = (None, 1.0)
    for phase in (0, 1):
        on = stage_kernels(b, rbb, B, phase)
        i = [n for n, _ in on].index("C_dw")
        assert on[i + 1:i + 3] == [("C_gnorm", GNORM), ("C_adam", CLIP_ADAM)], on
        assert on[:i] == lists[phase][:i] and on[i + 3:] == lists[phase][i + 1:], (phase, on)
    assert b.clip_info()["critic"]["step"] == b._counters()[0]      # the profiled step is a real clipped step


# ---------------------------------------------------------------- the other entry points
def test_prioritized_featured_step_with_clipping():
    """The weights touch the critic loss: the norm is of the weighted gradient."""
    S, p, u, noise = per.step_case("hc_layer", 2)
    pol, rb = _make(S, (cr.OPEN, cr.OPEN), prioritized=True)
    pol.per_beta = 1.0
    _set_all(rb, p)
    idx = per.draw(p, u)
    w = per.weights(p, idx, gen.BUFFER_ROWS, pol.per_beta)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L.total_it = L.critic_step = 1                   # the next step runs the actor phase
    probe = cr.clipped_featured_step(copy.deepcopy(L), S["buf"].gather(idx), noise, cr.relative((0.05, 0.05)), w=w)
    mn = tuple(probe["clip"][g]["max_norm"] for g in cr.GROUPS)
    unweighted = orc.featured_train_step(copy.deepcopy(L), S["buf"].gather(idx), noise)["critic_grads"]
    assert abs(cr.grad_norm(unweighted) / probe["clip"]["critic"]["grad_norm"] - 1) > 0.05     # the weights show
    _load_oracle_state(pol, L)
    pol.max_grad_norm = mn
    out = pol.train_step(rb, S["B"], noise=noise, stats=True, u=u)
    assert out["actor_step"]
    np.testing.assert_array_equal(out["idx"], idx)
    infos = {g: _check_clip_report(pol, out, g, mn[i], ("per", g)) for i, g in enumerate(cr.GROUPS)}
    rec = cr.clipped_featured_step(L, S["buf"].gather(idx), noise, mn,
                                   coefs={g: np.float32(i["coef"]) for g, i in infos.items()}, w=w)
    np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
    _check_grads_and_norm(pol, "critic", rec["critic_grads"], infos["critic"], cr.GRAD_TOL["critic"], "per")
    assert 0.04 < infos["critic"]["coef"] < 0.06 and 0.04 < infos["actor"]["coef"] < 0.06
    _check_moments(pol, L, ["critic"], "per")
    _check_params(pol, L, "per", groups=("critic", "critic_target"))


def test_prioritized_particle_step_with_clipping():
    from test_gpu_prioritized_particles import _policy, _ring
    S, p, u, noise = ppr.step_case("b20", 1)
    pol, rb = _policy(S), _ring(S)
    _set_all(rb, p)
    idx = per.draw(p, u)
    w = per.weights(p, idx, gen.BUFFER_ROWS, pol.per_beta)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    probe = cr.clipped_particle_step(copy.deepcopy(L), S["buf"].gather(idx), noise, cr.relative((None, 0.05)), w=w)
    mn = (None, probe["clip"]["critic"]["max_norm"])
    pol.max_grad_norm = mn
    out = pol.train_step(rb, S["B"], noise=noise, stats=True, u=u)
    np.testing.assert_array_equal(out["idx"], idx)
    info = _check_clip_report(pol, out, "critic", mn[1], "per particles")
    rec = cr.clipped_particle_step(L, S["buf"].gather(idx), noise, mn, coefs={"critic": np.float32(info["coef"])}, w=w)
    np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
    _check_grads_and_norm(pol, "critic", rec["critic_grads"], info, cr.GRAD_TOL["critic"], "per particles")
    assert 0.04 < info["coef"] < 0.06
    _check_moments(pol, L, ["critic"], "per particles")
    _check_params(pol, L, "per particles", groups=("critic",))


class _Foreign:
    """A duck-typed buffer: ``sample`` returns the reference's tensors."""

    def __init__(self, *arrays):
        self.arrays = arrays

    def sample(self, B):
        return tuple(np.asarray(a[:B], np.float32) for a in self.arrays)


def test_foreign_batch_with_clipping():
    S = featured_setup("hc_layer_b100")
    B = S["B"]
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], 128, gen.SEED)
    f32 = np.float32
    batch = (s[:B].astype(f32), a[:B].astype(f32), s2[:B].astype(f32), r[:B].astype(f32).reshape(B, 1),
             (1.0 - d[:B]).astype(f32).reshape(B, 1))
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    noise = np.random.RandomState(5).standard_normal((B, S["ad"])).astype(f32)
    probe = cr.clipped_featured_step(copy.deepcopy(L), batch, noise, cr.relative((None, 0.05)))
    mn = (None, probe["clip"]["critic"]["max_norm"])
    pol, _ = _make(S, mn)
    out = pol.train_step(_Foreign(s, a, s2, r, 1.0 - d), B, noise=noise, stats=True)      # td3_train_step_batch
    info = _check_clip_report(pol, out, "critic", mn[1], "foreign")
    rec = cr.clipped_featured_step(L, batch, noise, mn, coefs={"critic": np.float32(info["coef"])})
    _check_grads_and_norm(pol, "critic", rec["critic_grads"], info, cr.GRAD_TOL["critic"], "foreign")
    assert 0.04 < info["coef"] < 0.06
    _check_moments(pol, L, ["critic"], "foreign")
    _check_params(pol, L, "foreign", groups=("critic",))


def test_bc_step_with_the_actors_clipping():
    """bc_alpha = 2.5 with the actor clipping: the norm is of the BC gradient."""
    name, alpha = "hc_layer", 2.5
    S = cr.setup(name)
    idx, noise = cr.case_steps(name)[1]
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L.total_it = L.critic_step = 1
    batch = S["buf"].gather(idx)
    probe = cr.clipped_featured_step(copy.deepcopy(L), batch, noise, cr.relative((0.05, None)), alpha=alpha)
    plain = cr.clipped_featured_step(copy.deepcopy(L), batch, noise, cr.relative((0.05, None)))
    assert abs(plain["clip"]["actor"]["grad_norm"] / probe["clip"]["actor"]["grad_norm"] - 1) > 0.05   # BC shows
    mn = (probe["clip"]["actor"]["max_norm"], cr.OPEN)
    pol, rb = _make(S, mn)
    pol.bc_alpha = alpha
    out, rec, infos, Lt = _featured_step(pol, rb, L, S, idx, noise, mn, "bc", alpha=alpha)
    assert out["actor_step"] and 0.04 < infos["actor"]["coef"] < 0.06 and infos["critic"]["coef"] == 1.0
    np.testing.assert_allclose(out["bc_lambda"], rec["lambda"], rtol=1e-5)
    _check_featured_params(pol, L, Lt, "bc")


def test_training_log_is_unchanged_by_clipping():
    """Thresholds no gradient reaches: the logged entries equal those of the same run without clipping, and
    the log launch still comes behind the body."""
    S = featured_setup("hc_layer_b100")
    logs = []
    for mn in (None, cr.OPEN):
        pol, rb = _make(S, mn)
        log = pol.enable_train_log(capacity=4)
        for idx, noise in cr.case_steps("hc_layer_b100", 2):
            pol.train_step(rb, S["B"], indices=idx, noise=noise)
        logs.append(log.entries())
        if mn:
            assert pol.clip_info()["critic"]["coef"] == 1.0 and pol.clip_info()["critic"]["step"] == 2
    assert len(logs[0]) == len(logs[1]) == 2
    # coef is exactly 1.0f and g * 1.0f == g; the flat Adam pass runs adam_regs, the arithmetic of the fused dW
    # epilogue: both steps' entries are the same bits, field by field (NaN actor_loss of step 1 included)
    assert logs[0].dtype.names == logs[1].dtype.names and len(logs[0].dtype.names) >= 19
    for name in logs[0].dtype.names:
        np.testing.assert_array_equal(logs[0][name], logs[1][name], err_msg=name)


# ---------------------------------------------------------------- no rebuild on a new threshold
def test_new_threshold_rebuilds_nothing():
    S = featured_setup("hc_layer_b100")
    pol, rb = _make(S, (cr.OPEN, cr.OPEN))
    B = S["B"]
    pol.train_step(rb, B)
    flags, lists = _plan_flags(pol), [stage_kernels(pol, rb, B, ph) for ph in (1, 0)]
    norm = pol.clip_info()["critic"]["grad_norm"]
    for frac in (0.5, 0.1):
        pol.max_grad_norm = (cr.OPEN, frac * norm)
        assert pol.max_grad_norm == (cr.OPEN, frac * norm)
        out = pol.train_step(rb, B, stats=True)
        info = pol.clip_info()["critic"]
        assert info["coef"] == float(cr.clip_coef(info["grad_norm"], frac * norm)) < 1.0
        assert out["critic_clip_coef"] == info["coef"]
    assert _plan_flags(pol) == flags
    assert [stage_kernels(pol, rb, B, ph) for ph in (1, 0)] == lists
    assert pol.clip_info()["critic"]["step"] == pol._counters()[0]      # nothing was forgotten on the way


# ---------------------------------------------------------------- refusals
def test_refusals():
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    S = featured_setup("hc_layer")
    pol, rb = _make_featured(S, prioritized=False)
    lib = pol._lib
    for bad in (-0.5, float("nan"), float("inf")):
        assert lib.td3_set_grad_clip(pol._h, 1, bad) == -1 and b"max_norm" in lib.td3_last_error()
        with pytest.raises(TD3Error, match="max_norm"):
            pol.max_grad_norm = bad
    assert lib.td3_set_grad_clip(pol._h, 2, 1.0) == -1 and b"group" in lib.td3_last_error()
    assert pol.max_grad_norm is None and not pol.clip_info()["critic"]["enabled"]
    # both groups or neither: a pair whose second value is refused leaves the first group as it was, and the
    # property keeps agreeing with the handle
    for before in (None, (0.5, 2.0)):
        pol.max_grad_norm = before
        with pytest.raises(TD3Error, match="max_norm"):
            pol.max_grad_norm = (1.0, -1.0)
        ci = pol.clip_info()
        assert pol.max_grad_norm == before
        assert (ci["actor"]["max_norm"], ci["critic"]["max_norm"]) == ((0.0, 0.0) if before is None else before)
    pol.max_grad_norm = None
    W = featured_setup("hc_wn")
    wn, _ = _make_featured(W, prioritized=False)
    assert lib.td3_set_grad_clip(wn._h, 1, 1.0) == -1 and b"weight-normalised" in lib.td3_last_error()
    with pytest.raises(TD3Error, match="norm"):
        wn.max_grad_norm = 1.0
    # a local data-parallel group, in both orders
    pols = [_make_featured(S, prioritized=False)[0] for _ in range(2)]
    local_group(pols)
    assert lib.td3_set_grad_clip(pols[0]._h, 0, 1.0) == -1 and b"data-parallel" in lib.td3_last_error()
    with pytest.raises(TD3Error, match="data-parallel"):
        pols[1].max_grad_norm = (None, 1.0)
    pols = [_make_featured(S, prioritized=False)[0] for _ in range(2)]
    pols[1].max_grad_norm = (None, 1.0)
    with pytest.raises(TD3Error, match="clipping"):
        local_group(pols)
    assert pol._counters() == (0, 0, 0)
    pol.train(rb, 32)                                # and the handle still steps
