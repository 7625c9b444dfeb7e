"""TD3+BC in the featured actor step (include/td3.h, "TD3+BC") against the numpy reference of
tests/bc_reference.py, teacher-forced from the oracle's state, and the rules around it: every path gives
the same bits, off is off, the other step entry points take it, the refusals.

Tolerances are the project's (tests/test_gpu_parity.py, restated by tests/test_gpu_prioritized_step.py):
forward values and the BC scalars rtol 1e-5; post-Adam parameters within 1e-6 + 1e-5|x| on >= 99.9 % of
the elements and within 2*lr everywhere; the actor's Adam exp_avg within 2e-4 of its max."""
import numpy as np
import pytest

import bc_reference as bcr
import per_reference as per
from helpers import featured_setup, featured_setup_dims, gen, orc, particle_setup, stage_kernels
from test_gpu_prioritized_step import (Box, _copy_state, _load_oracle_state, _make as _make_plain, _params_close,
                                       _rel_to_max, _set_all, _views)

pytestmark = pytest.mark.gpu

BC_KERNEL = "td3::row_bc_kernel"         # kRowActorHeadBwdBc (bc.hip)
PLAIN_KERNEL = "td3::row_kernel<3>"      # kRowActorHeadBwd


def _make(S, alpha, use_graph=True, prioritized=False):
    pol, rb = _make_plain(S, use_graph=use_graph, prioritized=prioritized)
    pol.bc_alpha = alpha
    return pol, rb


def _check_actor_step(out, rec, pol, L, lr, what):
    """The actor step's outputs, the four parameter groups and the actor's first moment."""
    sq, sb = bcr.term_shares(rec)
    assert sq >= bcr.MIN_SHARE and sb >= bcr.MIN_SHARE, (what, sq, sb)      # neither term is decoration
    for k in ("y", "q1", "q2"):
        assert _rel_to_max(out[k], rec[k][:, 0]) <= 1e-5, (what, k)
    np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
    np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["bc_lambda"], rec["lambda"], rtol=1e-5)
    np.testing.assert_allclose(out["bc_q_abs_mean"], rec["q_abs_mean"], rtol=1e-5)
    np.testing.assert_allclose(out["bc_loss"], rec["bc_loss"], rtol=1e-5)
    np.testing.assert_allclose(out["bc_actor_loss"], out["bc_lambda"] * out["actor_loss"] + out["bc_loss"], rtol=1e-12)
    _params_close(pol.critic.numpy_dict(), L.critic, lr, (what, "critic"))
    _params_close(pol.critic_target.numpy_dict(), L.critic_target, lr, (what, "critic_target"))
    _params_close(pol.actor.numpy_dict(), L.actor, lr, (what, "actor"))
    _params_close(pol.actor_target.numpy_dict(), L.actor_target, lr, (what, "actor_target"))
    sd = pol.actor_optimizer.state_dict()
    for i, k in enumerate(L.actor):
        assert _rel_to_max(sd["state"][i]["exp_avg"].numpy(), L.actor_m[k]) <= bcr.MOMENT_TOL, (what, k)


def _teacher_forced(S, alpha, name, what):
    """Two steps from the oracle's state (critic-only, then the actor phase), injected rows and noise:
    the two steps tests/test_bc_reference.py checked the term shares of."""
    pol, rb = _make(S, alpha)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    lr, B = S["kw"].get("lr", 1e-4), S["B"]
    for step, (idx, noise) in enumerate(bcr.case_steps(S, name), start=1):
        _load_oracle_state(pol, L)
        rec = bcr.bc_featured_step(L, S["buf"].gather(idx), noise, alpha)
        out = pol.train_step(rb, B, indices=idx, noise=noise, stats=True)
        assert out["actor_step"] == (step == 2)
        assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
        if step == 1:
            assert "bc_loss" not in out and pol.bc_info()["step"] == 0
    _check_actor_step(out, rec, pol, L, lr, what)
    info = pol.bc_info()
    assert info["enabled"] and info["alpha"] == alpha and info["step"] == 2
    assert (info["lambda"], info["q_abs_mean"], info["bc_loss"]) == (out["bc_lambda"], out["bc_q_abs_mean"], out["bc_loss"])
    return pol, rb


@pytest.mark.parametrize("name,alpha", bcr.CASES)
def test_bc_step_teacher_forced(name, alpha):
    S = featured_setup(name)
    pol, rb = _teacher_forced(S, alpha, name, what=name)
    if name == "hum_layer":               # A = 17: the separate gather, the transposed W1 copy, the wide head
        st = stage_kernels(pol, rb, S["B"], 1)
        assert st[0][1] == "td3::gather_kernel" and dict(st)["actor_head_bwd"] == BC_KERNEL, st
        assert pol._lib.td3_debug_row_lds() == 17 * (512 + 320) * 4     # the LDS-staged wide head


@pytest.mark.parametrize("case", bcr.EDGES, ids=lambda c: "sd%d_ad%d_B%d" % (c[0], c[1], c[4]))
def test_bc_step_edge_shapes(case):
    sd, ad, ma, norm, B, alpha = case
    _teacher_forced(featured_setup_dims(sd, ad, ma, norm, B), alpha, None, what=case)


def _four_steps(S, alpha, use_graph=True, inject=None):
    """Parameters, moments and bc_info after four steps (two actor phases); inject: [(idx, noise)]."""
    pol, rb = _make(S, alpha, use_graph=use_graph)
    drawn = []
    for t in range(4):
        if inject is None:
            out = pol.train_step(rb, S["B"], stats=True)
            drawn.append((out["idx"], out["noise"]))
        else:
            pol.train_step(rb, S["B"], indices=inject[t][0], noise=inject[t][1])
    pol.sync()
    return [v.flat() for v in _views(pol)], pol.bc_info(), drawn


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a[0], b[0])):
        np.testing.assert_array_equal(u, v, err_msg=f"{what}: group {i}")
    assert a[1] == b[1], (what, a[1], b[1])


@pytest.mark.parametrize("sd,ad,B", [(17, 6, 256), (40, 17, 100), (60, 17, 64)])
def test_graph_equals_eager_and_philox_equals_injected(sd, ad, B):
    S = featured_setup_dims(sd, ad, 1.0, "layer", B)
    g = _four_steps(S, 2.5, use_graph=True)
    e = _four_steps(S, 2.5, use_graph=False)
    assert g[1]["step"] == 4 and np.isfinite(g[1]["lambda"]) and g[1]["bc_loss"] > 0
    _same(g, e, "graph vs eager")
    # the sample inside the fused layer-0/1 launch (sd = 17), inside the stand-alone layer 0 (sd = 40) and
    # by the separate gather (sd = 60: a record of 139 floats) against the same rows injected: bit for bit,
    # as tests/test_gpu_philox_shapes.py holds the plain step
    _same(g, _four_steps(S, 2.5, use_graph=True, inject=g[2]), "Philox vs injected")


def _actor_head_lds(S):
    """Dynamic LDS bytes of the BC actor_head_bwd launch (td3_debug_row_lds): the last row launch of a
    directly launched actor phase; > 0 when its workgroups staged the head's weight rows."""
    pol, rb = _make(S, 2.5)
    st = stage_kernels(pol, rb, S["B"], 1)          # td3_profile_stages: direct launches
    rows = [n for n, k in st if k.startswith("td3::row_")]
    assert rows[-1] == "actor_head_bwd" and dict(st)["actor_head_bwd"] == BC_KERNEL, st
    return pol._lib.td3_debug_row_lds()


def test_wide_and_narrow_heads_agree(monkeypatch):
    S = featured_setup_dims(40, 17, 2.0, "layer", 100)
    monkeypatch.setenv("TD3_WIDE_HEADS", "1")       # read at each row-kernel launch
    a = _four_steps(S, 2.5)
    # the wide path is really taken: 17 rows of the transposed W1 copy (512 floats) and of W4 (320 floats)
    assert _actor_head_lds(S) == 17 * (512 + 320) * 4
    monkeypatch.setenv("TD3_WIDE_HEADS", "0")
    b = _four_steps(S, 2.5)
    assert _actor_head_lds(S) == 0
    _same(a, b, "wide vs block-by-block head")


def test_repeatable():
    S = featured_setup("hc_layer_b100")
    _same(_four_steps(S, 2.5), _four_steps(S, 2.5), "two runs")


@pytest.mark.parametrize("use_graph", [True, False])
def test_off_is_off(use_graph):
    """bc_alpha set and cleared against a learner never touched: the same stage lists, the same bits."""
    S = featured_setup("hc_layer")
    B = S["B"]
    a, rba = _make_plain(S, use_graph=use_graph, prioritized=False)
    b, rbb = _make_plain(S, use_graph=use_graph, prioritized=False)
    a.bc_alpha = 2.5
    a.train(rba, B)                                  # a plan built with BC on, then rebuilt without
    a.train(rba, B)
    assert a.bc_info()["step"] == 2
    a.bc_alpha = None
    assert a.bc_alpha is None and not a.bc_info()["enabled"] and a.bc_info()["step"] == 0
    _copy_state(b, a)
    for _ in range(4):
        a.train(rba, B)
        b.train(rbb, B)
    for va, vb in zip(_views(a), _views(b)):
        np.testing.assert_array_equal(va.flat(), vb.flat())
    lists = {}
    for phase in (0, 1):                             # a real step each: after the comparison
        lists[phase] = stage_kernels(a, rba, B, phase)
        assert lists[phase] == stage_kernels(b, rbb, B, phase), phase
    assert dict(lists[1])["actor_head_bwd"] == PLAIN_KERNEL
    # with BC on, the actor-phase list differs in the actor_head_bwd stage's kernel and nowhere else
    b.bc_alpha = 2.5
    assert stage_kernels(b, rbb, B, 0) == lists[0]
    on = stage_kernels(b, rbb, B, 1)
    assert [n for n, _ in on] == [n for n, _ in lists[1]]
    diff = [(n, k) for (n, k), (_, k0) in zip(on, lists[1]) if k != k0]
    assert diff == [("actor_head_bwd", BC_KERNEL)], diff
    assert b.bc_info()["step"] == b._counters()[0]   # the profiled step is a real BC step


def test_prioritized_step_with_bc():
    """One teacher-forced actor step on a prioritized draw: the weights touch only the critic."""
    name, alpha = "hc_layer", 2.5
    S, p, u, noise = per.step_case(name, 2)
    pol, rb = _make(S, alpha, prioritized=True)
    pol.per_beta = 1.0
    _set_all(rb, p)
    idx = per.draw(p, u)
    w = per.weights(p, idx, gen.BUFFER_ROWS, pol.per_beta)
    assert w.min() <= 0.2
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L.total_it = L.critic_step = 1                   # the next step runs the actor phase
    _load_oracle_state(pol, L)
    rec = bcr.bc_featured_step(L, S["buf"].gather(idx), noise, alpha, w=w)
    out = pol.train_step(rb, S["B"], noise=noise, stats=True, u=u)
    assert out["actor_step"]
    np.testing.assert_array_equal(out["idx"], idx)
    np.testing.assert_allclose(out["weight"], w, rtol=1e-5)
    _check_actor_step(out, rec, pol, L, S["kw"].get("lr", 1e-4), "prioritized")


class _Foreign:
    """A duck-typed buffer: ``sample`` returns the reference's tensors."""

    def __init__(self, *arrays):
        self.arrays = arrays

    def sample(self, B):
        return tuple(np.asarray(a[:B], np.float32) for a in self.arrays)


def test_foreign_batch_with_bc():
    S = featured_setup("hc_layer_b100")
    alpha, B = 2.5, S["B"]
    pol, _ = _make(S, alpha)
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], 128, gen.SEED)
    f32 = np.float32
    batch = (s[:B].astype(f32), a[:B].astype(f32), s2[:B].astype(f32), r[:B].astype(f32).reshape(B, 1),
             (1.0 - d[:B]).astype(f32).reshape(B, 1))
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L.total_it = L.critic_step = 1
    _load_oracle_state(pol, L)
    noise = np.random.RandomState(5).standard_normal((B, S["ad"])).astype(f32)
    rec = bcr.bc_featured_step(L, batch, noise, alpha)
    out = pol.train_step(_Foreign(s, a, s2, r, 1.0 - d), B, noise=noise, stats=True)   # td3_train_step_batch
    assert out["actor_step"]
    _check_actor_step(out, rec, pol, L, S["kw"].get("lr", 1e-4), "foreign batch")


def test_training_log_keeps_actor_loss():
    S = featured_setup("hc_layer_b100")
    pol, rb = _make(S, 2.5)
    log = pol.enable_train_log(capacity=4)
    outs = [pol.train_step(rb, S["B"], stats=True) for _ in range(2)]
    e = log.entries()
    assert len(e) == 2 and outs[1]["actor_step"]
    minus_mean_q = outs[1]["actor_loss"]             # -mean Q1(s, pi(s)) of the step (td3_step_stats)
    assert abs(e[1]["actor_loss"] - minus_mean_q) <= 4 * S["B"] * 2.0 ** -53 * abs(minus_mean_q)
    assert outs[1]["bc_actor_loss"] != minus_mean_q
    assert pol.bc_info()["step"] == int(e[1]["step"]) == 2


def test_refusals():
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    from td3_amd.TD3_particles import TD3 as TD3P
    S = featured_setup("hc_layer")
    pol, rb = _make_plain(S, prioritized=False)
    lib = pol._lib
    for alpha in (-0.5, float("nan")):
        assert lib.td3_set_bc(pol._h, alpha) == -1 and b"alpha" in lib.td3_last_error()
        with pytest.raises(TD3Error, match="alpha"):
            pol.bc_alpha = alpha
    assert pol.bc_alpha is None and not pol.bc_info()["enabled"]
    P = particle_setup("part_layer")
    polp = TD3P((Box((P["F"],)), Box((P["N"], P["D"]))), Box((P["A"],)), norm=P["norm"], CDQ=P["cdq"], init="none")
    assert lib.td3_set_bc(polp._h, 2.5) == -1 and b"particle learner has no BC step yet" in lib.td3_last_error()
    with pytest.raises(TD3Error, match="particle"):
        polp.bc_alpha = 2.5
    # a local data-parallel group, in both orders
    pols = [_make_plain(S, prioritized=False)[0] for _ in range(2)]
    local_group(pols)
    assert lib.td3_set_bc(pols[0]._h, 2.5) == -1 and b"data-parallel" in lib.td3_last_error()
    pols = [_make_plain(S, prioritized=False)[0] for _ in range(2)]
    pols[1].bc_alpha = 2.5
    with pytest.raises(TD3Error, match="BC"):
        local_group(pols)
    assert pol._counters() == (0, 0, 0)
    pol.train(rb, 32)                                # and the handle still steps
