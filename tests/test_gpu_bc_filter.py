"""The filtered BC term of the featured actor step (include/td3.h, "BC on the demonstration rows, Q-filter")
against the numpy reference of tests/bc_filter_reference.py, teacher-forced from the oracle's state, and the
rules around it: every launch path gives the same bits, n_demo changes without a new plan, the switches
reduce to plain TD3+BC and to the plain step bit for bit, the other step kinds take it, the refusals.

Every teacher-forced case is one tests/test_bc_filter_reference.py qualified on the CPU (the filter exactly
decided, rows on both sides of it, both terms of dL/dpi present), and checks those conditions again on the
very step it compares.  Tolerances are the project's, as tests/test_gpu_bc.py states them: forward values
and the BC scalars rtol 1e-5; post-Adam parameters within 1e-6 + 1e-5|x| on >= 99.9 % of the elements and
within 2*lr everywhere; the actor's Adam exp_avg within 2e-4 of its max.  kept and the rows' keep flags are
compared exactly."""
import ctypes as C

import numpy as np
import pytest

import bc_filter_reference as bfr
import bc_reference as bcr
import per_reference as per
from helpers import featured_setup, featured_setup_dims, gen, orc, particle_setup, stage_kernels
from test_gpu_mixed import _fixed
from test_gpu_prioritized_step import (Box, _copy_state, _load_oracle_state, _make as _make_plain, _params_close,
                                       _rel_to_max, _set_all, _views)

pytestmark = pytest.mark.gpu

BCF_KERNEL = "td3::row_bcf_kernel"       # kRowActorHeadBwdBcF (bcf.hip)
BC_KERNEL = "td3::row_bc_kernel"         # kRowActorHeadBwdBc (bc.hip)
PLAIN_KERNEL = "td3::row_kernel<3>"      # kRowActorHeadBwd


def _switch(pol, mode):
    demo_rows, q_filter = bfr.MODES[mode] if mode else (0, 0)
    pol.bc_rows = "demo" if demo_rows else "all"
    pol.bc_q_filter = bool(q_filter)


def _make(S, alpha, mode, use_graph=True, prioritized=False):
    pol, rb = _make_plain(S, use_graph=use_graph, prioritized=prioritized)
    pol.bc_alpha = alpha
    _switch(pol, mode)
    return pol, rb


_RINGS = {}


def _rings(S, key):
    """The two rings of bfr.ring_indices, once per case (a step leaves a ring as it found it): the demo ring
    holds the case's buffer in order, the online ring holds it reversed."""
    if key not in _RINGS:
        from td3_amd.my_replay_buffer import MixedReplay, ReplayBuffer_featured
        data = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], gen.BUFFER_ROWS, gen.SEED)
        demo = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS, seed=11)
        demo.add_batch(*data)
        online = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS, seed=23)
        online.add_batch(*[np.ascontiguousarray(x[::-1]) for x in data])
        _RINGS[key] = MixedReplay(online, demo, 0.5)
    return _RINGS[key]


def _last_stages(pol):
    """[(stage name, kernel)] of the body the learner's last step ran (no step of its own)."""
    out = []
    while True:
        name = pol._lib.td3_debug_last_stage(pol._h, len(out), 0).decode()
        if not name:
            return out
        out.append((name, pol._lib.td3_debug_last_stage(pol._h, len(out), 1).decode()))


def _check_filtered_step(out, rec, pol, L, lr, n_demo, q_filter, what):
    """The actor step's outputs, the mask, the four parameter groups and the actor's first moment."""
    bfr.check_case(rec, n_demo, q_filter, what)          # the comparison means something on this very step
    for k in ("y", "q1", "q2"):
        assert _rel_to_max(out[k], rec[k][:, 0]) <= 1e-5, (what, k)
    np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
    np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["bc_lambda"], rec["lambda"], rtol=1e-5)
    np.testing.assert_allclose(out["bc_q_abs_mean"], rec["q_abs_mean"], rtol=1e-5)
    info = pol.bc_filter_info(keep=True)
    print(f"{what}: kept {info['kept']} of n_d {info['n_demo']} (reference {rec['kept']} of {rec['n_d']}), "
          f"bc_loss {info['bc_loss']:.6g} (reference {rec['bc_loss']:.6g})")
    assert info["step"] == pol._counters()[0] and info["n_demo"] == rec["n_d"] == out["bc_n_demo"]
    assert info["kept"] == rec["kept"] == out["bc_kept"], (what, info["kept"], rec["kept"])
    np.testing.assert_array_equal(info["keep"], rec["keep"], err_msg=f"{what}: keep")
    np.testing.assert_allclose(out["bc_loss"], rec["bc_loss"], rtol=1e-5)
    assert info["bc_loss"] == out["bc_loss"] == pol.bc_info()["bc_loss"]
    np.testing.assert_allclose(out["bc_actor_loss"], out["bc_lambda"] * out["actor_loss"] + out["bc_loss"], rtol=1e-12)
    _params_close(pol.critic.numpy_dict(), L.critic, lr, (what, "critic"))
    _params_close(pol.critic_target.numpy_dict(), L.critic_target, lr, (what, "critic_target"))
    _params_close(pol.actor.numpy_dict(), L.actor, lr, (what, "actor"))
    _params_close(pol.actor_target.numpy_dict(), L.actor_target, lr, (what, "actor_target"))
    sd = pol.actor_optimizer.state_dict()
    for i, k in enumerate(L.actor):
        assert _rel_to_max(sd["state"][i]["exp_avg"].numpy(), L.actor_m[k]) <= bcr.MOMENT_TOL, (what, k)


# ---------------------------------------------------------------- teacher-forced mixed steps
@pytest.mark.parametrize("p", bfr.tf_params(), ids=bfr.tf_id)
def test_mixed_step_teacher_forced(p):
    """Two mixed steps from the oracle's state (critic-only, then the actor phase), injected rows and noise."""
    case, n_demo, mode = p
    S, name, alpha = bfr.case_setup(case)
    demo_rows, q_filter = bfr.MODES[mode]
    what = bfr.tf_id(p)
    pol, rb = _make(S, alpha, mode)
    mix = _fixed(_rings(S, case), n_demo)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    lr, B = S["kw"].get("lr", 1e-4), S["B"]
    for step, (idx, noise) in enumerate(bcr.case_steps(S, name), start=1):
        _load_oracle_state(pol, L)
        rec = bfr.filtered_featured_step(L, S["buf"].gather(idx), noise, alpha, demo_rows, q_filter, n_demo)
        out = pol.train_step(mix, B, indices=bfr.ring_indices(idx, n_demo), noise=noise, stats=True)
        assert out["actor_step"] == (step == 2) and out["n_demo"] == n_demo
        assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)
        if step == 1:
            assert "bc_kept" not in out and pol.bc_filter_info()["step"] == 0
    _check_filtered_step(out, rec, pol, L, lr, n_demo, q_filter, what)
    assert dict(_last_stages(pol))["actor_head_bwd"] == BCF_KERNEL
    if case == "hum_layer" and mode == "both" and n_demo == B // 2:
        # A = 17: the separate gather of a plain step, the transposed W1 copy, the LDS-staged wide head
        st = stage_kernels(pol, rb, B, 1)
        assert st[0][1] == "td3::gather_kernel" and dict(st)["actor_head_bwd"] == BCF_KERNEL, st
        assert pol._lib.td3_debug_row_lds() == 17 * (512 + 320) * 4
        assert pol.bc_filter_info()["n_demo"] == B       # a profiled step draws from one ring: n_d = B


# ---------------------------------------------------------------- launch variants
def _four_steps(S, key, alpha, mode, nds, use_graph=True, inject=None):
    """Parameters, moments and the two actor steps' filter reports after four mixed steps whose n_demo is
    nds[t]; inject: [(idx, noise)].  The stage list of the two actor steps must be one list."""
    pol, _ = _make(S, alpha, mode, use_graph=use_graph)
    rings = _rings(S, key)
    drawn, infos, lists = [], [], []
    for t in range(4):
        mix = _fixed(rings, nds[t])
        if inject is None:
            out = pol.train_step(mix, S["B"], stats=True)
            drawn.append((out["idx"], out["noise"]))
        else:
            pol.train_step(mix, S["B"], indices=inject[t][0], noise=inject[t][1])
        if t % 2:
            info = pol.bc_filter_info(keep=True)
            assert info["step"] == t + 1 and info["n_demo"] == (nds[t] if bfr.MODES[mode][0] else S["B"])
            info["keep"] = tuple(info["keep"])
            infos.append(info)
            lists.append(_last_stages(pol))
        elif t:
            assert pol.bc_filter_info()["step"] == t     # no plan was rebuilt for the new n_demo
    assert lists[0] == lists[1] and dict(lists[0])["actor_head_bwd"] == BCF_KERNEL, lists
    pol.sync()
    return [v.flat() for v in _views(pol)], (infos, pol.bc_info()), drawn


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a[0], b[0])):
        np.testing.assert_array_equal(u, v, err_msg=f"{what}: group {i}")
    assert a[1] == b[1], (what, a[1], b[1])


def _nds(B):
    return [B // 2, B // 2, B // 3, B // 3]              # n_demo changes between the two actor steps


@pytest.mark.parametrize("sd,ad,B", [(17, 6, 256), (40, 17, 100)])
def test_graph_equals_eager_and_philox_equals_injected(sd, ad, B):
    S = featured_setup_dims(sd, ad, 1.0, "layer", B)
    key = (sd, ad, 1.0, "layer", B)
    g = _four_steps(S, key, 2.5, "both", _nds(B), use_graph=True)
    e = _four_steps(S, key, 2.5, "both", _nds(B), use_graph=False)
    infos = g[1][0]
    assert [i["n_demo"] for i in infos] == [B // 2, B // 3] and all(0 < i["kept"] < i["n_demo"] for i in infos)
    assert all(sum(i["keep"][i["n_demo"]:]) == 0 and sum(i["keep"]) == i["kept"] for i in infos)
    _same(g, e, "graph vs eager")
    _same(g, _four_steps(S, key, 2.5, "both", _nds(B), use_graph=True, inject=g[2]), "Philox vs injected")


def _actor_head_lds(S, mode):
    """Dynamic LDS bytes of the filtered actor_head_bwd launch (td3_debug_row_lds): the last row launch of
    a directly launched actor phase; > 0 when its workgroups staged the head's weight rows."""
    pol, rb = _make(S, 2.5, mode)
    st = stage_kernels(pol, rb, S["B"], 1)          # td3_profile_stages: direct launches
    rows = [n for n, k in st if k.startswith("td3::row_")]
    assert rows[-1] == "actor_head_bwd" and dict(st)["actor_head_bwd"] == BCF_KERNEL, st
    return pol._lib.td3_debug_row_lds()


def test_wide_and_narrow_heads_agree(monkeypatch):
    case = (40, 17, 2.0, "layer", 100)
    S = featured_setup_dims(*case)
    monkeypatch.setenv("TD3_WIDE_HEADS", "1")       # read at each row-kernel launch
    a = _four_steps(S, case, 2.5, "both", _nds(100))
    assert _actor_head_lds(S, "both") == 17 * (512 + 320) * 4
    monkeypatch.setenv("TD3_WIDE_HEADS", "0")
    b = _four_steps(S, case, 2.5, "both", _nds(100))
    assert _actor_head_lds(S, "both") == 0
    _same(a, b, "wide vs block-by-block head")


def test_repeatable():
    S = featured_setup("hc_layer_b100")
    a = _four_steps(S, "hc_layer_b100", 2.5, "both", _nds(100))
    _same(a, _four_steps(S, "hc_layer_b100", 2.5, "both", _nds(100)), "two runs")


# ---------------------------------------------------------------- reductions to existing behaviour
def _plain_steps(pol, rb, B, steps=4):
    for _ in range(steps):
        pol.train(rb, B)
    pol.sync()
    return [v.flat() for v in _views(pol)], pol.bc_info()


@pytest.mark.parametrize("use_graph", [True, False])
def test_demo_rows_on_a_one_ring_step_is_plain_bc(use_graph):
    S = featured_setup("hc_layer_b100")
    a, rba = _make(S, 2.5, "demo", use_graph=use_graph)
    b, rbb = _make(S, 2.5, None, use_graph=use_graph)
    ra, rb_ = _plain_steps(a, rba, S["B"]), _plain_steps(b, rbb, S["B"])
    _same(ra, rb_, "bc_rows='demo' on td3_train_step")
    info = a.bc_filter_info()
    assert info["step"] == 4 and info["n_demo"] == info["kept"] == S["B"] and info["bc_loss"] == ra[1]["bc_loss"] > 0
    assert dict(_last_stages(a))["actor_head_bwd"] == BCF_KERNEL
    assert dict(_last_stages(b))["actor_head_bwd"] == BC_KERNEL and b.bc_filter_info()["step"] == 0


@pytest.mark.parametrize("case", ["hc_layer_b100", (40, 17, 2.0, "layer", 100)], ids=bfr.case_id)
def test_demo_rows_on_an_all_demo_mixed_step_is_plain_bc(case):
    S, _, alpha = bfr.case_setup(case)
    B = S["B"]
    res = []
    for mode in ("demo", None):
        pol, _ = _make(S, alpha, mode)
        mix = _fixed(_rings(S, case), B)
        for _ in range(4):
            pol.train_step(mix, B)
        pol.sync()
        res.append(([v.flat() for v in _views(pol)], pol.bc_info()))
    _same(res[0], res[1], "bc_rows='demo' on a mixed step with n_demo = B")


@pytest.mark.parametrize("use_graph", [True, False])
def test_switches_cleared_is_a_learner_never_touched(use_graph):
    """Both switches set and cleared (BC on) against a learner that only ever had bc_alpha; then bc_alpha off
    against the plain kernel: the same stage lists, the same bits."""
    S = featured_setup("hc_layer")
    B = S["B"]
    a, rba = _make(S, 2.5, "both", use_graph=use_graph)
    b, rbb = _make(S, 2.5, None, use_graph=use_graph)
    a.train(rba, B)                                  # a plan built with the filtered kind, then rebuilt without
    a.train(rba, B)
    assert a.bc_filter_info()["step"] == 2 and 0 < a.bc_filter_info()["kept"] < B
    _switch(a, None)
    fi = a.bc_filter_info()
    assert a.bc_rows == "all" and a.bc_q_filter is False and not fi["demo_rows"] and not fi["q_filter"]
    assert fi["step"] == 0 and a.bc_info()["step"] == 0
    _copy_state(b, a)
    for _ in range(4):
        a.train(rba, B)
        b.train(rbb, B)
    for va, vb in zip(_views(a), _views(b)):
        np.testing.assert_array_equal(va.flat(), vb.flat())
    assert a.bc_info() == b.bc_info() and a.bc_filter_info()["step"] == 0
    for phase in (0, 1):                             # a real step each: after the comparison
        la = stage_kernels(a, rba, B, phase)
        assert la == stage_kernels(b, rbb, B, phase), phase
    assert dict(la)["actor_head_bwd"] == BC_KERNEL
    # with a switch on, the actor-phase list differs in the actor_head_bwd stage's kernel and nowhere else
    b.bc_q_filter = True
    on = stage_kernels(b, rbb, B, 1)
    assert [(n, k) for (n, k), (_, k0) in zip(on, la) if k != k0] == [("actor_head_bwd", BCF_KERNEL)]
    assert [n for n, _ in on] == [n for n, _ in la]
    b.bc_q_filter = False
    a.bc_alpha = b.bc_alpha = None
    assert dict(stage_kernels(a, rba, B, 1))["actor_head_bwd"] == PLAIN_KERNEL
    assert dict(stage_kernels(b, rbb, B, 1))["actor_head_bwd"] == PLAIN_KERNEL


def test_switches_without_bc_alpha_change_nothing():
    S = featured_setup("hc_layer")
    B = S["B"]
    a, rba = _make_plain(S, prioritized=False)
    b, rbb = _make_plain(S, prioritized=False)
    a.train(rba, B)
    b.train(rbb, B)
    _switch(a, "both")                               # between steps, BC off: stored, no plan rebuilt
    assert a.bc_filter_info() == {"demo_rows": True, "q_filter": True, "step": 0, "n_demo": 0, "kept": 0, "bc_loss": 0.0}
    for _ in range(3):
        a.train(rba, B)
        b.train(rbb, B)
    for va, vb in zip(_views(a), _views(b)):
        np.testing.assert_array_equal(va.flat(), vb.flat())
    for phase in (0, 1):
        la = stage_kernels(a, rba, B, phase)
        assert la == stage_kernels(b, rbb, B, phase), phase
    assert dict(la)["actor_head_bwd"] == PLAIN_KERNEL
    a.bc_alpha = 2.5                                 # and they take effect once BC is on
    assert dict(stage_kernels(a, rba, B, 1))["actor_head_bwd"] == BCF_KERNEL


# ---------------------------------------------------------------- the other step kinds
def test_prioritized_step_with_the_filter():
    """One teacher-forced actor step on a prioritized draw, n_d = B: the weights touch only the critic."""
    # (hc_layer_b100: at hc_layer this draw leaves a row 6.7e-5 of max |Q1| from the filter's edge, under
    # bfr.MIN_GAP; here the nearest is 2.1e-3)
    name, alpha = "hc_layer_b100", 2.5
    S, p, u, noise = per.step_case(name, 2)
    pol, rb = _make(S, alpha, "both", prioritized=True)
    pol.per_beta = 1.0
    _set_all(rb, p)
    idx = per.draw(p, u)
    w = per.weights(p, idx, gen.BUFFER_ROWS, pol.per_beta)
    assert w.min() <= 0.2
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L.total_it = L.critic_step = 1                   # the next step runs the actor phase
    _load_oracle_state(pol, L)
    rec = bfr.filtered_featured_step(L, S["buf"].gather(idx), noise, alpha, 1, 1, None, w=w)
    out = pol.train_step(rb, S["B"], noise=noise, stats=True, u=u)
    assert out["actor_step"]
    np.testing.assert_array_equal(out["idx"], idx)
    np.testing.assert_allclose(out["weight"], w, rtol=1e-5)
    _check_filtered_step(out, rec, pol, L, S["kw"].get("lr", 1e-4), None, 1, "prioritized")


class _Foreign:
    """A duck-typed buffer: ``sample`` returns the reference's tensors."""

    def __init__(self, *arrays):
        self.arrays = arrays

    def sample(self, B):
        return tuple(np.asarray(a[:B], np.float32) for a in self.arrays)


def test_foreign_batch_with_the_filter():
    S = featured_setup("hc_layer_b100")
    alpha, B = 2.5, S["B"]
    pol, _ = _make(S, alpha, "both")
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], 128, gen.SEED)
    f32 = np.float32
    batch = (s[:B].astype(f32), a[:B].astype(f32), s2[:B].astype(f32), r[:B].astype(f32).reshape(B, 1),
             (1.0 - d[:B]).astype(f32).reshape(B, 1))
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L.total_it = L.critic_step = 1
    _load_oracle_state(pol, L)
    # (seed 8: the nearest row is 7.2e-3 of max |Q1| from the filter's edge; seed 5 of tests/test_gpu_bc.py: 1.08e-4)
    noise = np.random.RandomState(8).standard_normal((B, S["ad"])).astype(f32)
    rec = bfr.filtered_featured_step(L, batch, noise, alpha, 1, 1, None)
    out = pol.train_step(_Foreign(s, a, s2, r, 1.0 - d), B, noise=noise, stats=True)   # td3_train_step_batch
    assert out["actor_step"]
    _check_filtered_step(out, rec, pol, L, S["kw"].get("lr", 1e-4), None, 1, "foreign batch")


# ---------------------------------------------------------------- refusals
def test_refusals_in_the_headers_order():
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    from td3_amd.TD3_featured import TD3
    from td3_amd.TD3_particles import TD3 as TD3P
    S = featured_setup("hc_layer")
    pol, rb = _make_plain(S, prioritized=False)
    lib = pol._lib
    P = particle_setup("part_layer")
    polp = TD3P((Box((P["F"],)), Box((P["N"], P["D"]))), Box((P["A"],)), norm=P["norm"], CDQ=P["cdq"], init="none")
    pols = [_make_plain(S, prioritized=False)[0] for _ in range(2)]
    local_group(pols)
    # a bad switch first, whatever the handle
    for h in (pol._h, None, polp._h, pols[0]._h):
        for sw in ((2, 0), (0, -1)):
            assert lib.td3_set_bc_filter(h, *sw) == -1 and b"0 or 1" in lib.td3_last_error()
    assert lib.td3_set_bc_filter(None, 1, 1) == -1 and b"null handle" in lib.td3_last_error()
    assert lib.td3_set_bc_filter(polp._h, 1, 0) == -1 and b"particle learner" in lib.td3_last_error()
    assert lib.td3_set_bc_filter(pols[0]._h, 0, 1) == -1 and b"data-parallel" in lib.td3_last_error()
    with pytest.raises(ValueError, match="bc_rows"):
        pol.bc_rows = "online"
    with pytest.raises(ValueError, match="bc_rows"):
        TD3(Box((S["sd"],)), Box((S["ad"],)), bc_rows="some", init="none")
    assert pol.bc_rows == "all" and pol.bc_q_filter is False
    fi = pol.bc_filter_info()
    assert not fi["demo_rows"] and not fi["q_filter"] and fi["step"] == 0
    assert lib.td3_bc_filter_keep(pol._h, (C.c_float * 4)(), 4) == -1
    assert b"no filtered BC step" in lib.td3_last_error()
    assert pol._counters() == (0, 0, 0)
    pol.train(rb, 32)                                # and the handle still steps
    # the constructor's keywords reach the handle
    q = TD3(Box((S["sd"],)), Box((S["ad"],)), init="none", bc_alpha=2.5, bc_rows="demo", bc_q_filter=True)
    assert q.bc_rows == "demo" and q.bc_q_filter is True
    fi = q.bc_filter_info()
    assert fi["demo_rows"] and fi["q_filter"]
