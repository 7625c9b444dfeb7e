"""The training log on the device (include/td3.h "training log", td3_amd/train_log.py) against the numpy
restatement of tests/train_log_reference.py fed with the step's own ``stats`` arrays.

Every field that follows from y, Q1 and Q2 is held bit for bit (the restatement sums in the kernel's
order).  ``critic_loss`` is held to ``td3_step_stats.critic_loss`` within rtol 4 B 2^-53: both are fp64 sums
of the same B non-negative fp32 terms per critic in different orders, each within (B - 1) 2^-53 of the
exact sum, plus the roundings of two divisions and one add.  ``actor_loss`` is held to the stats value
within 4 B nq 2^-53 mean|Q|, with |actor_loss| <= mean|Q| standing in for the mean of values the host
never sees (a bound no wider than the one it replaces)."""
import ctypes as C

import numpy as np
import pytest

import per_particles_reference as ppr
import per_reference as per
import train_log_reference as ref
from helpers import featured_setup, featured_setup_dims, gen
from test_gpu_prioritized_particles import _policy as _particle_policy
from test_gpu_prioritized_particles import _ring as _particle_ring
from test_gpu_prioritized_step import _copy_state, _make, _set_all, _views

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _inputs(B, ad, steps, seed=3):
    rs = np.random.RandomState(seed)
    return [(rs.randint(0, gen.BUFFER_ROWS, size=B), rs.standard_normal((B, ad)).astype(np.float32))
            for _ in range(steps)]


def _check(e, out, B, nq, twin, step, prioritized=False):
    """One entry against the restatement on the step's stats and against the stats' own losses."""
    r = ref.entry(out["y"], out["q1"], out["q2"] if twin else None, w=out["weight"] if prioritized else None)
    for k in ref.FROM_Q + ("w_mean", "w_min"):
        assert e[k] == r[k], (step, k, e[k], r[k])
    assert (int(e["step"]), int(e["batch"]), int(e["actor_step"]), int(e["prioritized"])) == \
        (step, B, int(out["actor_step"]), int(prioritized))
    assert e["nonfinite"] == 0
    assert abs(e["critic_loss"] - out["critic_loss"]) <= 4 * B * U * abs(out["critic_loss"]), \
        (step, e["critic_loss"], out["critic_loss"])
    if out["actor_step"]:
        assert abs(e["actor_loss"] - out["actor_loss"]) <= 4 * B * nq * U * abs(out["actor_loss"]), \
            (step, e["actor_loss"], out["actor_loss"])
    else:
        assert np.isnan(e["actor_loss"])
    if not twin:
        assert e["q2_mean"] == e["q1_mean"] and e["q_gap_mean"] == 0.0


def _run_and_check(pol, rb, B, nq, twin, steps):
    log = pol.enable_train_log(capacity=8)
    assert pol.train_log is log and log.count == 0
    outs = [pol.train_step(rb, B, indices=ix, noise=nz, stats=True) for ix, nz in _inputs(B, pol.action_dim, steps)]
    e = log.entries()
    assert log.count == len(e) == steps
    assert [bool(o["actor_step"]) for o in outs] == [(t + 1) % 2 == 0 for t in range(steps)]
    for t, out in enumerate(outs):
        _check(e[t], out, B, nq, twin, t + 1)
    return e


@pytest.mark.parametrize("name", ["hc_layer", "hc_layer_b100"])
def test_parity_with_stats_featured(name):
    """B = 256 and B = 100 (Bp = 128: a pad row read by mistake would show)."""
    S = featured_setup(name)
    pol, rb = _make(S, prioritized=False)
    assert pol.train_log is None
    _run_and_check(pol, rb, S["B"], 1, True, 4)


@pytest.mark.parametrize("name", ["part_layer", "part_nocdq"])
def test_parity_with_stats_particles(name):
    """nq = A outputs per row at the 32-float row stride, with and without a twin."""
    S = ppr.setup(name)
    pol, rb = _particle_policy(S, per_beta=None), _particle_ring(S, prioritized=False)
    assert S["A"] > 1
    _run_and_check(pol, rb, S["B"], S["A"], bool(S["cdq"]), 4)


@pytest.mark.parametrize("B", [1, 257])
def test_edge_batches(B):
    """One row; and 257, where thread 0 owns two elements and every other thread one."""
    S = featured_setup_dims(3, 1, B=B)
    pol, rb = _make(S, prioritized=False)
    _run_and_check(pol, rb, B, 1, True, 2)


def test_log_does_not_disturb_the_step():
    """The production Philox path, with and without the log, direct launches and graph replay."""
    S = featured_setup("hc_layer")
    entries = []
    for use_graph in (False, True):
        a, rba = _make(S, use_graph=use_graph, prioritized=False)
        b, rbb = _make(S, use_graph=use_graph, prioritized=False)
        a.enable_train_log(capacity=16, every=1)
        for _ in range(6):
            a.train(rba, S["B"])
            b.train(rbb, S["B"])
        for va, vb in zip(_views(a), _views(b)):
            np.testing.assert_array_equal(va.flat(), vb.flat())
        assert a._counters() == b._counters() == (6, 6, 3)
        e = a.train_log.entries()
        assert list(e["step"]) == [1, 2, 3, 4, 5, 6] and list(e["actor_step"]) == [0, 1, 0, 1, 0, 1]
        assert np.isfinite(e["critic_loss"]).all() and (e["nonfinite"] == 0).all()
        entries.append(e.tobytes())
    assert entries[0] == entries[1]


def test_ring_every_and_rebuild():
    from td3_amd import _lib
    S = featured_setup("hc_layer")
    pol, rb = _make(S, prioritized=False)
    log = pol.enable_train_log(capacity=3)
    for _ in range(8):
        pol.train(rb, 64)
    out = (_lib.td3_log_entry * 100)()
    f, n = C.c_int64(), C.c_int64()
    _lib.check(pol._lib.td3_log_read(pol._h, 0, 100, out, C.byref(f), C.byref(n)), "td3_log_read")
    assert (f.value, n.value) == (5, 3) and [out[i].step for i in range(3)] == [6, 7, 8]
    assert log.read()[0] == 5 and list(log.entries()["step"]) == [6, 7, 8]
    assert log.read(6, 1)[0] == 6 and list(log.entries(6, 1)["step"]) == [7]
    assert len(log.entries(100, 5)) == 0 and len(log.entries(0, 0)) == 0
    inf = log.info()
    assert (inf.enabled, inf.capacity, inf.every, inf.count) == (1, 3, 1, 8)
    # every = 3 from total_it = 4: the steps that end at 6 and 9
    pol2, rb2 = _make(S, prioritized=False)
    pol2._set_counters(4, 4, 2)
    log2 = pol2.enable_train_log(capacity=8, every=3)
    for _ in range(6):
        pol2.train(rb2, 64)
    e = log2.entries()
    assert list(e["step"]) == [6, 9] and list(e["actor_step"]) == [1, 0] and log2.count == 2
    # the log outlives the plan: B = 100, then a rebuild at B = 256
    pol3, rb3 = _make(S, prioritized=False)
    log3 = pol3.enable_train_log(capacity=4)
    pol3.train(rb3, 100)
    pol3.train(rb3, 256)
    e = log3.entries()
    assert list(e["batch"]) == [100, 256] and list(e["step"]) == [1, 2]
    inf = _lib.td3_log_info_t()
    pol4, _ = _make(S, prioritized=False)
    _lib.check(pol4._lib.td3_log_info(pol4._h, C.byref(inf)), "td3_log_info")
    assert (inf.enabled, inf.capacity, inf.every, inf.count) == (0, 0, 0, 0)


@pytest.mark.parametrize("kind", ["featured", "particles"])
def test_prioritized_step_logs_its_weights(kind):
    if kind == "featured":
        S, p, u, noise = per.step_case("hc_layer", 1)
        pol, rb = _make(S)
        _, plain = _make(S, prioritized=False)
        nq, twin = 1, True
    else:
        S, p, u, noise = ppr.step_case("part_layer", 1)
        pol, rb = _particle_policy(S), _particle_ring(S)
        plain = _particle_ring(S, prioritized=False)
        nq, twin = S["A"], True
    pol.per_beta = 1.0
    _set_all(rb, p)
    log = pol.enable_train_log(capacity=4)
    out = pol.train_step(rb, S["B"], noise=noise, stats=True, u=u)
    assert out["weight"].min() < 0.5 and out["weight"].max() == 1.0
    out2 = pol.train_step(plain, S["B"], stats=True)               # a uniform step: unit weights again
    e = log.entries()
    _check(e[0], out, S["B"], nq, twin, 1, prioritized=True)
    assert e[0]["w_min"] == float(out["weight"].min()) and e[0]["w_mean"] < 1.0
    _check(e[1], out2, S["B"], nq, twin, 2)
    assert e[1]["prioritized"] == 0 and e[1]["w_mean"] == 1.0 and e[1]["w_min"] == 1.0


class _Foreign:
    """A duck-typed buffer: ``sample`` returns the reference's tensors."""

    def __init__(self, *arrays):
        self.arrays = arrays

    def sample(self, B):
        return tuple(np.asarray(a[:B], np.float32) for a in self.arrays)


def test_foreign_buffer_path_and_actor_learn():
    S = featured_setup("hc_layer_b100")
    pol, _ = _make(S, prioritized=False)
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], 128, gen.SEED)
    log = pol.enable_train_log(capacity=4)
    buf = _Foreign(s, a, s2, r, 1.0 - d)
    outs = [pol.train_step(buf, S["B"], stats=True) for _ in range(2)]       # td3_train_step_batch
    e = log.entries()
    assert len(e) == 2
    for t, out in enumerate(outs):
        _check(e[t], out, S["B"], 1, True, t + 1)
    P = ppr.setup("part_layer")
    polp = _particle_policy(P, per_beta=None)
    f, p, a, f2, p2, r, d = gen.fill_particle_buffer(P["F"], P["N"], P["D"], P["A"], 64, gen.SEED)
    logp = polp.enable_train_log(capacity=4)
    out = polp.train_step(_Foreign(f, p, a, f2, p2, r, 1.0 - d), P["B"], stats=True)   # td3_train_step_batch_particles
    polp._actor_learn(f[:P["B"]], p[:P["B"]])                     # no critic step: no entry
    polp.sync()
    e = logp.entries()
    assert logp.count == len(e) == 1
    _check(e[0], out, P["B"], P["A"], True, 1)
    assert polp._counters() == (1, 1, 1)


def test_checkpoint_round_trip(tmp_path):
    from td3_amd.train_log import summarize
    S = featured_setup("hc_layer")
    B = 64
    a, rba = _make(S, prioritized=False)
    la = a.enable_train_log(capacity=5)
    for _ in range(4):
        a.train(rba, B)
    path = str(tmp_path / "train_log.npz")
    la.save(path)
    sd = la.state_dict()
    assert int(sd["count"]) == 4 and list(sd["entries"]["step"]) == [1, 2, 3, 4]
    b, rbb = _make(S, prioritized=False)
    _copy_state(a, a)                                          # both learners take their state the same way
    _copy_state(a, b)
    lb = b.enable_train_log(capacity=5)
    lb.load(path)
    assert lb.count == 4 and lb.entries().tobytes() == la.entries().tobytes()
    for _ in range(3):
        a.train(rba, B)
        b.train(rbb, B)
    ea, eb = la.entries(), lb.entries()
    assert list(ea["step"]) == [3, 4, 5, 6, 7] and la.count == lb.count == 7
    assert ea.tobytes() == eb.tobytes()
    assert la.read()[0] == lb.read()[0] == 2
    # a log restored into a smaller ring keeps the newest entries, and no older slot shows
    c, _ = _make(S, prioritized=False)
    lc = c.enable_train_log(capacity=2)
    lc.load_state_dict(la.state_dict())
    assert lc.read()[0] == 5 and lc.entries().tobytes() == ea[-2:].tobytes()
    lc.load_state_dict({"entries": ea[-1:], "count": 7})
    assert lc.read()[0] == 6 and lc.entries().tobytes() == ea[-1:].tobytes()
    # summary: the same numbers from entries() with numpy
    s = la.summary()
    assert s == summarize(ea) and s["steps"] == 5 and (s["first_step"], s["last_step"]) == (3, 7)
    for k in ("critic_loss", "q1_mean", "q2_mean", "y_mean", "q_gap_mean", "td_abs_mean", "w_mean"):
        assert s[k] == float(np.mean(ea[k].astype(np.float64))), k
    assert s["actor_loss"] == float(np.mean(ea["actor_loss"][ea["actor_step"] != 0]))
    assert s["td_abs_max"] == float(ea["td_abs_max"].max()) and s["w_min"] == 1.0 and s["nonfinite"] == 0
    s2 = la.summary(last=2)
    assert (s2["steps"], s2["first_step"], s2["last_step"]) == (2, 6, 7)
    assert s2["critic_loss"] == float(np.mean(ea["critic_loss"][-2:]))


def test_refusals_leave_the_learner_usable():
    from td3_amd import _lib
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    S = featured_setup("hc_layer")
    pol, rb = _make(S, prioritized=False)
    lib = pol._lib
    out = (_lib.td3_log_entry * 2)()
    f, n = C.c_int64(), C.c_int64()
    assert lib.td3_log_read(pol._h, 0, 2, out, C.byref(f), C.byref(n)) == -1      # a read before enable
    assert b"not enabled" in lib.td3_last_error()
    assert lib.td3_log_set(pol._h, out, 1, 1) == -1
    assert b"not enabled" in lib.td3_last_error()
    log = pol.enable_train_log(capacity=2)
    with pytest.raises(TD3Error, match="already enabled"):
        pol.enable_train_log()
    assert pol.train_log is log
    big = (_lib.td3_log_entry * 3)()
    assert lib.td3_log_set(pol._h, big, 3, 3) == -1
    assert b"capacity" in lib.td3_last_error()
    other, _ = _make(S, prioritized=False)
    with pytest.raises(TD3Error, match="training log"):            # td3_comm_init_local on an enabled handle
        local_group([other, pol])
    pols = [_make(S, prioritized=False)[0] for _ in range(2)]
    local_group(pols)
    with pytest.raises(TD3Error, match="data-parallel"):           # enable on a replica
        pols[0].enable_train_log()
    assert pols[0].train_log is None
    for p in (pol, other):                                          # neither joined a group: both still step
        p.train(rb, 32)
        p.sync()
    assert pol._counters() == other._counters() == (1, 1, 0)
    assert log.count == 1 and list(log.entries()["step"]) == [1]
