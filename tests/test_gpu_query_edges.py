"""The featured query path (select_action / eval_q, host and device: td3_amd/csrc/act.hip, kernels_query.h)
at the planner's edge shapes, against the float64 reference of tests/query_reference.py.

Every comparison is against ``forward64`` at 1e-5 of ``scale(case, head)`` (SURVEY §8c's forward
contract, relative to the largest reference value of the head over the case's whole pool;
tests/test_query_reference.py shows on the CPU that a correct fp32 implementation stays within a quarter
of it and that the modelled kernel errors exceed it a hundredfold).  The route a query takes is read
from ``td3_debug_query_route``, which asks the function the queries themselves dispatch on, and compared
with the hand-written expectation of the case table, so a test cannot pass on another kernel than the one
it is there for.

1. small queries (n = 1..4) of every case through the raw C ABI into NaN-guarded outputs: values, route,
   guards; Q on the pool's actions, not on the policy's output;
2. the launch chain (TD3_ACT1=0) at every one-launch case, held to the reference as well;
3. the stage routes (n = 5, 32, 33, 256, 257): values, guards, ``mapped`` up to 256 rows and ``device``
   beyond; the kernel lists are pinned to literals recorded from the first run on an MI355X and kept as a
   change detector (as tests/test_gpu_dw_schedules.py keeps its lists), not derived from anything;
4. history independence, bit for bit: n <= 4 queries share the 32-row plan and its scratch with n = 5..32;
5. the device queries (n = 1, 4, 33, 257) and the exploration epilogue at ad = 1 and ad = 32;
6. queries after a critic-only and a policy update at non-default widths, on the exported parameters;
7. td3_create's refusals for featured learners: ad = 33, pad32(sd + ad) > 512, a hidden width of 513 and
   of 0 (no existing test asserts these for a featured learner: tests/test_cabi.py tries ad = 40 only, on
   the CPU; tests/test_gpu_particle_edges.py part 3 covers the particle learner's).

Measured on an MI355X, worst |got - forward64| / scale(case, head) over the n of each route, as
action / Q1 / Q2 in units of 1e-7 (the bound is 100): every test prints its figures before it asserts.

    case      n <= 4 as planned          n <= 4, TD3_ACT1=0   n = 5 .. 257 (stages)   device queries
    min       act_kernel  1.8/4.6/1.3    1.8/4.6/1.3          5.2/6.6/3.8             5.2/6.6/3.8
    k32       act_kernel  5.1/1.0/1.0    3.9/1.8/2.8
    k33       act_kernel  3.1/1.6/2.1    5.3/1.2/1.3
    a17       act_kernel  2.9/1.9/0.5    3.6/1.9/1.5          6.3/4.9/4.9             6.3/4.9/4.9
    k64_a32   act_kernel  4.6/1.5/0.8    5.0/2.6/1.4
    k65       gemv x 3    4.3/1.4/1.3                         8.1/4.5/3.1             8.1/4.5/3.1
    s64       gemv x 3    1.1/1.2/0.9
    in512     gemv x 3    4.6/1.0/1.4                         9.1/4.9/3.9             9.0/4.9/3.9
    odd       act_kernel  2.9/1.0/1.3    3.1/2.3/1.9          5.8/4.8/4.1             5.8/4.8/4.1
    odd_none  act_kernel  0.7/0.9/0.5    0.7/0.8/0.4
    odd_wn    act_kernel  1.1/0.8/0.6    1.3/1.1/0.4          3.5/2.2/1.8             3.5/2.2/1.8
    one_wg    act_kernel  1.6/1.0/0.9    4.3/2.0/0.4
    grow      gemv01      3.3/2.4/1.9
    grow_q    gemv01      2.0/2.2/2.5
    wide      act_kernel  3.7/1.5/2.0    2.2/1.7/0.7
    w510      act_kernel  3.8/1.1/0.7    2.5/1.3/1.4          7.0/4.6/4.5             7.0/4.6/4.5

After a critic-only and a policy update (part 6): odd 3.7/3.5/3.3, odd_wn 2.1/1.5/1.5, a17 5.4/2.5/2.6.
The worst figure of the file is 9.1e-7 (in512, action, stages): a tenth of the bound, and within the
1.8e-6 the fp32 oracle itself shows against forward64 on the CPU.  With gemv_kernel's LayerNorm made to
divide by its row stride instead of K (mutation (a) of tests/query_reference.py, on a scratch build),
part 1 fails at k65, s64, in512, grow and grow_q -- the five cases whose route names gemv_kernel -- and
passes at the other eleven.
"""
import ctypes as C

import numpy as np
import pytest

import query_reference as qr
from helpers import gen

pytestmark = pytest.mark.gpu

GUARD = 64
TOL = qr.TOL
SMALL_N = (1, 2, 3, 4)
STAGE_N = (5, 32, 33, 256, 257)
STAGE_CASES = ("min", "a17", "k65", "odd", "odd_wn", "w510", "in512")
ONE_LAUNCH = tuple(k for k, c in qr.CASES.items() if "act_kernel" in c["route"]["act"])



def _k(*layers):
    """"td3::gemm_kernel<0, a, b>" per hidden layer, then the head: the kernels of one stage list."""
    return ",".join(f"td3::gemm_kernel<0, {a}, {b}>" for a, b in layers) + ",td3::head_kernel"


# The kernel lists of the stage routes (parts 3 and 5) as the first run on an MI355X reported them, per case
# and query: the lists of the plans of 32, 64, 256 and 288 rows (n = 5 and 32, 33, 256, 257; the device
# queries' plans of the same size launch the same kernels).  A change detector, not a derivation: the
# template arguments are gemm_kernel's <mode, wn, pro> as stages.hip names a stage's kernel.
_PLAIN = _k((4, 0), (0, 1), (0, 1))
_ODD = _k((4, 0), (4, 1), (4, 1))
_ODD_WN = _k((4, 0), (4, 0), (4, 0))
_TWIN = _k((4, 0), (1, 1), (0, 1))
_IN512 = _k((0, 0), (0, 1), (0, 1))
PLAN_ROWS = (32, 64, 256, 288)
STAGE_KERNELS = {
    "min": {"act": (_PLAIN, _PLAIN, _PLAIN, _PLAIN), "q": (_PLAIN, _PLAIN, _TWIN, _TWIN)},
    "a17": {"act": (_PLAIN, _PLAIN, _PLAIN, _PLAIN), "q": (_PLAIN, _PLAIN, _TWIN, _TWIN)},
    "k65": {"act": (_PLAIN, _PLAIN, _PLAIN, _PLAIN), "q": (_PLAIN, _PLAIN, _TWIN, _TWIN)},
    "odd": {"act": (_ODD, _ODD, _ODD, _ODD), "q": (_ODD, _ODD, _ODD, _ODD)},
    "odd_wn": {"act": (_ODD_WN, _ODD_WN, _ODD_WN, _ODD_WN), "q": (_ODD_WN, _ODD_WN, _ODD_WN, _ODD_WN)},
    "w510": {"act": (_PLAIN, _PLAIN, _PLAIN, _k((4, 0), (1, 1), (1, 1))),
             "q": (_PLAIN, _PLAIN, _k((4, 0), (2, 1), (2, 1)), _k((4, 0), (2, 1), (2, 1)))},
    "in512": {"act": (_IN512, _IN512, _IN512, _k((1, 0), (0, 1), (0, 1))),
              "q": (_IN512, _IN512, _k((2, 0), (1, 1), (0, 1)), _k((2, 0), (1, 1), (0, 1)))},
}


def _stage_kernels(case, which, n):
    return STAGE_KERNELS[case][which][PLAN_ROWS.index((n + 31) // 32 * 32)]


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _learner(case, weights=True):
    from td3_amd.TD3_featured import TD3
    c = qr.CASES[case]
    pol = TD3(Box((c["sd"],)), Box((c["ad"],)), max_action=c["ma"], norm=c["norm"], actor_arch=c["actor_arch"],
              q_arch=c["q_arch"], init="none")
    if weights:
        pol.set_weights(*qr.params(case))
    return pol


_learners = {}


def _shared(case):
    """One learner per case, built once: the tests that use it only query it."""
    if case not in _learners:
        _learners[case] = _learner(case)
    return _learners[case]


def _route(pol, n, q, device=False):
    from td3_amd import _lib
    buf = C.create_string_buffer(2048)
    _lib.check(pol._lib.td3_debug_query_route(pol._h, n, int(q), int(device), buf, 2048), "td3_debug_query_route")
    return buf.value.decode()


def _guarded(floats):
    from td3_amd import _lib
    buf = np.full(floats + 2 * GUARD, np.nan, np.float32)
    return buf, C.cast(C.c_void_p(buf.ctypes.data + 4 * GUARD), _lib._F)


def _guards_ok(buf, floats):
    return np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + floats:]).all()


def _select(pol, s, n):
    """td3_select_action of the first n rows of s through the raw ABI: [n][ad], guards checked."""
    from td3_amd import _lib
    st = np.ascontiguousarray(s[:n])
    buf, out = _guarded(n * pol.action_dim)
    _lib.check(pol._lib.td3_select_action(pol._h, _lib.fptr(st), out, n), "td3_select_action")
    assert _guards_ok(buf, n * pol.action_dim), "td3_select_action wrote outside [n][ad]"
    return buf[GUARD:GUARD + n * pol.action_dim].reshape(n, pol.action_dim).copy()


def _evalq(pol, s, a, n):
    """td3_eval_q of the first n (state, action) rows through the raw ABI: (Q1 [n], Q2 [n])."""
    from td3_amd import _lib
    st, ac = np.ascontiguousarray(s[:n]), np.ascontiguousarray(a[:n])
    buf, out = _guarded(2 * n)
    _lib.check(pol._lib.td3_eval_q(pol._h, _lib.fptr(st), _lib.fptr(ac), out, n), "td3_eval_q")
    assert _guards_ok(buf, 2 * n), "td3_eval_q wrote outside [2][n]"
    return buf[GUARD:GUARD + n].copy(), buf[GUARD + n:GUARD + 2 * n].copy()


def _errors(case, got, n, ref=None, scales=None):
    """|got - reference| of the first n pool rows per head, as fractions of scale."""
    ref = ref or qr.reference(case)
    out = []
    for head, g in zip(qr.HEADS, got):
        sc = scales[head] if scales else qr.scale(case, head)
        assert np.isfinite(g).all(), (case, head, n)
        out.append(float(np.abs(g.astype(np.float64) - ref[head][:n]).max() / sc))
    return out


def _query_host(pol, case, n):
    s, a = qr.pool(case)
    act = _select(pol, s, n)
    q1, q2 = _evalq(pol, s, a, n)
    return act, q1, q2


def _check(case, got, n, what):
    errs = _errors(case, got, n)
    print(f"{case} n={n} {what}: action {errs[0]:.2e} Q1 {errs[1]:.2e} Q2 {errs[2]:.2e} of scale")
    for head, e in zip(qr.HEADS, errs):
        assert e <= TOL, (case, n, what, head, e)


# ---------------------------------------------------------------- 1: small queries
_small = {}


def _run_small(case):
    """Part 1 of one case, memoised: {(n, which): route string}."""
    if case in _small:
        return _small[case]
    pol = _shared(case)
    routes = {}
    for n in SMALL_N:
        for which, q in (("act", False), ("q", True)):
            routes[(n, which)] = _route(pol, n, q)
            assert routes[(n, which)] == qr.expected_route(case, n, which), (case, n, which)
        _check(case, _query_host(pol, case, n), n, "small")
    _small[case] = routes
    return routes


@pytest.mark.parametrize("case", list(qr.CASES))
def test_small_queries(case):
    _run_small(case)


def test_small_queries_reach_every_route_and_instantiation():
    """Over the strings the small queries reported: the three n <= 4 routes, both KQ and R = 1, 2, 4."""
    seen = set()
    for case in qr.CASES:
        seen |= set(_run_small(case).values())
    names = {k for r in seen for k in r.split(",", 1)[1].replace(", ", " ").split(",")}
    for R in (1, 2, 4):
        for kq in (8, 16):
            assert f"td3::act_kernel<{R} {kq}>" in names, (R, kq)
        assert f"td3::gemv01_kernel<{R}>" in names and f"td3::gemv_kernel<{R}>" in names, R
    firsts = {r.split(",")[1].split("<")[0] for r in seen}
    assert firsts == {"td3::act_kernel", "td3::gemv01_kernel", "td3::gemv_kernel"}
    assert {r.split(",")[0] for r in seen} == {"args", "mapped"}
    assert any(r.startswith("mapped,") and r.count("td3::gemv_kernel") == 3 for r in seen)


# ---------------------------------------------------------------- 2: the launch chain
@pytest.mark.parametrize("case", ONE_LAUNCH)
def test_launch_chain_at_one_launch_cases(case, monkeypatch):
    """TD3_ACT1=0 (read when a query plan is built): the same shapes through gemv01 -> gemv -> head, held
    to the reference like the one-launch learner (part 1), not only to each other."""
    _run_small(case)
    monkeypatch.setenv("TD3_ACT1", "0")
    pol = _learner(case)
    for n in SMALL_N:
        R = qr.ROWS_OF_N[n]
        want = f"args,td3::gemv01_kernel<{R}>,td3::gemv_kernel<{R}>,td3::head_kernel"
        assert _route(pol, n, False) == want and _route(pol, n, True) == want, (case, n)
        _check(case, _query_host(pol, case, n), n, "chain")


# ---------------------------------------------------------------- 3: stage routes
@pytest.mark.parametrize("case", STAGE_CASES)
def test_stage_routes(case):
    pol = _shared(case)
    for n in STAGE_N:
        token = "mapped" if n <= 256 else "device"
        for which, q in (("act", False), ("q", True)):
            r = _route(pol, n, q)
            assert r == token + "," + _stage_kernels(case, which, n), (case, n, which, r)
        _check(case, _query_host(pol, case, n), n, "stages")


# ---------------------------------------------------------------- 4: history independence
@pytest.mark.parametrize("case", ["odd", "a17", "k65"])
def test_small_query_does_not_depend_on_history(case):
    """n <= 4 shares the 32-row plan and its H scratch with n = 5..32: rows 4..31 hold an earlier query's
    values.  The n = 3 result after n = 32, after n = 5 and after n = 1 is the fresh learner's, bit for bit."""
    pol = _learner(case)
    results = {}
    for i, n in enumerate((32, 3, 5, 3, 1, 3)):
        results[i] = _query_host(pol, case, n)
        if n != 3:
            _check(case, results[i], n, "history")
    fresh = _query_host(_learner(case), case, 3)
    for i in (1, 3, 5):
        for got, want in zip(results[i], fresh):
            np.testing.assert_array_equal(got, want)
    _check(case, fresh, 3, "history")


# ---------------------------------------------------------------- 5: device queries
def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _query_device(pol, case, n):
    """td3_select_action_device / td3_eval_q_device of the first n pool rows into NaN-guarded device
    allocations through the raw ABI."""
    import torch
    s, a = qr.pool(case)
    ds, da = _cuda(s[:n]), _cuda(a[:n])
    ad = pol.action_dim
    out = []
    for floats, call in ((n * ad, lambda p: pol._lib.td3_select_action_device(pol._h, ds.data_ptr(), n, None, p, None)),
                         (2 * n, lambda p: pol._lib.td3_eval_q_device(pol._h, ds.data_ptr(), da.data_ptr(), n, p, None))):
        buf = torch.full((floats + 2 * GUARD,), float("nan"), device=pol.device)
        with pol._torch_order():
            rc = call(buf.data_ptr() + 4 * GUARD)
        assert rc == 0, pol._lib.td3_last_error()
        b = buf.cpu().numpy()
        assert _guards_ok(b, floats), "a device query wrote outside its output"
        out.append(b[GUARD:GUARD + floats])
    return out[0].reshape(n, ad), out[1][:n], out[1][n:]


@pytest.mark.parametrize("case", STAGE_CASES)
def test_device_queries(case):
    pol = _shared(case)
    for n in (1, 4, 33, 257):
        for which, q in (("act", False), ("q", True)):
            assert _route(pol, n, q, device=True) == "device," + _stage_kernels(case, which, n), (case, n, which)
        _check(case, _query_device(pol, case, n), n, "device")


def _close(got, ref, scale):
    """tests/test_gpu_device_rollout.py's bound: 1e-6 * scale + 1e-6 * |x|, the rounding of the three fp32
    operations of one update (a relative 2^-24 = 6e-8 each), with or without FMA contraction."""
    return np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * scale + 1e-6 * np.abs(ref))


@pytest.mark.parametrize("case", ["min", "k64_a32"])
def test_exploration_epilogue_at_action_width_edges(case):
    """ad = 1 and ad = 32, n = 33: three ticks of the OU recurrence with injected z and a reset mask on
    some rows before the third, against the closed form in fp32 numpy."""
    from td3_amd.exploration import DeviceOUNoise
    pol = _shared(case)
    c = qr.CASES[case]
    n, ad, ma = 33, c["ad"], np.float32(c["ma"])
    dst = _cuda(qr.pool(case)[0][:n])
    pi = pol.select_action_device(dst).cpu().numpy()
    assert np.abs(pi - qr.reference(case)["action"][:n]).max() <= TOL * qr.scale(case, "action")
    mu, theta, sigma = np.float32(0.05), np.float32(0.15), np.float32(0.9 * c["ma"])
    noise = DeviceOUNoise(n, ad, mu=float(mu), theta=float(theta), sigma=float(sigma), device=pol.device)
    z = np.random.RandomState(11).standard_normal((3, n, ad)).astype(np.float32)
    X = np.full((n, ad), mu, np.float32)
    rows = [1, 3, 31, 32]
    clipped = 0
    for k in range(3):
        reset = None
        if k == 2:
            reset = np.zeros(n, bool)
            reset[rows] = True
            X[reset] = mu
        X = (X + (theta * (mu - X) + sigma * z[k])).astype(np.float32)
        a, zo = pol.select_action_device(dst, noise=noise, inject_z=_cuda(z[k]), return_z=True,
                                         reset=None if reset is None else _cuda(reset))
        np.testing.assert_array_equal(zo.cpu().numpy(), z[k])
        scale = max(1.0, float(np.abs(X).max()))
        assert _close(noise.X.cpu().numpy(), X.astype(np.float64), scale), f"X after call {k}"
        want = np.clip(pi.astype(np.float64) + X, -ma, ma)
        assert a.shape == (n, ad)
        assert _close(a.cpu().numpy(), want, scale), f"action after call {k}"
        assert np.abs(a.cpu().numpy()).max() <= ma
        clipped += int((np.abs(pi.astype(np.float64) + X) > ma).sum())
    assert 0 < clipped < 3 * n * ad, "sigma must make some, not all, elements clip"
    assert noise.step == 3
    one = (mu + (theta * (mu - mu) + sigma * z[2])).astype(np.float32)
    assert _close(noise.X.cpu().numpy()[rows], one[rows].astype(np.float64), 1.0)


# ---------------------------------------------------------------- 6: queries after updates
@pytest.mark.parametrize("case", ["odd", "odd_wn", "a17"])
def test_queries_after_updates(case):
    """A critic-only and a policy step (B = 64), then host and device queries against forward64 on the
    parameters the learner exports (g and v under weight normalisation): a query that read a stale
    row-major W beside fresh k-quad images, or a stale derived W, would show here."""
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    c = qr.CASES[case]
    sd, ad, ma, norm = c["sd"], c["ad"], c["ma"], c["norm"]
    pol = _learner(case)
    rows = 128
    rb = ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=rows, seed=3)
    rb.add_batch(*gen.fill_featured_buffer(sd, ad, ma, rows, gen.SEED))
    s, a = qr.pool(case)
    before = _select(pol, s, 3)                       # a query plan exists before the updates
    steps = [pol.train_step(rb, 64, stats=True) for _ in range(2)]
    assert [st["actor_step"] for st in steps] == [False, True]
    A, Cr = pol.actor.numpy_dict(), pol.critic.numpy_dict()
    ref = {"action": qr.actor64(A, norm, ma, s), "q1": qr.q64(Cr, "q1", norm, s, a), "q2": qr.q64(Cr, "q2", norm, s, a)}
    scales = {h: float(np.abs(v).max()) for h, v in ref.items()}
    assert np.abs(ref["action"][:3] - before).max() > 0, "the policy step must have moved the actor"
    dev = _query_device(pol, case, 33)
    got = {3: _query_host(pol, case, 3), 33: (_select(pol, s, 33), *_evalq(pol, s, a, 33)), "33 device": dev}
    for n, g in got.items():
        rows_n = 3 if n == 3 else 33
        errs = _errors(case, g, rows_n, ref, scales)
        print(f"{case} after updates n={n}: action {errs[0]:.2e} Q1 {errs[1]:.2e} Q2 {errs[2]:.2e} of scale")
        assert max(errs) <= TOL, (case, n, errs)


# ---------------------------------------------------------------- 7: refusals
@pytest.mark.parametrize("kw,msg", [
    (dict(sd=17, ad=33), "action_dim > 32"),
    (dict(sd=500, ad=13), "network input width must be <= 512"),
    (dict(sd=17, ad=6, actor_arch=(500, 513, 300)), r"actor hidden in \(0, 512\]"),
    (dict(sd=17, ad=6, q_arch=(500, 400, 0)), r"critic hidden in \(0, 512\]"),
])
def test_create_refusals(kw, msg):
    from td3_amd._lib import TD3Error
    from td3_amd.TD3_featured import TD3
    kw = dict(kw)
    sd, ad = kw.pop("sd"), kw.pop("ad")
    with pytest.raises(TD3Error, match=msg):
        TD3(Box((sd,)), Box((ad,)), init="none", **kw)
    pol = _learner("one_wg")                          # the process can still create and query a learner
    _check("one_wg", _query_host(pol, "one_wg", 2), 2, "after a refusal")
