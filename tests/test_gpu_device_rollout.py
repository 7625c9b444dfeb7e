"""Device-resident rollouts (include/td3.h: rb_add_device, td3_select_action_device,
td3_eval_q_device) on an MI355X: the ring add from device arrays against the host add bit for bit,
the device queries against the oracle and the host queries (SURVEY.md §8c forward tolerance: 1e-5 of
the output scale), the exploration epilogue against its fp32 numpy recurrence, the Philox draw's
reproducibility and moments, stream ordering behind queued steps, and the all-device loop.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import featured_setup, gen, orc

pytestmark = pytest.mark.gpu

SEED = 7            # the learners' Philox key (test 5 compares draws under the same key)


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _policy(S, lr=1e-4):
    from td3_amd.TD3_featured import TD3
    pol = TD3(Box((S["sd"],)), Box((S["ad"],)), max_action=S["ma"], norm=S["norm"], lr=lr, seed=SEED,
              init="none")
    pol.set_weights(S["actor"], S["critic"])
    return pol


def _ring(S, rows=None):
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    rows = rows or gen.BUFFER_ROWS
    rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=rows)
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], rows, gen.SEED)
    rb.add_batch(s, a, s2, r, d)
    return rb


_cache = {}


def _shared(name):
    """(setup, learner) of one configuration, built once: the tests below only query it."""
    if name not in _cache:
        S = featured_setup(name)
        _cache[name] = (S, _policy(S))
    return _cache[name]


def _states(n, sd, seed=0):
    return np.random.RandomState(100 + n + seed).standard_normal((n, sd)).astype(np.float32)


def _cuda(x, dtype=None):
    import torch
    return torch.as_tensor(x, dtype=dtype).cuda()


# ---------------------------------------------------------------- 1, 2: the ring add
def _transitions(rs, n, sd, ad, dtype):
    return (rs.standard_normal((n, sd)).astype(dtype), rs.uniform(-1, 1, (n, ad)).astype(dtype),
            rs.standard_normal((n, sd)).astype(dtype), rs.standard_normal(n).astype(dtype),
            (rs.uniform(size=n) < 0.3).astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sd,ad", [(17, 6), (3, 1)])
def test_device_add_bit_exact_with_host_add(sd, ad, dtype):
    """n=4 from ptr 0, n=8 wrapping a 10-row ring, n=25 > capacity: records, ptr and size equal the
    twin ring fed through the host add_batch; fp32-representable values, and float64 values that are
    not (both paths round them to fp32 once).  Record pads ((17, 6): 2 floats, (3, 1): 3) stay 0."""
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    dev = ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=10)
    host = ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=10)
    used = 2 * sd + ad + 2
    assert dev.record_floats > used
    rs = np.random.RandomState(sd)
    for n in (4, 8, 25):
        t = _transitions(rs, n, sd, ad, dtype)
        if dtype is np.float64:
            assert not np.array_equal(t[0], t[0].astype(np.float32).astype(np.float64))
        dev.add_batch(*[_cuda(x) for x in t])
        host.add_batch(*t)
        rd, rh = dev._records(), host._records()
        np.testing.assert_array_equal(rd, rh)
        assert (dev.ptr, dev.size) == (host.ptr, host.size)
        assert np.all(rd[:, used:] == 0)
    assert (dev.ptr, dev.size) == ((4 + 8 + 25) % 10, 10)
    assert set(np.unique(rd[:, used - 1])) <= {0.0, 1.0}        # not_done = 1 - done


def test_device_add_visible_to_sample_without_sync():
    import torch
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    sd, ad, n = 17, 6, 48
    rb = ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=64)
    s, a, s2, r, d = _transitions(np.random.RandomState(5), n, sd, ad, np.float32)
    rb.add_batch(*[_cuda(x) for x in (s, a, s2, r, d)])
    idx = np.random.RandomState(6).permutation(n)
    out = rb.sample(n, indices=idx)
    torch.cuda.synchronize()
    for got, ref in zip(out, (s, a, s2, r[:, None], 1 - d[:, None])):
        np.testing.assert_array_equal(got.cpu().numpy(), ref[idx])


# ---------------------------------------------------------------- 3: plain queries
def _raw_select(pol, states, n, guard=32):
    """td3_select_action_device into the middle of a NaN-filled allocation: (actions, the rest)."""
    import torch
    ad = pol.action_dim
    buf = torch.full(((n + 2 * guard) * ad,), float("nan"), device=pol.device)
    with pol._torch_order():
        rc = pol._lib.td3_select_action_device(pol._h, states.data_ptr(), n, None,
                                               buf.data_ptr() + guard * ad * 4, None)
    assert rc == 0, pol._lib.td3_last_error()
    got = buf.cpu().numpy()
    return got[guard * ad:(guard + n) * ad].reshape(n, ad), np.concatenate([got[:guard * ad], got[(guard + n) * ad:]])


@pytest.mark.parametrize("name", ["hc_layer", "hc_none"])
@pytest.mark.parametrize("n", [1, 4, 5, 33, 300])
def test_device_queries_match_oracle_and_host(name, n):
    """n = 1, 4 (the host path's gemv sizes), 5 and 33 (partial 32-row tiles), 300 (more than
    kMappedRows): actions within 1e-5 of max_action of the oracle and of select_action_batch, Q1 / Q2
    within 1e-5 of max|Q| of eval_q_batch and the oracle; nothing written outside [n][ad] / [2][n]."""
    import torch
    S, pol = _shared(name)
    ma = S["ma"]
    st = _states(n, S["sd"])
    dst = _cuda(st)
    got = pol.select_action_device(dst)
    assert got.shape == (n, S["ad"]) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    ref = np.stack([orc.featured_select_action(S["actor"], S["norm"], ma, x) for x in st])
    host = pol.select_action_batch(st)
    assert np.abs(got - ref).max() <= 1e-5 * ma
    assert np.abs(got - host).max() <= 1e-5 * ma
    raw, rest = _raw_select(pol, dst, n)
    np.testing.assert_array_equal(raw, got)
    assert np.isnan(rest).all(), "select_action_device wrote outside [n][ad]"

    act = np.random.RandomState(n).uniform(-ma, ma, (n, S["ad"])).astype(np.float32)
    q1, q2 = pol.eval_q_device(dst, _cuda(act))
    h1, h2 = pol.eval_q_batch(st, act)
    o1, _ = orc.featured_q(S["critic"], "q1", S["norm"], st, act)
    o2, _ = orc.featured_q(S["critic"], "q2", S["norm"], st, act)
    for q, h, o in ((q1, h1, o1[:, 0]), (q2, h2, o2[:, 0])):
        q = q.cpu().numpy()
        scale = np.abs(o).max()
        assert q.shape == (n,)
        assert np.abs(q - h).max() <= 1e-5 * scale
        assert np.abs(q - o).max() <= 1e-5 * scale
    guard = 64
    buf = torch.full((2 * n + 2 * guard,), float("nan"), device=pol.device)
    dact = _cuda(act)
    with pol._torch_order():
        rc = pol._lib.td3_eval_q_device(pol._h, dst.data_ptr(), dact.data_ptr(), n, buf.data_ptr() + guard * 4, None)
    assert rc == 0, pol._lib.td3_last_error()
    b = buf.cpu().numpy()
    np.testing.assert_array_equal(b[guard:guard + n], q1.cpu().numpy())
    np.testing.assert_array_equal(b[guard + n:guard + 2 * n], q2.cpu().numpy())
    assert np.isnan(b[:guard]).all() and np.isnan(b[guard + 2 * n:]).all(), "eval_q_device wrote outside [2][n]"


# ---------------------------------------------------------------- 4: the OU epilogue
def _close(got, ref, scale):
    """1e-6 * scale + 1e-6 * |x|: the rounding of the three fp32 operations of one update (a relative
    2^-24 = 6e-8 each), with or without FMA contraction -- from the number format, not measured."""
    return np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * scale + 1e-6 * np.abs(ref))


def test_ou_recurrence_with_injected_z():
    from td3_amd.exploration import DeviceGaussianNoise, DeviceOUNoise
    S, pol = _shared("hc_layer")
    n, ad, ma = 5, S["ad"], np.float32(S["ma"])
    dst = _cuda(_states(n, S["sd"]))
    pi = pol.select_action_device(dst).cpu().numpy()
    mu, theta, sigma = np.float32(0.05), np.float32(0.15), np.float32(0.9)
    noise = DeviceOUNoise(n, ad, mu=float(mu), theta=float(theta), sigma=float(sigma), device=pol.device)
    z = np.random.RandomState(11).standard_normal((3, n, ad)).astype(np.float32)
    X = np.full((n, ad), mu, np.float32)
    clipped = 0
    for k in range(3):
        reset = None
        if k == 2:
            reset = np.zeros(n, bool)
            reset[[1, 3]] = True
            X[reset] = mu
        X = (X + (theta * (mu - X) + sigma * z[k])).astype(np.float32)
        a, zo = pol.select_action_device(dst, noise=noise, inject_z=_cuda(z[k]), return_z=True,
                                         reset=None if reset is None else _cuda(reset))
        np.testing.assert_array_equal(zo.cpu().numpy(), z[k])
        scale = max(1.0, float(np.abs(X).max()))
        assert _close(noise.X.cpu().numpy(), X.astype(np.float64), scale), f"X after call {k}"
        want = np.clip(pi.astype(np.float64) + X, -ma, ma)
        assert _close(a.cpu().numpy(), want, scale), f"action after call {k}"
        assert np.abs(a.cpu().numpy()).max() <= ma
        clipped += int((np.abs(pi.astype(np.float64) + X) > ma).sum())
    assert 0 < clipped < 3 * n * ad, "sigma must make some, not all, elements clip"
    assert noise.step == 3
    # the reset rows restarted from mu: one update from mu, whatever they held before
    one = (mu + (theta * (mu - mu) + sigma * z[2])).astype(np.float32)
    assert _close(noise.X.cpu().numpy()[[1, 3]], one[[1, 3]].astype(np.float64), 1.0)
    # no OU state: a = clip(pi + sigma * z)
    g = DeviceGaussianNoise(sigma=float(sigma))
    a = pol.select_action_device(dst, noise=g, inject_z=_cuda(z[0])).cpu().numpy()
    want = np.clip(pi.astype(np.float64) + (sigma * z[0]).astype(np.float32), -ma, ma)
    assert _close(a, want, max(1.0, float(np.abs(sigma * z[0]).max())))


# ---------------------------------------------------------------- 5: the Philox draw
def _draw(pol, dst, seed, step):
    from td3_amd.exploration import DeviceOUNoise
    noise = DeviceOUNoise(dst.shape[0], pol.action_dim, device=pol.device, seed=seed)
    noise.step = step
    _, z = pol.select_action_device(dst, noise=noise, return_z=True)
    return z.cpu().numpy()


def test_philox_draw():
    S, pol = _shared("hc_layer")
    n, ad = 4096, S["ad"]
    dst = _cuda(_states(n, S["sd"]))
    z = _draw(pol, dst, SEED, 3)
    np.testing.assert_array_equal(_draw(pol, dst, SEED, 3), z)
    assert not np.array_equal(_draw(pol, dst, SEED, 4), z)
    assert not np.array_equal(_draw(pol, dst, SEED + 1, 3), z)
    assert len(np.unique(z, axis=0)) == n, "two rows drew the same values"
    assert np.isfinite(z).all()
    # 24,576 values: standard errors 1/sqrt(N) = 0.0064 (mean) and sqrt(2/N) = 0.0090 (variance)
    assert abs(z.mean()) < 0.03
    assert abs(z.var() - 1.0) < 0.05
    # another stream id than the training step's target-policy noise: same key, same step, other values
    B = 64
    train = _policy(S)
    rb = _ring(S)
    out = train.train_step(rb, B, stats=True)
    tn = out["noise"]
    assert np.isfinite(tn).all() and tn.std() > 0.5
    for step in (0, 1, 2):                       # the step's draw is counted by total_it (0 -> 1) at this call
        zs = _draw(pol, dst[:B], SEED, step)
        assert not np.array_equal(zs, tn)
        assert np.abs(zs - tn).max() > 0.1


# ---------------------------------------------------------------- 6: ordering
def test_device_query_ordered_after_queued_steps():
    """Four queued steps (two actor updates), then the device query with no sync in between: it reads
    the actor those steps leave, as select_action_batch does after sync()."""
    S = featured_setup("hc_layer")
    pol = _policy(S, lr=1e-3)
    rb = _ring(S)
    st = _states(33, S["sd"])
    dst = _cuda(st)
    before = pol.select_action_device(dst).cpu().numpy()
    pol.train_step(rb, 256)                      # builds the step plan (synchronises) before the timed part
    for _ in range(4):
        pol.train_step(rb, 256)
    got = pol.select_action_device(dst)
    pol.sync()
    assert pol.total_it == 5
    host = pol.select_action_batch(st)
    got = got.cpu().numpy()
    assert np.abs(got - host).max() <= 1e-5 * S["ma"]
    assert np.abs(got - before).max() > 1e-3 * S["ma"], "the steps did not move the policy: the test shows nothing"


# ---------------------------------------------------------------- 7: the loop
def test_device_train_loop():
    from td3_amd.loop import DeviceTrainLoop, SyntheticVecEnv
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    S = featured_setup("hc_layer")
    pol = _policy(S)
    env = SyntheticVecEnv(8, S["sd"], S["ad"], max_action=S["ma"], max_episode_steps=25, device=pol.device)
    rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=400)
    loop = DeviceTrainLoop(env, pol, rb, start_policy=5, start_training=10, batch_size=32, expl_noise=0.1)
    res = loop.run(60)
    assert res["env_steps"] == 480 and res["grad_steps"] == 50
    assert rb.size == 400 and rb.ptr == (60 * 8) % 400
    assert pol.total_it == 50
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
    rec = rb._records()
    sd, ad = S["sd"], S["ad"]
    assert np.isfinite(rec).all()
    assert np.abs(rec[:, sd:sd + ad]).max() <= S["ma"]
    assert np.all(rec[:, 2 * sd + ad + 1] == 1.0)     # time-limit ends are not terminal (done swap)
    assert np.abs(loop.noise.X.cpu().numpy()).max() > 0
