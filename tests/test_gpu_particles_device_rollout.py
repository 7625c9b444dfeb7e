"""Device-resident rollouts of the particle learner (include/td3.h: rb_add_particles_device,
td3_select_action_particles_device, td3_eval_q_particles_device) on an MI355X: the ring add from seven
device arrays against the host add bit for bit, the device queries against the oracle and the host
queries (SURVEY.md §8c forward tolerance: 1e-5 of the output scale + 1e-6, as
test_particle_select_action_batch), the exploration epilogue against its fp32 numpy recurrence (1e-6
from the number format, test_gpu_device_rollout._close), stream ordering behind queued steps, the
all-device loop, and the refusals between the featured and the particle entry points.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import featured_setup, gen, orc, particle_setup, particle_setup_dims

pytestmark = pytest.mark.gpu


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _obs(F, N, D):
    return (Box((F,)), Box((N, D)))


def _policy(S, lr=1e-4, max_action=1.0):
    from td3_amd.TD3_particles import TD3
    pol = TD3(_obs(S["F"], S["N"], S["D"]), Box((S["A"],)), norm=S["norm"], CDQ=S["cdq"], lr=lr, init="none",
              max_action=max_action)
    pol.set_weights(S["actor"], S["critic"])
    return pol


def _ring(F, N, D, A, rows):
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    return ReplayBuffer_particles(_obs(F, N, D), Box((A,)), max_size=rows)


_SETUPS = {"two_tiles": lambda: particle_setup_dims(3, 40, 4, 2)}    # N = 40: two encoder tiles, the second partial
_cache = {}


def _shared(name):
    """(setup, learner) of one configuration, built once: the query tests only read it."""
    if name not in _cache:
        S = _SETUPS[name]() if name in _SETUPS else particle_setup(name)
        _cache[name] = (S, _policy(S))
    return _cache[name]


def _cuda(x, dtype=None):
    import torch
    return torch.as_tensor(x, dtype=dtype).cuda()


def _close(got, ref, scale):
    """test_gpu_device_rollout._close: 1e-6 * scale + 1e-6 * |x|, the rounding of the three fp32
    operations of one update (a relative 2^-24 = 6e-8 each), with or without FMA contraction."""
    return np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * scale + 1e-6 * np.abs(ref))


def _fwd_close(got, ref):
    """SURVEY.md §8c forward tolerance as test_particle_select_action_batch states it."""
    return float(np.abs(got - ref).max()) <= 1e-5 * float(np.abs(ref).max()) + 1e-6


# ---------------------------------------------------------------- 1, 2: the ring add
def _transitions(rs, n, F, N, D, A, dtype):
    return (rs.standard_normal((n, F)).astype(dtype), rs.standard_normal((n, N, D)).astype(dtype),
            rs.uniform(-1, 1, (n, A)).astype(dtype), rs.standard_normal((n, F)).astype(dtype),
            rs.standard_normal((n, N, D)).astype(dtype), rs.standard_normal(n).astype(dtype),
            (rs.uniform(size=n) < 0.3).astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("F,N,D,A", [(7, 16, 9, 3), (3, 5, 3, 2)])
def test_device_add_bit_exact_with_host_add(F, N, D, A, dtype):
    """n=4 from ptr 0, n=8 wrapping a 10-row ring, n=25 > capacity: records, ptr and size equal the
    twin ring fed through the host add_batch.  (7, 16, 9, 3): the particle block starts at record
    column 7 (no 16-byte alignment), N*D = 144; (3, 5, 3, 2): N*D = 15, so the source rows start at
    odd 4-byte offsets.  fp32-representable values, and float64 values that are not (both paths
    round them to fp32 once).  The record pad stays 0, not_done is 1 - done."""
    dev, host = _ring(F, N, D, A, 10), _ring(F, N, D, A, 10)
    used = 2 * (F + N * D) + A + 2
    assert dev.record_floats >= used and dev.record_floats % 4 == 0
    rs = np.random.RandomState(F)
    for n in (4, 8, 25):
        t = _transitions(rs, n, F, N, D, A, dtype)
        if dtype is np.float64:
            assert not np.array_equal(t[1], t[1].astype(np.float32).astype(np.float64))
        dev.add_batch(*[_cuda(x) for x in t])
        host.add_batch(*t)
        rd, rh = dev._records(), host._records()
        np.testing.assert_array_equal(rd, rh)
        assert (dev.ptr, dev.size) == (host.ptr, host.size)
        assert np.all(rd[:, used:] == 0)
    assert (dev.ptr, dev.size) == ((4 + 8 + 25) % 10, 10)
    assert set(np.unique(rd[:, used - 1])) <= {0.0, 1.0}        # not_done = 1 - done
    assert np.isfinite(rd).all() and np.abs(rd[:, :used - 2]).max() > 0


def test_device_add_visible_to_sample_without_sync():
    import torch
    F, N, D, A, n = 7, 16, 9, 3, 48
    rb = _ring(F, N, D, A, 64)
    t = _transitions(np.random.RandomState(5), n, F, N, D, A, np.float32)
    rb.add_batch(*[_cuda(x) for x in t])
    idx = np.random.RandomState(6).permutation(n)
    out = rb.sample(n, indices=idx)
    torch.cuda.synchronize()
    f, p, a, f2, p2, r, d = t
    assert len(out) == 7
    for got, ref in zip(out, (f, p, a, f2, p2, r[:, None], 1 - d[:, None])):
        np.testing.assert_array_equal(got.cpu().numpy(), ref[idx])


# ---------------------------------------------------------------- 3: plain queries
def _states(S, n, seed=0):
    rs = np.random.RandomState(100 + n + seed)
    return (rs.standard_normal((n, S["F"])).astype(np.float32),
            rs.standard_normal((n, S["N"], S["D"])).astype(np.float32))


def _guarded(pol, floats, guard):
    """A NaN-filled device allocation with `floats` live floats in its middle: (tensor, address of
    the live part)."""
    import torch
    buf = torch.full((floats + 2 * guard,), float("nan"), device=pol.device)
    return buf, buf.data_ptr() + guard * 4


@pytest.mark.parametrize("name", ["part_layer", "part_nocdq", "part_none", "two_tiles"])
@pytest.mark.parametrize("n", [1, 5, 33, 300])
def test_device_queries_match_oracle_and_host(name, n):
    """n = 1, 5 and 33 (partial 32-row tiles), 300 (more than the host plans' mapped rows): actions and
    Q within the forward tolerance of the oracle and of the host queries; without CDQ the list has
    one entry and the raw q_out[1] repeats q_out[0]; nothing written outside [n][A] / [2][n][A]."""
    import torch
    S, pol = _shared(name)
    A = S["A"]
    f, p = _states(S, n)
    df, dp = _cuda(f), _cuda(p)
    got = pol.select_action_device((df, dp))
    assert got.shape == (n, A) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    ref, _ = orc.particle_net(S["actor"], "", S["norm"], f, p, actor=True)
    host = pol.select_action_batch((f, p))
    assert _fwd_close(got, ref)
    assert _fwd_close(got, host)
    guard = 32 * A
    buf, live = _guarded(pol, n * A, guard)
    with pol._torch_order():
        rc = pol._lib.td3_select_action_particles_device(pol._h, df.data_ptr(), dp.data_ptr(), n, None, live, None)
    assert rc == 0, pol._lib.td3_last_error()
    b = buf.cpu().numpy()
    np.testing.assert_array_equal(b[guard:guard + n * A].reshape(n, A), got)
    assert np.isnan(b[:guard]).all() and np.isnan(b[guard + n * A:]).all(), "select wrote outside [n][A]"

    act = np.random.RandomState(n).uniform(-1, 1, (n, A)).astype(np.float32)
    dact = _cuda(act)
    qs = pol.eval_q_device((df, dp), dact)
    hs = pol.eval_q_batch((f, p), act)
    nets = ("q1", "q2") if S["cdq"] else ("q1",)
    assert len(qs) == len(hs) == len(nets)
    for q, h, qn in zip(qs, hs, nets):
        o, _ = orc.particle_net(S["critic"], f"{qn}.", S["norm"], f, p, act)
        assert q.shape == (n, A) and q.is_cuda
        q = q.cpu().numpy()
        assert _fwd_close(q, o), qn
        assert _fwd_close(q, h), qn
    buf, live = _guarded(pol, 2 * n * A, guard)
    with pol._torch_order():
        rc = pol._lib.td3_eval_q_particles_device(pol._h, df.data_ptr(), dp.data_ptr(), dact.data_ptr(), n, live, None)
    assert rc == 0, pol._lib.td3_last_error()
    b = buf.cpu().numpy()
    raw = b[guard:guard + 2 * n * A].reshape(2, n, A)
    np.testing.assert_array_equal(raw[0], qs[0].cpu().numpy())
    np.testing.assert_array_equal(raw[1], qs[-1].cpu().numpy())        # without CDQ: Q1 again
    assert np.isnan(b[:guard]).all() and np.isnan(b[guard + 2 * n * A:]).all(), "eval_q wrote outside [2][n][A]"


# ---------------------------------------------------------------- 4: the OU epilogue
def test_ou_recurrence_with_injected_z():
    """max_action 0.5 under the tanh policy (|pi| < 1): the clip of main.py:252 acts on some elements
    and not on all."""
    from td3_amd.exploration import DeviceGaussianNoise, DeviceOUNoise
    S = particle_setup("part_layer")
    ma = np.float32(0.5)
    pol = _policy(S, max_action=float(ma))
    n, A = 5, S["A"]
    f, p = _states(S, n)
    dst = (_cuda(f), _cuda(p))
    pi = pol.select_action_device(dst).cpu().numpy()                # plain: the tanh rows, no clip
    ref, _ = orc.particle_net(S["actor"], "", S["norm"], f, p, actor=True)
    assert _fwd_close(pi, ref)
    mu, theta, sigma = np.float32(0.05), np.float32(0.15), np.float32(0.3)
    noise = DeviceOUNoise(n, A, mu=float(mu), theta=float(theta), sigma=float(sigma), device=pol.device)
    z = np.random.RandomState(11).standard_normal((3, n, A)).astype(np.float32)
    X = np.full((n, A), mu, np.float32)
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
    assert 0 < clipped < 3 * n * A, "sigma must make some, not all, elements clip"
    assert noise.step == 3
    one = (mu + (theta * (mu - mu) + sigma * z[2])).astype(np.float32)
    assert _close(noise.X.cpu().numpy()[[1, 3]], one[[1, 3]].astype(np.float64), 1.0)
    g = DeviceGaussianNoise(sigma=float(sigma))
    a = pol.select_action_device(dst, noise=g, inject_z=_cuda(z[0])).cpu().numpy()
    want = np.clip(pi.astype(np.float64) + (sigma * z[0]).astype(np.float32), -ma, ma)
    assert _close(a, want, max(1.0, float(np.abs(sigma * z[0]).max())))


# ---------------------------------------------------------------- 5: ordering
def test_device_query_ordered_after_queued_steps():
    """Four queued steps (two actor updates), then the device query with no sync in between: it reads
    the actor those steps leave, as select_action_batch does after sync()."""
    S = particle_setup("part_layer")
    pol = _policy(S, lr=1e-3)
    rb = _ring(S["F"], S["N"], S["D"], S["A"], gen.BUFFER_ROWS)
    rb.add_batch(*gen.fill_particle_buffer(S["F"], S["N"], S["D"], S["A"], gen.BUFFER_ROWS, gen.SEED))
    f, p = _states(S, 33)
    dst = (_cuda(f), _cuda(p))
    before = pol.select_action_device(dst).cpu().numpy()
    pol.train_step(rb, 32)                       # builds the step plan (synchronises) before the queued part
    for _ in range(4):
        pol.train_step(rb, 32)
    got = pol.select_action_device(dst)
    pol.sync()
    assert pol.total_it == 5
    host = pol.select_action_batch((f, p))
    got = got.cpu().numpy()
    assert np.abs(got - host).max() <= 1e-5
    assert np.abs(got - before).max() > 1e-3, "the steps did not move the policy: the test shows nothing"


# ---------------------------------------------------------------- 6: the loop
def test_device_train_loop_particles():
    from td3_amd.loop import DeviceTrainLoop, SyntheticParticleVecEnv
    S = particle_setup("part_layer")
    F, N, D, A = S["F"], S["N"], S["D"], S["A"]
    pol = _policy(S)
    env = SyntheticParticleVecEnv(8, F, N, D, A, max_episode_steps=25, device=pol.device)
    rb = _ring(F, N, D, A, 400)
    loop = DeviceTrainLoop(env, pol, rb, start_policy=5, start_training=10, batch_size=32, expl_noise=0.1)
    res = loop.run(60)
    assert res["env_steps"] == 480 and res["grad_steps"] == 50
    assert rb.size == 400 and rb.ptr == (60 * 8) % 400
    assert pol.total_it == 50
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
    rec = rb._records()
    o_a = F + N * D
    o_nd = 2 * (F + N * D) + A + 1
    assert np.isfinite(rec).all()
    assert np.abs(rec[:, o_a:o_a + A]).max() <= pol.max_action
    assert np.abs(rec[:, F:o_a]).max() > 0                  # the particle block arrived
    assert np.all(rec[:, o_nd] == 1.0)                      # time-limit ends are not terminal (done swap)
    assert np.abs(loop.noise.X.cpu().numpy()).max() > 0


# ---------------------------------------------------------------- 7: kind mismatches
def test_kind_mismatches_are_refused():
    """The featured calls on a particle handle / ring and the particle calls on a featured handle /
    ring return -1 with a message naming the right call, before any GPU work: the pointers given are
    not device memory (they would fault if a kernel read them)."""
    from td3_amd.TD3_featured import TD3 as FeaturedTD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    _, ppol = _shared("part_layer")
    Sf = featured_setup("hc_layer")
    fpol = FeaturedTD3(Box((Sf["sd"],)), Box((Sf["ad"],)), max_action=Sf["ma"], norm=Sf["norm"], init="none")
    prb = _ring(7, 16, 9, 3, 8)
    frb = ReplayBuffer_featured(Box((17,)), Box((6,)), max_size=8)
    lib = ppol._lib
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    err = lambda: lib.td3_last_error().decode()

    assert lib.rb_add_device(prb.handle, p, p, p, p, p, 1, None) == -1
    assert "rb_add_particles_device" in err()
    assert lib.rb_add_particles_device(frb.handle, p, p, p, p, p, p, p, 1, None) == -1
    assert "rb_add_device" in err() and "featured ring" in err()
    assert (prb.ptr, prb.size, frb.ptr, frb.size) == (0, 0, 0, 0)

    assert lib.td3_select_action_device(ppol._h, p, 1, None, p, None) == -1
    assert "td3_select_action_particles_device" in err()
    assert lib.td3_eval_q_device(ppol._h, p, p, 1, p, None) == -1
    assert "td3_eval_q_particles_device" in err()
    assert lib.td3_select_action_particles_device(fpol._h, p, p, 1, None, p, None) == -1
    assert "featured learner" in err() and "td3_select_action_device" in err()
    assert lib.td3_eval_q_particles_device(fpol._h, p, p, p, 1, p, None) == -1
    assert "featured learner" in err() and "td3_eval_q_device" in err()
