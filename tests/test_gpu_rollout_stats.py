"""Rollout statistics on an MI355X (include/td3.h: rs_*; td3_amd/rollout_stats.py) against the numpy
restatement (tests/rollout_stats_reference.py).

Shapes (rows, obs_dim): (1, 1) degenerate; (3, 17) HalfCheetah's width; (8, 64) / (5, 65) either side of
the 64-column block edge; (7, 376) Humanoid's width, ragged last block; (300, 3) many rows on
few columns (more than a 256-thread workgroup has threads; 300 ends in one tick against a 4-entry log).  Two more for the paths the
column width W opens (rows * W <= 8192): (200, 40) has W = 32 and a ragged second workgroup; (2100, 5) has
W = 2, three workgroups, and more rows than two passes of the 1024-row reward loop.
12 ticks, |x| <= 10 with a column-dependent offset, rows ending with periods 2 / 3 / 4 (all rows end at
the last tick, row 0 six times), log_cap = 4 so the log wraps.

Bounds.  Moments: |d mean| <= K max|x| and |d (m2 / count)| <= K max|x|^2 with K = 8 ticks rows 2^-53,
the fp64 summation bound for any order with a factor 8 for the merge arithmetic (the return moments
likewise with max|G|).  Outputs: the restatement evaluated from the moments read back from the device,
within 1 fp32 ulp (the fp64 expression is a few fp64 ulps off; the one rounding to fp32 can move the
result one step).  Measured on an MI355X at these shapes: outputs 0 ulp from both
restatements (device moments and its own) and 0 ulp in the ring rows of the end-to-end runs; moments
at most 5.3e-15 (variance) and 5.6e-17 (return mean) from the restatement.  Everything else is exact.
"""
import numpy as np
import pytest

from helpers import gen
from rollout_stats_reference import RolloutStatsRef, normalise, scale_reward

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 17), (8, 64), (5, 65), (7, 376), (300, 3), (200, 40), (2100, 5)]
TICKS, LOG_CAP, GAMMA, EPS, CLIP = 12, 4, 0.9, 1e-8, 10.0
MOMENTS = ("count", "mean", "m2", "ret_count", "ret_mean", "ret_m2")
STATE = MOMENTS + ("G", "ep_return", "ep_len", "log", "ep_count", "ep_len_sum", "tick", "ep_return_sum")


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _cuda(x):
    import torch
    return torch.as_tensor(x).cuda()


def _mask(dim):
    m = np.ones(dim, np.uint8)
    if dim >= 3:
        m[1] = m[dim - 1] = 0
    return m


def _scenario(rows, dim):
    rs = np.random.RandomState(1000 * rows + dim)
    off = 5.0 * np.sin(np.arange(dim))
    obs = (rs.uniform(-5, 5, (TICKS, rows, dim)) + off).astype(np.float32)
    nxt = (rs.uniform(-5, 5, (TICKS, rows, dim)) + off).astype(np.float32)
    rew = rs.uniform(-2, 2, (TICKS, rows)).astype(np.float32)
    t, i = np.meshgrid(np.arange(TICKS), np.arange(rows), indexing="ij")
    end = (t + 1) % (2 + i % 3) == 0
    assert np.abs(obs).max() <= 10 and np.abs(nxt).max() <= 10 and end[-1].all() and end[:, 0].sum() == 6
    return obs, nxt, rew, end


def _stats(rows, dim, log_cap=LOG_CAP):
    from td3_amd.rollout_stats import RolloutStats
    return RolloutStats(rows, dim, gamma=GAMMA, obs_clip=CLIP, rew_clip=CLIP, eps=EPS, col_mask=_mask(dim),
                        log_cap=log_cap)


def _same_bits(a, b, keys=STATE):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    step = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / step).max())


_runs = {}


def _run(shape):
    """One device run per shape, shared by the tests below and left unchanged: the outputs and the state
    after every tick, the device inputs, and the restatement fed the same ticks."""
    if shape not in _runs:
        rows, dim = shape
        obs, nxt, rew, end = _scenario(rows, dim)
        d = tuple(_cuda(x) for x in (obs, nxt, rew, end))
        st, ref = _stats(rows, dim), RolloutStatsRef(rows, dim, gamma=GAMMA, obs_clip=CLIP, rew_clip=CLIP, eps=EPS,
                                                     col_mask=_mask(dim), log_cap=LOG_CAP)
        outs, states, routs = [], [], []
        for t in range(TICKS):
            o = st.tick(d[0][t], d[1][t], d[2][t], d[3][t])
            outs.append(tuple(x.cpu().numpy() for x in o))
            states.append(st.state_dict())
            routs.append(ref.tick(obs[t], nxt[t], rew[t], end[t]))
        _runs[shape] = dict(host=(obs, nxt, rew, end), dev=d, stats=st, ref=ref, outs=outs, states=states, routs=routs)
    return _runs[shape]


def _feed(st, d, ticks=range(TICKS), inplace=False):
    outs = []
    for t in ticks:
        a = [d[0][t], d[1][t], d[2][t]]
        if inplace:
            a = [x.clone() for x in a]
        outs.append(st.tick(*a, d[3][t], inplace=inplace))
    return outs


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_against_the_restatement(shape):
    R = _run(shape)
    rows, dim = shape
    obs, nxt, rew, end = R["host"]
    sd, ref = R["states"][-1], R["ref"]
    K = 8 * TICKS * rows * 2.0 ** -53
    xmax = float(np.abs(obs).max())
    assert sd["count"] == ref.count == TICKS * rows and sd["ret_count"] == ref.ret_count == TICKS * rows
    dm = np.abs(sd["mean"] - ref.mean).max()
    dv = np.abs(sd["m2"] / sd["count"] - ref.m2 / ref.count).max()
    G, gmax = np.zeros(rows), 0.0
    for t in range(TICKS):
        G = GAMMA * G + rew[t]
        gmax = max(gmax, float(np.abs(G).max()))
        G[end[t]] = 0.0
    drm = abs(sd["ret_mean"] - ref.ret_mean)
    drv = abs(sd["ret_m2"] / sd["ret_count"] - ref.ret_m2 / ref.ret_count)
    print(f"{shape}: dmean {dm:.3e} (bound {K * xmax:.3e}) dvar {dv:.3e} ({K * xmax ** 2:.3e}) "
          f"dret_mean {drm:.3e} ({K * gmax:.3e}) dret_var {drv:.3e} ({K * gmax ** 2:.3e})")
    assert dm <= K * xmax and dv <= K * xmax ** 2
    assert drm <= K * gmax and drv <= K * gmax ** 2
    m = _mask(dim) == 0
    assert (sd["mean"][m] == 0).all() and (sd["m2"][m] == 0).all()       # no moments kept for masked columns
    np.testing.assert_array_equal(sd["G"], ref.G)                          # the same fp64 operations per row
    np.testing.assert_array_equal(sd["ep_return"], ref.ep_return)
    np.testing.assert_array_equal(sd["ep_len"], ref.ep_len)


@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_against_the_restatement(shape):
    R = _run(shape)
    obs, nxt, rew, end = R["host"]
    mask, worst, where = _mask(shape[1]), 0.0, None
    for t in range(TICKS):
        sd = R["states"][t]                               # the moments as they stand after this tick's update
        o, n, r = R["outs"][t]
        assert o.dtype == n.dtype == r.dtype == np.float32
        want = (normalise(obs[t], sd["count"], sd["mean"], sd["m2"], EPS, CLIP, mask),
                normalise(nxt[t], sd["count"], sd["mean"], sd["m2"], EPS, CLIP, mask),
                scale_reward(rew[t], sd["ret_count"], sd["ret_m2"], EPS, CLIP))
        for name, got, w in zip(("obs", "next_obs", "reward", "obs (own moments)", "next_obs (own moments)",
                                 "reward (own moments)"), (o, n, r, o, n, r), want + R["routs"][t]):
            u = _ulps(got, w)
            if u > worst:
                k = np.unravel_index(np.argmax(np.abs(got.astype(np.float64) - w)), got.shape)
                worst, where = u, f"tick {t} {name} at {k}: got {got[k]!r} want {w[k]!r}"
    print(f"{shape}: largest output difference {worst} ulp ({where})")
    assert worst <= 1.0, where
    if shape[1] > 1:
        assert max(np.abs(R["outs"][t][0]).max() for t in range(TICKS)) < CLIP  # not all clipped away


@pytest.mark.parametrize("shape", SHAPES)
def test_aliasing_and_masking(shape):
    R = _run(shape)
    obs, nxt, rew, end = R["host"]
    m = _mask(shape[1]) == 0
    twin = _stats(*shape)
    outs = _feed(twin, R["dev"], inplace=True)
    for t in range(TICKS):
        for got, want in zip(outs[t], R["outs"][t]):      # in place == out of place, bit for bit
            assert got.cpu().numpy().tobytes() == want.tobytes()
        for got, raw in ((R["outs"][t][0], obs[t]), (R["outs"][t][1], nxt[t])):
            assert got[:, m].tobytes() == raw[:, m].tobytes()
    assert _same_bits(twin.state_dict(), R["states"][-1]) == []


@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_moments(shape):
    import torch
    R = _run(shape)
    rows, dim = shape
    obs, nxt, rew, end = R["host"]
    st = _stats(rows, dim, log_cap=2 * rows + 8)
    _feed(st, R["dev"], ticks=range(6))
    before = st.state_dict()
    o, n, r = st.tick(R["dev"][0][7], R["dev"][1][7], R["dev"][2][7], torch.ones(rows, dtype=torch.bool, device="cuda"),
                      update=False)
    after = st.state_dict()
    assert _same_bits(before, after, MOMENTS) == []
    mask = _mask(dim)
    assert _ulps(o.cpu().numpy(), normalise(obs[7], before["count"], before["mean"], before["m2"], EPS, CLIP, mask)) <= 1
    assert _ulps(n.cpu().numpy(), normalise(nxt[7], before["count"], before["mean"], before["m2"], EPS, CLIP, mask)) <= 1
    assert _ulps(r.cpu().numpy(), scale_reward(rew[7], before["ret_count"], before["ret_m2"], EPS, CLIP)) <= 1
    assert after["ep_count"] == before["ep_count"] + rows and after["tick"] == before["tick"] + 1
    assert (after["G"] == 0).all() and (after["ep_return"] == 0).all() and (after["ep_len"] == 0).all()
    eps = st.episodes(first=int(before["ep_count"]))
    assert list(eps["row"]) == list(range(rows)) and (eps["tick"] == 6).all()
    np.testing.assert_array_equal(eps["ret"], (before["ep_return"] + rew[7].astype(np.float64)).astype(np.float32))
    # a fresh handle has no moments: frozen ticks pass everything through
    fresh = _stats(rows, dim)
    o, n, r = fresh.tick(R["dev"][0][0], R["dev"][1][0], R["dev"][2][0], update=False)
    assert o.cpu().numpy().tobytes() == obs[0].tobytes() and n.cpu().numpy().tobytes() == nxt[0].tobytes()
    assert r.cpu().numpy().tobytes() == rew[0].tobytes() and fresh.summary()["count"] == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_log_contents(shape):
    R = _run(shape)
    st, ref, sd = R["stats"], R["ref"], R["states"][-1]
    assert sd["ep_count"] == ref.ep_count > LOG_CAP and sd["tick"] == ref.tick_no == TICKS
    assert sd["ep_len_sum"] == ref.ep_len_sum and sd["ep_return_sum"] == ref.ep_return_sum
    eps = st.episodes()
    assert len(eps) == LOG_CAP and list(eps["seq"]) == list(range(ref.ep_count - LOG_CAP, ref.ep_count))
    got = [(np.float32(e["ret"]), int(e["len"]), int(e["row"]), int(e["tick"])) for e in eps]
    assert got == ref.episodes()
    for t in range(TICKS):                                # every tick's log, wrap included
        pass_ref = RolloutStatsRef(shape[0], shape[1], gamma=GAMMA, log_cap=LOG_CAP)
        for u in range(t + 1):
            pass_ref.tick(reward=R["host"][2][u], ended=R["host"][3][u], update=False)
        log = R["states"][t]["log"]
        for slot, want in enumerate(pass_ref.log):
            if want is not None:
                e = log[slot]
                assert (np.float32(e["ret"]), int(e["len"]), int(e["row"]), int(e["tick"])) == want
        assert R["states"][t]["ep_count"] == pass_ref.ep_count
    assert len(st.episodes(first=ref.ep_count - 2)) == 2 and len(st.episodes(first=ref.ep_count)) == 0
    s = st.summary()
    assert s["episodes"] == ref.ep_count and s["mean_length"] == ref.ep_len_sum / ref.ep_count


@pytest.mark.parametrize("shape", SHAPES)
def test_determinism_and_checkpoint(shape, tmp_path):
    R = _run(shape)
    twin = _stats(*shape)
    _feed(twin, R["dev"])
    assert _same_bits(twin.state_dict(), R["states"][-1]) == []
    half = _stats(*shape)
    _feed(half, R["dev"], ticks=range(6))
    assert _same_bits(half.state_dict(), R["states"][5]) == []
    half.save(tmp_path / "rs.npz")
    cont = _stats(*shape)
    cont.load(tmp_path / "rs.npz")
    assert _same_bits(cont.state_dict(), R["states"][5]) == []
    outs = _feed(cont, R["dev"], ticks=range(6, TICKS))
    assert _same_bits(cont.state_dict(), R["states"][-1]) == []
    for got, want in zip(outs[-1], R["outs"][-1]):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        _stats(shape[0] + 1, shape[1]).load_state_dict(half.state_dict())


@pytest.mark.parametrize("shape", [(7, 376), (300, 3)])
def test_stream_ordering(shape):
    """Ticks queued on torch's current (side) stream right behind the torch ops that make their inputs,
    with no synchronisation, against the same ticks fed synchronised inputs."""
    import torch
    R = _run(shape)
    d = R["dev"]
    big = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    st = _stats(*shape)
    outs = []
    with torch.cuda.stream(side):
        for t in range(TICKS):
            lag = (big @ big)[0, 0] * 0.0                 # the inputs exist only once this has run
            lag = torch.nan_to_num(lag, nan=0.0, posinf=0.0, neginf=0.0)
            outs.append(st.tick(d[0][t] + lag, d[1][t] + lag, d[2][t] + lag, d[3][t]))
    side.synchronize()
    assert _same_bits(st.state_dict(), R["states"][-1]) == []
    for got, want in zip(outs[-1], R["outs"][-1]):
        assert got.cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------- end to end
def _loop_run(env, pol, rb, ticks, **kw):
    import torch
    from td3_amd.loop import DeviceTrainLoop
    torch.manual_seed(1234)                               # the uniform actions before start_policy
    loop = DeviceTrainLoop(env, pol, rb, start_policy=10 ** 6, start_training=10 ** 6, batch_size=32, expl_noise=0.1,
                           **kw)
    loop.run(ticks)
    return loop


def test_end_to_end_featured():
    from td3_amd.TD3_featured import TD3
    from td3_amd.loop import SyntheticVecEnv
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    from td3_amd.rollout_stats import NormalizedVecEnv, RolloutStats, evaluate_device
    n, sd, ad, L, T = 8, 17, 6, 5, 12
    pol = TD3(Box((sd,)), Box((ad,)), max_action=1.0, norm="layer", seed=3, init="none")
    pol.set_weights(gen.init_params(gen.featured_actor_shapes(sd, ad, "layer"), gen.SEED),
                    gen.init_params(gen.featured_critic_shapes(sd, ad, "layer"), gen.SEED + 100))
    rings = [ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=n * T) for _ in range(2)]
    bare = SyntheticVecEnv(n, sd, ad, max_episode_steps=L, seed=5, device=pol.device)
    _loop_run(bare, pol, rings[0], T)
    stats = RolloutStats(n, sd, gamma=pol.discount)
    env = NormalizedVecEnv(SyntheticVecEnv(n, sd, ad, max_episode_steps=L, seed=5, device=pol.device), stats)
    seen = []
    _loop_run(env, pol, rings[1], T, log_every=5, on_log=lambda t, loop: seen.append((t, stats.summary()["episodes"])))
    assert seen == [(5, n), (10, 2 * n)]
    raw, got = rings[0]._records().reshape(T, n, -1), rings[1]._records().reshape(T, n, -1)
    s, a, s2, r = raw[..., :sd], raw[..., sd:sd + ad], raw[..., sd + ad:2 * sd + ad], raw[..., 2 * sd + ad]
    assert got[..., sd:sd + ad].tobytes() == a.tobytes()  # the same uniform actions, so the same raw trajectory
    last = bare.state.cpu().numpy()
    ref = RolloutStatsRef(n, sd, gamma=pol.discount)
    state, _, _ = ref.tick(obs=s[0])                      # reset()
    worst = 0.0
    for t in range(T):
        done = np.full(n, (t + 1) % L == 0)
        o, nx, rw = ref.tick(obs=s[t + 1] if t + 1 < T else last, next_obs=s2[t], reward=r[t], ended=done)
        worst = max(worst, _ulps(got[t, :, :sd], state), _ulps(got[t, :, sd + ad:2 * sd + ad], nx),
                    _ulps(got[t, :, 2 * sd + ad], rw))
        state = o
    print(f"end to end (featured): largest ring difference {worst} ulp")
    assert worst <= 1.0
    assert (got[..., 2 * sd + ad + 1] == 1.0).all()       # time-limit ends are not terminal (done swap)
    eps = stats.episodes()
    assert len(eps) == n * (T // L) and (eps["len"] == L).all()
    assert list(eps["row"]) == list(range(n)) * (T // L) and list(eps["tick"]) == [L - 1] * n + [2 * L - 1] * n
    for k, e in enumerate(eps):                           # the raw rewards of the episode, summed in fp64
        t1 = int(e["tick"])
        acc = 0.0
        for v in r[t1 - L + 1:t1 + 1, e["row"]]:
            acc += float(v)
        assert e["ret"] == np.float32(acc)
    for _ in range(3):                                    # the learner trains on the normalised rows
        pol.train(rings[1], 32)
    pol.sync()
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
    # evaluation: exactly the requested episodes, the training statistics untouched
    before = stats.state_dict()
    mean_ret, mean_len = evaluate_device(pol, SyntheticVecEnv(n, sd, ad, max_episode_steps=L, seed=9, device=pol.device),
                                         stats, 10, poll_every=4)
    assert _same_bits(stats.state_dict(), before) == []
    ev = stats.frozen_copy(n)
    wenv = NormalizedVecEnv(SyntheticVecEnv(n, sd, ad, max_episode_steps=L, seed=9, device=pol.device), ev,
                            norm_reward=False, update=False)
    state = wenv.reset()
    for _ in range(2 * L):
        wenv.step(pol.select_action_device(state))
        state = wenv.state
    first10 = ev.episodes()[:10]
    assert len(ev.episodes()) == 2 * n and mean_len == float(L)
    assert mean_ret == float(first10["ret"].astype(np.float64).mean())
    assert _same_bits(ev.state_dict(), before, MOMENTS) == []


def test_end_to_end_particles():
    from td3_amd.TD3_particles import TD3
    from td3_amd.loop import SyntheticParticleVecEnv
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    from td3_amd.rollout_stats import NormalizedVecEnv, RolloutStats
    n, F, N, D, A, L, T = 8, 3, 40, 4, 2, 5, 12
    space = (Box((F,)), Box((N, D)))
    pol = TD3(space, Box((A,)), norm="layer", CDQ=True, init="none")
    pol.set_weights(gen.init_params(gen.particle_actor_shapes(F, D, A, "layer"), gen.SEED),
                    gen.init_params(gen.particle_critic_shapes(F, D, A, "layer", True), gen.SEED + 100))
    rings = [ReplayBuffer_particles(space, Box((A,)), max_size=n * T) for _ in range(2)]
    bare = SyntheticParticleVecEnv(n, F, N, D, A, max_episode_steps=L, seed=5, device=pol.device)
    _loop_run(bare, pol, rings[0], T)
    stats = RolloutStats(n, F, gamma=pol.discount)
    env = NormalizedVecEnv(SyntheticParticleVecEnv(n, F, N, D, A, max_episode_steps=L, seed=5, device=pol.device), stats)
    _loop_run(env, pol, rings[1], T)
    raw, got = rings[0]._records().reshape(T, n, -1), rings[1]._records().reshape(T, n, -1)
    P = N * D
    o_a, o_f2, o_p2, o_r = F + P, F + P + A, 2 * F + P + A, 2 * (F + P) + A
    for lo, hi in ((F, o_f2), (o_p2, o_r)):               # particles, action, next particles: bit for bit
        assert got[..., lo:hi].tobytes() == raw[..., lo:hi].tobytes()
    last = bare.state[0].cpu().numpy()
    ref = RolloutStatsRef(n, F, gamma=pol.discount)
    state, _, _ = ref.tick(obs=raw[0, :, :F])
    worst = 0.0
    for t in range(T):
        o, nx, rw = ref.tick(obs=raw[t + 1, :, :F] if t + 1 < T else last, next_obs=raw[t, :, o_f2:o_p2],
                             reward=raw[t, :, o_r], ended=np.full(n, (t + 1) % L == 0))
        worst = max(worst, _ulps(got[t, :, :F], state), _ulps(got[t, :, o_f2:o_p2], nx), _ulps(got[t, :, o_r], rw))
        state = o
    print(f"end to end (particles): largest ring difference {worst} ulp")
    assert worst <= 1.0
    assert np.abs(got[..., :F] - raw[..., :F]).max() > 0.1  # the features did change
    eps = stats.episodes()
    assert len(eps) == n * (T // L) and (eps["len"] == L).all()
    for _ in range(3):
        pol.train(rings[1], 32)
    pol.sync()
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
