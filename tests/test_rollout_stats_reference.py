"""The numpy restatement of the rollout-statistics tick (tests/rollout_stats_reference.py) against
closed forms: after T updating ticks the running moments are numpy's mean / var over all T * rows
rows, the scaled reward divides by the spread of the discounted returns, and the log holds the
per-episode sums and lengths in row order within a tick."""
import numpy as np

from rollout_stats_reference import RolloutStatsRef, normalise


def _run(rows=5, dim=7, T=9, log_cap=64, seed=0, mask=None, update=True):
    rs = np.random.RandomState(seed)
    ref = RolloutStatsRef(rows, dim, gamma=0.9, col_mask=mask, log_cap=log_cap)
    obs = (rs.uniform(-10, 10, (T, rows, dim)) + np.arange(dim)).astype(np.float32)
    nxt = rs.uniform(-10, 10, (T, rows, dim)).astype(np.float32)
    rew = rs.uniform(-2, 2, (T, rows)).astype(np.float32)
    end = rs.uniform(size=(T, rows)) < 0.3
    outs = [ref.tick(obs[t], nxt[t], rew[t], end[t], update=update) for t in range(T)]
    return ref, obs, nxt, rew, end, outs


def test_moments_are_numpy_mean_and_var():
    ref, obs, *_ = _run()
    allrows = obs.reshape(-1, obs.shape[-1]).astype(np.float64)
    assert ref.count == allrows.shape[0]
    np.testing.assert_allclose(ref.mean, allrows.mean(axis=0), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref.m2 / ref.count, allrows.var(axis=0), rtol=1e-12)


def test_outputs_use_the_moments_after_the_update():
    ref, obs, nxt, rew, end, outs = _run(T=1)
    x = obs[0].astype(np.float64)
    want = np.clip((x - x.mean(0)) / np.sqrt(x.var(0) + 1e-8), -10, 10)
    np.testing.assert_allclose(outs[0][0], want, rtol=1e-6, atol=1e-6)
    y = nxt[0].astype(np.float64)
    want = np.clip((y - x.mean(0)) / np.sqrt(x.var(0) + 1e-8), -10, 10)
    np.testing.assert_allclose(outs[0][1], want, rtol=1e-6, atol=1e-6)
    g = rew[0].astype(np.float64)                      # the first G is the reward itself
    np.testing.assert_allclose(outs[0][2], np.clip(g / np.sqrt(g.var() + 1e-8), -10, 10), rtol=1e-6)
    assert outs[0][0].dtype == outs[0][2].dtype == np.float32


def test_return_moments_follow_the_discounted_return():
    ref, obs, nxt, rew, end, _ = _run()
    G, seen = np.zeros(rew.shape[1]), []
    for t in range(rew.shape[0]):
        G = 0.9 * G + rew[t]
        seen.append(G.copy())
        G[end[t]] = 0.0
    seen = np.concatenate(seen)
    assert ref.ret_count == seen.size
    np.testing.assert_allclose(ref.ret_mean, seen.mean(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref.ret_m2 / ref.ret_count, seen.var(), rtol=1e-12)


def test_log_holds_episode_sums_in_row_order():
    ref, obs, nxt, rew, end, _ = _run()
    want, start = [], np.zeros(rew.shape[1], int)
    for t in range(rew.shape[0]):
        for i in np.flatnonzero(end[t]):               # increasing row order within the tick
            seg = rew[start[i]:t + 1, i].astype(np.float64)
            want.append((np.float32(seg.sum()), t + 1 - start[i], i, t))
            start[i] = t + 1
    got = ref.episodes()
    assert len(got) == len(want) == ref.ep_count and ref.tick_no == rew.shape[0]
    for g, w in zip(got, want):
        assert g[1:] == tuple(int(v) for v in w[1:])
        assert abs(float(g[0]) - float(w[0])) <= 4e-7 * max(1.0, abs(float(w[0])))
    assert ref.ep_len_sum == sum(w[1] for w in want)
    np.testing.assert_allclose(ref.ep_return_sum, sum(float(w[0]) for w in want), rtol=1e-6, atol=1e-6)


def test_log_wraps_and_keeps_the_newest():
    ref, *_ = _run(log_cap=4)
    full, *_ = _run(log_cap=64)
    assert ref.ep_count == full.ep_count > 4
    assert ref.episodes() == full.episodes()[-4:]


def test_frozen_moments_and_masked_columns():
    mask = np.array([1, 0, 1, 1, 0, 1, 1], np.uint8)
    ref, obs, nxt, rew, end, outs = _run(mask=mask)
    assert (ref.mean[mask == 0] == 0).all() and (ref.m2[mask == 0] == 0).all()
    for t in range(obs.shape[0]):
        assert np.array_equal(outs[t][0][:, mask == 0].view(np.uint32), obs[t][:, mask == 0].view(np.uint32))
    before = (ref.count, ref.mean.copy(), ref.m2.copy(), ref.ret_count, ref.ret_mean, ref.ret_m2, ref.ep_count)
    o, n, r = ref.tick(obs[0], nxt[0], rew[0], np.ones(obs.shape[1], bool), update=False)
    assert (ref.count, ref.ret_count, ref.ret_mean, ref.ret_m2) == (before[0], before[3], before[4], before[5])
    assert np.array_equal(ref.mean, before[1]) and np.array_equal(ref.m2, before[2])
    assert ref.ep_count == before[6] + obs.shape[1]    # episodes are logged all the same
    assert np.array_equal(o, normalise(obs[0], ref.count, ref.mean, ref.m2, 1e-8, 10.0, mask))


def test_no_moments_yet_passes_through():
    ref = RolloutStatsRef(3, 2, gamma=0.9)
    x = np.arange(6, dtype=np.float32).reshape(3, 2)
    o, _, r = ref.tick(obs=x, reward=np.ones(3, np.float32), update=False)
    assert np.array_equal(o, x) and np.array_equal(r, np.ones(3, np.float32))
