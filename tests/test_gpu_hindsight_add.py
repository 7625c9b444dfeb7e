"""Hindsight fan-out adds (include/td3.h: rb_add_device_hindsight, rb_add_particles_device_hindsight;
``add_batch_hindsight``; ``DeviceTrainLoop(relabel=)``) on an MI355X.  The expected ring comes from a
twin ring fed the n * (1 + K) expanded rows of main.py:70-91, built with numpy here, through the
existing device ``add_batch``: the add is pure data movement, so every comparison of ring contents
is bit-exact and no tolerance is involved (the one exception is the loop's recomputed reward, an
fp32 torch op, at ``test_gpu_device_rollout._close``).

The particle shapes place the relabelled columns relative to the add kernel's tiles of
kPutTile = 1024 record columns (td3_amd/csrc/replay.hip); if that constant changes, re-derive them.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import featured_setup

pytestmark = pytest.mark.gpu

CAP = 10
ADDS = (2, 3, 9)          # with K = 3: 8, 12 (wraps inside a transition) and 36 rows (skip 26: copy 2 first)
CASES = [(1, 1, [2]), (3, 2, [2, 0])]     # (K, G, cols); the unsorted columns are deliberate


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _fring(sd, ad, rows, **kw):
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    return ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=rows, **kw)


def _pring(F, N, D, A, rows, **kw):
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    return ReplayBuffer_particles((Box((F,)), Box((N, D))), Box((A,)), max_size=rows, **kw)


def _cuda(x):
    import torch
    return torch.as_tensor(x).cuda()


def _relabels(rs, n, K, G, dtype):
    return rs.standard_normal((n, K, G)).astype(dtype), rs.standard_normal((n, K)).astype(dtype)


def _expand(arrs, state_slots, reward_slot, cols, goals, rewards):
    """E of the header: row i * (1 + K) is transition i, rows i * (1 + K) + j its relabels."""
    n, K = rewards.shape
    out = []
    for k, a in enumerate(arrs):
        e = np.repeat(a[:, None], 1 + K, axis=1).copy()          # [n][1 + K][...]
        if k in state_slots:
            for q, c in enumerate(cols):
                e[:, 1:, c] = goals[:, :, q]
        if k == reward_slot:
            e[:, 1:] = rewards
        out.append(e.reshape((n * (1 + K),) + a.shape[1:]))
    return out


def _same_ring(got, ref, used):
    rg, rr = got._records(), ref._records()
    np.testing.assert_array_equal(rg, rr)
    assert (got.ptr, got.size) == (ref.ptr, ref.size)
    assert np.all(rg[:, used:] == 0), "record pad"
    return rg


def _not_fp32(x):
    return not np.array_equal(x, x.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------- 1: featured
def _featured_rows(rs, n, sd, ad, dtype):
    return (rs.standard_normal((n, sd)).astype(dtype), rs.uniform(-1, 1, (n, ad)).astype(dtype),
            rs.standard_normal((n, sd)).astype(dtype), rs.standard_normal(n).astype(dtype),
            (rs.uniform(size=n) < 0.3).astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K,G,cols", CASES)
@pytest.mark.parametrize("sd,ad", [(17, 6), (3, 1)])
def test_featured_fanout_bit_exact(sd, ad, K, G, cols, dtype):
    """(3, 1): a record of 9 floats padded to 12.  Adds of 2, 3 and 9 transitions into 10 rows; after
    each, records, ptr and size equal the twin's, the pad is zero.  float64 inputs that fp32 cannot
    represent are rounded once on both paths."""
    fan, twin = _fring(sd, ad, CAP), _fring(sd, ad, CAP)
    used = 2 * sd + ad + 2
    assert fan.record_floats == -(-used // 4) * 4
    rs = np.random.RandomState(sd + K)
    total = 0
    for n in ADDS:
        t = _featured_rows(rs, n, sd, ad, dtype)
        goals, rewards = _relabels(rs, n, K, G, dtype)
        if dtype is np.float64:
            assert _not_fp32(t[0]) and _not_fp32(goals) and _not_fp32(rewards)
        fan.add_batch_hindsight(*[_cuda(x) for x in t], goal_cols=cols, goals=_cuda(goals), rewards=_cuda(rewards))
        twin.add_batch(*[_cuda(x) for x in _expand(t, (0, 2), 3, cols, goals, rewards)])
        rec = _same_ring(fan, twin, used)
        total += n * (1 + K)
        assert (fan.ptr, fan.size) == (total % CAP, min(total, CAP))
    if K == 3:      # the last add kept expanded rows 26..35 of 36: ring row ptr holds copy 2 of transition 6
        e = _expand(t, (0, 2), 3, cols, goals, rewards)
        first = rec[fan.ptr]
        np.testing.assert_array_equal(first[:sd], e[0][26].astype(np.float32))
        assert first[2 * sd + ad] == np.float32(rewards[6, 1])
        np.testing.assert_array_equal(first[cols], goals[6, 1].astype(np.float32))


# ---------------------------------------------------------------- 2: particles
def _particle_rows(rs, n, F, N, D, A, dtype):
    return (rs.standard_normal((n, F)).astype(dtype), rs.standard_normal((n, N, D)).astype(dtype),
            rs.uniform(-1, 1, (n, A)).astype(dtype), rs.standard_normal((n, F)).astype(dtype),
            rs.standard_normal((n, N, D)).astype(dtype), rs.standard_normal(n).astype(dtype),
            (rs.uniform(size=n) < 0.3).astype(dtype))


PARTICLE_CASES = [
    # one tile; the particle block starts unaligned at record column 7
    ((7, 16, 9, 3), 1, [2]), ((7, 16, 9, 3), 3, [2, 0]),
    # N * D = 15: the source rows start at odd 4-byte offsets
    ((3, 5, 3, 2), 1, [2]), ((3, 5, 3, 2), 3, [2, 0]),
    # record 2,180 floats, three tiles: feat in tile 0, next_feat (from column 1,090) in tile 1, the
    # reward (column 2,177) in tile 2 -- every patch lands in a different tile
    ((7, 120, 9, 3), 1, [2]), ((7, 120, 9, 3), 3, [2, 0]),
    # next_feat at columns 1,022..1,028 straddles the tile 0 / 1 boundary; goal columns 0 and 6 (and
    # 2, the first column of tile 1) fall on both sides of it
    ((7, 253, 4, 3), 1, [2]), ((7, 253, 4, 3), 3, [2, 0]), ((7, 253, 4, 3), 3, [0, 6]),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,K,cols", PARTICLE_CASES)
def test_particle_fanout_bit_exact(shape, K, cols, dtype):
    F, N, D, A = shape
    G = len(cols)
    fan, twin = _pring(F, N, D, A, CAP), _pring(F, N, D, A, CAP)
    o_a, o_f2 = F + N * D, F + N * D + A
    o_p2, o_r = o_f2 + F, 2 * (F + N * D) + A
    used = o_r + 2
    if shape == (7, 120, 9, 3):
        assert (fan.record_floats, o_f2, o_r) == (2180, 1090, 2177)
    if shape == (7, 253, 4, 3):
        assert o_f2 == 1022
    rs = np.random.RandomState(N + K)
    total = 0
    for n in ADDS:
        t = _particle_rows(rs, n, F, N, D, A, dtype)
        goals, rewards = _relabels(rs, n, K, G, dtype)
        if dtype is np.float64:
            assert _not_fp32(t[1]) and _not_fp32(goals)
        before = fan.ptr
        fan.add_batch_hindsight(*[_cuda(x) for x in t], goal_cols=cols, goals=_cuda(goals), rewards=_cuda(rewards))
        twin.add_batch(*[_cuda(x) for x in _expand(t, (0, 3), 5, cols, goals, rewards)])
        rec = _same_ring(fan, twin, used)
        total += n * (1 + K)
        assert (fan.ptr, fan.size) == (total % CAP, min(total, CAP))
        if n * (1 + K) > CAP:
            continue
        # every stored copy against its SOURCE transition (not through the expansion above)
        f32 = [x.astype(np.float32).reshape(n, -1) for x in t]
        for i in range(n):
            for j in range(1 + K):
                row = rec[(before + i * (1 + K) + j) % CAP]
                np.testing.assert_array_equal(row[F:o_a], f32[1][i])            # particles
                np.testing.assert_array_equal(row[o_p2:o_r], f32[4][i])         # next particles
                np.testing.assert_array_equal(row[o_a:o_f2], f32[2][i])         # action
                assert row[o_r + 1] == np.float32(1) - f32[6][i, 0]             # not_done
                if j == 0:
                    np.testing.assert_array_equal(row[:F], f32[0][i])
                    np.testing.assert_array_equal(row[o_f2:o_p2], f32[3][i])
                    assert row[o_r] == f32[5][i, 0]
                else:
                    keep = [c for c in range(F) if c not in cols]
                    g = goals[i, j - 1].astype(np.float32)
                    np.testing.assert_array_equal(row[:F][cols], g)
                    np.testing.assert_array_equal(row[o_f2:o_p2][cols], g)
                    np.testing.assert_array_equal(row[:F][keep], f32[0][i][keep])
                    np.testing.assert_array_equal(row[o_f2:o_p2][keep], f32[3][i][keep])
                    assert row[o_r] == np.float32(rewards[i, j - 1])


# ---------------------------------------------------------------- 3: sample sees the expanded rows
def test_hindsight_add_visible_to_sample_without_sync():
    import torch
    F, N, D, A, n, K, cols = 7, 16, 9, 3, 16, 3, [5, 1]
    rb = _pring(F, N, D, A, 64)
    rs = np.random.RandomState(5)
    t = _particle_rows(rs, n, F, N, D, A, np.float32)
    goals, rewards = _relabels(rs, n, K, 2, np.float32)
    rb.add_batch_hindsight(*[_cuda(x) for x in t], goal_cols=cols, goals=_cuda(goals), rewards=_cuda(rewards))
    idx = np.random.RandomState(6).permutation(n * (1 + K))
    out = rb.sample(len(idx), indices=idx)
    torch.cuda.synchronize()
    f, p, a, f2, p2, r, nd = (x.cpu().numpy() for x in out)
    i, j = idx // (1 + K), idx % (1 + K)
    np.testing.assert_array_equal(p, t[1][i])
    np.testing.assert_array_equal(p2, t[4][i])
    np.testing.assert_array_equal(a, t[2][i])
    np.testing.assert_array_equal(nd[:, 0], 1 - t[6][i])
    rel = j > 0
    np.testing.assert_array_equal(f[rel][:, cols], goals[i[rel], j[rel] - 1])       # the goals in feat ...
    np.testing.assert_array_equal(f2[rel][:, cols], goals[i[rel], j[rel] - 1])      # ... and in next_feat
    np.testing.assert_array_equal(r[rel, 0], rewards[i[rel], j[rel] - 1])           # a reward per copy
    np.testing.assert_array_equal(f[~rel], t[0][i[~rel]])
    np.testing.assert_array_equal(r[~rel, 0], t[5][i[~rel]])

    sd, ad = 17, 6
    frb = _fring(sd, ad, 64)
    ft = _featured_rows(rs, n, sd, ad, np.float32)
    g1, r1 = _relabels(rs, n, K, 1, np.float32)
    frb.add_batch_hindsight(*[_cuda(x) for x in ft], goal_cols=[16], goals=_cuda(g1[:, :, 0]), rewards=_cuda(r1))
    s, a, s2, r, nd = (x.cpu().numpy() for x in frb.sample(len(idx), indices=idx))
    es, ea, es2, er, ed = _expand(ft, (0, 2), 3, [16], g1, r1)
    for got, ref in ((s, es), (a, ea), (s2, es2), (r[:, 0], er), (nd[:, 0], 1 - ed)):
        np.testing.assert_array_equal(got, ref[idx])


# ---------------------------------------------------------------- 4: the host path
def test_host_inputs_match_cuda_inputs_and_round_trip(tmp_path):
    K, cols = 3, [2, 0]
    rs = np.random.RandomState(9)
    sd, ad = 17, 6
    dev, host = _fring(sd, ad, CAP), _fring(sd, ad, CAP, host_shadow=True)
    for n in ADDS[:2]:                           # 8 + 12 rows: the second add wraps
        t = _featured_rows(rs, n, sd, ad, np.float64)
        goals, rewards = _relabels(rs, n, K, 2, np.float64)
        dev.add_batch_hindsight(*[_cuda(x) for x in t], goal_cols=cols, goals=_cuda(goals), rewards=_cuda(rewards))
        host.add_batch_hindsight(*t, goal_cols=cols, goals=goals, rewards=rewards)
        _same_ring(host, dev, 2 * sd + ad + 2)
    # the float64 shadow holds the expanded rows unrounded; save -> load keeps them and the ring
    e = _expand(t, (0, 2), 3, cols, goals, rewards)
    assert host._shadow.valid
    last = (host.ptr - 1) % CAP
    np.testing.assert_array_equal(host._shadow.arrays["state"][last], e[0][-1])
    np.testing.assert_array_equal(host._shadow.arrays["reward"][last, 0], rewards[-1, -1])
    host.save(str(tmp_path / "f"))
    back = _fring(sd, ad, 1, load_folder=str(tmp_path / "f"), host_shadow=True)
    _same_ring(back, host, 2 * sd + ad + 2)
    for name, arr in host._shadow.arrays.items():
        np.testing.assert_array_equal(back._shadow.arrays[name], arr)
    assert _not_fp32(back._shadow.arrays["state"])

    F, N, D, A = 3, 5, 3, 2
    pdev, phost = _pring(F, N, D, A, CAP), _pring(F, N, D, A, CAP, host_shadow=True)
    for n in ADDS:
        t = _particle_rows(rs, n, F, N, D, A, np.float64)
        goals, rewards = _relabels(rs, n, K, 2, np.float64)
        pdev.add_batch_hindsight(*[_cuda(x) for x in t], goal_cols=cols, goals=_cuda(goals), rewards=_cuda(rewards))
        phost.add_batch_hindsight(*t, goal_cols=cols, goals=goals, rewards=rewards)
        _same_ring(phost, pdev, 2 * (F + N * D) + A + 2)
    phost.save(str(tmp_path / "p"))
    pback = _pring(F, N, D, A, 1, load_folder=str(tmp_path / "p"), host_shadow=True)
    _same_ring(pback, phost, 2 * (F + N * D) + A + 2)
    for name, arr in phost._shadow.arrays.items():
        np.testing.assert_array_equal(pback._shadow.arrays[name], arr)
    # a device add writes rows the host never saw: the shadow is invalid and save writes the fp32 ring
    for ring, rows in ((_fring(sd, ad, CAP, host_shadow=True), _featured_rows(rs, 2, sd, ad, np.float64)),
                       (_pring(F, N, D, A, CAP, host_shadow=True), _particle_rows(rs, 2, F, N, D, A, np.float64))):
        goals, rewards = _relabels(rs, 2, K, 2, np.float64)
        assert ring._shadow.valid
        ring.add_batch_hindsight(*[_cuda(x) for x in rows], goal_cols=cols, goals=_cuda(goals), rewards=_cuda(rewards))
        assert not ring._shadow.valid
        ring.save(str(tmp_path / "d"))
        saved = np.load(str(tmp_path / "d" / "reward.pkl"))
        np.testing.assert_array_equal(saved[1:1 + K, 0], rewards[0].astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------- 5: refusals
def _hs(K, cols, buf):
    from td3_amd import _lib
    hs = _lib.rb_hindsight()
    hs.k, hs.g = K, len(cols)
    for j, c in enumerate(cols):
        hs.cols[j] = c
    hs.goals = hs.rewards = C.cast(buf, C.c_void_p)
    return hs


def test_refusals_leave_the_ring_unchanged():
    """Kind mismatches and out-of-range columns return -1 before any GPU work (the pointers given are
    host memory: a kernel reading them would fault); a row-count mismatch is a ValueError before any
    call into the library."""
    sd, ad, F, N, D, A = 17, 6, 7, 16, 9, 3
    frb, prb = _fring(sd, ad, 8), _pring(F, N, D, A, 8)
    rs = np.random.RandomState(3)
    ft, pt = _featured_rows(rs, 3, sd, ad, np.float32), _particle_rows(rs, 3, F, N, D, A, np.float32)
    frb.add_batch(*[_cuda(x) for x in ft])
    prb.add_batch(*[_cuda(x) for x in pt])
    state = lambda: (frb._records(), frb.ptr, frb.size, prb._records(), prb.ptr, prb.size)
    ref = state()
    lib = frb._lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.td3_last_error().decode()

    assert lib.rb_add_device_hindsight(prb.handle, p, p, p, p, p, 1, _hs(2, [1], buf), None) == -1
    assert "particle ring" in err() and "rb_add_particles_device_hindsight" in err()
    assert lib.rb_add_particles_device_hindsight(frb.handle, p, p, p, p, p, p, p, 1, _hs(2, [1], buf), None) == -1
    assert "featured ring" in err() and "rb_add_device_hindsight" in err()
    assert lib.rb_add_device_hindsight(frb.handle, p, p, p, p, p, 1, _hs(2, [1, sd], buf), None) == -1
    assert "hs->cols" in err() and "state_dim" in err()
    assert lib.rb_add_particles_device_hindsight(prb.handle, p, p, p, p, p, p, p, 1, _hs(2, [F], buf), None) == -1
    assert "hs->cols" in err() and "feat_dim" in err()

    from td3_amd._lib import TD3Error
    g, r = _cuda(np.zeros((3, 2, 1), np.float32)), _cuda(np.zeros((3, 2), np.float32))
    cf, cp = [_cuda(x) for x in ft], [_cuda(x) for x in pt]
    with pytest.raises(TD3Error, match="state_dim"):
        frb.add_batch_hindsight(*cf, goal_cols=[sd], goals=g, rewards=r)
    with pytest.raises(TD3Error, match="feat_dim"):
        prb.add_batch_hindsight(*cp, goal_cols=[F], goals=g, rewards=r)
    with pytest.raises(ValueError):
        frb.add_batch_hindsight(*cf, goal_cols=[0], goals=g[:2], rewards=r[:2])
    with pytest.raises(ValueError):
        frb.add_batch_hindsight(cf[0], cf[1][:2], *cf[2:], goal_cols=[0], goals=g, rewards=r)
    with pytest.raises(ValueError):
        prb.add_batch_hindsight(*cp, goal_cols=[0, 1], goals=g, rewards=r)
    with pytest.raises(ValueError):
        prb.add_batch_hindsight(*cp[:6], cp[6][:1], goal_cols=[0], goals=g, rewards=r)
    with pytest.raises(ValueError):
        frb.add_batch_hindsight(*ft, goal_cols=[0], goals=np.zeros((3, 2, 1)), rewards=np.zeros((2, 2)))
    now = state()
    for a, b in zip(now, ref):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- 6: the loop
def _close(got, ref, scale):
    """tests/test_gpu_device_rollout._close: 1e-6 * scale + 1e-6 * |x|, the rounding of a few fp32
    operations (a relative 2^-24 = 6e-8 each), with or without FMA contraction."""
    return np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * scale + 1e-6 * np.abs(ref))


def _policy(S):
    from td3_amd.TD3_featured import TD3
    pol = TD3(Box((S["sd"],)), Box((S["ad"],)), max_action=S["ma"], norm=S["norm"], lr=1e-4, seed=7, init="none")
    pol.set_weights(S["actor"], S["critic"])
    return pol


def test_device_train_loop_with_relabels():
    from td3_amd.loop import DeviceTrainLoop, SyntheticGoalVecEnv, hindsight_relabel
    S = featured_setup("hc_layer")
    sd, ad, G, K, n, ticks = S["sd"], S["ad"], 2, 2, 8, 20
    pol = _policy(S)
    env = SyntheticGoalVecEnv(n, sd, ad, G, max_action=S["ma"], max_episode_steps=7, device=pol.device)
    assert env.goal_cols == [sd - 2, sd - 1] and env.observation_space.shape == (sd,)
    rb = _fring(sd, ad, 1024)
    loop = DeviceTrainLoop(env, pol, rb, start_policy=3, start_training=5, batch_size=32, expl_noise=0.1,
                           relabel=hindsight_relabel(K))
    res = loop.run(ticks)
    assert res["env_steps"] == n * ticks and res["grad_steps"] == ticks - 5 == pol.total_it
    assert rb.size == n * (1 + K) * ticks == rb.ptr
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
    rec = rb._records()[:rb.size].reshape(n * ticks, 1 + K, -1)
    o_s2, o_r = sd + ad, 2 * sd + ad
    same = np.ones(rec.shape[2], bool)
    same[env.goal_cols] = same[[o_s2 + c for c in env.goal_cols]] = same[o_r] = False
    P = sd - G
    for j in (1, 2):
        np.testing.assert_array_equal(rec[:, j][:, same], rec[:, 0][:, same])
        assert np.all(rec[:, j][:, ~same] != rec[:, 0][:, ~same])          # fresh goals, another reward
        np.testing.assert_array_equal(rec[:, j, sd - G:sd], rec[:, j, o_s2 + sd - G:o_s2 + sd])
    # every stored reward (copy 0 included) is imagine_reward of the row's own goals, recomputed in float64
    p2 = rec[:, :, o_s2:o_s2 + P].astype(np.float64)
    w = rec[:, :, o_s2 + P:o_s2 + sd].astype(np.float64)
    want = -(p2 * p2).sum(axis=2) / P + (w * p2[:, :, :G]).sum(axis=2)
    assert _close(rec[:, :, o_r], want, 1.0 + G)     # |p'| < 1 (tanh), w in [0, 1): every term is below 1 + G
    assert np.all(rec[:, :, o_r + 1] == 1.0)         # time-limit ends are not terminal (done swap)
    assert np.unique(rec[:, 0, sd - G:sd], axis=0).shape[0] > n      # episodes of 7 ticks: goals redrawn at reset


def test_device_train_loop_without_relabel_is_unchanged():
    """relabel=None makes the calls the loop made before: the ring equals one filled by direct
    add_batch calls on an environment of the same seed under the same torch seed (uniform actions
    throughout: start_policy beyond the run)."""
    import torch
    from td3_amd.loop import DeviceTrainLoop, SyntheticGoalVecEnv
    S = featured_setup("hc_layer")
    sd, ad, n, ticks = S["sd"], S["ad"], 8, 12
    pol = _policy(S)
    rings = []
    for direct in (False, True):
        env = SyntheticGoalVecEnv(n, sd, ad, 2, max_action=S["ma"], max_episode_steps=5, seed=3, device=pol.device)
        rb = _fring(sd, ad, 64)
        loop = DeviceTrainLoop(env, pol, rb, start_policy=ticks, start_training=ticks, batch_size=32, expl_noise=0.1)
        assert loop.relabel is None
        torch.manual_seed(11)
        if not direct:
            loop.run(ticks)
        else:
            state = env.reset()
            for _ in range(ticks):
                action = (torch.rand((n, ad), device=pol.device, dtype=torch.float32) * 2 - 1) * float(pol.max_action)
                s2, r, d, tl = env.step(action)
                rb.add_batch(state, action, s2, r, d & ~tl)
                state = env.state
        rings.append((rb._records(), rb.ptr, rb.size))
    np.testing.assert_array_equal(rings[0][0], rings[1][0])
    assert rings[0][1:] == rings[1][1:] == ((n * ticks) % 64, 64)
    assert np.abs(rings[0][0]).max() > 0
