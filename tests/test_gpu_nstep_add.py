"""N-step adds (include/td3.h: rb_add_device_nstep, rb_add_particles_device_nstep; ``add_batch_nstep``;
``DeviceTrainLoop(n_step=)``) on an MI355X.  The expected ring is the header's closed form, computed
from the recorded inputs of every tick (never by replaying the in-place update): the row of
environment i's transition of tick t holds s_t, a_t and s'_{t+m-1} bit for bit,
not_done = gpow[m-1] * (1 - d_{t+m-1}) bit for bit, and a reward within n * 2^-23 * sum|gamma^k r_{t+k}|
of the float64 sum over the fp32 inputs ((m + 1) roundings of at most 2^-24 * sum|terms| each: one per
gpow, one per product, one per addition, with or without FMA contraction).

The particle shapes place the next-state blocks relative to the add kernel's tiles of kPutTile = 1024
record columns (td3_amd/csrc/replay.hip); if that constant changes, re-derive them.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import featured_setup, orc
from test_gpu_hindsight_add import Box, _cuda, _fring, _policy, _pring

pytestmark = pytest.mark.gpu

f32 = np.float32
GAMMA = 0.9


def _gpow(gamma, count=8):
    """gpow[j]: j factors of gamma multiplied left to right as Python floats, then fp32."""
    out, g = [], 1.0
    for _ in range(count):
        out.append(f32(g))
        g = g * gamma
    return out


def _script(t):
    """(done, ended) of three environments at tick t: environment 0 has a terminal end that only
    ``done`` reports (tick 2), a time-limit end (tick 6: ended, not done) and a terminal end with both
    set (tick 9); environment 1 ends on two consecutive ticks (4: time limit, 5: terminal);
    environment 2 never ends."""
    return [float(t in (2, 9)), float(t == 5), 0.0], [t in (6, 9), t in (4, 5), False]


def _ftick(rs, rows, sd, ad, done, ended):
    fields = [rs.standard_normal((rows, sd)).astype(f32), rs.uniform(-1, 1, (rows, ad)).astype(f32),
              rs.standard_normal((rows, sd)).astype(f32)]
    return dict(fields=fields, r=rs.standard_normal(rows).astype(f32), d=np.asarray(done, f32),
                e=np.asarray(ended, bool))


def _ptick(rs, rows, F, N, D, A, done, ended):
    fields = [rs.standard_normal((rows, F)).astype(f32), rs.standard_normal((rows, N, D)).astype(f32),
              rs.uniform(-1, 1, (rows, A)).astype(f32), rs.standard_normal((rows, F)).astype(f32),
              rs.standard_normal((rows, N, D)).astype(f32)]
    return dict(fields=fields, r=rs.standard_normal(rows).astype(f32), d=np.asarray(done, f32),
                e=np.asarray(ended, bool))


def _feed(rb, tick, n, gamma=GAMMA):
    rb.add_batch_nstep(*[_cuda(x) for x in tick["fields"]], _cuda(tick["r"]), _cuda(tick["d"]),
                       ended=_cuda(tick["e"]), n=n, gamma=gamma)


def _expected(ticks, n, gamma, n_pre):
    """The closed form after the ticks of one uninterrupted lane: (t, i) -> (the record's columns up to
    the reward, not_done, the float64 reward sum, its bound, m).  ``n_pre`` fields (state, action;
    feat, particles, action) come from tick t, the rest (the next state) from tick t + m - 1."""
    T, rows, gp = len(ticks), len(ticks[0]["r"]), _gpow(gamma)
    out = {}
    for i in range(rows):
        for t in range(T):
            e = next((u for u in range(t, T) if ticks[u]["e"][i] or ticks[u]["d"][i] != 0), None)
            m = min(n, T - t) if e is None else min(n, e - t + 1, T - t)
            last = ticks[t + m - 1]
            prefix = np.concatenate([x[i].reshape(-1) for x in ticks[t]["fields"][:n_pre]] +
                                    [x[i].reshape(-1) for x in last["fields"][n_pre:]])
            nd = gp[m - 1] * (f32(1) - last["d"][i])
            assert nd.dtype == f32
            terms = [gamma ** k * float(ticks[t + k]["r"][i]) for k in range(m)]
            out[t, i] = (prefix, nd, sum(terms), n * 2.0 ** -23 * sum(abs(x) for x in terms), m)
    return out


def _check_ring(rb, ticks, n, n_pre, gamma=GAMMA, base=0, after=0):
    """Every ring row of the lane's ticks that is still live (``after`` rows were written behind the
    lane; the lane's first row went to ring row ``base``) against the closed form; the pad is zero.
    Returns the number of rows checked and the largest horizon met."""
    rec, cap = rb._records(), rb.max_size
    T, rows = len(ticks), len(ticks[0]["r"])
    exp = _expected(ticks, n, gamma, n_pre)
    o_r = exp[0, 0][0].size
    assert rb.record_floats == -(-(o_r + 2) // 4) * 4
    assert np.all(rec[:, o_r + 2:] == 0), "record pad"
    live, deepest, worst = 0, 0, 0.0
    for (t, i), (prefix, nd, rsum, bound, m) in exp.items():
        g = t * rows + i
        if T * rows + after - g > cap:
            continue                                  # overwritten since
        row = rec[(base + g) % cap]
        np.testing.assert_array_equal(row[:o_r], prefix, err_msg=f"tick {t} row {i} m {m} of {T}")
        assert row[o_r + 1] == nd, (t, i, m, row[o_r + 1], nd)
        err = abs(float(row[o_r]) - rsum)
        assert err <= bound, (t, i, m, row[o_r], rsum, err, bound)
        live += 1
        deepest = max(deepest, m)
        worst = max(worst, err / bound if bound else 0.0)
    print(f"T={T}: {live} live rows, horizons up to {deepest}, largest reward error / bound {worst:.3f}")
    return live, deepest


# ---------------------------------------------------------------- 1: featured, closed form
@pytest.mark.parametrize("n,rows,cap", [(2, 3, 10), (3, 3, 10), (8, 3, 25)])
@pytest.mark.parametrize("sd,ad", [(17, 6), (3, 1)])
def test_featured_closed_form(sd, ad, n, rows, cap):
    """(3, 1): a record of 9 floats padded to 12 whose next-state block starts at the aligned column
    4; (17, 6): it starts at column 23, inside a 16-byte unit that also holds the action's last three
    columns.  12 ticks of 3 rows wrap both rings, so history rows lie on both sides of the wrap and
    old rows are overwritten."""
    rb = _fring(sd, ad, cap)
    rs = np.random.RandomState(sd + n)
    ticks, deepest = [], 0
    for t in range(12):
        ticks.append(_ftick(rs, rows, sd, ad, *_script(t)))
        _feed(rb, ticks[-1], n)
        T = len(ticks)
        live, m = _check_ring(rb, ticks, n, 2)
        assert live == min(rows * T, cap)
        assert (rb.ptr, rb.size) == (rows * T % cap, min(rows * T, cap))
        deepest = max(deepest, m)
    assert deepest == n          # environment 2 never ends: its rows reach the full horizon


# ---------------------------------------------------------------- 2: n = 1 is the plain add
def test_n1_is_the_plain_add():
    rs = np.random.RandomState(1)
    sd, ad, F, N, D, A = 17, 6, 7, 120, 9, 3
    for make, tick, dims in ((_fring, _ftick, (sd, ad)), (_pring, _ptick, (F, N, D, A))):
        one, twin = make(*dims, 10), make(*dims, 10)
        for t in range(5):
            k = tick(rs, 3, *dims, *_script(t))
            _feed(one, k, 1)
            twin.add_batch(*[_cuda(x) for x in k["fields"]], _cuda(k["r"]), _cuda(k["d"]))
            np.testing.assert_array_equal(one._records(), twin._records())
            assert (one.ptr, one.size) == (twin.ptr, twin.size) == (3 * (t + 1) % 10, min(3 * (t + 1), 10))


# ---------------------------------------------------------------- 3: particles, closed form
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("shape", [(7, 16, 9, 3), (3, 5, 3, 2), (7, 120, 9, 3), (7, 253, 4, 3)])
def test_particle_closed_form(shape, n):
    """One tile; N * D = 15 (odd source alignment); three tiles with next_feat in tile 1 and the
    reward in tile 2; next_feat at columns 1,022..1,028 across the tile 0 / 1 boundary."""
    F, N, D, A = shape
    rows, cap = 3, 10
    rb = _pring(F, N, D, A, cap)
    o_a, o_f2 = F + N * D, F + N * D + A
    if shape == (7, 120, 9, 3):
        assert (rb.record_floats, o_f2, 2 * (F + N * D) + A) == (2180, 1090, 2177)
    if shape == (7, 253, 4, 3):
        assert o_f2 == 1022
    rs = np.random.RandomState(N + n)
    ticks = []
    for t in range(8):
        ticks.append(_ptick(rs, rows, F, N, D, A, *_script(t)))
        _feed(rb, ticks[-1], n)
        T = len(ticks)
        live, _ = _check_ring(rb, ticks, n, 3)
        assert live == min(rows * T, cap)
        assert (rb.ptr, rb.size) == (rows * T % cap, min(rows * T, cap))
        # feat, particles and action of every live row are those of the tick that created it
        rec = rb._records()
        for u in range(max(0, T - cap // rows), T):
            for i in range(rows):
                row = rec[(u * rows + i) % cap]
                np.testing.assert_array_equal(row[:F], ticks[u]["fields"][0][i])
                np.testing.assert_array_equal(row[F:o_a], ticks[u]["fields"][1][i].reshape(-1))
                np.testing.assert_array_equal(row[o_a:o_f2], ticks[u]["fields"][2][i])


# ---------------------------------------------------------------- 4: interruption
def test_another_write_or_other_rows_start_a_new_lane():
    sd, ad, n, cap = 17, 6, 3, 40
    rs = np.random.RandomState(4)
    # three n-step ticks, a plain add of two rows, three more
    rb = _fring(sd, ad, cap)
    first = [_ftick(rs, 3, sd, ad, [0, 0, 0], [False] * 3) for _ in range(3)]
    for k in first:
        _feed(rb, k, n)
    plain = _ftick(rs, 2, sd, ad, [0, 1], [False] * 2)
    rb.add_batch(*[_cuda(x) for x in plain["fields"]], _cuda(plain["r"]), _cuda(plain["d"]))
    second = [_ftick(rs, 3, sd, ad, [0, 0, 0], [False] * 3) for _ in range(3)]
    for k in second:
        _feed(rb, k, n)
    assert (rb.ptr, rb.size) == (20, 20)
    # no episode ends anywhere: a tick of the first lane that matured further would show m = 2 or 3
    assert _check_ring(rb, first, n, 2, base=0, after=11) == (9, 3)
    assert _check_ring(rb, second, n, 2, base=11) == (9, 3)
    rec = rb._records()
    np.testing.assert_array_equal(rec[9:11, :sd], plain["fields"][0])
    np.testing.assert_array_equal(rec[9:11, 2 * sd + ad + 1], 1 - plain["d"])
    # another row count between two ticks
    rb = _fring(sd, ad, cap)
    for k in first:
        _feed(rb, k, n)
    narrow = [_ftick(rs, 2, sd, ad, [0, 0], [False] * 2) for _ in range(3)]
    for k in narrow:
        _feed(rb, k, n)
    assert (rb.ptr, rb.size) == (15, 15)
    assert _check_ring(rb, first, n, 2, base=0, after=6) == (9, 3)
    assert _check_ring(rb, narrow, n, 2, base=9) == (6, 3)
    # another horizon or another discount does too
    for kw in (dict(n=2), dict(n=3, gamma=0.5)):
        rb = _fring(sd, ad, cap)
        for k in first:
            _feed(rb, k, n)
        for k in second:
            _feed(rb, k, **kw)
        assert _check_ring(rb, first, n, 2, base=0, after=9) == (9, 3)
        assert _check_ring(rb, second, kw["n"], 2, gamma=kw.get("gamma", GAMMA), base=9) == (9, kw["n"])


# ---------------------------------------------------------------- 5: refusals
def test_refusals_leave_ring_and_lane_unchanged():
    """Each refused call returns before any GPU work (the kind mismatches are given host pointers: a
    kernel reading them would fault); ring, ptr and size stay, and the next tick matures the earlier
    rows as if the refused calls had not been made."""
    from td3_amd import _lib
    from td3_amd._lib import TD3Error
    sd, ad, F, N, D, A, n = 17, 6, 7, 16, 9, 3, 3
    frb, prb = _fring(sd, ad, 10), _pring(F, N, D, A, 10)
    rs = np.random.RandomState(3)
    ft = [_ftick(rs, 3, sd, ad, *_script(t)) for t in range(3)]
    pt = [_ptick(rs, 3, F, N, D, A, *_script(t)) for t in range(3)]
    for t in range(2):
        _feed(frb, ft[t], n)
        _feed(prb, pt[t], n)
    state = lambda: (frb._records(), frb.ptr, frb.size, prb._records(), prb.ptr, prb.size)
    ref = state()
    lib = frb._lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ns = _lib.rb_nstep()
    ns.n, ns.gamma, ns.ended = n, GAMMA, p
    err = lambda: lib.td3_last_error().decode()

    assert lib.rb_add_device_nstep(prb.handle, p, p, p, p, p, 1, ns, None) == -1
    assert "particle ring" in err() and "rb_add_particles_device_nstep" in err()
    assert lib.rb_add_particles_device_nstep(frb.handle, p, p, p, p, p, p, p, 1, ns, None) == -1
    assert "featured ring" in err() and "rb_add_device_nstep" in err()

    def feed(rb, k, **kw):
        args = dict(ended=_cuda(k["e"]), n=n, gamma=GAMMA)
        args.update(kw)
        rb.add_batch_nstep(*[_cuda(x) for x in k["fields"]], _cuda(k["r"]), _cuda(k["d"]), **args)

    for rb, k in ((frb, ft[2]), (prb, pt[2])):
        for bad, field in ((dict(n=0), "ns->n"), (dict(n=9), "ns->n"), (dict(gamma=0.0), "ns->gamma"),
                           (dict(gamma=1.5), "ns->gamma"), (dict(n=4), "max_size")):      # 4 * 3 rows > 10
            with pytest.raises(TD3Error, match=field):
                feed(rb, k, **bad)
        with pytest.raises(TypeError, match="CUDA"):
            rb.add_batch_nstep(*k["fields"], k["r"], k["d"], ended=k["e"], n=n, gamma=GAMMA)
        with pytest.raises(TypeError, match="CUDA"):
            rb.add_batch_nstep(*[_cuda(x) for x in k["fields"]], _cuda(k["r"]), _cuda(k["d"]), ended=k["e"],
                               n=n, gamma=GAMMA)
        with pytest.raises(ValueError):
            rb.add_batch_nstep(_cuda(k["fields"][0][:2]), *[_cuda(x) for x in k["fields"][1:]], _cuda(k["r"]),
                               _cuda(k["d"]), ended=_cuda(k["e"]), n=n, gamma=GAMMA)
        with pytest.raises(ValueError):
            feed(rb, k, ended=_cuda(k["e"][:2]))
    for a, b in zip(state(), ref):
        np.testing.assert_array_equal(a, b)
    _feed(frb, ft[2], n)
    _feed(prb, pt[2], n)
    assert _check_ring(frb, ft, n, 2)[0] == 9
    assert _check_ring(prb, pt, n, 3)[0] == 9
    # a tick of no rows is not a write: it returns 0 on a real ring and leaves the lane alone
    e = _cuda(np.zeros(0, bool))
    z = lambda *shape: _cuda(np.zeros(shape, f32))
    frb.add_batch_nstep(z(0, sd), z(0, ad), z(0, sd), z(0), z(0), ended=e, n=n, gamma=GAMMA)
    assert (frb.ptr, frb.size) == (9, 9)


# ---------------------------------------------------------------- 6: the learner consumes the rows
def test_learner_trains_on_matured_rows():
    S = featured_setup("hc_layer")
    sd, ad, n, rows, ticks = S["sd"], S["ad"], 3, 8, 8
    pol = _policy(S)
    rb = _fring(sd, ad, rows * ticks)
    rs = np.random.RandomState(6)
    fed = []
    for t in range(ticks):
        done = (rs.uniform(size=rows) < 0.15).astype(f32)
        ended = (rs.uniform(size=rows) < 0.15) | (done != 0)
        fed.append(_ftick(rs, rows, sd, ad, done, ended))
        _feed(rb, fed[-1], n, gamma=pol.discount)
    assert _check_ring(rb, fed, n, 2, gamma=pol.discount) == (rows * ticks, n)
    B = rows * ticks
    idx = rs.permutation(B)
    noise = rs.standard_normal((B, ad)).astype(f32)
    rec = rb._records()[idx]
    o_s2, o_r = sd + ad, 2 * sd + ad
    batch = (rec[:, :sd], rec[:, sd:o_s2], rec[:, o_s2:o_r], rec[:, o_r:o_r + 1], rec[:, o_r + 1:o_r + 2])
    nd = batch[4]
    assert np.any((nd > 0) & (nd < 1)) and np.any(nd == 0) and np.any(nd == 1)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    assert L.discount == pol.discount
    ref = orc.featured_train_step(L, batch, noise)
    out = pol.train_step(rb, B, indices=idx, noise=noise, stats=True)
    np.testing.assert_array_equal(out["idx"], idx)
    from test_gpu_parity import _rel_to_max
    for k in ("y", "q1", "q2"):
        err = _rel_to_max(out[k], ref[k][:, 0])
        print(k, "relative to max:", err)
        assert err <= 1e-5, (k, err)


# ---------------------------------------------------------------- 7: sample sees matured rows
def test_nstep_add_visible_to_sample_without_sync():
    import torch
    sd, ad, n, rows = 17, 6, 3, 16
    rb = _fring(sd, ad, 64)
    rs = np.random.RandomState(7)
    ticks = []
    for t in range(4):
        done = (rs.uniform(size=rows) < 0.2).astype(f32)
        ticks.append(_ftick(rs, rows, sd, ad, done, rs.uniform(size=rows) < 0.2))
    idx = rs.permutation(4 * rows)
    for k in ticks:
        _feed(rb, k, n)
    out = rb.sample(len(idx), indices=idx)
    torch.cuda.synchronize()
    s, a, s2, r, nd = (x.cpu().numpy() for x in out)
    exp = _expected(ticks, n, GAMMA, 2)
    horizons = set()
    for b, g in enumerate(idx):
        prefix, want_nd, rsum, bound, m = exp[g // rows, g % rows]
        np.testing.assert_array_equal(np.concatenate([s[b], a[b], s2[b]]), prefix)
        assert nd[b, 0] == want_nd
        assert abs(float(r[b, 0]) - rsum) <= bound
        horizons.add(m)
    assert horizons == {1, 2, 3}


# ---------------------------------------------------------------- 8: the loop
@pytest.mark.parametrize("done_swap", [True, False])
def test_device_train_loop_n_step(done_swap):
    import torch
    from td3_amd.loop import DeviceTrainLoop, SyntheticVecEnv
    S = featured_setup("hc_layer")
    sd, ad, rows, T, n = S["sd"], S["ad"], 8, 20, 3
    pol = _policy(S)
    rings = {}
    for n_step in (1, n):
        env = SyntheticVecEnv(rows, sd, ad, max_action=S["ma"], max_episode_steps=5, seed=3, device=pol.device)
        rb = _fring(sd, ad, 256)
        loop = DeviceTrainLoop(env, pol, rb, start_policy=T, start_training=T, batch_size=32, expl_noise=0.1,
                               done_swap=done_swap, n_step=n_step)
        torch.manual_seed(11)
        loop.run(T)
        assert (rb.ptr, rb.size) == (rows * T, rows * T)
        rings[n_step] = rb
    one = rings[1]._records()[:rows * T].reshape(T, rows, -1)
    o_s2, o_r = sd + ad, 2 * sd + ad
    ticks = []
    for t in range(T):
        k = one[t]
        ended = np.full(rows, t % 5 == 4)
        done = 1 - k[:, o_r + 1]
        np.testing.assert_array_equal(done, np.zeros(rows) if done_swap else ended.astype(f32))
        ticks.append(dict(fields=[k[:, :sd], k[:, sd:o_s2], k[:, o_s2:o_r]], r=k[:, o_r], d=done.astype(f32), e=ended))
    assert _check_ring(rings[n], ticks, n, 2, gamma=pol.discount) == (rows * T, n)
    nd = rings[n]._records()[:rows * T, o_r + 1]
    if done_swap:       # a time-limit end bootstraps: the horizon's discount, never 0
        assert set(np.unique(nd)) == {f32(x) for x in _gpow(pol.discount, n)}
    else:
        assert np.count_nonzero(nd == 0) == rows * n * 4      # the last 3 transitions of each of 4 episodes


def test_device_train_loop_n_step_refuses_relabel_and_trains():
    from td3_amd.loop import DeviceTrainLoop, SyntheticGoalVecEnv, SyntheticVecEnv, hindsight_relabel
    S = featured_setup("hc_layer")
    sd, ad, rows, T = S["sd"], S["ad"], 8, 12
    pol = _policy(S)
    genv = SyntheticGoalVecEnv(rows, sd, ad, 2, max_action=S["ma"], max_episode_steps=5, device=pol.device)
    with pytest.raises(ValueError, match="relabel"):
        DeviceTrainLoop(genv, pol, _fring(sd, ad, 256), start_policy=0, start_training=0, batch_size=32,
                        expl_noise=0.1, relabel=hindsight_relabel(2), n_step=3)
    env = SyntheticVecEnv(rows, sd, ad, max_action=S["ma"], max_episode_steps=5, device=pol.device)
    rb = _fring(sd, ad, 256)
    loop = DeviceTrainLoop(env, pol, rb, start_policy=3, start_training=5, batch_size=32, expl_noise=0.1, n_step=3)
    res = loop.run(T)
    assert res["env_steps"] == rows * T and res["grad_steps"] == T - 5 == pol.total_it
    assert rb.size == rows * T
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
    nd = rb._records()[:rb.size, 2 * sd + ad + 1]
    assert np.any((nd > 0) & (nd < 1))
