"""Dataset normalisation on an MI355X (include/td3.h: rb_state_moments, rb_normalize_states, rb_norm_info;
ReplayBuffer_*.state_moments / normalize_states) against the float64 reference
(tests/ring_moments_reference.py) and rs_tick's own normalisation.

Shapes.  State widths 1, 3, 17 (HalfCheetah), 64 / 65 (a ragged 128-wide column mapping), 376 (Humanoid:
two blocks of 256 columns, the field staged without the rest of the record); sizes 1, 63, R - 1, R, R + 1,
2R + 1 and 5000 rows with R = 1024 the documented row chunk; every size on a partly filled ring (cap >
size) and on a wrapped one (size = cap, ptr mid-ring).  The wide cases carry the cancellation column
1e3 + 1e-2 N(0, 1) of tests/test_ring_moments_reference.py.

Bounds.  count exact.  |mean - ref| <= 1e-11 mean|x| per column: any order of n fp64 additions is within
n 2^-53 sum|x| / n of the exact mean, 5.6e-13 mean|x| at n = 5000; the bound is 20 times that.  m2 within
1e-9 relative: the sound algorithm is 1e-13 off on the cancellation column and a raw sum of squares
1e-5 (the CPU test).  Normalised values: the numpy expression on the moments read back from the device,
within 1 fp32 ulp -- the bound tests/test_gpu_rollout_stats.py holds rs_tick to.  Everything else is
bit for bit."""
import numpy as np
import pytest

from helpers import featured_setup_dims, gen, orc
from ring_moments_reference import CHUNK as R, cancellation_column, merged, moments, normalise

pytestmark = pytest.mark.gpu

EPS, CLIP = 1e-8, 10.0
WIDTHS = {1: 1, 3: 1, 17: 6, 64: 1, 65: 6, 376: 6}          # sd -> ad
SIZES = [1, 63, R - 1, R, R + 1, 2 * R + 1, 5000]
PART = (7, 16, 9, 3)                                          # per_particles_reference.setup("b20")'s dims


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    step = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / step).max()) if a.size else 0.0


def _rows(sd, ad, n, seed=0):
    """Featured transitions: states |x| <= 10 about a column-dependent offset; column 2 of a wide state is
    the cancellation column."""
    rs = np.random.RandomState(1000 * sd + n + seed)
    off = 5.0 * np.sin(np.arange(sd))
    s = rs.uniform(-5, 5, (n, sd)) + off
    s2 = rs.uniform(-5, 5, (n, sd)) + off
    if sd >= 17:
        s[:, 2] = cancellation_column(n, seed=seed + 1)
        s2[:, 2] = cancellation_column(n, seed=seed + 2)
    return (s.astype(np.float32), rs.uniform(-1, 1, (n, ad)).astype(np.float32), s2.astype(np.float32),
            rs.standard_normal(n).astype(np.float32), (rs.uniform(size=n) < 0.1).astype(np.float32))


def _ring(sd, ad, cap, rows=None, **kw):
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    rb = ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=cap, **kw)
    if rows is not None:
        rb.add_batch(*rows)
    return rb


def _prows(n, seed=0):
    F, N, D, A = PART
    f, p, a, f2, p2, r, d = gen.fill_particle_buffer(F, N, D, A, n, gen.SEED + seed)
    off = 3.0 * np.cos(np.arange(F))
    return tuple(np.asarray(x, np.float32) for x in (2.0 * f + off, p, a, 2.0 * f2 + off, p2, r, d))


def _pring(cap, rows=None, **kw):
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    F, N, D, A = PART
    rb = ReplayBuffer_particles((Box((F,)), Box((N, D))), Box((A,)), max_size=cap, **kw)
    if rows is not None:
        rb.add_batch(*rows)
    return rb


def _stats(dim, n_envs=1, mask=None, **kw):
    from td3_amd.rollout_stats import RolloutStats
    return RolloutStats(n_envs, dim, gamma=0.99, obs_clip=CLIP, eps=EPS, col_mask=mask, **kw)


def _mask(dim):
    m = np.ones(dim, np.uint8)
    if dim >= 3:
        m[1] = m[dim - 1] = 0
    return m


def _check_moments(sd, ref, what, mask=None):
    """``sd`` (a state_dict) against ``ref`` = (count, mean, m2, mean|x|) within the module's bounds."""
    count, mean, m2, mabs = ref
    on = np.ones(mean.shape, bool) if mask is None else np.asarray(mask) != 0
    dm = np.abs(sd["mean"] - mean)[on]
    dq = (np.abs(sd["m2"] - m2) / np.where(m2 > 0, m2, 1.0))[on]
    print(f"{what}: count {sd['count']:.0f}, worst dmean / mean|x| {np.max(dm / mabs[on]):.2e} (bound 1e-11), "
          f"worst dm2 / m2 {dq.max():.2e} (bound 1e-9)")
    assert sd["count"] == count, what
    assert (dm <= 1e-11 * mabs[on]).all(), what
    assert (dq <= 1e-9).all(), what


_refs = {}


def _ref(sd, n):
    """The rows of one (sd, n) and their float64 moments, computed once and left unchanged."""
    if (sd, n) not in _refs:
        rows = _rows(sd, WIDTHS[sd], n)
        _refs[sd, n] = rows, moments(rows[0]) + (np.abs(rows[0].astype(np.float64)).mean(axis=0),)
    return _refs[sd, n]


# ---------------------------------------------------------------- 1: moments
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sd", list(WIDTHS))
def test_moments_against_the_float64_reference(sd, n):
    rows, ref = _ref(sd, n)
    ad = WIDTHS[sd]
    part = _ring(sd, ad, n + 5, rows)                        # partly filled
    assert (part.size, part.ptr) == (n, n)
    _check_moments(part.state_moments().state_dict(), ref, f"sd {sd} n {n} partly filled")
    k = n // 2                                               # wrapped: the same n rows, rotated by k
    wrap = _ring(sd, ad, n, tuple(np.concatenate([x[:k], x]) for x in rows))
    assert (wrap.size, wrap.ptr) == (n, k % n)
    _check_moments(wrap.state_moments().state_dict(), ref, f"sd {sd} n {n} wrapped")


def test_moments_of_a_particle_ring():
    rows = _prows(R + 7)
    rb = _pring(R + 9, rows)
    ref = moments(rows[0]) + (np.abs(rows[0].astype(np.float64)).mean(axis=0),)
    st = rb.state_moments()
    assert st.obs_dim == PART[0]
    _check_moments(st.state_dict(), ref, "particle ring")


# ---------------------------------------------------------------- 2: repeatability
@pytest.mark.parametrize("sd,n", [(17, 5000), (376, 2 * R + 1), (3, R + 1)])
def test_moments_repeat_bit_for_bit(sd, n):
    import torch
    rows, _ = _ref(sd, n)
    a, b = _ring(sd, WIDTHS[sd], n + 5, rows), _ring(sd, WIDTHS[sd], n + 3, rows)
    sa, sb = a.state_moments().state_dict(), b.state_moments().state_dict()
    own = _stats(sd)
    assert a._lib.rb_state_moments(a.handle, own._h, 0, None) == 0        # the ring's own stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sc = a.state_moments().state_dict()                               # a side stream of the caller's
    so = own.state_dict()
    for k in ("count", "mean", "m2"):
        for other in (sb, sc, so):
            assert np.asarray(sa[k]).tobytes() == np.asarray(other[k]).tobytes(), k


# ---------------------------------------------------------------- 3: column mask
@pytest.mark.parametrize("sd", [3, 17, 376])
def test_masked_columns_are_left_alone(sd):
    n = R + 1
    rows, ref = _ref(sd, n)
    mask = _mask(sd)
    rb = _ring(sd, WIDTHS[sd], n + 5, rows)
    st = _stats(sd, mask=mask)
    seed = st.state_dict()
    seed["count"], seed["mean"], seed["m2"] = np.float64(5.0), np.full(sd, 7.0), np.full(sd, 3.0)
    st.load_state_dict(seed)
    assert rb.state_moments(st) is st
    sd_ = st.state_dict()
    off = mask == 0
    assert (sd_["mean"][off] == 7.0).all() and (sd_["m2"][off] == 3.0).all()
    _check_moments(sd_, ref, f"sd {sd} masked", mask)
    before = rb._records()
    rb.normalize_states(st)
    after = rb._records()
    ad = WIDTHS[sd]
    for o in (0, sd + ad):
        assert after[:, o:o + sd][:, off].tobytes() == before[:, o:o + sd][:, off].tobytes()
        on = ~off
        want = normalise(before[:n, o:o + sd], sd_["count"], sd_["mean"], sd_["m2"], EPS, CLIP, mask)
        assert _ulps(after[:n, o:o + sd][:, on], want[:, on]) <= 1.0
        assert (after[:n, o:o + sd][:, on] != before[:n, o:o + sd][:, on]).any()


# ---------------------------------------------------------------- 4: merge
def test_merge_of_two_rings_and_into_a_ticked_handle():
    import torch
    sd, ad = 65, 6
    ra, rb_ = _rows(sd, ad, R + 5, seed=1), _rows(sd, ad, 700, seed=2)
    a, b = _ring(sd, ad, R + 9, ra), _ring(sd, ad, 701, rb_)
    both = np.concatenate([ra[0], rb_[0]])
    ref = moments(both) + (np.abs(both.astype(np.float64)).mean(axis=0),)
    st = a.state_moments()
    b.state_moments(st, merge=True)
    _check_moments(st.state_dict(), ref, "ring A merged with ring B")
    # into a handle that has ticked: 4 rows of 65 columns make two column workgroups, so two count copies
    n_envs = 4
    tk = _stats(sd, n_envs, log_cap=8)
    rs = np.random.RandomState(9)
    obs = [(rs.uniform(-5, 5, (n_envs, sd)) + 1.0).astype(np.float32) for _ in range(4)]
    for t in range(3):
        tk.tick(torch.as_tensor(obs[t]).cuda(), None, torch.as_tensor(rs.uniform(-1, 1, n_envs).astype(np.float32)).cuda(),
                torch.as_tensor(np.array([t == 1, False, True, t == 2])).cuda())
    before = tk.state_dict()
    assert before["ep_count"] == 5 and before["count"] == 12
    a.state_moments(tk, merge=True)
    after = tk.state_dict()
    for k in after:
        if k not in ("count", "mean", "m2"):
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    seen = np.concatenate(obs[:3] + [ra[0]])
    _check_moments(after, moments(seen) + (np.abs(seen.astype(np.float64)).mean(axis=0),), "merged into a ticked handle")
    c, m, q = merged((before["count"], before["mean"], before["m2"]), moments(ra[0]))
    np.testing.assert_allclose(after["mean"], m, rtol=0, atol=1e-11 * np.abs(seen).mean())
    tk.tick(torch.as_tensor(obs[3]).cuda())                  # every count copy was set: the next update merges into it
    last = np.concatenate([seen, obs[3]])
    _check_moments(tk.state_dict(), moments(last) + (np.abs(last.astype(np.float64)).mean(axis=0),),
                   "a tick after the merge")


# ---------------------------------------------------------------- 5: normalise
@pytest.mark.parametrize("sd,n", [(1, 63), (3, R + 1), (17, 5000), (64, R), (65, R - 1), (376, 2 * R + 1)])
def test_normalise_against_the_expression(sd, n):
    rows, _ = _ref(sd, n)
    ad = WIDTHS[sd]
    cap = n + 5
    rb = _ring(sd, ad, cap, rows)
    st = rb.state_moments()
    before = rb._records()
    rb.normalize_states(st)
    after = rb._records()
    m = st.state_dict()
    worst = 0.0
    for o in (0, sd + ad):
        want = normalise(before[:n, o:o + sd], m["count"], m["mean"], m["m2"], EPS, CLIP)
        worst = max(worst, _ulps(after[:n, o:o + sd], want))
    print(f"sd {sd} n {n}: largest difference to the expression {worst} ulp")
    assert worst <= 1.0
    assert after[:n, sd:sd + ad].tobytes() == before[:n, sd:sd + ad].tobytes()          # action
    assert after[:n, 2 * sd + ad:].tobytes() == before[:n, 2 * sd + ad:].tobytes()      # reward, not_done, pad
    assert after[n:].tobytes() == before[n:].tobytes()                                  # rows at or past size


def test_normalise_a_particle_ring():
    F, N, D, A = PART
    n = R + 7
    rows = _prows(n)
    rb = _pring(n + 2, rows)
    st = rb.state_moments()
    before = rb._records()
    rb.normalize_states(st)
    after = rb._records()
    m = st.state_dict()
    nd = N * D
    o2 = F + nd + A
    for o in (0, o2):
        want = normalise(before[:n, o:o + F], m["count"], m["mean"], m["m2"], EPS, CLIP)
        assert _ulps(after[:n, o:o + F], want) <= 1.0
    assert after[:, F:o2].tobytes() == before[:, F:o2].tobytes()                        # particles, action
    assert after[:, o2 + F:].tobytes() == before[:, o2 + F:].tobytes()                  # next particles, reward, ...
    assert after[n:].tobytes() == before[n:].tobytes()
    assert (after[:n, :F] != before[:n, :F]).any()


# ---------------------------------------------------------------- 6: cross-path
@pytest.mark.parametrize("kind,masked", [("featured", False), ("featured", True), ("particles", False)])
def test_ring_normalised_rows_equal_tick_normalised_rows(kind, masked):
    import torch
    n = 300
    if kind == "featured":
        sd, ad = 17, 6
        rows, mk = _rows(sd, ad, n, seed=4), (lambda cap: _ring(sd, ad, cap))
        data = _ring(sd, ad, 2000, _rows(sd, ad, 1500, seed=5))
        i_s, i_s2 = 0, 2
    else:
        sd = PART[0]
        rows, mk = _prows(n, seed=4), _pring
        data = _pring(600, _prows(500, seed=5))
        i_s, i_s2 = 0, 3
    st = _stats(sd, mask=_mask(sd) if masked else None)
    data.state_moments(st)
    dev = [torch.as_tensor(x).cuda() for x in rows]
    via_tick, via_ring = mk(n + 3), mk(n + 3)
    o, o2, _ = st.frozen_copy(n).tick(obs=dev[i_s], next_obs=dev[i_s2], update=False)
    ticked = list(dev)
    ticked[i_s], ticked[i_s2] = o, o2
    via_tick.add_batch(*ticked)
    via_ring.add_batch(*dev)
    via_ring.normalize_states(st)
    np.testing.assert_array_equal(via_ring._records(), via_tick._records())
    assert (via_ring._records()[:n, :sd] != rows[i_s]).any()


# ---------------------------------------------------------------- 7: ordering
def test_queued_steps_and_samples_are_ordered_against_the_write():
    """normalize_states with no synchronisation of the caller's around it: the step queued before it trains
    on the raw rows, the sample and the step queued behind it on the normalised ones, on a learner whose
    graph was captured on this ring.  The unsynchronised sequence equals, bit for bit, the same sequence
    with a device synchronisation between every two calls; the step on the normalised rows matches the
    oracle's at the plain step's tolerances."""
    import torch
    from td3_amd.TD3_featured import TD3
    S = featured_setup_dims(17, 6, 1.0, "layer", 64)
    n, B = 500, 64
    rows = tuple(x[:n] for x in gen.fill_featured_buffer(17, 6, 1.0, gen.BUFFER_ROWS, gen.SEED))
    rs = np.random.RandomState(11)
    idx = [rs.randint(0, n, B) for _ in range(3)]
    noise = [rs.standard_normal((B, 6)).astype(np.float32) for _ in range(3)]
    runs = []
    for sync in (False, True):
        pol = TD3(Box((17,)), Box((6,)), max_action=1.0, norm="layer", lr=1e-4, use_graph=True, init="none")
        pol.set_weights(S["actor"], S["critic"])
        rb = _ring(17, 6, n + 12, rows)
        st = rb.state_moments()
        raw = rb._records()
        pol.train_step(rb, B, indices=idx[0], noise=noise[0])         # the graph is captured on this ring
        pol.sync()
        torch.cuda.synchronize()
        pol.train_step(rb, B, indices=idx[1], noise=noise[1])         # queued: raw rows
        if sync:
            pol.sync()
            torch.cuda.synchronize()
        rb.normalize_states(st)
        if sync:
            torch.cuda.synchronize()
        batch, drawn = rb.sample(B, return_indices=True)              # (given indices would be checked on the host)
        if sync:
            torch.cuda.synchronize()
        out = pol.train_step(rb, B, indices=idx[2], noise=noise[2], stats=True)
        pol.sync()
        runs.append(dict(out=out, batch=[t.cpu().numpy() for t in batch], drawn=drawn.cpu().numpy(), raw=raw,
                         rec=rb._records(),
                         params=[v.flat().copy() for v in (pol.actor, pol.critic, pol.actor_target, pol.critic_target)],
                         moments=st.state_dict()))
    free, held = runs
    for k in ("y", "q1", "q2"):
        np.testing.assert_array_equal(free["out"][k], held["out"][k], err_msg=k)
    assert free["out"]["critic_loss"] == held["out"]["critic_loss"]
    for u, v in zip(free["params"], held["params"]):
        np.testing.assert_array_equal(u, v)
    rec = free["rec"]
    for got, cols in zip(free["batch"], (slice(0, 17), slice(17, 23), slice(23, 40), slice(40, 41), slice(41, 42))):
        np.testing.assert_array_equal(got, rec[free["drawn"]][:, cols])    # the sample saw the normalised rows
    np.testing.assert_array_equal(free["drawn"], held["drawn"])
    assert (rec[:n, :17] != free["raw"][:n, :17]).any()
    # the oracle on the same three batches: two raw, one normalised by the expression on the device's moments
    m = free["moments"]
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])

    def gather(records, ix, norm):
        r = records[ix]
        s, s2 = r[:, :17], r[:, 23:40]
        if norm:
            s, s2 = (normalise(x, m["count"], m["mean"], m["m2"], EPS, CLIP) for x in (s, s2))
        return s, r[:, 17:23], s2, r[:, 40:41], r[:, 41:42]
    for t in range(2):
        orc.featured_train_step(L, gather(free["raw"], idx[t], False), noise[t])
    want = orc.featured_train_step(L, gather(free["raw"], idx[2], True), noise[2])
    out = free["out"]
    for k in ("y", "q1", "q2"):
        err = float(np.abs(out[k] - want[k][:, 0]).max() / np.abs(want[k]).max())
        print(f"{k}: {err:.2e} of the largest value (bound 1e-5)")
        assert err <= 1e-5, k
    np.testing.assert_allclose(out["critic_loss"], want["critic_loss"], rtol=1e-5)
    assert out["actor_step"] == ("actor_loss" in want)


# ---------------------------------------------------------------- 8: ring state
def test_ring_state_around_the_write(tmp_path):
    import torch
    sd, ad, n = 17, 6, 300
    rows = _rows(sd, ad, n, seed=6)
    rb = _ring(sd, ad, 400, rows)
    rb.enable_priorities()
    rb.set_priorities(torch.arange(0, n, 3, device="cuda"), torch.linspace(0.5, 4.0, n // 3, device="cuda"))
    before = rb.priorities()
    assert rb.normalized is False
    st = rb.state_moments()
    np.testing.assert_array_equal(rb.priorities(), before)
    rb.normalize_states(st)
    assert rb.normalized is True
    np.testing.assert_array_equal(rb.priorities(), before)
    rec = rb._records()
    folder = str(tmp_path / "ring")
    rb.save(folder)
    back = _ring(sd, ad, 400)
    back.load(folder)
    assert back.normalized is False and (back.size, back.ptr) == (n, n)   # a loaded ring may be normalised (again)
    np.testing.assert_array_equal(back._records(), rec)
    rb.add_batch(*(x[:5] for x in rows))                                  # adds leave the flag
    assert rb.normalized is True
    rb.fill_synthetic(10)
    assert rb.normalized is False
    rb.load(folder)
    assert rb.normalized is False
    # the n-step lane ends: the tick after the write matures nothing from before it
    ns = _ring(sd, ad, 64)
    dev = [torch.as_tensor(x[:8]).cuda() for x in _rows(sd, ad, 8, seed=7)]
    ended = torch.zeros(8, dtype=torch.bool, device="cuda")
    ns.add_batch_nstep(*dev, ended=ended, n=3, gamma=0.9)
    ns.normalize_states(ns.state_moments())
    first = ns._records()[:8].copy()
    ns.add_batch_nstep(*dev, ended=ended, n=3, gamma=0.9)
    np.testing.assert_array_equal(ns._records()[:8], first)
    ns.add_batch_nstep(*dev, ended=ended, n=3, gamma=0.9)                  # the lane is a lane again from there
    assert (ns._records()[8:16, 2 * sd + ad] != ns._records()[16:24, 2 * sd + ad]).any()


# ---------------------------------------------------------------- 9: refusals
def test_refusals_on_real_handles_in_the_headers_order():
    import torch
    from td3_amd._lib import TD3Error
    from td3_amd.TD3_featured import TD3
    sd, ad = 17, 6
    rb = _ring(sd, ad, 64)
    good, wide = _stats(sd), _stats(sd + 1)
    for call in (lambda s: rb.state_moments(s), rb.normalize_states):
        with pytest.raises(TD3Error, match="dims"):                       # before "empty"
            call(wide)
        with pytest.raises(TD3Error, match="empty"):
            call(good)
    assert rb._lib.rb_state_moments(rb.handle, good._h, 2, None) == -1
    assert b"merge must be 0 or 1" in rb._lib.td3_last_error()            # before "dims" and "empty"
    assert rb._lib.rb_state_moments(rb.handle, wide._h, 2, None) == -1
    assert b"merge must be 0 or 1" in rb._lib.td3_last_error()
    rows = _rows(sd, ad, 40, seed=8)
    rb.add_batch(*rows)
    with pytest.raises(TD3Error, match="dims"):
        rb.state_moments(wide)
    if torch.cuda.device_count() >= 2:
        from td3_amd.rollout_stats import RolloutStats
        far = RolloutStats(1, sd, gamma=0.99, device=1)
        with pytest.raises(TD3Error, match="another device"):
            rb.state_moments(far)
        with pytest.raises(TD3Error, match="another device"):
            rb.normalize_states(far)
    rb.state_moments(good)
    rb.normalize_states(good)
    rec = rb._records()
    with pytest.raises(TD3Error, match="already normalised"):
        rb.normalize_states(good)
    with pytest.raises(TD3Error, match="dims"):                           # still before "already normalised"
        rb.normalize_states(wide)
    np.testing.assert_array_equal(rb._records(), rec)                     # a refusal does no GPU work
    rb.state_moments(good)                                                # moments of a normalised ring are allowed
    assert abs(good.state_dict()["mean"]).max() < 1e-5
    rb.add_batch(*rows)                                                   # the handle still adds, samples and trains
    assert rb.size == 64 and rb.sample(16)[0].shape == (16, sd)
    S = featured_setup_dims(sd, ad, 1.0, "layer", 32)
    pol = TD3(Box((sd,)), Box((ad,)), max_action=1.0, norm="layer", init="none")
    pol.set_weights(S["actor"], S["critic"])
    out = pol.train_step(rb, 32, stats=True)
    assert np.isfinite(out["critic_loss"])


# ---------------------------------------------------------------- 10: the workflow
def test_offline_to_online_workflow():
    import torch
    from td3_amd.TD3_featured import TD3
    from td3_amd.loop import DeviceTrainLoop, SyntheticVecEnv
    from td3_amd.my_replay_buffer import MixedReplay
    from td3_amd.rollout_stats import NormalizedVecEnv
    sd, ad, n_env, T, L = 17, 6, 16, 20, 7
    S = featured_setup_dims(sd, ad, 1.0, "layer", 32)

    def policy():
        pol = TD3(Box((sd,)), Box((ad,)), max_action=1.0, norm="layer", seed=3, init="none", bc_alpha=2.5,
                  bc_rows="demo")
        pol.set_weights(S["actor"], S["critic"])
        return pol
    demo = _ring(sd, ad, 2048, _rows(sd, ad, 2000, seed=9))
    stats = demo.state_moments()
    demo.normalize_states(stats)
    assert demo.normalized and stats.state_dict()["count"] == 2000
    demo_rec = demo._records()
    # the raw trajectory: the same environment and the same uniform actions, nothing normalised, no training
    pol = policy()
    raw = _ring(sd, ad, n_env * T)
    torch.manual_seed(77)
    DeviceTrainLoop(SyntheticVecEnv(n_env, sd, ad, max_episode_steps=L, seed=5, device=pol.device), pol, raw,
                    start_policy=10 ** 6, start_training=10 ** 6, batch_size=32, expl_noise=0.1).run(T)
    online = _ring(sd, ad, n_env * T)
    mix = MixedReplay(online, demo, 0.5)
    env = NormalizedVecEnv(SyntheticVecEnv(n_env, sd, ad, max_episode_steps=L, seed=5, device=pol.device),
                           stats.frozen_copy(n_env), norm_reward=False, update=False)
    log = pol.enable_train_log(64)
    torch.manual_seed(77)
    res = DeviceTrainLoop(env, pol, mix, start_policy=10 ** 6, start_training=0, batch_size=32, expl_noise=0.1).run(T)
    assert res["grad_steps"] == T and online.size == n_env * T
    got, want = online._records(), raw._records()
    assert got[:, sd:sd + ad].tobytes() == want[:, sd:sd + ad].tobytes()       # the same actions: the same raw rows
    m = stats.state_dict()
    worst = 0.0
    for o in (0, sd + ad):
        worst = max(worst, _ulps(got[:, o:o + sd], normalise(want[:, o:o + sd], m["count"], m["mean"], m["m2"], EPS, CLIP)))
    print(f"workflow: online rows {worst} ulp from the reference normalisation of the raw rows")
    assert worst <= 1.0
    assert got[:, 2 * sd + ad:].tobytes() == want[:, 2 * sd + ad:].tobytes()   # the reward is not scaled
    np.testing.assert_array_equal(demo._records(), demo_rec)                   # the loop leaves the demonstrations alone
    e = log.entries()
    assert len(e) == T and np.isfinite(e["critic_loss"]).all()
    assert np.isfinite(e["actor_loss"][e["actor_step"] != 0]).all() and (e["actor_step"] != 0).sum() == T // 2
    out = pol.train_step(mix, 32, stats=True)
    assert out["n_demo"] == 16 and np.isfinite(out["critic_loss"])
    f = stats.host_normalizer()                                                # the host loop's form of the same map
    assert _ulps(f(want[:5, :sd]), got[:5, :sd]) <= 1.0
