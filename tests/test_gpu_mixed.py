"""Demonstration replay on the device (include/td3.h "Demonstration replay": td3_train_step_mixed, the
input launch of csrc/mixed.hip; ``MixedReplay``) at the smallest shapes at which that launch can go wrong.

The launch is a copy and the body is the one the injected-index steps run, so every comparison is bit for
bit (``assert_array_equal``) over the four parameter groups, both optimizers' moments and the stats
arrays, after two steps (critic only, then the actor phase).  The two rings always have different seeds
and are filled to ``size < cap``."""
import ctypes as C

import numpy as np
import pytest

from helpers import featured_setup_dims, gen, particle_setup_dims, stage_kernels
from test_gpu_prioritized_step import Box, _copy_state, _views

pytestmark = pytest.mark.gpu

DEMO_SEED, ONLINE_SEED = 11, 23          # the rings' Philox seeds
STATS = ("y", "q1", "q2", "noise")

# (sd, ad, B, norm, demo rows, online rows, n_demo values)
FEATURED = [
    (17, 6, 256, "layer", 40, 90, (0, 1, 127, 128, 255, 256)),       # fused-sample plan dims
    (11, 3, 33, "layer", 40, 90, (0, 5, 33)),                        # ragged batch; 5: the boundary inside a workgroup
    (60, 17, 100, None, 40, 90, (3, 50)),                            # 139-float record, separate-gather plan
    (500, 12, 33, "layer", 20, 40, (17,)),                           # the widest featured learner (input 512): rec = 1016
]
# (F, N, D, A, B, cdq, demo rows, online rows, n_demo values)
PARTICLES = [
    (7, 16, 9, 3, 20, True, 24, 40, (0, 7, 20)),                     # rec = 307, staged
    (3, 65, 16, 2, 33, False, 24, 40, (9,)),                         # rec = 2090, unstaged
    (5, 33, 3, 1, 33, True, 24, 40, (32,)),                          # N D = 99 odd, o_p = 5 unaligned
    (3, 140, 16, 2, 9, False, 24, 40, (4,)),                         # N D = 2240: two trips of the block copy's loop
]


# ---------------------------------------------------------------- setups (weights once per shape)
_SETUPS = {}


def _fsetup(sd, ad, B, norm):
    key = ("f", sd, ad, B, norm)
    if key not in _SETUPS:
        _SETUPS[key] = featured_setup_dims(sd, ad, 1.0, norm, B)
    return _SETUPS[key]


def _psetup(F, N, D, A, B, cdq):
    key = ("p", F, N, D, A, B, cdq)
    if key not in _SETUPS:
        _SETUPS[key] = particle_setup_dims(F, N, D, A, "layer", cdq, B, rows=4)
    return _SETUPS[key]


def _fpol(S, use_graph=True, **kw):
    from td3_amd.TD3_featured import TD3
    pol = TD3(Box((S["sd"],)), Box((S["ad"],)), max_action=S["ma"], norm=S["norm"], lr=1e-4,
              use_graph=use_graph, init="none", **kw)
    pol.set_weights(S["actor"], S["critic"])
    return pol


def _fring(S, rows, seed, cap=None, data_seed=None, **kw):
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=cap or (64 if rows < 64 else 128),
                               seed=seed, **kw)
    if rows:
        rb.add_batch(*gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], rows, gen.SEED + (data_seed or seed)))
    return rb


def _pspaces(S):
    return (Box((S["F"],)), Box((S["N"], S["D"]))), Box((S["A"],))


def _ppol(S, use_graph=True, **kw):
    from td3_amd.TD3_particles import TD3
    obs, act = _pspaces(S)
    pol = TD3(obs, act, norm=S["norm"], CDQ=S["cdq"], use_graph=use_graph, init="none", **kw)
    pol.set_weights(S["actor"], S["critic"])
    return pol


def _pring(S, rows, seed, cap=64, data_seed=None):
    from td3_amd.my_replay_buffer import ReplayBuffer_particles
    obs, act = _pspaces(S)
    rb = ReplayBuffer_particles(obs, act, max_size=cap, seed=seed)
    if rows:
        rb.add_batch(*gen.fill_particle_buffer(S["F"], S["N"], S["D"], S["A"], rows, gen.SEED + (data_seed or seed)))
    return rb


class _Kind:
    """The two learner kinds behind one face: setup, learner, ring."""

    def __init__(self, particles, S):
        self.particles, self.S, self.B = particles, S, S["B"]
        self.A = S["A"] if particles else S["ad"]

    def pol(self, **kw):
        return _ppol(self.S, **kw) if self.particles else _fpol(self.S, **kw)

    def ring(self, rows, seed, **kw):
        return _pring(self.S, rows, seed, **kw) if self.particles else _fring(self.S, rows, seed, **kw)

    def rings(self, nd_rows, no_rows):
        return self.ring(no_rows, ONLINE_SEED), self.ring(nd_rows, DEMO_SEED)

    def noise(self, step):
        return np.random.RandomState(100 + step).standard_normal((self.B, self.A)).astype(np.float32)


def _fkind(sd, ad, B, norm):
    return _Kind(False, _fsetup(sd, ad, B, norm))


def _pkind(F, N, D, A, B, cdq):
    return _Kind(True, _psetup(F, N, D, A, B, cdq))


def _mixed(online, demo, fraction=0.5):
    from td3_amd.my_replay_buffer import MixedReplay
    return MixedReplay(online, demo, fraction)


def _state(pol):
    pol.sync()
    return [v.flat().copy() for v in _views(pol)]    # 4 parameter groups, both optimizers' m and v


def _same_state(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(u, v, err_msg=f"{what}: group {i}")


def _same_stats(oa, ob, what, keys=STATS):
    for k in keys:
        np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"{what}: {k}")
    assert oa["critic_loss"] == ob["critic_loss"] and oa["actor_step"] == ob["actor_step"], what
    if oa["actor_step"]:
        assert oa["actor_loss"] == ob["actor_loss"], what


def _mixed_steps(pol, mix, B, n_demo, idx=None, noise=None, steps=2):
    """``steps`` mixed steps through the C call (n_demo given, not derived from a fraction)."""
    fixed = _fixed(mix, n_demo)
    return [pol.train_step(fixed, B, indices=None if idx is None else idx[t],
                           noise=None if noise is None else noise[t], stats=True) for t in range(steps)]


def _fixed(mix, n_demo):
    """A MixedReplay of the same rings whose n_demo is given outright (the edge counts are not round fractions)."""
    from td3_amd.my_replay_buffer import MixedReplay

    class Fixed(MixedReplay):
        def n_demo(self, batch):
            return n_demo
    return Fixed(mix.online, mix.demo, mix.demo_fraction)


# ---------------------------------------------------------------- the combined references
def _combined_ring(K, online, demo):
    """Check 1's third ring: the demo ring's rows followed by the online ring's (its records, as stored)."""
    nd, no = demo.size, online.size
    rec = np.ascontiguousarray(np.concatenate([demo._records()[:nd], online._records()[:no]]))
    comb = K.ring(0, seed=5, cap=nd + no + 7)
    from td3_amd import _lib
    _lib.check(comb._lib.rb_write_records(comb.handle, 0, nd + no, _lib.fptr(rec), nd + no, nd + no), "rb_write_records")
    return comb


class _Foreign:
    """Check 2's batch: the concatenation of the two rings' stand-alone samples of the injected rows."""

    def __init__(self, online, demo, idx_d, idx_o):
        import torch
        parts = [r.sample(len(i), indices=i) for r, i in ((demo, idx_d), (online, idx_o)) if len(i)]
        self.batch = tuple(torch.cat(f, dim=0) for f in zip(*parts))

    def sample(self, batch_size):
        assert self.batch[0].shape[0] == batch_size
        return self.batch


def _reference_steps(K, online, demo, n_demo, idx, noise, **pol_kw):
    """The same rows through the path that predates the feature: the combined-ring injected step
    (featured) / td3_train_step_batch_particles on the concatenated samples (particles)."""
    pol = K.pol(**pol_kw)
    outs = []
    comb = None if K.particles else _combined_ring(K, online, demo)
    for t in range(len(idx)):
        idx_d, idx_o = idx[t][:n_demo], idx[t][n_demo:]
        if K.particles:
            outs.append(pol.train_step(_Foreign(online, demo, idx_d, idx_o), K.B, noise=noise[t], stats=True))
        else:
            outs.append(pol.train_step(comb, K.B, indices=np.concatenate([idx_d, demo.size + idx_o]),
                                       noise=noise[t], stats=True))
    return pol, outs


def _twin_draws(K, ring, steps=2):
    """The plain step's draws on `ring` at total_it = 0, 1, ..: what each side of the mixed draw must match."""
    pol = K.pol()
    outs = [pol.train_step(ring, K.B, stats=True) for _ in range(steps)]
    return pol, outs


def _check_shape(K, nd_rows, no_rows, n_demo):
    """Checks 1 / 2 (injected equals the older path), 3 (the draw), 4 (Philox equals injected) and 5
    (n_demo = 0 and B are the plain step) at one shape and one n_demo."""
    B = K.B
    online, demo = K.rings(nd_rows, no_rows)
    mix = _mixed(online, demo)
    # Philox draw, the learner's own noise
    pm = K.pol()
    om = _mixed_steps(pm, mix, B, n_demo)
    td, od = _twin_draws(K, demo)
    to, oo = _twin_draws(K, online)
    for t in range(2):
        idx = om[t]["idx"]
        np.testing.assert_array_equal(idx[:n_demo], od[t]["idx"][:n_demo], err_msg=f"step {t}: demo side of the draw")
        np.testing.assert_array_equal(idx[n_demo:], oo[t]["idx"][n_demo:], err_msg=f"step {t}: online side of the draw")
        assert (idx[:n_demo] >= 0).all() and (idx[:n_demo] < nd_rows).all()
        assert (idx[n_demo:] >= 0).all() and (idx[n_demo:] < no_rows).all()
        assert om[t]["n_demo"] == n_demo and om[t]["actor_step"] == (t == 1)
    if n_demo == 0 or n_demo == B:
        twin, ot = (to, oo) if n_demo == 0 else (td, od)
        for t in range(2):
            _same_stats(om[t], ot[t], f"n_demo = {n_demo} vs the plain step, step {t}", STATS + ("idx",))
        _same_state(_state(pm), _state(twin), f"n_demo = {n_demo} vs the plain step")
    # the same rows and noise injected: bit for bit the Philox step ...
    idx = [o["idx"] for o in om]
    noise = [o["noise"] for o in om]
    pi = K.pol()
    oi = _mixed_steps(pi, mix, B, n_demo, idx=idx, noise=noise)
    for t in range(2):
        _same_stats(om[t], oi[t], f"Philox vs injected, step {t}", STATS + ("idx",))
    _same_state(_state(pm), _state(pi), "Philox vs injected")
    # ... and the path that predates the feature
    pr, orf = _reference_steps(K, online, demo, n_demo, idx, noise)
    for t in range(2):
        _same_stats(oi[t], orf[t], f"mixed vs the combined reference, step {t}")
    _same_state(_state(pi), _state(pr), "mixed vs the combined reference")
    assert pm._counters() == pr._counters() == (2, 2, 1)


@pytest.mark.parametrize("case", [(c[:4], c[4], c[5], n) for c in FEATURED for n in c[6]],
                         ids=lambda c: "sd%d_ad%d_B%d_n%d" % (c[0][0], c[0][1], c[0][2], c[3]))
def test_featured_edge_shapes(case):
    (sd, ad, B, norm), nd_rows, no_rows, n_demo = case
    _check_shape(_fkind(sd, ad, B, norm), nd_rows, no_rows, n_demo)


@pytest.mark.parametrize("case", [(c[:6], c[6], c[7], n) for c in PARTICLES for n in c[8]],
                         ids=lambda c: "F%d_N%d_D%d_B%d_n%d" % (c[0][0], c[0][1], c[0][2], c[0][4], c[3]))
def test_particle_edge_shapes(case):
    dims, nd_rows, no_rows, n_demo = case
    _check_shape(_pkind(*dims), nd_rows, no_rows, n_demo)


def test_a_featured_record_wider_than_the_lds_slot_cannot_exist():
    """(1030, 2): rec = 2064 > kMaxRecord.  rb_create refuses such a featured ring and td3_create such a
    learner (network input <= 512), so a featured mixed step never takes the unstaged path; the particle
    cases above (rec = 2090) are the ones that run it, small fields included, and (500, 12) is the widest
    featured record a learner can train on."""
    from td3_amd._lib import TD3Error
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    with pytest.raises(TD3Error, match="record too wide"):
        ReplayBuffer_featured(Box((1030,)), Box((2,)), max_size=64, seed=DEMO_SEED)
    with pytest.raises(TD3Error, match="input width"):
        TD3(Box((1030,)), Box((2,)), init="none")


KINDS = {"featured": lambda: _fkind(11, 3, 33, "layer"), "particles": lambda: _pkind(7, 16, 9, 3, 20, True)}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("demo_rows,n_demo", [(1, 7), (3, 7)])
def test_ring_fill_cases(kind, demo_rows, n_demo):
    """A demo ring of one row, and of 3 rows with n_demo = 7: rows repeat inside the batch."""
    _check_shape(KINDS[kind](), demo_rows, 40, n_demo)


def test_fused_sample_plan_is_the_one_under_test():
    """(17, 6, 256) is a plan whose plain step samples inside F_fwd0; (60, 17, 100) gathers separately."""
    for (sd, ad, B, norm), fused in (((17, 6, 256, "layer"), True), ((60, 17, 100, None), False)):
        K = _fkind(sd, ad, B, norm)
        st = stage_kernels(K.pol(), K.ring(40, 3), B, 0)
        assert (st[0][1] != "td3::gather_kernel") == fused, st[0]


# ---------------------------------------------------------------- 4: path equivalences
def _plan_flags(pol):
    f = C.c_int()
    assert pol._lib.td3_debug_plan_flags(pol._h, C.byref(f)) == 0
    return f.value


@pytest.mark.parametrize("kind", list(KINDS))
def test_graph_eager_repeat_and_changing_n_demo(kind):
    K = KINDS[kind]()
    B = K.B
    online, demo = K.rings(24, 40)
    mix = _mixed(online, demo)

    def run(use_graph):
        pol = K.pol(use_graph=use_graph)
        outs = _mixed_steps(pol, mix, B, B // 2, steps=4)
        return pol, outs, _state(pol)
    g, og, sg = run(True)
    e, oe, se = run(False)
    g2, og2, sg2 = run(True)
    for t in range(4):
        _same_stats(og[t], oe[t], f"graph vs eager, step {t}", STATS + ("idx",))
        _same_stats(og[t], og2[t], f"two runs, step {t}", STATS + ("idx",))
    _same_state(sg, se, "graph vs eager")
    _same_state(sg, sg2, "two runs")
    # n_demo changes between steps: the same plan, no rebuild (its flags and stage lists stay), and each
    # step equals a fresh learner's given that value
    pol = K.pol()
    flags = None
    for n_demo in (B // 2, B // 4, B):
        before = _state(pol)
        fresh = K.pol()
        _copy_state(pol, pol)
        _copy_state(pol, fresh)
        oa = _mixed_steps(pol, mix, B, n_demo, steps=1)[0]
        ob = _mixed_steps(fresh, mix, B, n_demo, steps=1)[0]
        _same_stats(oa, ob, f"n_demo -> {n_demo}", STATS + ("idx",))
        _same_state(_state(pol), _state(fresh), f"n_demo -> {n_demo}")
        assert oa["n_demo"] == n_demo and any((x != y).any() for x, y in zip(before, _state(pol)))
        if flags is None:
            flags = _plan_flags(pol)
        assert _plan_flags(pol) == flags


# ---------------------------------------------------------------- 6: mixed leaves plain alone
@pytest.mark.parametrize("kind", list(KINDS) + ["featured_fused"])
def test_plain_steps_after_mixed_are_bit_exact(kind):
    K = _fkind(17, 6, 256, "layer") if kind == "featured_fused" else KINDS[kind]()
    B = K.B
    online, demo = K.rings(24, 40)
    a, b = K.pol(), K.pol()
    ref_kernels = [stage_kernels(K.pol(), online, B, ph) for ph in (0, 1)]
    _mixed_steps(a, _mixed(online, demo), B, B // 2)
    _copy_state(a, a)
    _copy_state(a, b)
    for t in range(4):
        oa = a.train_step(online, B, stats=True)
        ob = b.train_step(online, B, stats=True)
        _same_stats(oa, ob, f"plain step {t} after mixed", STATS + ("idx",))
    _same_state(_state(a), _state(b), "plain steps after mixed")
    for ph in (0, 1):                       # the plain plan's kernels are the ones of a learner that never mixed
        assert stage_kernels(a, online, B, ph) == ref_kernels[ph]


@pytest.mark.parametrize("kind", list(KINDS))
def test_prioritized_and_mixed_steps_keep_their_contracts(kind):
    K = KINDS[kind]()
    B = K.B
    kw = dict(per_beta=1.0) if K.particles else {}
    online, demo = K.rings(24, 40)
    pri = K.ring(40, 31)
    pri.enable_priorities(alpha=0.6, eps=1e-6)
    import torch
    p = np.linspace(0.05, 3.0, 40).astype(np.float32)
    pri.set_priorities(torch.arange(40, device="cuda"), torch.as_tensor(p, device="cuda"))
    u = (np.arange(B, dtype=np.float32) + 0.5) / B
    mix = _mixed(online, demo)
    a, b = K.pol(**kw), K.pol(**kw)
    if not K.particles:
        a.per_beta = b.per_beta = 1.0
    out = a.train_step(pri, B, stats=True, u=u)                    # non-unit weights are now in the plan
    assert out["weight"].min() < 0.9
    _copy_state(a, a)
    _copy_state(a, b)
    oa = _mixed_steps(a, mix, B, B // 2, steps=1)[0]               # mixed after prioritized: unit weights again
    ob = _mixed_steps(b, mix, B, B // 2, steps=1)[0]
    _same_stats(oa, ob, "mixed after prioritized", STATS + ("idx",))
    _same_state(_state(a), _state(b), "mixed after prioritized")
    # prioritized after mixed: against a twin that takes the same prioritized step without the mixed one before
    pri_b = K.ring(40, 31)
    pri_b.enable_priorities(alpha=0.6, eps=1e-6)
    pri_b.set_priorities(torch.arange(40, device="cuda"), torch.as_tensor(p, device="cuda"))
    pri.set_priorities(torch.arange(40, device="cuda"), torch.as_tensor(p, device="cuda"))
    _copy_state(a, a)
    _copy_state(a, b)
    oa = a.train_step(pri, B, stats=True, u=u)
    ob = b.train_step(pri_b, B, stats=True, u=u)
    _same_stats(oa, ob, "prioritized after mixed", STATS + ("idx", "weight", "td_abs"))
    _same_state(_state(a), _state(b), "prioritized after mixed")
    np.testing.assert_array_equal(pri.priorities(), pri_b.priorities())


# ---------------------------------------------------------------- 7: ordering
@pytest.mark.parametrize("kind", list(KINDS))
def test_stream_ordering_with_adds(kind):
    import torch
    K = KINDS[kind]()
    B, S = K.B, K.S
    if K.particles:
        fresh = gen.fill_particle_buffer(S["F"], S["N"], S["D"], S["A"], 16, gen.SEED + 77)
    else:
        fresh = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], 16, gen.SEED + 77)

    def dev(rows):
        return [torch.as_tensor(np.asarray(x)[rows], dtype=torch.float32, device="cuda") for x in fresh]
    idx_d = (24 + np.arange(B // 2) % 8).astype(np.int64)           # the rows the adds below write
    idx_o = (40 + np.arange(B - B // 2) % 8).astype(np.int64)
    noise = K.noise(0)
    res = []
    for sync_first in (True, False):
        online, demo = K.rings(24, 40)
        mix = _mixed(online, demo)
        pol = K.pol()
        _mixed_steps(pol, mix, B, B // 2, steps=1)                   # the plan exists: nothing synchronises below
        t_d, t_o = dev(slice(0, 8)), dev(slice(8, 16))
        torch.cuda.synchronize()
        demo.add_batch(*t_d)                                         # on torch's stream, right before the step
        online.add_batch(*t_o)
        if sync_first:
            torch.cuda.synchronize()
        out = pol.train_step(mix, B, indices=(idx_d, idx_o), noise=noise, stats=True)
        res.append((out, _state(pol)))
    _same_stats(res[0][0], res[1][0], "adds queued right before the step")
    _same_state(res[0][1], res[1][1], "adds queued right before the step")
    # rows the step sampled, overwritten by adds queued right behind it
    res = []
    for overwrite in (False, True):
        online = K.ring(40, ONLINE_SEED, cap=44)                     # the next 8 rows wrap onto rows 0..3
        demo = K.ring(24, DEMO_SEED, cap=28)
        mix = _mixed(online, demo)
        pol = K.pol()
        _mixed_steps(pol, mix, B, B // 2, steps=1)
        t_d, t_o = dev(slice(0, 8)), dev(slice(8, 16))
        torch.cuda.synchronize()
        pol.train_step(mix, B, indices=((np.arange(B // 2) % 4), (np.arange(B - B // 2) % 4)), noise=noise)
        if overwrite:
            demo.add_batch(*t_d)
            online.add_batch(*t_o)
        res.append(_state(pol))
    _same_state(res[0], res[1], "sampled rows overwritten right after the step")


# ---------------------------------------------------------------- 8: with the other features
def test_bc_on_a_mixed_step():
    K = _fkind(11, 3, 33, "layer")
    B, n_demo = K.B, 5
    online, demo = K.rings(24, 40)
    rs = np.random.RandomState(3)
    idx = [np.concatenate([rs.randint(0, 24, n_demo), rs.randint(0, 40, B - n_demo)]) for _ in range(2)]
    noise = [K.noise(t) for t in range(2)]
    a, b = K.pol(bc_alpha=2.5), K.pol(bc_alpha=2.5)
    oa = _mixed_steps(a, _mixed(online, demo), B, n_demo, idx=idx, noise=noise)
    comb = _combined_ring(K, online, demo)
    for t in range(2):
        ob = b.train_step(comb, B, indices=np.concatenate([idx[t][:n_demo], 24 + idx[t][n_demo:]]), noise=noise[t],
                          stats=True)
        _same_stats(oa[t], ob, f"BC step {t}")
    assert oa[1]["bc_loss"] == ob["bc_loss"] > 0 and oa[1]["bc_lambda"] == ob["bc_lambda"]
    assert a.bc_info() == b.bc_info() and a.bc_info()["step"] == 2
    _same_state(_state(a), _state(b), "BC on a mixed step")


@pytest.mark.parametrize("kind", list(KINDS))
def test_clipping_on_a_mixed_step(kind):
    K = KINDS[kind]()
    B, n_demo = K.B, 7
    online, demo = K.rings(24, 40)
    rs = np.random.RandomState(4)
    idx = [np.concatenate([rs.randint(0, 24, n_demo), rs.randint(0, 40, B - n_demo)]) for _ in range(2)]
    noise = [K.noise(t) for t in range(2)]
    a = K.pol(max_grad_norm=1.0)
    oa = _mixed_steps(a, _mixed(online, demo), B, n_demo, idx=idx, noise=noise)
    assert a.clip_info()["critic"]["step"] == 2
    b, ob = _reference_steps(K, online, demo, n_demo, idx, noise, max_grad_norm=1.0)
    for t in range(2):
        _same_stats(oa[t], ob[t], f"clipped step {t}")
        assert oa[t]["critic_grad_norm"] == ob[t]["critic_grad_norm"] > 0
    assert a.clip_info() == b.clip_info()
    _same_state(_state(a), _state(b), "clipping on a mixed step")


def test_train_log_entry_of_a_mixed_step():
    K = _fkind(11, 3, 33, "layer")
    online, demo = K.rings(24, 40)
    pol = K.pol()
    log = pol.enable_train_log(capacity=16)
    outs = _mixed_steps(pol, _mixed(online, demo), K.B, 5)
    e = log.entries()
    assert len(e) == 2 and list(e["step"]) == [1, 2]
    assert (e["prioritized"] == 0).all() and (e["batch"] == K.B).all() and list(e["actor_step"]) == [0, 1]
    np.testing.assert_allclose(e["critic_loss"], [o["critic_loss"] for o in outs], rtol=1e-5)


# ---------------------------------------------------------------- 9: refusals on real handles
def test_refusals_in_the_headers_order():
    from td3_amd._lib import TD3Error
    from td3_amd.data_parallel import local_group
    K, KP = KINDS["featured"](), KINDS["particles"]()
    B = K.B
    online, demo = K.rings(24, 40)
    pol = K.pol()
    lib = pol._lib

    def step(h, rb, dm, n_demo=5, idx=None, batch=B):
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        from td3_amd import _lib
        rc = lib.td3_train_step_mixed(h, rb.handle, dm.handle, batch, n_demo, None,
                                      _lib.i64ptr(ix) if ix is not None else None, None, None)
        return rc, lib.td3_last_error()

    def refused(rc_err, word):
        rc, err = rc_err
        assert rc == -1 and word in err, (rc, err, word)
        assert pol._counters() == (0, 0, 0)

    refused(step(pol._h, online, online), b"same ring")
    narrow = _fring(_fsetup(17, 6, 256, "layer"), 8, 3)
    pring = KP.ring(8, 3)
    refused(step(pol._h, pring, demo), b"kind")
    refused(step(pol._h, online, pring), b"kind")
    refused(step(pol._h, narrow, demo), b"dims")
    refused(step(pol._h, online, narrow), b"dims")
    import torch
    if torch.cuda.device_count() > 1:
        other = _fring(K.S, 8, 3, device=1)
        refused(step(pol._h, other, demo), b"another device")
        refused(step(pol._h, online, other), b"another device")
    pri = K.ring(8, 3)
    pri.enable_priorities()
    refused(step(pol._h, pri, demo), b"priorities")
    refused(step(pol._h, online, pri), b"priorities")
    refused(step(pol._h, pri, narrow), b"dims")                  # the ring checks come before the priority check
    empty = K.ring(0, 3)
    refused(step(pol._h, empty, demo), b"empty")
    refused(step(pol._h, online, empty), b"empty")
    refused(step(pol._h, empty, demo, n_demo=0), b"empty")
    idx = np.zeros(B, np.int64)
    for pos, ring_cap in ((0, demo.max_size), (4, demo.max_size), (5, online.max_size), (B - 1, online.max_size)):
        bad = idx.copy()
        bad[pos] = ring_cap
        refused(step(pol._h, online, demo, idx=bad), b"out of range")
        bad[pos] = -1
        refused(step(pol._h, online, demo, idx=bad), b"out of range")
    assert lib.td3_debug_mixed_input(pol._h, online.handle, demo.handle, None) == -1     # no mixed step yet
    # a ring that contributes no row may be empty; and the handle still steps
    assert step(pol._h, online, empty, n_demo=0)[0] == 0
    assert step(pol._h, empty, demo, n_demo=B)[0] == 0
    assert step(pol._h, online, demo)[0] == 0
    pol.sync()
    assert pol._counters() == (3, 3, 1)
    assert lib.td3_debug_mixed_input(pol._h, online.handle, demo.handle, None) == 0, lib.td3_last_error()
    assert lib.td3_debug_mixed_input(pol._h, demo.handle, online.handle, None) == -1     # not that step's rings
    assert lib.td3_debug_mixed_input(pol._h, online.handle, empty.handle, None) == -1
    pol.train(online, B)
    assert lib.td3_debug_mixed_input(pol._h, online.handle, demo.handle, None) == -1     # the last step was plain
    pol.sync()
    with pytest.raises(TD3Error, match="same ring"):
        _step_same(pol, online, B)
    pols = [K.pol() for _ in range(2)]
    local_group(pols)
    rc, err = step(pols[0]._h, online, demo)
    assert rc == -1 and b"data-parallel" in err
    assert pols[0]._counters() == (0, 0, 0)
    pri2 = K.ring(8, 3)
    pri2.enable_priorities()
    rc, err = step(pols[0]._h, pri2, demo)                       # priorities are checked before the group
    assert rc == -1 and b"priorities" in err


def _step_same(pol, ring, B):
    """train_step on a MixedReplay made (past its constructor's check) of one ring twice: the C call refuses."""
    from td3_amd.my_replay_buffer import MixedReplay
    m = MixedReplay.__new__(MixedReplay)
    m.online = m.demo = ring
    m.demo_fraction, m.device = 0.5, ring.device
    pol.train_step(m, B)


# ---------------------------------------------------------------- 10: Python
def test_mixed_replay_surface():
    from td3_amd.my_replay_buffer import MixedReplay
    K, KP = KINDS["featured"](), KINDS["particles"]()
    online, demo = K.rings(24, 40)
    with pytest.raises(ValueError, match="kind"):
        MixedReplay(online, KP.ring(8, 3))
    with pytest.raises(ValueError, match="dims"):
        MixedReplay(online, _fring(_fsetup(17, 6, 256, "layer"), 8, 3))
    with pytest.raises(ValueError, match="dims"):
        MixedReplay(KP.ring(8, 3), _pring(_psetup(5, 33, 3, 1, 33, True), 8, 3))
    with pytest.raises(ValueError, match="two rings"):
        MixedReplay(online, online)
    with pytest.raises(ValueError):
        MixedReplay(online, object())
    pri = K.ring(8, 3)
    pri.enable_priorities()
    for pair in ((online, pri), (pri, demo)):
        with pytest.raises(ValueError, match="prioritized"):
            MixedReplay(*pair)
    mix = MixedReplay(online, demo, 1.0 / 3.0)
    assert mix.prioritized is False and mix.size == 40 and mix.ptr == 40 and mix.n_demo(33) == 11
    batch = mix.sample(33)
    S = K.S
    assert len(batch) == 5 and [t.shape[0] for t in batch] == [33] * 5
    assert tuple(batch[0].shape) == (33, S["sd"]) and tuple(batch[1].shape) == (33, S["ad"])
    drec, orec = demo._records()[:24], online._records()[:40]
    s = batch[0].cpu().numpy()
    sd = S["sd"]

    def rows_of(x, rec):
        return [(rec[:, :sd] == r).all(axis=1).any() for r in x]
    assert all(rows_of(s[:11], drec)) and all(rows_of(s[11:], orec))       # demo rows first, then online rows
    assert not any(rows_of(s[:11], orec))
    pb = _mixed(KP.ring(40, ONLINE_SEED), KP.ring(24, DEMO_SEED)).sample(20)
    P = KP.S
    assert len(pb) == 7 and tuple(pb[1].shape) == (20, P["N"], P["D"]) and tuple(pb[0].shape) == (20, P["F"])
    pol = K.pol()
    for f, want in ((0.5, 17), (0.25, 8), (1.0, 33), (0.0, 0)):
        mix.demo_fraction = f
        out = pol.train_step(mix, 33, stats=True)
        assert out["n_demo"] == want
        assert (out["idx"][:want] < 24).all() and (out["idx"] < 40).all()
    with pytest.raises(ValueError, match="prioritized"):
        pol.train_step(mix, 33, u=np.full(33, 0.5, np.float32))
    out = pol.train_step(mix, 33, indices=(np.arange(4), np.arange(29)), stats=True)
    assert out["n_demo"] == 4
    np.testing.assert_array_equal(out["idx"], np.concatenate([np.arange(4), np.arange(29)]))
    with pytest.raises(ValueError, match="batch"):
        pol.train_step(mix, 33, indices=(np.arange(4), np.arange(4)))


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_train_loop_on_a_mixed_replay(kind):
    """Fine-tuning from tick 0 on loaded demonstrations: the online ring starts empty."""
    from td3_amd.loop import DeviceTrainLoop, SyntheticParticleVecEnv, SyntheticVecEnv
    K = KINDS[kind]()
    S = K.S
    pol = K.pol()
    demo = K.ring(64, DEMO_SEED, cap=128)
    online = K.ring(0, ONLINE_SEED, cap=512)
    mix = _mixed(online, demo, 0.5)
    assert mix.n_demo(16) == 16                                    # all-demo while nothing was collected
    if K.particles:
        env = SyntheticParticleVecEnv(8, S["F"], S["N"], S["D"], S["A"], max_episode_steps=25, device=pol.device)
    else:
        env = SyntheticVecEnv(8, 11, 3, max_episode_steps=25, device=pol.device)
    loop = DeviceTrainLoop(env, pol, mix, start_policy=5, start_training=0, batch_size=16, expl_noise=0.1)
    res = loop.run(40)
    assert online.size == 320 and demo.size == 64 and mix.size == 320
    assert res["env_steps"] == 320 and res["grad_steps"] == pol.total_it and pol.total_it >= 39
    assert pol._counters() == (pol.total_it, pol.total_it, pol.total_it // 2)
    assert mix.n_demo(16) == 8
    for view in (pol.actor, pol.critic, pol.actor_target, pol.critic_target):
        assert np.isfinite(view.flat()).all()
