"""The product's data-parallel path with more than one replica, on one MI355X.

RCCL cannot put two ranks on one GPU, so n replicas of one process form a
``td3_comm_init_local`` group: the same data-parallel stage lists as ``td3_comm_init`` (grad-only
dW, all-reduce, flat Adam with grad scale 1/n, Polyak), with the all-reduce a fixed-order device sum
over the replicas' gradient arenas.  Replica k samples its own ring at rows
``idx[k*B/n:(k+1)*B/n]`` of a golden batch (TD3_featured.py:148-164; noise likewise).

Checks, per step (teacher-forced from the oracle's state):
* the replicas end bit-identical (actor, critic, targets, Adam moments);
* the all-reduced gradient (the G arena: sum over replicas; / n = mean of the shard gradients)
  equals the oracle's gradient of the ONE global-batch loss (SURVEY §8e equivalence: the losses
  are batch means) at the SURVEY §8c gradient tolerance;
* the post-Adam parameters equal the oracle's global-batch step within 2*lr everywhere and within
  1e-6 + 1e-5|x| on >= 99 % of the elements.  (The single-device tests hold 99.9 %: here the
  gradient is a different fp32 summation -- two shard sums added -- and Adam's m / sqrt(v) turns
  the rounding of near-zero gradients into up to lr-sized moves of a few more elements.)  Against
  the oracle restated in the data-parallel form itself (``oracle_dp_step``: the same shard sums in
  replica order) the HalfCheetah critics hold the single-device 99.9 % contract (the actor's
  gradient runs through the critic the step has just updated, see ``_check_grads``);
  ``tests/test_dp_oracle.py`` (CPU) shows that the oracle's own DP form and its global-batch step
  differ by the same kind of rounding.
"""
import numpy as np
import pytest

import copy

from helpers import gen, orc, load_golden, featured_setup, oracle_dp_actor_phase, oracle_dp_step, particle_setup
from test_gpu_parity import _make, _load_oracle_state, _params_close, _rel_to_max

pytestmark = pytest.mark.gpu


def _replicas(S, n, maker):
    from td3_amd.data_parallel import local_group
    pols, rbs = [], []
    for _ in range(n):
        p, rb = maker(S)
        pols.append(p)
        rbs.append(rb)
    local_group(pols)
    return pols, rbs


def _all_views(pol):
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    return [pol.actor.flat(), pol.critic.flat(), pol.actor_target.flat(), pol.critic_target.flat(),
            _ParamView(pol, _lib.TD3_ACTOR_ADAM_M, 0).flat(), _ParamView(pol, _lib.TD3_CRITIC_ADAM_V, 1).flat()]


def _check_grads(pol, n, rec, what, actor_ref=None):
    """All-reduced gradients / n vs the oracle, per tensor relative to its largest element (as
    tests/test_oracle_golden.py).  The critic gradient comes from exactly the oracle's state: SURVEY
    §8c's gradient tolerance (2e-4 of the tensor's scale) against the global-batch gradient.  The
    actor gradient is taken through the critic AFTER this step's update; ``actor_ref`` is the
    oracle's data-parallel actor gradient teacher-forced from the GPU's post-step critic
    (helpers.oracle_dp_actor_phase), held to 1e-4 of scale (the particle test, without it, keeps
    the global-batch oracle at 1e-2: a moved critic weight can flip a ReLU of Q1 on a row).
    Weight-normalised Linears keep dL/dW in the arena (wn_kernel forms dg / dv in registers): their
    biases are compared."""
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    groups = [("critic", _lib.TD3_CRITIC_GRAD, 1, rec["critic_grads"], 2e-4)]
    if actor_ref is not None:
        groups.append(("actor", _lib.TD3_ACTOR_GRAD, 0, actor_ref, 1e-4))
    elif "actor_grads" in rec:
        groups.append(("actor", _lib.TD3_ACTOR_GRAD, 0, rec["actor_grads"], 1e-2))
    for name, which, g, ref, tol in groups:
        got = _ParamView(pol, which, g).numpy_dict()
        for k, v in ref.items():
            if k.endswith(("weight_g", "weight_v")):
                continue
            assert _rel_to_max(got[k] / n, v) <= tol, (what, name, k, _rel_to_max(got[k] / n, v))


def _check_actor_phase(pols, n, L0, s, rec, Ldp, what, dp_frac=0.999):
    """The actor phase of a policy step, teacher-forced: the oracle's data-parallel actor phase run
    from the GPU's own post-step critic (gradient at 1e-4 of scale, actor and actor_target at the
    single-device 99.9 % contract), and the actor / actor_target also against the oracle's free
    data-parallel step ``Ldp`` at ``dp_frac`` (99.9 %; C5 99.8 %: there Ldp's actor gradient runs
    through Ldp's own post-step critic, which differs from the GPU's at the post-Adam contract, and
    at B = 8192 that moved 216 of 200,000 layer-1 weights past the tight bound -- 99.892 % measured,
    every element within 2*lr -- while the teacher-forced phase holds 99.9 %).  The oracle's actor backward runs on each
    replica's own relu' masks (as tests/test_gpu_gradients.py), which differ from the oracle's only
    where a pre-activation is within fp32 rounding of zero (checked there)."""
    if "actor_loss" not in rec:
        return
    from test_gpu_gradients import _gpu_masks
    pol = pols[0]
    b = s.shape[0] // n
    masks = [{k: v for k, v in _gpu_masks(p, b, True).items() if k in ("actor", "aq")} for p in pols]
    Lt, red = oracle_dp_actor_phase(L0, s, n, pol.critic.numpy_dict(), masks=masks)
    norm_wn = any(k.endswith("weight_v") for k in red)
    _check_grads(pol, n, {"critic_grads": {}}, what, actor_ref=red)
    if not norm_wn:
        for grp in ("actor", "actor_target"):
            _params_close(getattr(pol, grp).numpy_dict(), getattr(Lt, grp), L0.lr, (what, "teacher-forced", grp))
    for grp in ("actor", "actor_target"):
        _params_close(getattr(pol, grp).numpy_dict(), getattr(Ldp, grp), L0.lr, (what, "dp-oracle", grp),
                      frac=dp_frac)


def _check_replicas_equal(pols):
    ref = _all_views(pols[0])
    for p in pols[1:]:
        for a, b in zip(ref, _all_views(p)):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name,n,shard", [("hc_layer", 2, "1"), ("hc_layer", 4, "1"), ("hc_layer", 8, "1"),
                                          ("hc_layer", 2, "0"), ("hc_none", 2, "1"), ("hc_wn", 2, "1")])
def test_local_replicas_equal_global_batch_step(name, n, shard, monkeypatch):
    """shard "1": the sharded optimizer step -- replica k sums slice k, runs Adam on it and hands the
    parameters to the others (the seam's all-gather); "0" (the default): all-reduce + replicated
    Adam.  Adam moments are compared after the seam consolidates the owners' slices."""
    from td3_amd.data_parallel import train_local
    monkeypatch.setenv("TD3_DP_SHARD", shard)
    G = load_golden("featured", name)
    S = featured_setup(name)
    pols, rbs = _replicas(S, n, _make)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    B = S["B"]
    b = B // n
    for step in range(1, S["steps"] + 1):
        p = f"step{step}"
        idx, noise = G[f"{p}/idx"], G[f"{p}/noise"]
        for pol in pols:
            _load_oracle_state(pol, L)
        L0 = copy.deepcopy(L)
        Ldp = oracle_dp_step(L, S["buf"].gather(idx), noise, n)
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        outs = train_local(pols, rbs, b, indices=idx.reshape(n, b), noise=noise.reshape(n, b, -1), stats=True)
        y = np.concatenate([o["y"][:, 0] for o in outs])
        q1 = np.concatenate([o["q1"][:, 0] for o in outs])
        assert _rel_to_max(y, rec["y"][:, 0]) <= 1e-5, (p, "y")
        assert _rel_to_max(q1, rec["q1"][:, 0]) <= 1e-5, (p, "q1")
        # each replica's loss is its shard's; their mean is the global batch-mean loss
        np.testing.assert_allclose(np.mean([o["critic_loss"] for o in outs]), rec["critic_loss"], rtol=1e-5)
        assert all(o["actor_step"] == ("actor_loss" in rec) for o in outs)
        if "actor_loss" in rec:
            np.testing.assert_allclose(np.mean([o["actor_loss"] for o in outs]), rec["actor_loss"],
                                       rtol=1e-5, atol=1e-7)
        _check_replicas_equal(pols)
        pol = pols[0]
        _check_grads(pol, n, {"critic_grads": rec["critic_grads"]}, p)
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (p, "critic"), frac=0.99)
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, L.lr, (p, "critic_target"), frac=0.99)
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (p, "actor"), frac=0.99)
        _params_close(pol.actor_target.numpy_dict(), L.actor_target, L.lr, (p, "actor_target"), frac=0.99)
        # the same step restated by the oracle in the product's data-parallel form: the critic holds
        # the single-device 99.9 % contract against it; the actor phase is checked teacher-forced
        # from the GPU's post-step critic and against the DP-form oracle at the same contract
        for grp, ref in (("critic", Ldp.critic), ("critic_target", Ldp.critic_target)):
            _params_close(getattr(pol, grp).numpy_dict(), ref, L.lr, (p, "dp-oracle", grp))
        _check_actor_phase(pols, n, L0, S["buf"].gather(idx)[0], rec, Ldp, p)
        assert all(q._counters() == (L.total_it, L.critic_step, L.actor_step) for q in pols)


@pytest.mark.parametrize("buckets,shard", [("0", "1"), ("0", "0"), ("1", "1")])
def test_c5_eight_replicas_global_batch_8192(buckets, shard, monkeypatch):
    """BASELINE config 5 (Humanoid-v4, 8 x MI355X, 1024 rows per GPU = global batch 8192) through
    the product's data-parallel stage lists: 8 replicas of one process at Humanoid widths, each on
    its 1024-row shard (split-K grad-only dW at B >= 512, the fixed-order sum in place of RCCL's
    all-reduce, flat Adam with grad scale 1/8), against the oracle's ONE global-batch step at
    B = 8192 (TD3_featured.py:148-164).  A critic-only and a policy step, teacher-forced;
    with the critic as one exchange and as the overlapped schedule's two buckets (TD3_DP_BUCKETS).
    The critic and critic_target are held to the single-device 99.9 % post-Adam contract against the
    oracle's data-parallel form (oracle_dp_step at 8 x 1024)."""
    from helpers import featured_setup_dims
    from td3_amd.data_parallel import train_local
    monkeypatch.setenv("TD3_DP_BUCKETS", buckets)
    monkeypatch.setenv("TD3_DP_SHARD", shard)
    n, b = 8, 1024
    S = featured_setup_dims(376, 17, 0.4, "layer", B=n * b, steps=2)
    pols, rbs = _replicas(S, n, _make)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rs = np.random.RandomState(55)
    for step in (1, 2):
        idx = rs.randint(0, gen.BUFFER_ROWS, size=n * b)
        noise = rs.standard_normal((n * b, S["ad"])).astype(np.float32)
        for pol in pols:
            _load_oracle_state(pol, L)
        L0 = copy.deepcopy(L)
        Ldp = oracle_dp_step(L, S["buf"].gather(idx), noise, n)
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        outs = train_local(pols, rbs, b, indices=idx.reshape(n, b), noise=noise.reshape(n, b, -1), stats=True)
        y = np.concatenate([o["y"][:, 0] for o in outs])
        q2 = np.concatenate([o["q2"][:, 0] for o in outs])
        assert _rel_to_max(y, rec["y"][:, 0]) <= 1e-5, (step, "y")
        assert _rel_to_max(q2, rec["q2"][:, 0]) <= 1e-5, (step, "q2")
        np.testing.assert_allclose(np.mean([o["critic_loss"] for o in outs]), rec["critic_loss"], rtol=1e-5)
        assert all(o["actor_step"] == ("actor_loss" in rec) for o in outs)
        if "actor_loss" in rec:
            np.testing.assert_allclose(np.mean([o["actor_loss"] for o in outs]), rec["actor_loss"],
                                       rtol=1e-5, atol=1e-7)
        _check_replicas_equal(pols)
        _check_grads(pols[0], n, {"critic_grads": rec["critic_grads"]}, step)
        # the critic and its target at the single-device 99.9 % contract against the oracle restated in
        # the product's data-parallel form (the same 8 shard sums in replica order, oracle_dp_step);
        # the actor phase teacher-forced from the GPU's post-step critic and against that DP-form
        # oracle, both at the same contract (_check_actor_phase)
        for grp, ref in (("critic", Ldp.critic), ("critic_target", Ldp.critic_target)):
            _params_close(getattr(pols[0], grp).numpy_dict(), ref, L.lr, (step, "dp-oracle", grp))
        for grp, ref in (("actor", L.actor), ("actor_target", L.actor_target)):
            _params_close(getattr(pols[0], grp).numpy_dict(), ref, L.lr, (step, grp), frac=0.99)
        _check_actor_phase(pols, n, L0, S["buf"].gather(idx)[0], rec, Ldp, step, dp_frac=0.998)
        assert all(q._counters() == (L.total_it, L.critic_step, L.actor_step) for q in pols)


def test_rebuild_leaving_sharded_schedule_gathers_moments(monkeypatch):
    """the Adam moments of a sharded schedule live on their slice owners.  A plan rebuilt
    without sharding (TD3_DP_SHARD changed, a new batch size) must first bring every replica the
    whole moments, or each carries on with stale moments for the slices it did not own.  Two
    policy steps sharded at 128 rows per replica, then two all-reduce steps at 64 rows (a new
    plan), against the same four steps all-reduce throughout: parameters, targets and all four
    Adam moment arenas bit-identical on every replica (the sharded and the replicated Adam are the
    same element-wise update of the same summed gradient)."""
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    from td3_amd.data_parallel import train_local
    G = load_golden("featured", "hc_layer")
    S = featured_setup("hc_layer")
    n = 2

    def views(pol):
        return _all_views(pol) + [_ParamView(pol, w, g).flat() for w, g in (
            (_lib.TD3_ACTOR_ADAM_V, 0), (_lib.TD3_CRITIC_ADAM_M, 1))]

    def run(first):
        monkeypatch.setenv("TD3_DP_SHARD", first)
        pols, rbs = _replicas(S, n, _make)
        for step, b in ((1, 128), (2, 128), (3, 64), (4, 64)):
            if step == 3:
                monkeypatch.setenv("TD3_DP_SHARD", "0")
            idx, noise = G[f"step{step}/idx"][:n * b], G[f"step{step}/noise"][:n * b]
            train_local(pols, rbs, b, indices=idx.reshape(n, b), noise=noise.reshape(n, b, -1))
        from test_gpu_w4 import _flags
        flags = [_flags(p) for p in pols]
        return [views(p) for p in pols], flags

    ref, ref_flags = run("0")
    got, got_flags = run("2")
    assert all(f & 2 == 0 for f in ref_flags + got_flags)     # both end on the all-reduce plan
    for r, g in zip(ref, got):
        for a, b in zip(r, g):
            np.testing.assert_array_equal(a, b)


def test_local_replicas_free_running_philox():
    """Production draws (each replica's Philox stream over its own ring, device noise): four
    free-running steps keep the replicas bit-identical although their batches differ."""
    from td3_amd.data_parallel import train_local
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    from test_gpu_parity import Box
    S = featured_setup("hc_layer")
    pols, _ = _replicas(S, 2, _make)
    rbs = []
    data = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], gen.BUFFER_ROWS, gen.SEED)
    for seed in (11, 12):                  # one Philox stream per replica's ring
        rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS, seed=seed)
        rb.add_batch(*data)
        rbs.append(rb)
    for _ in range(4):
        outs = train_local(pols, rbs, 128, stats=True)
        assert all(np.isfinite(o["critic_loss"]) for o in outs)
    _check_replicas_equal(pols)


def test_local_replica_queries_after_policy_steps():
    """Replica k > 0 of a local group steps on replica 0's stream: its policy steps record an event
    there (step.hip note_actor_update) that its queries wait for.  Queries right after each step,
    without syncs, equal across replicas (lock-step actors) and equal the query after a device sync."""
    from td3_amd.data_parallel import train_local
    S = featured_setup("hc_layer")
    pols, rbs = _replicas(S, 2, _make)
    s = np.random.RandomState(5).standard_normal((4, S["sd"])).astype(np.float32)
    got = []
    for _ in range(4):                     # critic-only, policy, critic-only, policy
        train_local(pols, rbs, 128)
        got.append([p.select_action(s[len(got)]) for p in pols])
    for p in pols:
        p.sync()
    for t, (x0, x1) in enumerate(got):
        np.testing.assert_array_equal(x0, x1, err_msg=f"t={t}")
    np.testing.assert_array_equal(got[-1][1], pols[1].select_action(s[3]))
    _check_replicas_equal(pols)


def test_particle_local_replicas_equal_global_batch_step():
    from test_gpu_particles import _make as make_particles
    from td3_amd.data_parallel import train_local
    G = load_golden("particles", "part_layer")
    S = particle_setup("part_layer")
    n, B = 2, S["B"]
    b = B // n
    pols, rbs = _replicas(S, n, make_particles)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in range(1, S["steps"] + 1):
        p = f"step{step}"
        idx, noise = G[f"{p}/idx"], G[f"{p}/noise"]
        for pol in pols:
            _load_oracle_state(pol, L)
        rec = orc.particle_train_step(L, S["buf"].gather(idx), noise)
        outs = train_local(pols, rbs, b, indices=idx.reshape(n, b), noise=noise.reshape(n, b, -1), stats=True)
        assert _rel_to_max(np.concatenate([o["y"] for o in outs]), rec["y"]) <= 1e-5, p
        _check_replicas_equal(pols)
        _check_grads(pols[0], n, rec, p)
        _params_close(pols[0].critic.numpy_dict(), L.critic, L.lr, (p, "critic"), frac=0.99)
        _params_close(pols[0].actor.numpy_dict(), L.actor, L.lr, (p, "actor"), frac=0.99)
        _params_close(pols[0].critic_target.numpy_dict(), L.critic_target, L.lr, (p, "critic_target"), frac=0.99)


def test_local_replica_refuses_single_train():
    from td3_amd import _lib
    S = featured_setup("hc_layer")
    pols, rbs = _replicas(S, 2, _make)
    with pytest.raises(_lib.TD3Error, match="td3_train_step_local"):
        pols[0].train(rbs[0], 64)
