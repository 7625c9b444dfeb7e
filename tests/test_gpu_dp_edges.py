"""The data-parallel step (td3_comm_init_local groups: gradient-only dW, the fixed-order sum, the flat or
sharded optimizer tail of dp.hip) at the planner's edge shapes (dp_reference.EDGES) against the oracle's
data-parallel form and its global-batch step, teacher-forced from the oracle's state; the sharded
schedule against the all-reduce bit for bit; identical shards against one replica bit for bit; free
running on partly filled rings; the refusals of the group's two entry points.

Each case is there for one choice of the planner or one corner of the seam: ragged per-replica batches
and one row, replica counts whose slices run into the arena's pad (grad_scale 1/n no power of two),
dw_kernel / dw64_kernel / split-K in gradient-only mode, no LayerNorm, weight norm behind a split-K dW,
the separate gather, the head widths, the widest input, odd hidden widths, the two critic buckets.
tests/test_dp_reference.py holds on the CPU that a step which forgot the 1/n scale or the last shard is
more than 100x the moment tolerance away and that no relu' of the oracle is ambiguous.

Tolerances are the project's (tests/test_gpu_data_parallel.py, tests/test_gpu_parity.py): forward values
and losses rtol 1e-5, the summed critic gradient / n within 2e-4 of its scale, post-Adam parameters within
1e-6 + 1e-5|x| on >= 99.9 % of the elements against the oracle's data-parallel form and within 2*lr
everywhere, Adam exp_avg within 2e-4 and exp_avg_sq within 4e-4 of their max."""
import ctypes as C

import numpy as np
import pytest

import dp_reference as dp
from helpers import gen, orc
from per_reference import MOMENT_TOL
from test_gpu_data_parallel import _all_views, _check_actor_phase, _check_grads, _check_replicas_equal, _replicas
from test_gpu_dw_schedules import KNOBS, _group_tails
from test_gpu_parity import Box, _load_oracle_state, _params_close, _rel_to_max
from test_gpu_prioritized_edges import _make as _make_edge

pytestmark = pytest.mark.gpu

V_TOL = 4e-4                # exp_avg_sq (test_gpu_parity, test_gpu_philox_shapes)
C_DW = {"dw64": "td3::dw64_kernel<true>", "dwsk": "td3::dwsk_kernel<true, ", "none": "td3::dwsk_kernel<true, ",
        "wn_sk": "td3::dwsk_kernel<true, ", "hum_buckets": "td3::dwsk_kernel<true, "}
A_DW = {"dw64": "td3::dw64_kernel<false>", "dwsk": "td3::dwsk_kernel<false, ", "none": "td3::dwsk_kernel<false, ",
        "wn_sk": "td3::dwsk_kernel<false, ", "hum_buckets": "td3::dwsk_kernel<false, "}
_STEP_CASES = [(c, s) for c in dp.EDGES for s in dp.case_shards(c)]
_BITWISE = [c for c in dp.EDGES + dp.PARTICLE_EDGES if dp.case_shards(c) == ("1", "0")]


def _maker(case):
    if dp.is_particles(case):
        from test_gpu_particles import _make as make_particles
        return make_particles
    return lambda S: _make_edge(S, prioritized=False)


def _environment(monkeypatch, case, shard):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TD3_DP_SHARD", shard)
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)


def _last_stages(pol):
    """[(stage name, HIP kernel)] of the stage list the replica's last step ran (td3_debug_last_stage:
    td3_profile_stages cannot run on a replica, its collective stages refuse to launch)."""
    out = []
    while True:
        name = pol._lib.td3_debug_last_stage(pol._h, len(out), 0).decode()
        if not name:
            return out
        out.append((name, pol._lib.td3_debug_last_stage(pol._h, len(out), 1).decode()))


def _check_tail(case, shard, stages, policy_step):
    """The dW kernel the case is there for and the optimizer tail behind it, by name, for the critic and on a
    policy step the actor: the all-reduce + flat Adam (wn_kernel under weight normalization), the sharded
    step + its Polyak or image pack, the two critic buckets; the particle learner's encoder step in between."""
    name = case["name"]
    tails = _group_tails(stages)
    names, kernels = [s[0] for s in tails], dict(tails)
    part = ["{0}_enc_adam"] if dp.is_particles(case) else []
    small = "td3::dw_kernel<false>" if dp.is_particles(case) else None
    want = []
    for tag in ("C", "A") if policy_step else ("C",):
        polyak = policy_step                          # Polyak of both groups rides the policy step's tails
        if name == "hum_buckets" and tag == "C":
            want += ["C_dw_0", "C_dw_1", "C_0_allreduce", "C_1_allreduce", "C_join"]
            assert kernels["C_dw_0"].startswith(C_DW[name]) and kernels["C_dw_1"].startswith(C_DW[name]), tails
            continue
        dw = kernels[f"{tag}_dw"]
        expect = (C_DW if tag == "C" else A_DW).get(name, small or f"td3::dw_kernel<{'true' if tag == 'C' else 'false'}>")
        assert dw.startswith(expect), (name, tag, dw)
        if case["norm"] == "weight_normalization":
            want += [f"{tag}_dw", f"{tag}_allreduce", f"{tag}_wn"]
            assert kernels[f"{tag}_wn"] == "td3::wn_kernel", tails
        elif shard == "1":
            got = [x for x in names if x.startswith(tag + "_")]
            assert got[:len(part) + 2] == [f"{tag}_dw"] + [p.format(tag) for p in part] + [f"{tag}_rs_adam_ag"], tails
            assert set(got[len(part) + 2:]) <= {f"{tag}_polyak", f"{tag}_w4"}, tails
            assert (f"{tag}_polyak" in got) == polyak, tails
            if polyak:
                assert kernels[f"{tag}_polyak"] in ("td3::polyak_w4_kernel", "td3::polyak_flat_kernel"), tails
            want += got
        else:
            want += [f"{tag}_dw"] + [p.format(tag) for p in part] + [f"{tag}_allreduce", f"{tag}_adam"]
            assert kernels[f"{tag}_adam"] == "td3::adam_flat_kernel", tails
    assert names == want, (name, shard, tails)


def _moment_errors(pol, which_m, which_v, group, ref_m, ref_v):
    from td3_amd.TD3_featured import _ParamView
    m = _ParamView(pol, which_m, group).numpy_dict()
    v = _ParamView(pol, which_v, group).numpy_dict()
    return (max((_rel_to_max(m[k], ref_m[k]), k) for k in ref_m), max((_rel_to_max(v[k], ref_v[k]), k) for k in ref_v))


@pytest.mark.parametrize("case,shard", _STEP_CASES, ids=[f"{c['name']}-shard{s}" for c, s in _STEP_CASES])
def test_dp_step_edge_shapes(case, shard, monkeypatch):
    """Two steps (critic-only, then the actor phase), each from the oracle's state loaded into every replica,
    injected rows and noise: every output of the step, the replicas bit for bit, the summed gradient, the
    parameters and both Adam moments against the oracle's data-parallel form, and the stage list by name."""
    from td3_amd import _lib
    from td3_amd.data_parallel import train_local
    _environment(monkeypatch, case, shard)
    name, n, b = case["name"], case["n"], case["b"]
    S, steps = dp.edge_reference(case)
    pols, rbs = _replicas(S, n, _maker(case))
    lr = S["kw"].get("lr", 1e-4)
    for t, st in enumerate(steps):
        what = (name, shard, t + 1)
        L0, Ldp, L, rec = st["L0"], st["Ldp"], st["L"], st["rec"]
        for pol in pols:
            _load_oracle_state(pol, L0)
        outs = train_local(pols, rbs, b, indices=st["idx"], noise=st["noise"], stats=True)
        stages = [_last_stages(p) for p in pols]
        # forward values against the global-batch oracle; each replica's loss is its shard's mean
        np.testing.assert_array_equal(np.concatenate([o["idx"] for o in outs]), st["idx"].reshape(-1))
        for k in ("y", "q1", "q2"):
            assert _rel_to_max(np.concatenate([o[k][:, 0] for o in outs]), rec[k][:, 0]) <= 1e-5, what + (k,)
        np.testing.assert_allclose(np.mean([o["critic_loss"] for o in outs]), rec["critic_loss"], rtol=1e-5)
        assert all(o["actor_step"] == (t == 1) for o in outs)
        if t == 1:
            np.testing.assert_allclose(np.mean([o["actor_loss"] for o in outs]), rec["actor_loss"], rtol=1e-5, atol=1e-7)
        assert all(q._counters() == (L.total_it, L.critic_step, L.actor_step) for q in pols)
        _check_replicas_equal(pols)
        pol = pols[0]
        _check_grads(pol, n, {"critic_grads": rec["critic_grads"]}, what)
        cm, cv = _moment_errors(pol, _lib.TD3_CRITIC_ADAM_M, _lib.TD3_CRITIC_ADAM_V, 1, Ldp.critic_m, Ldp.critic_v)
        am = av = (0.0, "")
        if t == 1:
            am, av = _moment_errors(pol, _lib.TD3_ACTOR_ADAM_M, _lib.TD3_ACTOR_ADAM_V, 0, Ldp.actor_m, Ldp.actor_v)
        print(f"dp edge {name} shard {shard} step {t + 1}: critic exp_avg {cm[0]:.3e} ({cm[1]}) exp_avg_sq {cv[0]:.3e}, "
              f"actor exp_avg {am[0]:.3e} ({am[1]}) exp_avg_sq {av[0]:.3e}; bounds {MOMENT_TOL:.0e} / {V_TOL:.0e}")
        for grp, ref in (("critic", Ldp.critic), ("critic_target", Ldp.critic_target)):
            _params_close(getattr(pol, grp).numpy_dict(), ref, lr, what + ("dp-oracle", grp))
        _check_actor_phase(pols, n, L0, st["batch"][0], rec, Ldp, what)
        assert cm[0] <= MOMENT_TOL and cv[0] <= V_TOL, what + ("critic moments", cm, cv)
        assert am[0] <= MOMENT_TOL and av[0] <= V_TOL, what + ("actor moments", am, av)
        # the same stage list on every replica, and the kernels the case is there for
        assert all(s == stages[0] for s in stages), what
        print(f"dp edge {name} shard {shard} step {t + 1} tail: {_group_tails(stages[0])}")
        _check_tail(case, shard, stages[0], t == 1)
    from test_gpu_w4 import _flags
    assert all(bool(_flags(p) & 2) == (shard == "1") for p in pols)


def _views(pol):
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    return _all_views(pol) + [_ParamView(pol, w, g).flat() for w, g in ((_lib.TD3_ACTOR_ADAM_V, 0), (_lib.TD3_CRITIC_ADAM_M, 1))]


def _free_standing(case, shard, monkeypatch, n=None, same_rows=False):
    """Every replica's views after the case's two injected steps from the initial weights; ``same_rows``: every
    replica is fed replica 0's rows and noise."""
    from td3_amd.data_parallel import train_local
    _environment(monkeypatch, case, shard)
    n = n or case["n"]
    S = dp.edge_setup(case)
    pols, rbs = _replicas(S, n, _maker(case))
    for step in (1, 2):
        idx, noise = dp.edge_step(case, S, step)
        if same_rows:
            idx, noise = np.repeat(idx[:1], n, axis=0), np.repeat(noise[:1], n, axis=0)
        train_local(pols, rbs, case["b"], indices=idx, noise=noise)
    assert all(p._counters() == (2, 2, 1) for p in pols)
    return [_views(p) for p in pols]


@pytest.mark.parametrize("case", _BITWISE, ids=[c["name"] for c in _BITWISE])
def test_sharded_equals_allreduce(case, monkeypatch):
    """The sharded and the replicated Adam are the same element-wise update of the same summed gradient:
    after the case's two steps, parameters, targets and all four moment arenas are bit-identical on every
    replica -- a slice lost in the arena's pad, a stale slice or a moment copied short cannot hide."""
    ref = _free_standing(case, "0", monkeypatch)
    got = _free_standing(case, "1", monkeypatch)
    for k, (r, g) in enumerate(zip(ref, got)):
        for i, (x, y) in enumerate(zip(r, g)):
            np.testing.assert_array_equal(x, y, err_msg=f"{case['name']} replica {k} view {i}")
        for i, (x, y) in enumerate(zip(ref[0], g)):
            np.testing.assert_array_equal(x, y, err_msg=f"{case['name']} replica {k} against replica 0, view {i}")


@pytest.mark.parametrize("shard", ["0", "1"])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("name", ["r2_b1", "dw64", "a32"])
def test_identical_shards_equal_one_replica(name, n, shard, monkeypatch):
    """n replicas fed the same rows and noise against a one-replica group on those rows, bit for bit: the
    fixed-order sum of n equal gradients is n g exactly (g + g; 3g rounds by at most half an ulp of 4g, and
    adding g lands on 4g) and the scales 1/2, 1/4 are powers of two -- local_sum_kernel and grad_scale alone."""
    case = dp.BY_NAME[name]
    one = _free_standing(case, shard, monkeypatch, n=1, same_rows=True)[0]
    for k, got in enumerate(_free_standing(case, shard, monkeypatch, n=n, same_rows=True)):
        for i, (x, y) in enumerate(zip(one, got)):
            np.testing.assert_array_equal(x, y, err_msg=f"{name} n={n} replica {k} view {i}")


@pytest.mark.parametrize("case,shard", [(c, s) for c in dp.PARTICLE_EDGES for s in ("1", "0")],
                         ids=[f"{c['name']}-shard{s}" for c in dp.PARTICLE_EDGES for s in ("1", "0")])
def test_particle_dp_step_edge_shapes(case, shard, monkeypatch):
    """test_gpu_data_parallel.test_particle_local_replicas_equal_global_batch_step at ragged shards, three
    replicas and sharded, at its tolerances against the global-batch oracle; the critic's exp_avg at the
    moment tolerance (what sees a lost scale or shard, tests/test_dp_reference.py); the tail by name."""
    from td3_amd import _lib
    from td3_amd.data_parallel import train_local
    _environment(monkeypatch, case, shard)
    name, n, b = case["name"], case["n"], case["b"]
    S = dp.edge_setup(case)
    pols, rbs = _replicas(S, n, _maker(case))
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in (1, 2):
        what = (name, shard, step)
        idx, noise = dp.edge_step(case, S, step)
        for pol in pols:
            _load_oracle_state(pol, L)
        rec = orc.particle_train_step(L, S["buf"].gather(idx.reshape(-1)), noise.reshape(n * b, -1))
        outs = train_local(pols, rbs, b, indices=idx, noise=noise, stats=True)
        stages = [_last_stages(p) for p in pols]
        assert _rel_to_max(np.concatenate([o["y"] for o in outs]), rec["y"]) <= 1e-5, what
        np.testing.assert_allclose(np.mean([o["critic_loss"] for o in outs]), rec["critic_loss"], rtol=1e-5)
        assert all(o["actor_step"] == (step == 2) for o in outs)
        _check_replicas_equal(pols)
        _check_grads(pols[0], n, rec, what)
        cm, _ = _moment_errors(pols[0], _lib.TD3_CRITIC_ADAM_M, _lib.TD3_CRITIC_ADAM_V, 1, L.critic_m, L.critic_v)
        print(f"dp edge {name} shard {shard} step {step}: critic exp_avg {cm[0]:.3e} ({cm[1]}); bound {MOMENT_TOL:.0e}")
        _params_close(pols[0].critic.numpy_dict(), L.critic, L.lr, what + ("critic",), frac=0.99)
        _params_close(pols[0].actor.numpy_dict(), L.actor, L.lr, what + ("actor",), frac=0.99)
        _params_close(pols[0].critic_target.numpy_dict(), L.critic_target, L.lr, what + ("critic_target",), frac=0.99)
        assert cm[0] <= MOMENT_TOL, what + cm
        assert all(q._counters() == (L.total_it, L.critic_step, L.actor_step) for q in pols)
        assert all(s == stages[0] for s in stages), what
        print(f"dp edge {name} shard {shard} step {step} tail: {_group_tails(stages[0])}")
        _check_tail(case, shard, stages[0], step == 2)


@pytest.mark.parametrize("sd,ad", [(17, 6), (60, 17)], ids=["fused_sample", "separate_gather"])
def test_free_running_on_partly_filled_rings(sd, ad, monkeypatch):
    """Three replicas, 100 rows each, every ring its own Philox stream over only 300 filled rows of 1000: four
    production steps draw inside the filled rows, stay finite and keep the replicas bit-identical.  The
    sample runs inside the fused layer-0/1 launch (sd = 17) and as the separate gather (sd = 60)."""
    from td3_amd.data_parallel import train_local
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    case = dp.edge_case(f"free{sd}", sd, ad, 1.0, "layer", 3, 100, sd)
    _environment(monkeypatch, case, "0")
    S = dp.edge_setup(case)
    n, b, fill = case["n"], case["b"], 300
    pols, _ = _replicas(S, n, _maker(case))
    data = gen.fill_featured_buffer(sd, ad, 1.0, gen.BUFFER_ROWS, gen.SEED)
    rbs = []
    for seed in (21, 22, 23):
        rb = ReplayBuffer_featured(Box((sd,)), Box((ad,)), max_size=gen.BUFFER_ROWS, seed=seed)
        rb.add_batch(*(x[:fill] for x in data))
        assert rb.size == fill
        rbs.append(rb)
    drawn = []
    for _ in range(4):
        outs = train_local(pols, rbs, b, stats=True)
        assert all(np.isfinite(o["critic_loss"]) and np.isfinite(o["y"]).all() for o in outs)
        assert all(o["idx"].min() >= 0 and o["idx"].max() < fill for o in outs), [o["idx"].max() for o in outs]
        drawn.append([o["idx"].copy() for o in outs])
    assert all(p._counters() == (4, 4, 2) for p in pols)
    assert not np.array_equal(drawn[0][0], drawn[0][1]) and not np.array_equal(drawn[0][0], drawn[1][0])
    _check_replicas_equal(pols)
    # the path: with the record in 128 floats the free-running step's first stage samples the ring itself,
    # an injected step's (always behind the separate gather) does not; wider records gather in both
    free_first = _last_stages(pols[0])[0]
    train_local(pols, rbs, b, indices=np.zeros((n, b), np.int64))
    print(f"free running sd={sd}: first stage {free_first}, injected {_last_stages(pols[0])[0]}")
    assert (free_first != _last_stages(pols[0])[0]) == (2 * sd + ad + 2 <= 128)


def test_local_group_refusals():
    """Every refusal of td3_comm_init_local and td3_train_step_local once through the C ABI (rc -1, the
    message), each followed by a step of the group: the counters did not move at the refusal and the group
    still steps.  Replicas out of step are reached with td3_set_counters on one replica (the learner's
    public counter setter), without stepping a replica alone."""
    from td3_amd import _lib
    from td3_amd.data_parallel import train_local
    from test_gpu_particles import _make as make_particles
    hc = dp.edge_case("hc", 17, 6, 1.0, "layer", 2, 32, 5)
    S = dp.edge_setup(hc)
    make = _maker(hc)
    pols, rbs = _replicas(S, 2, make)
    lib = pols[0]._lib
    n, b = 2, hc["b"]
    rs = np.random.RandomState(5)
    stepped = [0]

    def handles(ps):
        return (C.c_void_p * len(ps))(*[p._h.value for p in ps])

    def rings(rs_):
        return (C.c_void_p * len(rs_))(*[r.handle.value for r in rs_])

    def refused(rc, text):
        assert rc == -1, (text, rc, lib.td3_last_error())
        assert text.encode() in lib.td3_last_error(), (text, lib.td3_last_error())
        assert all(p._counters()[0] == stepped[0] for p in pols), text
        idx = rs.randint(0, gen.BUFFER_ROWS, size=(n, b))
        train_local(pols, rbs, b, indices=idx, noise=rs.standard_normal((n, b, 6)).astype(np.float32))
        stepped[0] += 1
        assert all(p._counters()[0] == stepped[0] for p in pols), text

    def step(ps, rs_, count, batch, idx=None):
        ix = None if idx is None else _lib.i64ptr(np.ascontiguousarray(idx, np.int64))
        return lib.td3_train_step_local(handles(ps), rings(rs_), count, batch, ix, None, None)

    free = [make(S) for _ in range(3)]
    # td3_comm_init_local
    refused(lib.td3_comm_init_local(handles([free[0][0]]), 0), "1 .. 8 local replicas")
    refused(lib.td3_comm_init_local(handles([p for p, _ in free] * 3), 9), "1 .. 8 local replicas")
    refused(lib.td3_comm_init_local(handles([free[0][0], free[1][0], free[0][0]]), 3), "a handle appears twice")
    refused(lib.td3_comm_init_local(handles([free[0][0], pols[1]]), 2), "handle already in a data-parallel group")
    part, _ = make_particles(dp.edge_setup(dp.BY_NAME["part_r2"]))
    refused(lib.td3_comm_init_local(handles([free[0][0], part]), 2), "local replicas must have the same configuration")
    odd, _ = make(dp.edge_setup(dp.BY_NAME["odd"]))
    refused(lib.td3_comm_init_local(handles([free[0][0], odd]), 2), "local replicas must have the same configuration")
    # other dims in arenas of the same size: (3, 1) pads to the (17, 6) layout's 376512 and 666432 floats
    a1, a1_rb = make(dp.edge_setup(dp.BY_NAME["a1"]))
    assert dp.arena_sizes(dp.BY_NAME["a1"]) == dp.arena_sizes(hc)
    refused(lib.td3_comm_init_local(handles([free[0][0], a1]), 2), "local replicas must have the same configuration")
    # td3_train_step_local
    refused(step(pols[::-1], rbs[::-1], 2, b), "handles must be passed in the group's rank order")
    refused(step(pols[:1], rbs[:1], 1, b), "handles are not one td3_comm_init_local group")
    refused(step([free[0][0], free[1][0]], [free[0][1], free[1][1]], 2, b), "handles are not one td3_comm_init_local group")
    refused(step(pols, [rbs[0], a1_rb], 2, b), "replay buffer does not match")
    bad = rs.randint(0, gen.BUFFER_ROWS, size=(n, b))
    bad[1, b - 1] = gen.BUFFER_ROWS                                  # the ring's capacity: one past its last row
    refused(step(pols, rbs, 2, b, bad), "injected index out of range")
    bad[1, b - 1] = -1
    refused(step(pols, rbs, 2, b, bad), "injected index out of range")
    t, c, a = pols[1]._counters()
    pols[1]._set_counters(t + 1, c, a)
    rc = step(pols, rbs, 2, b)
    pols[1]._set_counters(t, c, a)
    refused(rc, "replicas out of step")
    refused(step(pols, rbs, 2, 0), "batch must be positive")
    _check_replicas_equal(pols)
    # the handles the refusals named are untouched: they still form a group of their own and step
    from td3_amd.data_parallel import local_group
    local_group([p for p, _ in free])
    train_local([p for p, _ in free], [r for _, r in free], b)
    assert all(p._counters() == (1, 1, 0) for p, _ in free)
