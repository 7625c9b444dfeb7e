"""CPU checks of the data-parallel edge cases (tests/dp_reference.py) that tests/test_gpu_dp_edges.py leans
on: the table covers every branch it claims, the odd replica counts put the last slice into the arena's
pad, the two forms of the oracle agree at the contract of tests/test_dp_oracle.py, a step that forgot the
1/n scale or the last shard is far outside the GPU's moment tolerance, and no relu' of the fp32 oracle is
ambiguous (tests/test_gpu_gradients.py)."""
import copy

import numpy as np
import pytest

import dp_reference as dp
import per_reference as per
from helpers import gen, oracle_dp_step, orc
from test_dp_oracle import _tight_fraction

_FEATURED = [c["name"] for c in dp.EDGES]
_PARTICLES = [c["name"] for c in dp.PARTICLE_EDGES]
SEPARATION = 100 * per.MOMENT_TOL


def _rel_to_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.abs(b).max() + 1e-30))


def test_edge_table():
    assert _FEATURED == ["r2_b1", "r5_b33", "r7_b16", "dw64", "dwsk", "none", "wn_sk", "hum", "hum_buckets",
                         "rec139", "a32", "a1", "in512", "odd"]
    assert _PARTICLES == ["part_r3", "part_r2"]
    assert len(dp.BY_NAME) == len(dp.EDGES) + len(dp.PARTICLE_EDGES)              # names are unique
    by = dp.BY_NAME
    for c in by.values():
        assert 1 <= c["n"] <= dp.MAX_REPLICAS and 1 <= c["b"] and c["n"] * c["b"] <= 2560, c["name"]
    shape = lambda k: (by[k]["sd"], by[k]["ad"], by[k]["norm"], by[k]["n"], by[k]["b"])   # noqa: E731
    # ragged per-replica batches (Bp > b), one row; the row tile of 16
    assert shape("r2_b1") == (17, 6, "layer", 2, 1) and shape("r5_b33") == (17, 6, "layer", 5, 33)
    assert shape("r7_b16") == (17, 6, "layer", 7, 16)
    # the dW kernels (stages.hip make_dw_work): 64 x 64 tiles from 512 rows, split-K where 64 | b
    assert shape("dw64") == (17, 6, "layer", 2, 544) and by["dw64"]["b"] >= 512 and by["dw64"]["b"] % 64
    assert shape("dwsk") == (17, 6, "layer", 2, 576) and by["dwsk"]["b"] % 64 == 0
    assert shape("none") == (17, 6, None, 5, 512) and shape("wn_sk") == (17, 6, "weight_normalization", 2, 512)
    # widths: the separate gather (a record of more than 128 floats), the heads, the widest input, odd widths
    assert shape("hum") == (376, 17, "layer", 3, 128) and shape("hum_buckets") == (376, 17, "layer", 2, 512)
    assert shape("rec139") == (60, 17, "layer", 2, 100) and 2 * 60 + 17 + 2 == 139
    assert by["rec139"]["max_action"] == 2.0
    assert shape("a32") == (9, 32, "layer", 3, 64) and shape("a1") == (3, 1, "layer", 5, 33)
    assert shape("in512") == (480, 32, "layer", 2, 64) and 480 + 32 == 512
    assert shape("odd") == (11, 3, "layer", 5, 96)
    assert (by["odd"]["actor_arch"], by["odd"]["q_arch"]) == ((64, 48, 40), (96, 72, 33))
    # the knobs, and the cases whose schedule keeps the all-reduce
    assert [(k, by[k]["env"]) for k in _FEATURED if "env" in by[k]] == [("hum_buckets", {"TD3_DP_BUCKETS": "1"})]
    assert [k for k in by if dp.case_shards(by[k]) != ("1", "0")] == ["wn_sk", "hum_buckets"]
    assert dp.case_shards(by["wn_sk"]) == dp.case_shards(by["hum_buckets"]) == ("0",)
    # odd replica counts beside the powers of two tests/test_gpu_data_parallel.py runs (2, 4, 8)
    assert sorted({c["n"] for c in by.values()}) == [2, 3, 5, 7]
    assert [k for k in _FEATURED if not dp.seed_sets_margin(by[k])] == ["dw64", "dwsk", "none", "wn_sk", "hum_buckets"]
    assert [(by[k]["dims"], by[k]["n"], by[k]["b"]) for k in _PARTICLES] == [((7, 16, 9, 3), 3, 11), ((7, 16, 9, 3), 2, 32)]


def test_arena_sizes_restate_the_layout():
    """dp.arena_sizes against the parameter count for widths that need no padding, and the known pads."""
    case = dp.edge_case("x", 32, 32, 1.0, "layer", 2, 64, 0, actor_arch=(64, 64, 64), q_arch=(64, 64, 64))
    S = dp.edge_setup(case)
    actor, critic = dp.arena_sizes(case)
    assert actor == sum(v.size for v in S["actor"].values())
    # the critic's one-column head is stored as 32 rows: 31 * (64 + 1) pad floats per network
    assert critic == sum(v.size for v in S["critic"].values()) + 2 * 31 * 65
    for c in dp.EDGES + dp.PARTICLE_EDGES:
        if c["norm"] != "weight_normalization":
            assert all(x % 32 == 0 for x in dp.arena_sizes(c)), c["name"]


@pytest.mark.parametrize("name", [c["name"] for c in dp.EDGES + dp.PARTICLE_EDGES if c["n"] & (c["n"] - 1)])
def test_odd_replica_counts_slice_into_the_pad(name):
    """With n no power of two, n slices of ceil(size / 4n) * 4 floats overrun at least one arena: the last
    replica's slice Adam, its parameter copies and copy_local_moments all reach into the pad, and stay
    inside the 256 floats the arena keeps for that (learner.h Group::cap)."""
    case = dp.BY_NAME[name]
    n = case["n"]
    over = [dp.shard_slice(size, n) * n - size for size in dp.arena_sizes(case)]
    assert max(over) > 0, over
    assert all(0 <= o <= 256 for o in over), over
    assert float(np.float32(1.0 / n)) != 1.0 / n              # grad_scale 1/n is a rounded float


# ---------------------------------------------------------------- the featured cases
_analysis = {}


def _analyse(name):
    """Every figure the tests below assert for one featured case, from one chain of reference steps."""
    if name in _analysis:
        return _analysis[name]
    case = dp.BY_NAME[name]
    S, steps = dp.edge_reference(case)
    n = case["n"]
    lr = S["kw"].get("lr", 1e-4)
    out = dict(lr=lr, agree=[], apart=[], flips=[])
    for t, st in enumerate(steps):
        Ldp, L, L0, rec = st["Ldp"], st["L"], st["L0"], st["rec"]
        assert ("actor_loss" in rec) == (t == 1)
        assert (Ldp.total_it, Ldp.critic_step, Ldp.actor_step) == (L.total_it, L.critic_step, L.actor_step)
        for grp in ("critic", "critic_target", "actor", "actor_target"):
            a, b = getattr(Ldp, grp), getattr(L, grp)
            worst = max(float(np.max(np.abs(np.asarray(a[k], np.float64) - b[k]))) for k in b)
            out["agree"].append((t + 1, grp, worst, _tight_fraction(a, b)))
        nz = st["noise"].reshape(n * case["b"], -1)
        for vname, reduce in dp.VARIANTS.items():
            Lv = oracle_dp_step(copy.deepcopy(L0), st["batch"], nz, n, reduce=reduce)
            for k in Ldp.critic_m:
                out["apart"].append((t + 1, vname, "critic", k, _rel_to_max(Lv.critic_m[k], Ldp.critic_m[k])))
            if t == 1:
                for k in Ldp.actor_m:
                    out["apart"].append((t + 1, vname, "actor", k, _rel_to_max(Lv.actor_m[k], Ldp.actor_m[k])))
        s, a = st["batch"][0], st["batch"][1]
        out["flips"].append((t + 1,) + dp.relu_mask_flips(L0, Ldp.critic, s, a, n, t == 1))
    _analysis[name] = out
    return out


@pytest.mark.parametrize("name", _FEATURED)
def test_dp_oracle_agrees_with_global_batch_oracle(name):
    """helpers.oracle_dp_step against orc.featured_train_step on the n * b rows at the contract of
    tests/test_dp_oracle.py: within 2*lr everywhere, >= 99 % within 1e-6 + 1e-5|x|."""
    r = _analyse(name)
    for step, grp, worst, frac in r["agree"]:
        assert worst <= 2 * r["lr"] * 1.001, (name, step, grp, worst)
        assert frac >= 0.99, (name, step, grp, frac)


@pytest.mark.parametrize("name", _FEATURED)
def test_wrong_reductions_are_far_outside_the_moment_tolerance(name):
    """A step that sums without the 1/n scale, and one that drops the last replica's shard, each leave the
    critic's exp_avg (both steps) and the actor's (step 2) more than 100x MOMENT_TOL from the correct
    data-parallel step's, tensor by tensor: the GPU test's moment check cannot pass either."""
    r = _analyse(name)
    assert len(r["apart"]) > 0
    for step, variant, grp, k, d in r["apart"]:
        assert d > SEPARATION, (name, step, variant, grp, k, d)


@pytest.mark.parametrize("name", _FEATURED)
def test_no_relu_of_the_oracle_is_ambiguous(name):
    """The fp32 oracle's relu' masks (Q1, Q2; on step 2 the actor and Q1(s, pi) on the updated critic), on
    every shard, equal those of the same forward in float64, and no float64 pre-activation lies within
    dp.RELU_MARGIN (2 ulp of its layer's largest) of zero, where two correct fp32 implementations may decide
    differently and then differ by a whole row's gradient (held where the seed chooses the rows,
    dp.seed_sets_margin).  Mask equality alone let a32's first seed through:
    the oracle agreed with float64 at z = -2.4e-7 and the GPU did not (noted beside the case)."""
    r = _analyse(name)
    for step, flips, total, margin in r["flips"]:
        assert total > 0 and flips == 0, (name, step, flips, total)
        print(f"dp edge {name} step {step}: smallest |z| {margin:.2e} of its layer's max (margin {dp.RELU_MARGIN:.2e})")
        if dp.seed_sets_margin(dp.BY_NAME[name]):
            assert margin >= dp.RELU_MARGIN, (name, step, margin)


# ---------------------------------------------------------------- the particle cases
@pytest.mark.parametrize("name", _PARTICLES)
def test_particle_wrong_reductions_are_far_outside_the_moment_tolerance(name):
    case = dp.BY_NAME[name]
    S = dp.edge_setup(case)
    n, b = case["n"], case["b"]
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in (1, 2):
        idx, noise = dp.edge_step(case, S, step)
        assert idx.shape == (n, b) and noise.shape == (n, b, S["A"])
        assert idx.min() >= 0 and idx.max() < gen.BUFFER_ROWS
        batch, nz = S["buf"].gather(idx.reshape(-1)), noise.reshape(n * b, -1)
        L0 = copy.deepcopy(L)
        rec = orc.particle_train_step(L, batch, nz)
        assert ("actor_loss" in rec) == (step == 2)
        for variant in dp.VARIANTS:
            cm, am = dp.particle_variant_moments(L0, batch, nz, n, b, variant)
            for k in L.critic_m:
                assert _rel_to_max(cm[k], L.critic_m[k]) > SEPARATION, (name, step, variant, k)
            if step == 2:
                for k in L.actor_m:
                    assert _rel_to_max(am[k], L.actor_m[k]) > SEPARATION, (name, step, variant, k)
