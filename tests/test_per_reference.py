"""CPU checks of the prioritized-replay references (tests/per_reference.py) that the GPU tests lean on."""
import copy

import numpy as np
import pytest

import bc_reference as bcr
import per_reference as per
from helpers import featured_setup, gen, orc


def _rel_to_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("name", ["hc_layer", "hc_layer_b100"])
def test_unit_weights_reproduce_the_oracle_step(name):
    """weighted_featured_step with w = 1 is orc.featured_train_step exactly: two steps (the second with
    the actor phase), every recorded value and every piece of learner state bit for bit."""
    S = featured_setup(name)
    La = orc.Learner(S["actor"], S["critic"], **S["kw"])
    Lb = copy.deepcopy(La)
    rs = np.random.RandomState(3)
    for step in (1, 2):
        batch = S["buf"].gather(rs.randint(0, gen.BUFFER_ROWS, size=S["B"]))
        noise = rs.standard_normal((S["B"], S["ad"])).astype(np.float32)
        ra = per.weighted_featured_step(La, batch, noise, np.ones(S["B"], np.float32))
        rb = orc.featured_train_step(Lb, batch, noise)
        for k in ("y", "q1", "q2", "next_action"):
            np.testing.assert_array_equal(ra[k], rb[k])
        assert ra["critic_loss"] == rb["critic_loss"] and ("actor_loss" in ra) == ("actor_loss" in rb) == (step == 2)
        for grp in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
            for k, v in getattr(La, grp).items():
                np.testing.assert_array_equal(v, getattr(Lb, grp)[k], err_msg=f"{grp}/{k}")
        assert (La.total_it, La.critic_step, La.actor_step) == (Lb.total_it, Lb.critic_step, Lb.actor_step)


@pytest.mark.parametrize("name", ["hc_layer", "hc_layer_b100"])
def test_weighted_reference_separates_from_unweighted(name):
    """CPU side of the teacher-forced test: the unweighted oracle's critic exp_avg differs from the
    weighted one's by more than 100x the tolerance the GPU is held to, tensor by tensor -- a step that
    ignored the weights cannot pass.  """
    for step in (1, 2):
        S, p, u, noise = per.step_case(name, step)
        idx = per.draw(p, u)
        w = per.weights(p, idx, gen.BUFFER_ROWS, 1.0)
        assert w.min() <= 0.2 and w.max() == 1.0
        Lw = orc.Learner(S["actor"], S["critic"], **S["kw"])
        Lu = copy.deepcopy(Lw)
        batch = S["buf"].gather(idx)
        per.weighted_featured_step(Lw, batch, noise, w)
        orc.featured_train_step(Lu, batch, noise)
        for k in Lw.critic_m:
            assert _rel_to_max(Lu.critic_m[k], Lw.critic_m[k]) > 100 * per.MOMENT_TOL, k


@pytest.mark.parametrize("rows,batches,bound", [(1000, 160, 1222.0), (100, 40, 169.0)])
def test_reference_draw_meets_the_chi_square_bound(rows, batches, bound):
    """The stratified reference draw stays under dof + 5 sqrt(2 dof), the bound the GPU draw is held to,
    and a draw that ignores the priorities is far above it."""
    B = 256
    p = np.exp(np.random.RandomState(rows).standard_normal(rows)).astype(np.float32)
    dof = rows - 1
    assert abs(dof + 5 * np.sqrt(2 * dof) - bound) < 1.0
    for seed in range(3):
        rs = np.random.RandomState(seed)
        u = ((np.arange(B)[None, :] + rs.uniform(size=(batches, B))) / B).astype(np.float32)
        idx = np.minimum(per.draw(p, u.ravel()), rows - 1)
        chi2, d = per.chi_square(np.bincount(idx, minlength=rows).astype(np.float64), p)
        assert d == dof and chi2 < bound, (seed, chi2)
    uniform = np.random.RandomState(9).randint(0, rows, size=batches * B)
    assert per.chi_square(np.bincount(uniform, minlength=rows).astype(np.float64), p)[0] > 10 * bound


# ---------------------------------------------------------------- the edge cases (per.EDGES)
_EDGE_IDS = [c["name"] for c in per.EDGES]
_DUPLICATES = ("b257", "dw64", "dwsk", "hum1024")


def test_step_case_is_unchanged():
    """The inputs of the two golden cases' callers, as they were before EDGES existed."""
    S, p, u, noise = per.step_case("hc_layer", 1)
    assert (S["B"], p.shape, u.shape, noise.shape) == (256, (gen.BUFFER_ROWS,), (256,), (256, 6))
    assert p[:8].tolist() == [8.0, 9.0, 1.0, 4.0, 14.0, 6.0, 15.0, 8.0]
    assert [float(x).hex() for x in u[:8]] == [
        "0x1.4401aa0000000p-2", "0x1.abdd860000000p-2", "0x1.d25ec20000000p-3", "0x1.c8ee080000000p-1",
        "0x1.ae570e0000000p-3", "0x1.da84440000000p-1", "0x1.beedd20000000p-1", "0x1.ea686c0000000p-2"]


def test_edge_table():
    assert _EDGE_IDS == ["b1", "b33", "b257", "dw64", "dwsk", "none", "wn", "hum", "hum1024", "rec139", "a32",
                         "a1", "in512", "odd", "part", "bc17", "bc1000"]
    by = {c["name"]: c for c in per.EDGES}
    assert [(n, by[n]["beta"]) for n in _EDGE_IDS if by[n]["beta"] != 1.0] == [("b257", 0.4), ("hum1024", 0.4)]
    assert [(n, per.edge_fill(by[n])) for n in _EDGE_IDS if "fill" in by[n]] == [("in512", 300), ("part", 300)]
    assert [(n, by[n]["bc_alpha"]) for n in _EDGE_IDS if "bc_alpha" in by[n]] == [("bc17", 2.5), ("bc1000", 2.5)]
    assert (by["odd"]["actor_arch"], by["odd"]["q_arch"]) == ((64, 48, 40), (96, 72, 33))
    assert max(c["B"] for c in per.EDGES) == 1024


def _edge_reference_step(case, L, batch, noise, w):
    """The reference step the GPU test compares with: weighted, with the BC actor loss in the bc* cases;
    ``w`` None: the same step without weights."""
    if case.get("bc_alpha"):
        return bcr.bc_featured_step(L, batch, noise, case["bc_alpha"], w=w)
    if w is None:
        return orc.featured_train_step(L, batch, noise)
    return per.weighted_featured_step(L, batch, noise, w)


@pytest.mark.parametrize("case", per.EDGES, ids=_EDGE_IDS)
def test_edge_case_inputs(case):
    """The conditions the GPU test (tests/test_gpu_prioritized_edges.py) leans on, for the same two steps
    from the same chain of oracle states: the draw is exact and stays inside the filled rows, the
    weights spread, rows repeat where the case is there for that, both BC terms carry weight, and the
    critic's exp_avg of a step that ignored the weights is more than 100x MOMENT_TOL away, tensor by tensor.
    b1 is exempt from the spread and the separation: its one weight is 1 and both steps are the same."""
    S = per.edge_setup(case)
    fill, B, beta = S["fill"], S["B"], case["beta"]
    assert S["buf"].size == fill and (S["sd"], S["ad"], S["ma"], S["norm"]) == \
        (case["sd"], case["ad"], case["max_action"], case["norm"])
    Lw = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in (1, 2):
        p, u, noise = per.edge_step(case, S, step)
        assert p.shape == (fill,) and u.shape == (B,) and noise.shape == (B, S["ad"])
        assert p.min() >= 1 and p.max() <= 15 and (p == np.round(p)).all()
        assert float(np.float32(p.sum())) == p.astype(np.float64).sum()        # exact prefix sums
        assert ((u * np.float32(p.sum())).astype(np.float32) < p.sum()).all()
        idx = per.draw(p, u)
        assert idx.min() >= 0 and idx.max() < fill
        w = per.weights(p, idx, fill, beta)
        assert w.max() == 1.0
        if B == 1:
            assert w[0] == 1.0
        else:
            assert w.min() <= (0.2 if beta == 1.0 else 0.5), w.min()
        if case["name"] in _DUPLICATES:
            assert B - np.unique(idx).size >= 1
        Lu = copy.deepcopy(Lw)
        batch = S["buf"].gather(idx)
        rec = _edge_reference_step(case, Lw, batch, noise, w)
        _edge_reference_step(case, Lu, batch, noise, None)
        assert ("actor_loss" in rec) == (step == 2)
        if B > 1:
            for k in Lw.critic_m:
                assert _rel_to_max(Lu.critic_m[k], Lw.critic_m[k]) > 100 * per.MOMENT_TOL, (step, k)
        if case.get("bc_alpha") and step == 2:
            sq, sb = bcr.term_shares(rec)
            assert sq >= bcr.MIN_SHARE and sb >= bcr.MIN_SHARE, (sq, sb)


@pytest.mark.parametrize("name", ["wn", "odd"])
def test_unit_weights_reproduce_the_oracle_step_at_edges(name):
    """As test_unit_weights_reproduce_the_oracle_step, without LayerNorm (weight norm's g / v gradients)
    and at the custom widths."""
    case = {c["name"]: c for c in per.EDGES}[name]
    S = per.edge_setup(case)
    La = orc.Learner(S["actor"], S["critic"], **S["kw"])
    Lb = copy.deepcopy(La)
    for step in (1, 2):
        p, u, noise = per.edge_step(case, S, step)
        batch = S["buf"].gather(per.draw(p, u))
        ra = per.weighted_featured_step(La, batch, noise, np.ones(S["B"], np.float32))
        rb = orc.featured_train_step(Lb, batch, noise)
        for k in ("y", "q1", "q2", "next_action"):
            np.testing.assert_array_equal(ra[k], rb[k])
        assert ra["critic_loss"] == rb["critic_loss"] and ra.get("actor_loss") == rb.get("actor_loss")
        assert ("actor_loss" in ra) == (step == 2)
        for grp in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
            for k, v in getattr(La, grp).items():
                np.testing.assert_array_equal(v, getattr(Lb, grp)[k], err_msg=f"{grp}/{k}")
