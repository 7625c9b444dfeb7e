"""CPU proofs about tests/query_reference.py, the reference side of tests/test_gpu_query_edges.py:

* the case table reaches every planner decision it claims (recomputed here from the dimensions);
* the 1e-5 tolerance of the GPU suite is attainable: the project's own fp32 oracle lies within a quarter
  of it of ``forward64`` on every case, head and pool row;
* the comparison can fail: every mutation of ``forward64`` that applies to a case moves the action or Q1
  of the first four pool rows by more than 100 tolerances;
* ``forward64`` agrees with the fp32 oracle on the golden configurations (the oracle itself is pinned to
  the reference implementation by tests/test_oracle_golden.py).
"""
import numpy as np
import pytest

import query_reference as qr
from helpers import featured_setup, orc

CASES = qr.CASES
QUARTER = 0.25 * qr.TOL


def _widths(c, net):
    """[K0, N0, N1, N2, nout] of a case's actor / critic."""
    arch = c["actor_arch"] if net == "actor" else c["q_arch"]
    return [c["sd"] if net == "actor" else c["sd"] + c["ad"], *arch, c["ad"] if net == "actor" else 1]


def _small_route(c):
    """The n <= 4 route of a case from its dimensions alone (act.hip build_act's flags): only to check
    that the hand-written table reaches all three routes, never used as an expectation."""
    a, q = _widths(c, "actor"), _widths(c, "q")
    if a[0] > 64 or q[0] > 64:
        return "gemv"
    rides = a[3] <= a[2] and q[3] <= q[2]
    return "act1" if rides else "gemv01"


def test_table_reaches_every_planner_edge():
    kq = {"actor": set(), "q": set()}
    k0, nout, nb, norms, routes, widths = set(), set(), set(), set(), {}, []
    for name, c in CASES.items():
        a, q = _widths(c, "actor"), _widths(c, "q")
        route = _small_route(c)
        routes.setdefault(route, []).append(name)
        norms.add(c["norm"])
        nout.add(a[4])
        for net, w in (("actor", a), ("q", q)):
            k0.add(w[0])
            widths.append(w)
            if route == "act1":
                kq[net].add(8 if w[0] <= 32 else 16)
                nb.add((w[2] + 15) // 16)
        # the literal route of the table names the kernels this route launches
        for which in ("act", "q"):
            lit = qr.expected_route(name, 3, which)
            want = {"act1": "td3::act_kernel<4, ", "gemv01": "td3::gemv01_kernel<4>", "gemv": "mapped,td3::gemv_kernel<4>"}
            assert want[route] in lit, (name, which, lit)
            assert ("gemv01" in lit) == (route == "gemv01") and ("act_kernel" in lit) == (route == "act1")
    assert kq == {"actor": {8, 16}, "q": {8, 16}}
    for name, c in CASES.items():                 # the KQ in the literal is the one the width asks for
        if _small_route(c) == "act1":
            for which, net in (("act", "actor"), ("q", "q")):
                k = 8 if _widths(c, net)[0] <= 32 else 16
                assert qr.expected_route(name, 1, which) == f"args,td3::act_kernel<1, {k}>", (name, which)
    assert {32, 33, 64, 65} <= k0 and 1 in k0 and 2 in k0
    assert 1 in nout and 32 in nout and any(8 < o < 32 for o in nout)
    assert 1 in nb and 32 in nb
    hidden = [w[1:4] for w in widths]
    assert any(h[1] % 16 != 0 for h in hidden)            # a ragged last column group
    assert any(h[2] % 4 != 0 for h in hidden)             # a wave with fewer than 4 live columns
    assert any(h[2] % 4 == 1 for h in hidden)             # ... with one
    assert any(h[2] == h[1] for h in hidden)
    assert any(h[2] > h[1] for h in hidden)
    assert any(x % 4 != 0 for h in hidden for x in h) and any(x % 32 != 0 for h in hidden for x in h)
    assert any(w[0] == 512 for w in widths) and any(h[0] == 512 for h in hidden)
    assert norms == {"layer", None, "weight_normalization"}
    # every route reached by its shapes alone (no TD3_ACT1 in the environment of the GPU suite's part 1)
    assert set(routes) == {"act1", "gemv01", "gemv"}, routes
    assert qr.ROWS_OF_N == {1: 1, 2: 2, 3: 4, 4: 4}
    seeds = [c["seed"] for c in CASES.values()]
    assert len(set(seeds)) == len(seeds)


def test_pool_shape_and_range():
    for name, c in CASES.items():
        s, a = qr.pool(name)
        assert s.shape == (257, c["sd"]) and a.shape == (257, c["ad"])
        assert s.dtype == a.dtype == np.float32
        assert np.abs(a).max() <= c["ma"]
        s2, a2 = qr.pool(name)
        np.testing.assert_array_equal(s, s2)
        np.testing.assert_array_equal(a, a2)


def _oracle(name):
    c = CASES[name]
    a0, c0 = qr.params(name)
    s, a = qr.pool(name)
    return {"action": orc.featured_actor(a0, c["norm"], c["ma"], s)[0],
            "q1": orc.featured_q(c0, "q1", c["norm"], s, a)[0][:, 0],
            "q2": orc.featured_q(c0, "q2", c["norm"], s, a)[0][:, 0]}


@pytest.mark.parametrize("name", list(CASES))
def test_tolerance_is_attainable(name):
    """The fp32 oracle within 1/4 of the GPU suite's tolerance of forward64, whole pool, every head."""
    got, ref = _oracle(name), qr.reference(name)
    for head in qr.HEADS:
        err = np.abs(got[head].astype(np.float64) - ref[head]).max() / qr.scale(name, head)
        print(f"{name} {head}: oracle vs forward64 {err:.2e} of scale")
        assert err <= QUARTER, (name, head, err)


@pytest.mark.parametrize("name", list(CASES))
def test_mutations_show(name):
    """Every applicable mutation moves the action or Q1 of the first four pool rows by > 100 tolerances
    (a condition on the case's pool seed: a dropped column that is ReLU-dead on those rows shows nothing)."""
    c = CASES[name]
    a0, c0 = qr.params(name)
    s, a = (x[:4] for x in qr.pool(name))
    ref = qr.reference(name)
    tried = 0
    for mut in qr.MUTATIONS:
        moved = []
        if qr.applies(name, mut, "actor"):
            moved.append(np.abs(qr.actor64(a0, c["norm"], c["ma"], s, mut) - ref["action"][:4]).max() / qr.scale(name, "action"))
        if qr.applies(name, mut, "q"):
            moved.append(np.abs(qr.q64(c0, "q1", c["norm"], s, a, mut) - ref["q1"][:4]).max() / qr.scale(name, "q1"))
        if not moved:
            continue
        tried += 1
        print(f"{name} {mut}: moves {max(moved):.2e} of scale")
        assert max(moved) > 100 * qr.TOL, (name, mut, moved)
    # (b) x 3, (d), (e) always apply; (a) wherever a LayerNorm runs over a width that is no multiple of 32
    assert tried >= 5
    if c["norm"] == "layer" and any(w % 32 for w in c["actor_arch"] + c["q_arch"]):
        assert tried >= 6
    assert qr.applies(name, "c", "actor") == (c["ad"] > 8)


def test_mutations_are_mutations():
    """Unmutated, forward64 is itself; row 0 is never moved by the row-0 mutation."""
    a0, _ = qr.params("a17")
    s, _ = qr.pool("a17")
    np.testing.assert_array_equal(qr.forward64(a0, "", "layer", s[:4]), qr.forward64(a0, "", "layer", s[:4], None))
    np.testing.assert_array_equal(qr.forward64(a0, "", "layer", s[:4], "d")[0], qr.forward64(a0, "", "layer", s[:4])[0])
    got = qr.forward64(a0, "", "layer", s[:4], "c")
    np.testing.assert_array_equal(got[:, :8], qr.forward64(a0, "", "layer", s[:4])[:, :8])


@pytest.mark.parametrize("name", ["hc_layer", "hc_none", "hc_wn", "pend_layer"])
def test_forward64_agrees_with_oracle_on_golden_configs(name):
    S = featured_setup(name)
    rs = np.random.RandomState(77)
    s = rs.standard_normal((257, S["sd"])).astype(np.float32)
    a = rs.uniform(-S["ma"], S["ma"], (257, S["ad"])).astype(np.float32)
    pairs = [(orc.featured_actor(S["actor"], S["norm"], S["ma"], s)[0], qr.actor64(S["actor"], S["norm"], S["ma"], s))]
    for q in ("q1", "q2"):
        pairs.append((orc.featured_q(S["critic"], q, S["norm"], s, a)[0][:, 0], qr.q64(S["critic"], q, S["norm"], s, a)))
    for got, ref in pairs:
        assert np.abs(got.astype(np.float64) - ref).max() <= QUARTER * np.abs(ref).max()
