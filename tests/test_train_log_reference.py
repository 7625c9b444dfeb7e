"""The numpy restatement of a training-log entry (tests/train_log_reference.py) against plain numpy, and
its fixed summation order pinned on a case where the order changes the fp64 result."""
import numpy as np
import pytest

import train_log_reference as ref


def _case(B, nq, twin, seed):
    rs = np.random.RandomState(seed)
    y = (3.0 * rs.standard_normal((B, nq))).astype(np.float32)
    q1 = (y + rs.standard_normal((B, nq))).astype(np.float32)
    q2 = (y + rs.standard_normal((B, nq))).astype(np.float32) if twin else None
    J = 2 if twin else 1
    sq = (rs.standard_normal((J, B)) ** 2).astype(np.float32)
    aq = rs.standard_normal((B, nq)).astype(np.float32)
    w = rs.uniform(0.05, 1.0, B).astype(np.float32)
    return y, q1, q2, sq, aq, w


@pytest.mark.parametrize("twin", [True, False])
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_restatement_equals_plain_numpy(B, nq, twin):
    y, q1, q2, sq, aq, w = _case(B, nq, twin, 1000 * B + 10 * nq + twin)
    e = ref.entry(y, q1, q2, sq, aq, w)
    d = lambda a: np.asarray(a, np.float64)                              # noqa: E731
    qb = d(q2) if twin else d(q1)
    J, n = (2 if twin else 1), B * nq
    t = (np.abs(d(q1) - d(y)).sum(axis=1) + (np.abs(qb - d(y)).sum(axis=1) if twin else 0.0)) / (J * nq)
    want = {"critic_loss": d(sq).sum() / n, "actor_loss": -d(aq).mean(), "q1_mean": d(q1).mean(),
            "q2_mean": qb.mean(), "y_mean": d(y).mean(), "q_min": min(d(q1).min(), qb.min()),
            "q_max": max(d(q1).max(), qb.max()), "y_min": d(y).min(), "y_max": d(y).max(),
            "q_gap_mean": np.abs(d(q1) - qb).mean(), "td_abs_mean": t.mean(), "td_abs_max": t.max(),
            "w_mean": d(w).mean(), "w_min": d(w).min()}
    assert set(want) == set(ref.FIELDS)
    for k, v in want.items():
        np.testing.assert_allclose(e[k], v, rtol=1e-12, atol=0, err_msg=k)
    for k in ("q_min", "q_max", "y_min", "y_max", "w_min"):
        assert e[k] == want[k], k                                       # an extremum is one of the values
    assert e["nonfinite"] == 0
    if not twin:
        assert e["q2_mean"] == e["q1_mean"] and e["q_gap_mean"] == 0.0


def test_optional_inputs():
    y, q1, q2, sq, aq, w = _case(37, 3, True, 5)
    e = ref.entry(y, q1, q2, sq)
    assert np.isnan(e["actor_loss"]) and e["w_mean"] == 1.0 and e["w_min"] == 1.0
    assert "critic_loss" not in ref.entry(y, q1, q2)


def test_featured_td_abs_is_half_the_two_errors():
    y, q1, q2, *_ = _case(100, 1, True, 6)
    d = lambda a: np.asarray(a, np.float64).reshape(-1)                  # noqa: E731
    t = 0.5 * (np.abs(d(q1) - d(y)) + np.abs(d(q2) - d(y)))
    e = ref.entry(y, q1, q2)
    assert e["td_abs_max"] == t.max()
    np.testing.assert_allclose(e["td_abs_mean"], t.mean(), rtol=1e-12)


def test_nonfinite_counts_elements_of_y_q1_q2():
    y, q1, q2, *_ = _case(70, 3, True, 7)
    y[3, 1] = np.nan
    q1[69, 2] = np.inf
    q2[0, 0] = -np.inf
    q2[5, 0] = np.nan
    assert ref.entry(y, q1, q2)["nonfinite"] == 4
    assert ref.entry(y, q1, None)["nonfinite"] == 2                      # without a twin there is no Q2


def test_fixed_order_is_pinned():
    """Thread 0 owns elements 0 and 256, thread 1 element 1.  In the fixed order 2^60 and -2^60 cancel
    inside thread 0 before the tree adds thread 1's 1.0; summed left to right the 1.0 is absorbed by
    2^60 (ulp 256) and lost."""
    x = np.zeros((257, 1), np.float32)
    x[0, 0], x[1, 0], x[256, 0] = 2.0 ** 60, 1.0, -2.0 ** 60
    left_to_right = 0.0
    for v in x.reshape(-1).astype(np.float64):
        left_to_right += v
    assert left_to_right == 0.0
    assert ref.fixed_sum(x.astype(np.float64)) == 1.0
    e = ref.entry(x, x, None)
    assert e["y_mean"] == e["q1_mean"] == 1.0 / 257.0
    # and the tree's own order: partials 2^60 in thread 0, 1.0 in thread 1 and -2^60 in thread 128 meet as
    # (2^60 + -2^60) at s = 128 and + 1.0 at s = 1; pairing threads 0 and 1 first would lose the 1.0
    z = np.zeros(256)
    z[0], z[1], z[128] = 2.0 ** 60, 1.0, -2.0 ** 60
    assert ref.fixed_sum(z) == 1.0
    z[128], z[2] = 0.0, -2.0 ** 60                                       # now thread 2 holds it: s = 2 comes before s = 1
    assert ref.fixed_sum(z) == 1.0
    z[2], z[255] = 0.0, -2.0 ** 60                                       # 255 -> 127 -> 63 -> ... -> 1: meets the 1.0 first
    assert ref.fixed_sum(z) == 0.0
