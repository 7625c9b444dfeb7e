"""The float64 reference of the dataset normalisation (tests/ring_moments_reference.py) against exact
rational arithmetic, and the teeth of the cancellation case: on a column 1e3 + 1e-2 N(0, 1) a raw fp64
sum of squares is 1e-6 .. 1e-4 (relative) off in m2 (measured 8.5e-6, 4.4e-5, 9.2e-5 at n = 1000, 2049,
5000), the chunked two-pass with Chan's merge at most 1.1e-13 (4e-16, 0, 1.0e-13): what it has left is the
rounding of the chunk means, 2^-53 * 1e3 = 1.1e-13 absolute, in the between-chunk term of the merge.  So
the GPU test's bound of 1e-9 passes the sound algorithm by three to four orders and fails the unsound one
by three or more.  No GPU."""
import numpy as np
import pytest

import ring_moments_reference as ref

M2_BOUND = 1e-9             # tests/test_gpu_ring_norm.py holds the device to this


@pytest.mark.parametrize("n", [1, 7, 1000, 2049])
def test_reference_against_exact_arithmetic(n):
    rs = np.random.RandomState(n)
    x = np.stack([rs.uniform(-5, 5, n), ref.cancellation_column(n, seed=n), rs.standard_normal(n) * 1e-3], axis=1)
    x = x.astype(np.float32)
    count, mean, m2 = ref.moments(x)
    assert count == n
    for c in range(x.shape[1]):
        em, eq = ref.exact_moments(x[:, c])
        assert abs(mean[c] - em) <= 2 * np.spacing(abs(em))
        assert abs(m2[c] - eq) <= 1e-13 * eq + 1e-300


@pytest.mark.parametrize("n", [1000, 2049, 5000])
def test_cancellation_column_separates_the_two_algorithms(n):
    col = ref.cancellation_column(n)
    _, exact = ref.exact_moments(col)
    raw = abs(ref.raw_m2(col) - exact) / exact
    _, q = ref.chunked_m2(col)
    sound = abs(q - exact) / exact
    print(f"n = {n}: raw sum of squares {raw:.2e}, chunked two-pass + Chan {sound:.2e} (relative, m2)")
    assert raw >= 1e3 * M2_BOUND, "the unsound algorithm would pass the GPU bound: the case has no teeth"
    assert sound <= 1e-3 * M2_BOUND


def test_merged_equals_the_moments_of_the_concatenation():
    rs = np.random.RandomState(5)
    a = rs.uniform(-3, 3, (700, 4)).astype(np.float32) + 2.0
    b = rs.uniform(-3, 3, (1300, 4)).astype(np.float32) - 1.0
    tot, mean, m2 = ref.merged(ref.moments(a), ref.moments(b))
    n, em, eq = ref.moments(np.concatenate([a, b]))
    assert tot == n
    np.testing.assert_allclose(mean, em, rtol=0, atol=1e-14)
    np.testing.assert_allclose(m2, eq, rtol=1e-13)


def test_normalise_is_the_rollout_statistics_expression():
    from rollout_stats_reference import normalise
    assert ref.normalise is normalise
