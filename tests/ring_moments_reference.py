"""Float64 moments of a ring's state columns, for the dataset normalisation (include/td3.h, "dataset
normalisation"), with exact helpers to judge them by.

``moments`` is the reference the device is held to: per column the mean by ``math.fsum`` (the correctly
rounded sum) and m2 = fsum((x - mean)^2).  ``exact_moments`` is the same in rational arithmetic, rounded
to fp64 once at the end.  ``raw_m2`` is the unsound sum(x^2) - n mean^2 in fp64 and ``chunked_m2`` the
sound structure the header documents (chunks of ``chunk`` rows, per-chunk mean then squared deviations,
Chan's merge in ascending order); the CPU test shows that the bound the GPU test uses separates the two.
``normalise`` is rs_tick's element expression, from the rollout statistics' restatement.
"""
from fractions import Fraction
import math

import numpy as np

from rollout_stats_reference import chan_merge, normalise  # noqa: F401  (normalise: re-exported)

CHUNK = 1024                # rb_state_moments' documented row chunk R


def moments(x):
    """``(count, mean[d], m2[d])`` of fp32 rows ``x`` ([n][d]) in fp64, every sum by ``math.fsum``."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, d = x.shape
    mean = np.array([math.fsum(x[:, c]) / n for c in range(d)])
    m2 = np.array([math.fsum((x[:, c] - mean[c]) ** 2) for c in range(d)])
    return float(n), mean, m2


def exact_moments(col):
    """Mean and m2 of one fp32 column in exact rational arithmetic, each rounded to fp64 once."""
    xs = [Fraction(float(v)) for v in np.asarray(col, np.float32)]
    n = len(xs)
    mean = sum(xs, Fraction(0)) / n
    m2 = sum(((v - mean) ** 2 for v in xs), Fraction(0))
    return float(mean), float(m2)


def raw_m2(col):
    """The unsound form: a running fp64 sum of squares less n mean^2."""
    x = np.asarray(col, np.float32).astype(np.float64)
    s = q = 0.0
    for v in x:
        s += v
        q += v * v
    return q - len(x) * (s / len(x)) ** 2


def chunked_m2(col, chunk=CHUNK):
    """Per-chunk mean, squared deviations about it, the chunks merged by Chan in ascending order."""
    x = np.asarray(col, np.float32).astype(np.float64)
    count, mean, m2 = 0.0, 0.0, 0.0
    for k in range(0, len(x), chunk):
        count, mean, m2 = chan_merge(count, mean, m2, x[k:k + chunk])
    return mean, m2


def cancellation_column(n, seed=0):
    """The column the issue names: 1e3 + 1e-2 N(0, 1) cast to fp32 -- a spread 1e5 below the offset."""
    return (1e3 + 1e-2 * np.random.RandomState(seed).standard_normal(n)).astype(np.float32)


def merged(a, b):
    """Chan's merge of two ``(count, mean, m2)`` triples, rs_tick's expressions."""
    (ca, ma, qa), (cb, mb, qb) = a, b
    delta, tot = mb - ma, ca + cb
    return tot, ma + delta * cb / tot, qa + qb + delta * delta * ca * cb / tot
