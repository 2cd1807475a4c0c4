"""Host side of Ensemble.trajectory_summary (no GPU): the ranks the device is asked for, the 'linear' interpolation on the host and
the argument refusals, which are all raised before the library is called."""
from fractions import Fraction

import numpy as np
import pytest

from vgsim_amd import ensemble
from vgsim_amd.ensemble import _summary_groups, _summary_lerp, _summary_ranks

SIZES = (1, 2, 3, 64, 65, 1000)
QS = (0, 0.025, 0.25, 0.5, 0.975, 1)


def vector(m):
    return np.random.default_rng(1000 + m).integers(0, 2 ** 31, m)


@pytest.mark.parametrize("method", ["lower", "higher"])
@pytest.mark.parametrize("m", SIZES)
def test_ranks_pick_numpys_element(m, method):
    v = vector(m)
    r = _summary_ranks(QS, m, method)
    assert r.dtype == np.int64 and r.shape == (len(QS),) and r.min() >= 0 and r.max() < m
    want = np.quantile(v, QS, method=method)
    assert np.array_equal(np.sort(v)[r], want)
    for q in QS:    # one at a time as well
        assert np.sort(v)[_summary_ranks([q], m, method)[0]] == np.quantile(v, q, method=method)


@pytest.mark.parametrize("m", SIZES)
def test_linear_formula_against_numpy(m):
    """lower + (upper - lower) t is two floating-point operations on whole numbers below 2^31 (exact in float64) and on t, the
    fractional part of q (m - 1), which is formed in numpy's own order: the result is within a few ulp of numpy's, far inside
    rtol 1e-12."""
    v = vector(m)
    s = np.sort(v)
    r = _summary_ranks(QS, m, 'linear')
    Q = len(QS)
    assert r.shape == (2 * Q,) and r.min() >= 0 and r.max() < m
    assert np.all(r[Q:] - r[:Q] >= 0) and np.all(r[Q:] - r[:Q] <= 1)
    got = _summary_lerp(s[r[:Q]], s[r[Q:]], np.asarray(QS, dtype=np.float64), m)
    np.testing.assert_allclose(got, np.quantile(v, QS), rtol=1e-12, atol=0)
    # the ends are the extremes exactly
    assert got[0] == s[0] and got[-1] == s[-1]


def test_lerp_broadcasts_over_columns():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2 ** 31, (37, 4, 3))
    s = np.sort(x, axis=0)
    q = np.asarray([0.1, 0.5, 0.9])
    r = _summary_ranks(q, 37, 'linear')
    got = _summary_lerp(s[r[:3]], s[r[3:]], q.reshape(3, 1, 1), 37)
    np.testing.assert_allclose(got, np.quantile(x, q, axis=0), rtol=1e-12, atol=0)


def test_ranks_of_an_empty_group_are_zero():
    for method, n in (("lower", 3), ("higher", 3), ("linear", 6)):
        assert np.array_equal(_summary_ranks([0.1, 0.5, 0.9], 0, method), np.zeros(n, dtype=np.int64))


def test_groups():
    of = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    g, G = _summary_groups('auto', None, 6, of, 3)
    assert G == 3 and g.dtype == np.int64 and np.array_equal(g, of)
    g, G = _summary_groups('auto', None, 6, None, 1)
    assert G == 1 and np.array_equal(g, np.zeros(6))
    g, G = _summary_groups('auto', [4, 0, 5], 6, of, 3)
    assert G == 3 and np.array_equal(g, [0, -1, -1, -1, 1, 2])
    g, G = _summary_groups(np.array([3, 0, 0, 3, 1, 1]), np.array([True, True, False, True, True, False]), 6, of, 3)
    assert G == 4 and np.array_equal(g, [3, 0, -1, 3, 1, -1])


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def bare_ensemble(R=6, traj_points=5, scenarios=None):
    """An Ensemble as a simulate(traj_points=...) call leaves it, without an engine: any use of the library fails the test."""
    e = ensemble.Ensemble.__new__(ensemble.Ensemble)
    e.R, e.engine = R, _NoLibrary()
    e.scenarios = [object()] * scenarios if scenarios else None
    e.scenario_of = np.arange(R, dtype=np.int32) % scenarios if scenarios else None
    e.traj_shape = (R, traj_points, 3, 2) if traj_points else None
    return e


@pytest.mark.parametrize("kwargs, text", [
    (dict(quantiles=(0.5, 1.5)), "quantiles must lie in"),
    (dict(quantiles=(-0.01,)), "quantiles must lie in"),
    (dict(quantiles=(float("nan"),)), "quantiles must lie in"),
    (dict(by=np.zeros(5, dtype=np.int64)), "one integer group label per replicate"),
    (dict(by=np.zeros((6, 1), dtype=np.int64)), "one integer group label per replicate"),
    (dict(by=np.zeros(6)), "one integer group label per replicate"),
    (dict(by=np.array([0, 1, -1, 0, 1, 0])), "must not be negative"),
    (dict(by=np.array([0, 1, 10 ** 9, 0, 1, 0])), "below the number of replicates"),
    (dict(by=np.array([0, 1, 6, 0, 1, 0])), "below the number of replicates"),
    (dict(by='scenario'), "by must be 'auto'"),
    (dict(method='nearest'), "method must be"),
    (dict(replicates=[0, 6]), "replicate index out of range"),
])
def test_refusals_come_before_the_library(kwargs, text):
    with pytest.raises(ValueError, match=text):
        bare_ensemble(scenarios=2).trajectory_summary(**kwargs)


def test_no_trajectories_is_refused():
    with pytest.raises(ValueError, match="recorded none"):
        bare_ensemble(traj_points=0).trajectory_summary()


def test_variance_from_exact_integers():
    """sumsq beyond 2^64 and sums whose squares cancel all but the last bits: the variance is the correctly rounded quotient."""
    s = ensemble.TrajectorySummary()
    big = 2 ** 31 - 1
    vals = [[big, big, big, big, big - 1], [0, 0, 0, 0, 0], [1, 2, 3, 4, 10]]
    s.count = np.array([5, 0])
    s.sum = np.array([[sum(v) for v in vals], [0, 0, 0]], dtype=np.int64)
    s.sumsq = np.array([[sum(x * x for x in v) for v in vals], [0, 0, 0]], dtype=object)
    assert s.sumsq[0, 0] > 2 ** 64
    got = s.var()
    for ddof in (0, 1):
        exact = [float(Fraction(5 * sum(x * x for x in v) - sum(v) ** 2, 5 * (5 - ddof))) for v in vals]
        assert np.array_equal(s.var(ddof=ddof)[0], exact)
        shifted = [np.var(np.asarray(v, dtype=np.float64) - v[0], ddof=ddof) for v in vals]   # (numpy on shifted values: a few ulp)
        np.testing.assert_allclose(s.var(ddof=ddof)[0], shifted, rtol=1e-13)
    assert np.all(np.isnan(got[1]))
    assert np.all(np.isnan(s.var(ddof=5)))
