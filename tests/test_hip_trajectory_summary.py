"""Summaries across replicates on the GPU (vgx_colsummary.hip): count, min, max, exact sums and order statistics per group of rows
and column.  Everything is integer work, so every comparison below is bit for bit.

First the kernels on raw matrices through vgx_test_column_summary, against numpy on the same matrix, at the smallest shapes at which
they can go wrong: group sizes on each side of the handover from the wavefront form to the workgroup form (64 | 65), of every power
of two the workgroup form pads to (128 .. 16 384) and the documented maximum; column counts around the 64-column transpose tile and
across two column chunks; ties, extremes and the high word of the sum of squares.  Then Ensemble.trajectory_summary on the small
scenario family of tests/test_hip_param_sets.py and on a tau ensemble, against numpy applied to trajectories() of the same call."""
import ctypes as C

import numpy as np
import pytest

import helpers
import models
from test_hip_param_sets import base_sim, scenarios_of

pytestmark = pytest.mark.gpu

MAX_GROUP = 16384
WAVE_MAX = 64       # the wavefront form takes groups up to this size
PADS = [128 << i for i in range(8)]    # 128 .. 16384: what the workgroup form pads a segment to


def reference(x, group_of, G, ranks):
    """numpy and Python integers on the same matrix."""
    x = np.asarray(x)
    R, N = x.shape
    K = np.asarray(ranks).reshape(G, -1).shape[1]
    want = {k: np.zeros((G, N), dtype=np.int64) for k in ("sum", "min", "max")}
    want["count"] = np.zeros(G, dtype=np.int64)
    want["stat"] = np.zeros((G, K, N), dtype=np.int64)
    want["sumsq_int"] = np.zeros((G, N), dtype=object)
    for g in range(G):
        rows = x[np.asarray(group_of) == g].astype(np.int64)
        want["count"][g] = len(rows)
        if len(rows) == 0:
            continue
        s = np.sort(rows, axis=0)
        want["stat"][g] = s[np.asarray(ranks).reshape(G, -1)[g]]
        want["min"][g], want["max"][g] = rows.min(axis=0), rows.max(axis=0)
        o = rows.astype(object)
        want["sum"][g] = o.sum(axis=0)
        want["sumsq_int"][g] = (o * o).sum(axis=0)
    return want


def check(x, group_of, G, ranks, what=""):
    from vgsim_amd import _capi
    got = _capi.column_summary(x, group_of, G, ranks)
    want = reference(x, group_of, G, ranks)
    for k in ("count", "sum", "min", "max", "stat"):
        assert np.array_equal(got[k], want[k]), (what, k)
    sq = got["sumsq"][..., 0].astype(object) + got["sumsq"][..., 1].astype(object) * (1 << 64)
    assert np.array_equal(sq, want["sumsq_int"]), (what, "sumsq")
    return got, want


def spread_ranks(m, K=6):
    """K ranks of a group of m: the ends, the middle, a duplicate."""
    return np.array([0, m - 1, m // 2, m // 2, (m - 1) // 3, min(1, m - 1)][:K], dtype=np.int64)


GROUP_SIZES = sorted({1, 2, 63, WAVE_MAX, WAVE_MAX + 1} | {p + d for p in PADS for d in (-1, 0, 1) if p + d <= MAX_GROUP})


@pytest.mark.parametrize("m", GROUP_SIZES)
def test_group_sizes(m):
    """One group of m rows, three columns of random values over the whole range (and a column of few distinct ones)."""
    rng = np.random.default_rng(m)
    x = rng.integers(0, 2 ** 31, (m, 3))
    x[:, 1] = rng.integers(0, 7, m)
    check(x, np.zeros(m, dtype=np.int64), 1, spread_ranks(m)[None], m)


def test_group_beyond_the_limit_is_refused():
    from vgsim_amd import _capi
    assert _capi.COLSUMMARY_MAX_GROUP == MAX_GROUP
    m = MAX_GROUP + 1
    x = np.zeros((m + 3, 1))
    group_of = np.concatenate([[0, 0, 0], np.ones(m, dtype=np.int64)])
    with pytest.raises(_capi.VgxError, match=r"group 1 has 16385 members; at most 16384") as ei:
        _capi.column_summary(x, group_of, 2, np.zeros((2, 1), dtype=np.int64))
    assert ei.value.code == 1    # VGX_ERR_ARG


@pytest.mark.parametrize("N", [1, 3, 31, 32, 33, 63, 64, 65])
def test_column_counts(N):
    """Around the transpose tile (64 columns), with a wavefront-form and a workgroup-form group side by side and rows left out."""
    rng = np.random.default_rng(N)
    R = 110
    x = rng.integers(0, 2 ** 31, (R, N))
    group_of = np.array([0] * 30 + [-1] * 5 + [1] * 70 + [-1] * 5)
    rng.shuffle(group_of)
    check(x, group_of, 2, np.stack([spread_ranks(30), spread_ranks(70)]), N)


def test_two_column_chunks(monkeypatch):
    """N = 70 is no multiple of the tile; with the scratch bound set to 64 columns the call takes two chunks (64 + 6 columns)."""
    rng = np.random.default_rng(70)
    R, N = 100, 70
    x = rng.integers(0, 1000, (R, N))
    group_of = np.array([0] * 30 + [1] * 70)
    monkeypatch.setenv("VGX_COLSUMMARY_CHUNK_BYTES", str(64 * R * 4))
    got, _ = check(x, group_of, 2, np.stack([spread_ranks(30), spread_ranks(70)]))
    assert got["passes"] == 2
    monkeypatch.delenv("VGX_COLSUMMARY_CHUNK_BYTES")
    got, _ = check(x, group_of, 2, np.stack([spread_ranks(30), spread_ranks(70)]))
    assert got["passes"] == 1


@pytest.mark.parametrize("m", [5, 64, 65, 300])
def test_contents(m):
    """Columns: all equal; strictly descending; heavy ties; random; 2^31 - 1 throughout (the sum of squares passes 2^64)."""
    rng = np.random.default_rng(m)
    big = 2 ** 31 - 1
    x = np.stack([np.full(m, 12345), np.arange(m)[::-1] * 7 + 1, rng.integers(0, 3, m), rng.integers(0, 2 ** 31, m), np.full(m, big)], axis=1)
    ranks = np.arange(m, dtype=np.int64)[None] if m <= 65 else spread_ranks(m)[None]    # small groups: every rank
    got, want = check(x, np.zeros(m, dtype=np.int64), 1, ranks, m)
    assert want["sumsq_int"][0, 4] == m * big * big > 2 ** 64
    assert got["sumsq"][0, 4, 1] != 0
    assert np.array_equal(got["stat"][0, :, 1], np.sort(x[:, 1])[ranks[0]])


@pytest.mark.parametrize("bad", [2.0 ** 31, -1.0, 0.5, float("nan")])
def test_values_outside_the_domain_are_refused(bad):
    from vgsim_amd import _capi
    x = np.zeros((6, 4))
    x[4, 2] = bad
    with pytest.raises(_capi.VgxError, match=r"x\[4\]\[2\] is not a whole number in \[0, 2\^31\)") as ei:
        _capi.column_summary(x, np.zeros(6, dtype=np.int64), 1, np.zeros((1, 1), dtype=np.int64))
    assert ei.value.code == 1


def test_interleaved_groups_an_empty_one_and_rows_left_out():
    """G = 5: sizes 7, 0, 66, 64, 9 interleaved, some rows in no group; ranks 0, m - 1 and duplicates."""
    rng = np.random.default_rng(9)
    sizes = [7, 0, 66, 64, 9]
    group_of = np.concatenate([np.full(n, g) for g, n in enumerate(sizes)] + [np.full(11, -1)])
    rng.shuffle(group_of)
    R, N = len(group_of), 33
    x = rng.integers(0, 50, (R, N))
    ranks = np.stack([np.array([0, max(n - 1, 0), 0, max(n - 1, 0), n // 2, n // 2]) for n in sizes])
    ranks[1] = 10 ** 6    # an empty group's ranks are not read
    from vgsim_amd import _capi
    got = _capi.column_summary(x, group_of, 5, ranks)
    ranks[1] = 0
    want = reference(x, group_of, 5, ranks)
    for k in ("count", "sum", "min", "max", "stat"):
        assert np.array_equal(got[k], want[k]), k
    assert got["count"][1] == 0 and not got["stat"][1].any() and not got["sumsq"][1].any()
    assert np.array_equal(got["stat"][2, 0], got["min"][2]) and np.array_equal(got["stat"][2, 1], got["max"][2])


def test_rank_outside_the_group_is_refused():
    from vgsim_amd import _capi
    with pytest.raises(_capi.VgxError, match=r"rank 4 of group 0 is outside \[0, 4\)"):
        _capi.column_summary(np.zeros((4, 2)), np.zeros(4, dtype=np.int64), 1, np.array([[0, 4]]))


# ---- simulated ensembles ---------------------------------------------------------------------------------------------------------
SEEDS = [1000, 1001, 1002, 1003]
BLOCK, CYCLE = np.repeat(np.arange(4), 4), np.arange(16) % 4
T = 7
WINDOW = (0.0, 3.0)


def run_scenarios(scenario_of):
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    # (sixteen different seeds: in either layout the four replicates of a scenario are four different runs)
    ens = Ensemble(base, 16, seeds=1000 + np.arange(16, dtype=np.int64), scenarios=scenarios_of(base), scenario_of=scenario_of)
    ens.simulate(2000, sample_size=10 ** 9, attempts=20, traj_points=T, traj_window=WINDOW)
    return ens


def numpy_summary(traj, group_of, G, q, method):
    """The route a user had before: the whole block on the host, split by group, numpy per group (None for an empty group)."""
    out = []
    for g in range(G):
        rows = traj[np.asarray(group_of) == g]
        if len(rows) == 0:
            out.append(None)
            continue
        ints = rows.astype(np.int64).astype(object)
        n = len(rows)
        s, sq = ints.sum(axis=0), (ints * ints).sum(axis=0)
        out.append(dict(count=n, sum=s, sumsq=sq, min=rows.min(axis=0), max=rows.max(axis=0), mean=s.astype(np.float64) / n,
                        var=((n * sq - s * s) / (n * n)).astype(np.float64), quantiles=np.quantile(rows, q, axis=0, method=method)))
    return out


def assert_summary(s, traj, group_of, G, q, method):
    want = numpy_summary(traj, group_of, G, q, method)
    assert np.array_equal(s.groups, np.arange(G)) and s.quantiles.shape == (G, len(q)) + traj.shape[1:]
    var = s.var()
    for g in range(G):
        w = want[g]
        assert s.count[g] == w["count"]
        for k in ("sum", "sumsq", "min", "max", "mean"):
            assert np.array_equal(getattr(s, k)[g], w[k]), (g, k)
        assert np.array_equal(var[g], w["var"]), g
        if method == 'linear':
            np.testing.assert_allclose(s.quantiles[g], w["quantiles"], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(s.quantiles[g], w["quantiles"]), (g, method)


Q = (0.0, 0.025, 0.3, 0.5, 0.975, 1.0)


@pytest.mark.parametrize("scenario_of", [BLOCK, CYCLE], ids=["block", "cycle"])
def test_scenario_ensemble_per_scenario(scenario_of):
    ens = run_scenarios(scenario_of)
    traj = ens.trajectories()
    assert traj.shape == (16, T, 3, 2)
    assert any(np.ptp(traj[scenario_of == g], axis=0).max() > 0 for g in range(4))    # the replicates of a scenario do differ
    for method in ("lower", "higher", "linear"):
        s = ens.trajectory_summary(quantiles=Q, method=method)
        assert s.method == method and np.array_equal(s.count, [4, 4, 4, 4])
        assert_summary(s, traj, scenario_of, 4, Q, method)
    assert s.kernel_ms > 0 and s.wall_ms >= s.kernel_ms and s.passes == 1
    assert np.array_equal(ens.trajectories(), traj)    # the summary only reads the block
    # explicit labels (with a label nobody carries) and a subset of the replicates
    labels = np.array([0, 0, 3, 3, 3, 1, 1, 1, 1, 1, 0, 3, 1, 0, 0, 3])
    s = ens.trajectory_summary(quantiles=Q, by=labels, method='lower')
    assert np.array_equal(s.count, [5, 6, 0, 5])
    want = numpy_summary(traj, labels, 4, Q, 'lower')
    for g in (0, 1, 3):
        w = want[g]
        assert np.array_equal(s.quantiles[g], w["quantiles"]) and np.array_equal(s.sum[g], w["sum"]) and np.array_equal(s.mean[g], w["mean"])
    assert np.all(np.isnan(s.quantiles[2])) and np.all(np.isnan(s.mean[2])) and not s.sum[2].any() and not s.max[2].any()
    subset = np.array([15, 0, 1, 2, 5, 6, 9, 10, 12])
    s = ens.trajectory_summary(quantiles=Q, replicates=subset, method='higher')
    left = np.full(16, -1)
    left[subset] = scenario_of[subset]
    assert np.array_equal(s.count, np.bincount(scenario_of[subset], minlength=4)) and s.count.min() > 0
    assert_summary(s, traj, left, 4, Q, 'higher')
    assert np.array_equal(ens.trajectories(), traj)
    ens.close()


def test_tau_ensemble_one_group():
    """A plain (non-scenario) ensemble after simulate_tau(traj_points=5): one group of all replicates."""
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        sim, phases = models.build(Simulator, "tau_a")
        setup, kw = phases[0]
        setup(sim)
        sim.simulate(**kw)
    nt = phases[1][1]["iterations"]
    ens = Ensemble(sim, 6, seeds=np.array([3, 17, 101, 4242, 9, 77], dtype=np.int64))
    t0 = float(ens.model.currentTime)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    t1 = max(float(ens.replicate_state(r).currentTime) for r in range(6))
    assert t1 > t0
    ens.simulate_tau(nt, sample_size=10 ** 12, traj_points=5, traj_window=(t0, t1))
    traj = ens.trajectories()
    assert np.ptp(traj, axis=0).max() > 0
    for method in ("lower", "higher", "linear"):
        s = ens.trajectory_summary(quantiles=Q, method=method)
        assert np.array_equal(s.count, [6])
        assert_summary(s, traj, np.zeros(6, dtype=np.int64), 1, Q, method)
    assert np.array_equal(ens.trajectories(), traj)
    ens.close()


def test_no_trajectories_recorded_and_the_ensemble_stays_usable():
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    ens = Ensemble(base_sim(), 4, seeds=np.array(SEEDS, dtype=np.int64))
    ens.simulate(500, sample_size=10 ** 9, attempts=20)
    with pytest.raises(ValueError, match="recorded none"):
        ens.trajectory_summary()
    # the library says the same in the words of vgx_get_trajectories
    io = _capi.VgxTrajSummaryIO()
    eng = ens.engine
    with pytest.raises(_capi.VgxError, match="vgx_get_trajectory_summary: the last call recorded none"):
        eng._check(eng.lib.vgx_get_trajectory_summary(eng.handle, C.byref(io)))
    with pytest.raises(_capi.VgxError, match="vgx_get_trajectories: the last call recorded none"):
        eng._check(eng.lib.vgx_get_trajectories(eng.handle, np.zeros(1).ctypes.data_as(C.c_void_p), 0))
    ens.simulate(500, sample_size=10 ** 9, attempts=20, traj_points=T, traj_window=WINDOW)
    traj = ens.trajectories()
    s = ens.trajectory_summary(quantiles=(0.5,), method='lower')
    assert_summary(s, traj, np.zeros(4, dtype=np.int64), 1, (0.5,), 'lower')
    ens.close()
