"""Ensemble.susceptibles(): susceptible hosts per grid time, population and class of susceptibility groups of every replicate on
the device (vgx_get_susceptibles).  Expected values come from the chain replicate_events() gives (the route there was before)
through the literal restatement of the rule in test_susceptibles_rule.py, from replicate_state(), from trajectories() and from the
conservation with prevalence(), never from the code under test; every comparison is array_equal on integers.

The shapes are those of test_hip_prevalence.py: the scenario family of test_hip_param_sets.py (16 replicates, 4 scenarios, at most
2000 events, P = 3, two susceptibility groups with immunity loss and migration) with tiles of 64 events, so that chains span many
tiles and intervals change inside tiles, and T = 9."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_timelines import _ensemble
from test_hip_incidence import Q, assert_summary, event_chain
from test_hip_param_sets import ATTEMPTS, BLOCK, N_EVENTS, SEEDS, base_sim, reference, scenarios_of
from test_hip_prevalence import CLOSE, T, WINDOW, grid_of
from test_susceptibles_rule import fold, restate

pytestmark = pytest.mark.gpu

P, S = 3, 2
IDENT = np.arange(S, dtype=np.int64)
ONE = np.array([0, -1], dtype=np.int64)       # group 1 not tracked


@pytest.fixture(scope="module")
def family():
    """The scenario ensemble, run once with trajectories on the grid, and its results; shared and never changed."""
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    ens = Ensemble(base, 16, seeds=np.array(SEEDS * 4, dtype=np.int64), scenarios=scenarios_of(base), scenario_of=BLOCK)
    assert (ens.model.popNum, ens.model.susNum) == (P, S)
    res = ens.simulate(N_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True, traj_points=T, traj_window=WINDOW)
    yield ens, res
    ens.close()


@pytest.fixture
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")


def want_rows(ens, reps, grid, class_of, G):
    got = [restate(*event_chain(ens, int(r)), P, grid, class_of, G, fold(ens.replicate_state(int(r)).initial_susceptible, class_of, G)) for r in reps]
    return [np.stack([g[k] for g in got]) for k in range(3)]


def assert_equals(sv, want, what=""):
    assert sv.values.dtype == np.int32 and sv.final.dtype == np.int32 and sv.values.shape == want[0].shape, what
    assert np.array_equal(sv.values, want[0]), what
    assert np.array_equal(sv.final, want[1]), what
    assert np.array_equal(sv.outside, want[2]), what


def test_every_replicate_equals_the_restatement(oracle_mod, family, tile64):
    ens, res = family
    ref = reference(oracle_mod)
    runs = [ref[g][k].simulation for g in range(4) for k in range(4)]                    # BLOCK: replicate 4 g + k
    assert sum(m.good_attempt > 1 for m in runs) >= 4                                    # restarted replicates
    assert sum(m.good_attempt == 0 and m.events.ptr == 0 for m in runs) >= 2            # ... and some whose every attempt failed
    assert [int(n) for n in res.events] == [m.events.ptr for m in runs] and max(res.events) > 20 * 64
    assert (res.restarts > 0).sum() >= 4 and (res.restarts == 0).sum() >= 4
    kinds = np.concatenate([event_chain(ens, r)[1][0] for r in range(16)])
    assert (kinds == 4).sum() > 10 and (kinds == 5).sum() > 10                           # immunity changes and migrations
    grid = grid_of(T, WINDOW)
    for class_of, G, groups in ((IDENT, S, None), (ONE, 1, ONE)):
        sv = ens.susceptibles(points=T, window=WINDOW, groups=groups)
        assert np.array_equal(sv.times, grid) and np.array_equal(sv.class_of, class_of) and list(sv.replicates) == list(range(16))
        assert sv.values.shape == (16, T, P, G) and sv.final.shape == (16, P, G)
        assert_equals(sv, want_rows(ens, range(16), grid, class_of, G), G)
        for r in range(16):
            assert np.array_equal(sv.final[r], fold(ens.replicate_state(r).susceptible, class_of, G)), (G, r)
        assert len(np.unique(sv.values)) > 10 and sv.outside.any()
    lists = ens.susceptibles(times=grid, groups=[[0]])
    assert np.array_equal(lists.class_of, ONE) and np.array_equal(lists.values, sv.values)
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0


def test_susceptible_plus_infectious_is_the_population(family, tile64):
    """Both calls cut by the same host clock, so nothing is left out: every replicate, every point."""
    ens, _ = family
    grid = grid_of(T, WINDOW)
    sizes = np.asarray(ens.model.sizes, dtype=np.int64)
    sv, pv = ens.susceptibles(times=grid), ens.prevalence(times=grid)
    assert np.array_equal(sv.outside, pv.outside)
    total = sv.values.sum(axis=-1, dtype=np.int64) + pv.values.sum(axis=-1, dtype=np.int64)
    assert np.array_equal(total, np.broadcast_to(sizes, (16, T, P)))
    assert np.array_equal(sv.final.sum(axis=-1, dtype=np.int64) + pv.final.sum(axis=-1, dtype=np.int64), np.broadcast_to(sizes, (16, P)))
    assert pv.values.any() and (sv.values != sv.values[:, :1]).any()
    share = sv.share()
    assert np.allclose(share.sum(axis=-1), 1.0) and share.dtype == np.float64


def test_sum_over_groups_equals_the_trajectories(oracle_mod, family, tile64):
    """The trajectories hold the susceptible totals per population on the same grid, written by the simulating kernel with its own
    clock; susceptibles() cuts by the host clock.  Where no event time lies within 1e-9 of a grid point the two clocks cannot
    disagree on which side of the point an event falls (the exclusions of test_hip_prevalence.py)."""
    ens, res = family
    grid = grid_of(T, WINDOW)

    def clear(t):
        return not len(t) or not (np.abs(t[:, None] - grid[None, :]) <= CLOSE * np.maximum(1.0, np.abs(t))[:, None]).any()
    sv = ens.susceptibles(points=T, window=WINDOW)
    traj = ens.trajectories()
    assert traj.shape == (16, T, P, 2)
    compared = 0
    for r in range(16):
        if res.restarts[r] != 0 or not clear(event_chain(ens, r)[0]):
            continue
        assert np.array_equal(sv.values[r].sum(axis=-1), traj[r, :, :, 1]), r
        compared += 1
    assert compared >= 4


def test_tiles_chunks_and_subsets_give_the_same_rows(family, monkeypatch):
    ens, _ = family
    grid = grid_of(T, WINDOW)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")
    small = ens.susceptibles(times=grid)
    assert small.passes == 1 and len(np.unique(small.values)) > 10
    for tile in ("257", None):
        if tile is None:
            monkeypatch.delenv("VGX_PREVALENCE_TILE_EVENTS")
        else:
            monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", tile)
        assert_equals(ens.susceptibles(times=grid), [small.values, small.final, small.outside], tile)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "20000")
    split = ens.susceptibles(times=grid)
    assert split.passes > 4
    assert_equals(split, [small.values, small.final, small.outside], "chunks")
    order = np.array([11, 2, 7, 14, 0])
    sub = ens.susceptibles(times=grid, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_equals(sub, [small.values[order], small.final[order], small.outside[order]], "subset")
    assert_equals(sub, want_rows(ens, order, grid, IDENT, S), "subset against the restatement")


def test_summary_per_scenario_without_the_block(family, tile64):
    ens, _ = family
    block = ens.susceptibles(points=T, window=WINDOW).values
    assert np.ptp(block[BLOCK == 0], axis=0).max() > 0
    for method in ("linear", "lower"):
        band = ens.susceptibles(points=T, window=WINDOW, summary=dict(quantiles=Q, method=method), values=False)
        assert band.values is None and band.final.shape == (16, P, S) and band.summary.method == method
        assert_summary(band.summary, block, BLOCK, 4, method)
    # a subset in another order: the groups hold the selected replicates only
    reps = np.array([13, 0, 2, 5, 4])
    band = ens.susceptibles(points=T, window=WINDOW, replicates=reps, summary=dict(quantiles=Q, method='lower'))
    assert np.array_equal(band.values, block[reps]) and np.array_equal(band.summary.count, [2, 2, 0, 1])
    assert np.array_equal(band.summary.sum[0], block[[0, 2]].astype(np.int64).sum(axis=0))
    assert np.array_equal(band.summary.max[3], block[13])


def test_a_plain_ensemble_on_the_automatic_kernel(tile64):
    ens, _ = _ensemble("g9_short", 100 + np.arange(6, dtype=np.int64), n_max=2000)
    assert ens.engine.last_kernel != "wave"          # a second producer of the log
    m = ens.model
    t_end = min(float(ens.replicate_state(r).currentTime) for r in range(6))
    grid = grid_of(T, (0.1 * t_end, 0.9 * t_end))
    co = np.arange(m.susNum, dtype=np.int64) % 2
    sv = ens.susceptibles(times=grid, groups=co, summary=dict(quantiles=Q))
    pv = ens.prevalence(times=grid)
    for r in range(6):
        st = ens.replicate_state(r)
        values, final, outside = restate(*event_chain(ens, r), m.popNum, grid, co, 2, fold(st.initial_susceptible, co, 2))
        assert np.array_equal(sv.values[r], values) and np.array_equal(sv.final[r], final) and np.array_equal(sv.outside[r], outside), r
        assert np.array_equal(sv.final[r], fold(st.susceptible, co, 2))
    assert np.array_equal(sv.values.sum(axis=-1, dtype=np.int64) + pv.values.sum(axis=-1, dtype=np.int64),
                          np.broadcast_to(np.asarray(m.sizes, dtype=np.int64), (6, T, m.popNum)))
    assert_summary(sv.summary, sv.values, np.zeros(6, dtype=np.int64), 1, 'linear')
    ens.close()


def test_refusals_leave_the_ensemble_usable(family, tile64):
    from vgsim_amd import _capi
    ens, _ = family
    eng = ens.engine
    grid = grid_of(T, WINDOW)
    i32 = C.POINTER(C.c_int32)

    def library(reps=(0, 1), g=grid, co=IDENT, G=S):
        """vgx_get_susceptibles itself, past the facade's checks"""
        io = _capi.VgxSusceptiblesIO()
        reps = np.asarray(reps, dtype=np.int64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        co = np.ascontiguousarray(co, dtype=np.int32)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        block = np.zeros((len(reps), len(g), P, max(G, 1)), dtype=np.int32)
        io.n, io.replicates, io.T, io.grid, io.G, io.class_of = len(reps), _capi._p(reps), len(g), _capi._p(g), G, co.ctypes.data_as(i32)
        io.values, io.outside = block.ctypes.data_as(i32), _capi._p(outside)
        eng._check(eng.lib.vgx_get_susceptibles(eng.handle, C.byref(io)))
        return block

    prev0 = ens.prevalence(times=grid)
    chains = [ens.replicate_events(r) for r in (0, 9, 15)]
    good = ens.susceptibles(times=grid)
    assert np.array_equal(library(), good.values[:2])
    for kw, text in ((dict(reps=(1, 1)), "vgx_get_susceptibles: replicates must be distinct"),
                     (dict(reps=(0, 16)), "vgx_get_susceptibles: replicate index out of range"),
                     (dict(g=[0.0, 1.0, 1.0]), "vgx_get_susceptibles: grid must increase strictly"),
                     (dict(g=[0.0, float("nan")]), r"vgx_get_susceptibles: grid.1. is not finite"),
                     (dict(g=[]), "vgx_get_susceptibles: T = 0"),
                     (dict(G=0), "vgx_get_susceptibles: G = 0"),
                     (dict(co=[0, 2]), r"vgx_get_susceptibles: class_of\[1\] = 2 is outside \[-1, 2\)"),
                     (dict(co=[-2, 0]), r"vgx_get_susceptibles: class_of\[0\] = -2 is outside"),
                     (dict(co=[0, 6000], G=6001), "vgx_get_susceptibles: 3 populations x 6001 classes need 72012 bytes")):
        with pytest.raises(_capi.VgxError, match=text) as ei:
            library(**kw)
        assert ei.value.code == 1
        assert np.array_equal(ens.susceptibles(times=grid).values, good.values)
    with pytest.raises(ValueError, match="distinct"):
        ens.susceptibles(times=grid, replicates=[1, 1])
    # the other consumers of the log see what they saw before
    prev1 = ens.prevalence(times=grid)
    assert np.array_equal(prev0.values, prev1.values) and np.array_equal(prev0.outside, prev1.outside) and prev0.values.any()
    for r, chain in zip((0, 9, 15), chains):
        assert np.array_equal(ens.replicate_events(r), chain)


def test_the_wrong_last_call_is_refused_by_the_library_too():
    from vgsim_amd import _capi
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)
    eng = ens.engine
    grid = np.array([0.0, 0.5, 1.0])
    ens.susceptibles(times=grid)

    def library():
        io = _capi.VgxSusceptiblesIO()
        reps, co = np.arange(2, dtype=np.int64), np.zeros(ens.model.susNum, dtype=np.int32)
        outside = np.zeros((2, 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.grid, io.G, io.class_of = 2, _capi._p(reps), 3, _capi._p(grid), 1, co.ctypes.data_as(C.POINTER(C.c_int32))
        io.outside = _capi._p(outside)
        eng._check(eng.lib.vgx_get_susceptibles(eng.handle, C.byref(io)))

    library()
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"susceptibles\(\).*record_events"):
        ens.susceptibles(times=grid)
    with pytest.raises(_capi.VgxError, match="vgx_get_susceptibles: the last call did not record events"):
        library()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"^susceptibles\(\).*direct chains only"):
        ens.susceptibles(times=grid)
    with pytest.raises(_capi.VgxError, match="vgx_get_susceptibles: the last call was vgx_simulate_tau"):
        library()
    ens.close()
