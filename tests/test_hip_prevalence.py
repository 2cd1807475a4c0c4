"""Ensemble.prevalence(): infectious hosts per grid time, population and variant class of every replicate on the device
(vgx_get_prevalence).  Expected values come from the chain replicate_events() gives (the route there was before) through the
literal restatement of the rule in test_prevalence_rule.py, from replicate_state() and from trajectories(), never from the code
under test; every comparison is array_equal on integers.

The shapes are the smallest at which the kernels can still go wrong: the scenario family of test_hip_param_sets.py (16
replicates, 4 scenarios, at most 2000 events, P = 3, H = 16) with tiles of 64 events, so that chains span many tiles and
intervals change inside tiles, and T = 9."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_timelines import _ensemble
from test_hip_incidence import event_chain
from test_hip_param_sets import ATTEMPTS, BLOCK, N_EVENTS, SEEDS, base_sim, reference, scenarios_of
from test_prevalence_rule import fold, restate

pytestmark = pytest.mark.gpu

T = 9
WINDOW = (0.5, 8.5)           # grid 0.5, 1.5, .. 8.5: inside every chain that is compared with the trajectories (they end after t = 15)
P, H = 3, 16
THREE = np.arange(H, dtype=np.int64) % 3
THREE[5] = -1                 # three classes, haplotype 5 not tracked
IDENT = np.arange(H, dtype=np.int64)
CLOSE = 1e-9


def grid_of(points, window):
    t0, t1 = window
    dt = (t1 - t0) / (points - 1)
    return np.array([t0 + j * dt for j in range(points)], dtype=np.float64)


@pytest.fixture(scope="module")
def family():
    """The scenario ensemble, run once with trajectories on the grid, and its results; shared and never changed."""
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    ens = Ensemble(base, 16, seeds=np.array(SEEDS * 4, dtype=np.int64), scenarios=scenarios_of(base), scenario_of=BLOCK)
    res = ens.simulate(N_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True, traj_points=T, traj_window=WINDOW)
    yield ens, res
    ens.close()


@pytest.fixture
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")


def start_of(ens, r):
    """The start of replicate r's chain: the index case in (0, 0), for a first attempt and for a restart alike in this family."""
    start = np.zeros((P, H), dtype=np.int64)
    start[0, 0] = 1
    assert np.array_equal(ens.replicate_state(r).initial_infectious, start)
    return start


def want_rows(ens, reps, grid, variant_of, V):
    got = [restate(*event_chain(ens, int(r)), P, grid, variant_of, V, fold(start_of(ens, int(r)), variant_of, V)) for r in reps]
    return [np.stack([g[k] for g in got]) for k in range(3)]


def assert_equals(pv, want, what=""):
    assert pv.values.dtype == np.int32 and pv.final.dtype == np.int32 and pv.values.shape == want[0].shape, what
    assert np.array_equal(pv.values, want[0]), what
    assert np.array_equal(pv.final, want[1]), what
    assert np.array_equal(pv.outside, want[2]), what


def test_every_replicate_equals_the_restatement(oracle_mod, family, tile64):
    ens, res = family
    ref = reference(oracle_mod)
    runs = [ref[g][k].simulation for g in range(4) for k in range(4)]                    # BLOCK: replicate 4 g + k
    assert sum(m.good_attempt > 1 for m in runs) >= 4                                    # restarted replicates
    assert sum(m.good_attempt == 0 and m.events.ptr == 0 for m in runs) >= 2            # ... and some whose every attempt failed
    assert [int(n) for n in res.events] == [m.events.ptr for m in runs] and max(res.events) > 20 * 64
    assert (res.restarts > 0).sum() >= 4 and (res.restarts == 0).sum() >= 4
    grid = grid_of(T, WINDOW)
    for variant_of, V, variants in ((IDENT, H, None), (THREE, 3, THREE)):
        pv = ens.prevalence(points=T, window=WINDOW, variants=variants)
        assert np.array_equal(pv.times, grid) and np.array_equal(pv.variant_of, variant_of) and list(pv.replicates) == list(range(16))
        assert pv.values.shape == (16, T, P, V) and pv.final.shape == (16, P, V)
        assert_equals(pv, want_rows(ens, range(16), grid, variant_of, V), V)
        for r in range(16):
            assert np.array_equal(pv.final[r], fold(ens.replicate_state(r).infectious, variant_of, V)), (V, r)
        assert len(np.unique(pv.values)) > 10 and pv.outside.any()
        total = pv.values.sum(axis=-1, keepdims=True)
        assert (total == 0).any() and np.array_equal(pv.share(), pv.values / np.where(total == 0, 1, total))
    lists = ens.prevalence(times=grid, variants=[[h for h in range(H) if THREE[h] == k] for k in range(3)])
    assert np.array_equal(lists.variant_of, THREE) and np.array_equal(lists.values, pv.values)
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0


def test_sum_over_classes_equals_the_trajectories(oracle_mod, family, tile64):
    """The trajectories hold the totals per population on the same grid, written by the simulating kernel with its own clock;
    prevalence cuts by the host clock.  Where no event time lies within 1e-9 of a grid point the two clocks cannot disagree
    on which side of the point an event falls."""
    ens, res = family
    grid = grid_of(T, WINDOW)

    def clear(t):
        return not len(t) or not (np.abs(t[:, None] - grid[None, :]) <= CLOSE * np.maximum(1.0, np.abs(t))[:, None]).any()
    ref = reference(oracle_mod)
    runs = [ref[g][k].simulation for g in range(4) for k in range(4)]
    assert sum(m.good_attempt == 1 and clear(m.events.times[:m.events.ptr]) for m in runs) >= 4
    pv = ens.prevalence(points=T, window=WINDOW)
    traj = ens.trajectories()
    assert traj.shape == (16, T, P, 2)
    compared = 0
    for r in range(16):
        if res.restarts[r] != 0 or not clear(event_chain(ens, r)[0]):
            continue
        assert np.array_equal(pv.values[r].sum(axis=-1), traj[r, :, :, 0]), r
        assert traj[r, :, :, 0].max() > 1
        compared += 1
    assert compared >= 4


def test_tiles_chunks_and_subsets_give_the_same_rows(family, monkeypatch):
    ens, _ = family
    grid = grid_of(T, WINDOW)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")
    small = ens.prevalence(times=grid, variants=THREE)
    assert small.passes == 1 and len(np.unique(small.values)) > 10
    for tile in ("257", None):
        if tile is None:
            monkeypatch.delenv("VGX_PREVALENCE_TILE_EVENTS")
        else:
            monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", tile)
        assert_equals(ens.prevalence(times=grid, variants=THREE), [small.values, small.final, small.outside], tile)
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "20000")
    split = ens.prevalence(times=grid, variants=THREE)
    assert split.passes > 4
    assert_equals(split, [small.values, small.final, small.outside], "chunks")
    order = np.array([11, 2, 7, 14, 0])
    sub = ens.prevalence(times=grid, variants=THREE, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_equals(sub, [small.values[order], small.final[order], small.outside[order]], "subset")
    assert_equals(sub, want_rows(ens, order, grid, THREE, 3), "subset against the restatement")


Q = (0.025, 0.5, 0.975)


def test_summary_per_scenario_without_the_block(family, tile64):
    from vgsim_amd.ensemble import _summary_lerp, _summary_ranks
    ens, _ = family
    band = ens.prevalence(points=T, window=WINDOW, variants=THREE, summary=dict(quantiles=Q), values=False)
    block = ens.prevalence(points=T, window=WINDOW, variants=THREE).values
    assert band.values is None and band.final.shape == (16, P, 3)
    s = band.summary
    assert s.quantiles.shape == (4, len(Q), T, P, 3) and s.method == 'linear'
    rk = _summary_ranks(Q, 4, 'linear')                # the two neighbours of every quantile's fractional index
    for g in range(4):
        rows = block[BLOCK == g].astype(np.int64)
        srt = np.sort(rows, axis=0)
        assert s.count[g] == 4
        assert np.array_equal(s.sum[g], rows.sum(axis=0)) and np.array_equal(s.min[g], rows.min(axis=0)) and np.array_equal(s.max[g], rows.max(axis=0))
        assert np.array_equal(s.sumsq[g], (rows.astype(object) ** 2).sum(axis=0))
        assert np.array_equal(s.quantiles[g], _summary_lerp(srt[rk[:len(Q)]], srt[rk[len(Q):]], np.asarray(Q).reshape(len(Q), 1, 1, 1), 4))
    assert np.ptp(block[BLOCK == 0], axis=0).max() > 0
    # a subset in another order: the groups hold the selected replicates only
    reps = np.array([13, 0, 2, 5, 4])
    band = ens.prevalence(points=T, window=WINDOW, variants=THREE, replicates=reps, summary=dict(quantiles=Q, method='lower'))
    assert np.array_equal(band.values, block[reps]) and np.array_equal(band.summary.count, [2, 2, 0, 1])
    assert np.array_equal(band.summary.sum[0], block[[0, 2]].astype(np.int64).sum(axis=0))
    assert np.array_equal(band.summary.max[3], block[13])


def test_a_plain_ensemble_on_the_automatic_kernel(tile64):
    ens, _ = _ensemble("g9_short", 100 + np.arange(6, dtype=np.int64), n_max=2000)
    assert ens.engine.last_kernel != "wave"          # a second producer of the log
    m = ens.model
    t_end = min(float(ens.replicate_state(r).currentTime) for r in range(6))
    grid = grid_of(T, (0.1 * t_end, 0.9 * t_end))
    vo = np.arange(m.hapNum, dtype=np.int64) % 3
    pv = ens.prevalence(times=grid, variants=vo, summary=dict(quantiles=Q))
    for r in range(6):
        st = ens.replicate_state(r)
        start = st.infectious * 0
        start[0, 0] = 1
        assert np.array_equal(st.initial_infectious, start)
        values, final, outside = restate(*event_chain(ens, r), m.popNum, grid, vo, 3, fold(start, vo, 3))
        assert np.array_equal(pv.values[r], values) and np.array_equal(pv.final[r], final) and np.array_equal(pv.outside[r], outside), r
        assert np.array_equal(pv.final[r], fold(st.infectious, vo, 3))
    assert np.array_equal(pv.summary.count, [6]) and np.array_equal(pv.summary.sum[0], pv.values.astype(np.int64).sum(axis=0))
    assert pv.values.max() > 10
    ens.close()


def test_refusals_leave_the_ensemble_usable(family, tile64):
    from vgsim_amd import _capi
    ens, _ = family
    eng = ens.engine
    grid = grid_of(T, WINDOW)
    i32 = C.POINTER(C.c_int32)

    def library(reps=(0, 1), g=grid, vo=THREE, V=3):
        """vgx_get_prevalence itself, past the facade's checks"""
        io = _capi.VgxPrevalenceIO()
        reps = np.asarray(reps, dtype=np.int64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        vo = np.ascontiguousarray(vo, dtype=np.int32)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        block = np.zeros((len(reps), len(g), P, max(V, 1)), dtype=np.int32)
        io.n, io.replicates, io.T, io.grid, io.V, io.variant_of = len(reps), _capi._p(reps), len(g), _capi._p(g), V, vo.ctypes.data_as(i32)
        io.values, io.outside = block.ctypes.data_as(i32), _capi._p(outside)
        eng._check(eng.lib.vgx_get_prevalence(eng.handle, C.byref(io)))
        return block

    inc0 = ens.incidence(bins=T, window=WINDOW)
    chains = [ens.replicate_events(r) for r in (0, 9, 15)]
    good = ens.prevalence(times=grid, variants=THREE)
    assert np.array_equal(library(), good.values[:2])
    wide = np.arange(H) * 400                                   # 3 x 6001 classes: 72012 bytes
    for kw, text in ((dict(reps=(1, 1)), "vgx_get_prevalence: replicates must be distinct"),
                     (dict(reps=(0, 16)), "vgx_get_prevalence: replicate index out of range"),
                     (dict(g=[0.0, 1.0, 1.0]), "vgx_get_prevalence: grid must increase strictly"),
                     (dict(g=[0.0, float("nan")]), r"vgx_get_prevalence: grid.1. is not finite"),
                     (dict(g=[]), "vgx_get_prevalence: T = 0"),
                     (dict(V=0), "vgx_get_prevalence: V = 0"),
                     (dict(vo=np.where(THREE == 2, 3, THREE)), r"vgx_get_prevalence: variant_of\[2\] = 3 is outside \[-1, 3\)"),
                     (dict(vo=np.where(THREE == 2, -2, THREE)), r"vgx_get_prevalence: variant_of\[2\] = -2 is outside"),
                     (dict(vo=wide, V=6001), "vgx_get_prevalence: 3 populations x 6001 classes need 72012 bytes")):
        with pytest.raises(_capi.VgxError, match=text) as ei:
            library(**kw)
        assert ei.value.code == 1
        assert np.array_equal(ens.prevalence(times=grid, variants=THREE).values, good.values)
    with pytest.raises(ValueError, match="distinct"):
        ens.prevalence(times=grid, replicates=[1, 1])
    # the other consumers of the log see what they saw before
    inc1 = ens.incidence(bins=T, window=WINDOW)
    assert np.array_equal(inc0.counts, inc1.counts) and np.array_equal(inc0.outside, inc1.outside) and inc0.counts.any()
    for r, chain in zip((0, 9, 15), chains):
        assert np.array_equal(ens.replicate_events(r), chain)


def test_the_wrong_last_call_is_refused_by_the_library_too():
    from vgsim_amd import _capi
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)
    eng = ens.engine
    grid = np.array([0.0, 0.5, 1.0])
    good = ens.prevalence(times=grid)

    def library():
        io = _capi.VgxPrevalenceIO()
        reps, vo = np.arange(2, dtype=np.int64), np.zeros(ens.model.hapNum, dtype=np.int32)
        outside = np.zeros((2, 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.grid, io.V, io.variant_of = 2, _capi._p(reps), 3, _capi._p(grid), 1, vo.ctypes.data_as(C.POINTER(C.c_int32))
        io.outside = _capi._p(outside)
        eng._check(eng.lib.vgx_get_prevalence(eng.handle, C.byref(io)))

    library()
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"prevalence\(\).*record_events"):
        ens.prevalence(times=grid)
    with pytest.raises(_capi.VgxError, match="vgx_get_prevalence: the last call did not record events"):
        library()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"prevalence\(\).*direct chains only"):
        ens.prevalence(times=grid)
    with pytest.raises(_capi.VgxError, match="vgx_get_prevalence: the last call was vgx_simulate_tau"):
        library()
    ens.close()
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)   # ... and a fresh direct call counts again
    again = ens.prevalence(times=grid)
    assert np.array_equal(again.values, good.values) and np.array_equal(again.final, good.final)
    ens.close()
