"""Ensemble.tau_susceptibles(): susceptible hosts per grid time, population and class of susceptibility groups of every replicate
of a tau ensemble on the device (vgx_get_tau_susceptibles), on both tau paths.  As in test_hip_tau_prevalence.py the expected
blocks are the literal restatement of the rule (test_tau_susceptibles_rule.restate_weighted) over the chain the engine itself
recorded, assembled from read-outs that exist without this feature.  Three checks need no restatement: `final` against
replicate_states_tau(), the sum over the groups against the tau trajectories binned by the step kernels themselves, and the
conservation with tau_prevalence().  Every comparison is array_equal on integers.

Net changes and values beyond 2^32 in one cell are covered by the CPU hook test (tests/test_tau_susceptibles_rule.py)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_tau_timelines import SEEDS
from test_hip_incidence import Q, assert_summary
from test_hip_tau_prevalence import BIG, POINTS, _ensemble, chains_of, final_times
from test_hip_tau_trajectories import PATHS, warm
from test_susceptibles_rule import fold
from test_tau_susceptibles_rule import maps_of, restate_weighted

pytestmark = pytest.mark.gpu


def start_of(ens, host, co, G):
    """The susceptible state the chain starts from: the initial state when it starts at the beginning of the model's history (a
    restart, or a model that held events before the call), else the state the call started from."""
    from_initial = host.restarted or ens.model.events.ptr > 0 or not ens.model.first_simulation
    return fold(host.initial_susceptible if from_initial else ens.model.susceptible, co, G)


def want_block(ens, chains, reps, grid, co, G):
    got = []
    for r in reps:
        host, mev, events, rows = chains[int(r)]
        got.append(restate_weighted(events, mev, ens.model.popNum, grid, co, G, start_of(ens, host, co, G), rows))
    return tuple(np.stack([g[k] for g in got]) for k in range(3))


def assert_equals(sv, values, final, outside, what=""):
    assert sv.values.dtype == np.int64 and sv.values.shape == values.shape and sv.final.dtype == np.int64, what
    assert np.array_equal(sv.values, values), what
    assert np.array_equal(sv.final, final), what
    assert sv.outside.dtype == np.int64 and np.array_equal(sv.outside, outside), what


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_b", "tau_c"])
def test_warm_up_cases_equal_the_restatement(name, path, monkeypatch):
    """A tau call that continues a direct warm-up: prefix rows and own rows lie before, between and behind the grid's points;
    tiles of 64 rows, so that a chain spans several tiles and intervals change inside a tile."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    m = ens.model
    assert m.events.ptr > 0 and m.susNum == {"tau_b": 2, "tau_c": 3}[name]
    t_pre = float(m.events.times[m.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    chains = chains_of(ens)
    assert all(c[0].own_steps > 1 and not c[0].restarted for c in chains.values())
    final_sus = ens.replicate_states_tau()[1]
    for k, (co, G) in enumerate(maps_of(m.susNum)):
        for points in POINTS:
            sv = ens.tau_susceptibles(points=points, window=window, groups=None if k == 0 else co)
            assert_equals(sv, *want_block(ens, chains, range(6), sv.times, co, G), what=(name, path, points, G))
            assert sv.outside.any() and sv.passes == 2 and np.array_equal(sv.class_of, co)
            assert k != 0 or (sv.values.any() and np.array_equal(sv.final, final_sus))
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["fresh", "warm", "restarted"])
def test_final_state_conservation_and_trajectories(kind, path, monkeypatch):
    """Independent of the restatement: with every group tracked the running sum over the whole chain ends in the susceptible
    state the engine holds; added to tau_prevalence() on the same grid the total per population is its size; and over a window
    behind the prefix the sum over the groups is the susceptible total the tau kernels binned themselves, at every point of every
    replicate, restarted ones included."""
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, res, call = _ensemble(kind)
    states = ens.replicate_states_tau()
    sizes = np.asarray(ens.model.sizes, dtype=np.int64)
    t_end = float(states[3].max())
    for times in ([0.5 * t_end], [-1.0], [t_end + 1.0], np.linspace(0.1 * t_end, 0.9 * t_end, 12)):
        sv, pv = ens.tau_susceptibles(times=times), ens.tau_prevalence(times=times)
        assert np.array_equal(sv.final, states[1]), (kind, path, len(times))
        assert np.array_equal(sv.outside, pv.outside)
        assert np.array_equal(sv.values.sum(axis=-1) + pv.values.sum(axis=-1), np.broadcast_to(sizes, sv.values.shape[:3]))
        assert np.array_equal(sv.final.sum(axis=-1) + pv.final.sum(axis=-1), np.broadcast_to(sizes, sv.final.shape[:2]))
    assert not np.array_equal(sv.values[:, 0], sv.values[:, -1])
    behind = ens.tau_susceptibles(times=[t_end + 1.0])
    assert np.array_equal(behind.values[:, 0], states[1]) and not behind.outside[:, 1].any()
    if kind != "fresh":
        t_start, t_last = float(ens.model.currentTime), float(final_times(ens).max())
        assert ens.model.events.ptr > 0 and float(ens.model.events.times[ens.model.events.ptr - 1]) <= t_start < t_last
        window = (t_start + 0.05 * (t_last - t_start), t_last - 0.05 * (t_last - t_start))
        for T in (33, 1):
            again = ens.simulate_tau(traj_points=T, traj_window=window, **call)
            assert np.array_equal(again.events, res.events) and np.array_equal(again.restarts, res.restarts)
            traj = ens.trajectories()
            sv = ens.tau_susceptibles(points=T, window=window)
            assert traj.shape == (ens.R, T, ens.model.popNum, 2) and sv.values.shape[:3] == traj.shape[:3]
            assert np.array_equal(sv.values.sum(axis=-1), traj[..., 1])
            assert T == 1 or any(not np.array_equal(traj[r, 0, :, 1], traj[r, -1, :, 1]) for r in range(ens.R))
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_restarted_replicates_have_no_prefix(path, monkeypatch):
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, res, _ = _ensemble("restarted")
    chains = chains_of(ens)
    m = ens.model
    t_pre = float(m.events.times[int(m.events.ptr) - 1])
    grid = np.array([0.5 * t_pre, np.nextafter(t_pre, np.inf), 2.0 * t_pre + 1.0, 0.9 * float(final_times(ens).max()) + 2.0 * t_pre + 2.0])
    co = np.arange(m.susNum)
    sv = ens.tau_susceptibles(times=grid)
    assert_equals(sv, *want_block(ens, chains, range(16), grid, co, m.susNum), what="restart")
    assert any(chains[r][0].restarted for r in range(16)) and not all(chains[r][0].restarted for r in range(16))
    ens.close()


@pytest.fixture(scope="module")
def tau_b_ensemble():
    """tau_b with chains of more than two tiles of 64 rows, its window and the whole block at 100 points and the default tile."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    for mult in (1, 2, 4, 8, 16):
        ens.simulate_tau(nt * mult, sample_size=BIG, record_events=True)
        own_rows = [len(ens.engine.multievents(r)["num"]) for r in range(6)]
        if min(own_rows) > 2 * 64:
            break
    assert min(own_rows) > 2 * 64, own_rows
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    yield ens, window, ens.tau_susceptibles(points=100, window=window)
    ens.close()


def test_tiles_chunks_and_subsets_give_the_same_rows(tau_b_ensemble, monkeypatch):
    ens, window, whole = tau_b_ensemble
    S = ens.model.susNum
    assert whole.passes == 2                                                   # the prefix, then all replicates
    assert_equals(whole, *want_block(ens, chains_of(ens), range(6), whole.times, np.arange(S), S), what="default tile")
    for tile in ("1", "64"):
        monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", tile)
        sv = ens.tau_susceptibles(points=100, window=window)
        monkeypatch.delenv("VGX_PREVALENCE_TILE_EVENTS")
        assert_equals(sv, whole.values, whole.final, whole.outside, what=tile)
    order = [4, 0, 5, 2, 1]
    sub = ens.tau_susceptibles(points=100, window=window, replicates=order)
    assert list(sub.replicates) == order and sub.passes == 2
    assert_equals(sub, whole.values[order], whole.final[order], whole.outside[order], what="subset")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "1000")                   # 102 bounds of 4 bytes + 64 per replicate: 2 per chunk
    split = ens.tau_susceptibles(points=100, window=window, replicates=order)
    assert split.passes == 1 + 3
    assert_equals(split, whole.values[order], whole.final[order], whole.outside[order], what="chunks")


def test_summary_in_the_same_call(tau_b_ensemble):
    ens, window, _ = tau_b_ensemble
    block = ens.tau_susceptibles(points=9, window=window).values
    assert 0 <= block.min() and block.max() < 2 ** 31 and np.ptp(block, axis=0).max() > 0
    by = np.array([0, 1, 0, 1, 0, 1])
    for method in ("lower", "linear"):
        band = ens.tau_susceptibles(points=9, window=window, summary=dict(quantiles=Q, by=by, method=method), values=False)
        assert band.values is None and band.summary.method == method and band.final.shape == block[:, 0].shape
        assert_summary(band.summary, block, by, 2, method)
    reps = np.array([5, 0, 2, 3])                                               # group_of follows the order of `replicates`
    band = ens.tau_susceptibles(points=9, window=window, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.values, block[reps]) and np.array_equal(band.summary.count, [2, 2])
    left = np.full(6, -1)
    left[reps] = by[reps]
    assert_summary(band.summary, block, left, 2, 'lower')
    share = band.share()
    assert share.shape == band.values.shape and np.allclose(share.sum(axis=-1), 1.0)


def test_the_librarys_own_refusals():
    """Ensemble.tau_susceptibles checks its arguments before the library is called; these calls go to vgx_get_tau_susceptibles
    itself.  After every refused call a good one still works."""
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 3, seeds=np.array([3, 4, 5]))
    eng = ens.engine
    P, S = ens.model.popNum, ens.model.susNum

    def call(reps=(0, 1, 2), grid=(0.0, 1.0, 2.0), pre=None, null_prefix=False, G=None, co=None):
        reps, grid = np.array(reps, dtype=np.int64), np.array(grid, dtype=np.float64)
        G = S if G is None else G
        co = np.arange(S, dtype=np.int32) if co is None else np.asarray(co, dtype=np.int32)
        io = _capi.VgxTauSusceptiblesIO()
        values = np.zeros((len(reps), len(grid), P, G), dtype=np.int64)
        final = np.zeros((len(reps), P, G), dtype=np.int64)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.grid = len(reps), _capi._p(reps), len(grid), _capi._p(grid)
        io.G, io.class_of = G, co.ctypes.data_as(C.POINTER(C.c_int32))
        io.values, io.final, io.outside = _capi._p(values), _capi._p(final), _capi._p(outside)
        eng._check(eng.lib.vgx_get_tau_susceptibles(eng.handle, C.byref(io), None if null_prefix else C.byref(pre)))
        return values, final, outside

    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_susceptibles: the last call was not vgx_simulate_tau"):
        call(null_prefix=True)
    with pytest.raises(ValueError, match=r"^tau_susceptibles\(\) counts tau chains only"):
        ens.tau_susceptibles(times=[0.0])
    ens.simulate_tau(nt, sample_size=BIG, record_events=False)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_susceptibles: the last call recorded no multievent rows"):
        call(null_prefix=True)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_susceptibles(times=[0.0])
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    t_end = float(final_times(ens).max())
    good = ens.tau_susceptibles(times=[0.0, 0.5 * t_end, t_end])
    assert good.values.any() and np.array_equal(good.final, ens.replicate_states_tau()[1])

    def still_works():
        values, final, outside = call(grid=(0.0, 0.5 * t_end, t_end), pre=ens._tau_prefix_struct())
        assert np.array_equal(values, good.values) and np.array_equal(final, good.final) and np.array_equal(outside, good.outside)

    still_works()
    pre = ens._tau_prefix_struct()
    n_pre = int(pre.ev_ptr)
    assert n_pre > 1
    wide = 65536 // (8 * P) + 1                                                # P * G * 8 just above the LDS budget
    for kw, msg in ((dict(reps=(1, 1)), "replicates must be distinct"), (dict(reps=(0, 3)), "replicate index out of range"),
                    (dict(grid=(0.0, 1.0, 1.0)), r"grid must increase strictly \(grid\[2\]\)"),
                    (dict(grid=(0.0, float("inf"))), r"grid\[1\] is not finite"), (dict(grid=()), "T = 0 grid points"),
                    (dict(G=0), "G = 0 classes"), (dict(co=[S] + [0] * (S - 1)), r"class_of\[0\] = %d is outside \[-1, %d\)" % (S, S)),
                    (dict(G=wide, co=[wide - 1] * S), "%d populations x %d classes need %d bytes of cells, above the 65536 bytes of LDS" % (P, wide, 8 * P * wide))):
        with pytest.raises(_capi.VgxError, match="vgx_get_tau_susceptibles: " + msg):
            call(pre=pre, **kw)
        still_works()
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_susceptibles: replicate 0: its chain continues a log of %d events, the prefix holds 0" % n_pre):
        call(null_prefix=True)
    pre.ev_ptr, pre.ev_types = n_pre, None
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_susceptibles: null prefix column"):
        call(pre=pre)
    still_works()
    for kw, msg in ((dict(times=[0.0], replicates=[1, 1]), "distinct"), (dict(times=[0.0, 0.0]), "increase strictly"),
                    (dict(times=[0.0], groups=np.full(S, wide - 1)), "bytes of cells")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_susceptibles(**kw)
    with pytest.raises(ValueError, match=r"^susceptibles\(\) counts direct chains only: the last call was simulate_tau"):
        ens.susceptibles(times=[0.0])
    still_works()
    ens.close()
