"""Ensemble.tau_prevalence(): infectious hosts per grid time, population and variant class of every replicate of a tau ensemble on
the device (vgx_get_tau_prevalence), on both tau paths.  The engine's tau chain is distributional, not oracle-identical, so the
expected blocks are the literal restatement of the rule (test_tau_prevalence_rule.restate_weighted_prevalence) over the chain the
engine itself recorded, assembled from read-outs that exist without this feature (test_hip_ensemble_tau_timelines.recorded_chain;
no prefix for a restarted replicate).  Two checks need no restatement: `final` against replicate_states_tau(), and the sum over
the classes against the tau trajectories binned by the step kernels themselves.  Every comparison is array_equal on integers.

Not covered here: the summary's refusal of a value outside [0, 2^31) cannot be reached by a run of a few seconds; net changes and
values beyond 2^32 in one cell are covered by the CPU hook test (tests/test_tau_prevalence_rule.py)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_tau_timelines import EV_COLUMNS, SEEDS, _fresh, _near_critical_warm, recorded_chain
from test_hip_incidence import Q, assert_summary
from test_hip_tau_trajectories import PATHS, warm
from test_prevalence_rule import fold
from test_tau_prevalence_rule import restate_weighted_prevalence, rows_of_events

pytestmark = pytest.mark.gpu

POINTS = (100, 7, 1)
BIG = 10 ** 12


def chains_of(ens, reps=None):
    """replicate -> (host, mev, events, rows): the recorded chain and its rows, formed once."""
    states = ens.replicate_states_tau()
    out = {}
    for r in (range(ens.R) if reps is None else reps):
        host, mev = recorded_chain(ens, int(r), states)
        events = [host.events.times] + [getattr(host.events, c) for c in EV_COLUMNS]
        out[int(r)] = (host, mev, events, rows_of_events(events, mev))
    return out


def start_of(ens, host, vo, V):
    """The state the chain starts from: the initial state when it starts at the beginning of the model's history (a restart, or a
    model that held events before the call), else the state the call started from.  On a model's first call the two are one: the
    call's preparation (the index case included) forms the initial state, which the model object itself does not hold yet."""
    from_initial = host.restarted or ens.model.events.ptr > 0 or not ens.model.first_simulation
    return fold(host.initial_infectious if from_initial else ens.model.infectious, vo, V)


def want_block(ens, chains, reps, grid, vo, V):
    got = []
    for r in reps:
        host, mev, events, rows = chains[int(r)]
        got.append(restate_weighted_prevalence(events, mev, ens.model.popNum, grid, vo, V, start_of(ens, host, vo, V), rows))
    return tuple(np.stack([g[k] for g in got]) for k in range(3))


def assert_equals(pv, values, final, outside, what=""):
    assert pv.values.dtype == np.int64 and pv.values.shape == values.shape and pv.final.dtype == np.int64, what
    assert np.array_equal(pv.values, values), what
    assert np.array_equal(pv.final, final), what
    assert pv.outside.dtype == np.int64 and np.array_equal(pv.outside, outside), what


def final_times(ens):
    return ens.replicate_states_tau()[3]


def three_classes(ens, chains):
    """h % 3 with one haplotype the chains touch not tracked (a model with one haplotype: that one), and its V as variant_map forms it."""
    H = ens.model.hapNum
    seen = np.array([r[2] for c in chains.values() for ev in c[3] for r in ev if 0 <= r[2] < H], dtype=np.int64)
    vo = np.arange(H) % 3
    vo[np.bincount(seen, minlength=H).argsort()[::-1][min(1, H - 1)]] = -1
    return vo, max(int(vo.max()) + 1, 1)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_warm_up_cases_equal_the_restatement(name, path, monkeypatch):
    """A tau call that continues a direct warm-up: the grid runs from half of the prefix's last time to 0.9 of the latest final
    time, so prefix rows and own rows lie before, between and behind its points; tiles of 64 rows, so that a chain spans several
    tiles and intervals change inside a tile."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", "64")
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    m = ens.model
    assert m.events.ptr > 0
    t_pre = float(m.events.times[m.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    chains = chains_of(ens)
    assert all(c[0].own_steps > 1 and not c[0].restarted for c in chains.values())
    ident = ens.replicate_states_tau()[0]
    for variants, V in ((None, m.hapNum), three_classes(ens, chains)):
        vo = np.arange(m.hapNum) if variants is None else variants
        for points in POINTS:
            pv = ens.tau_prevalence(points=points, window=window, variants=variants)
            assert_equals(pv, *want_block(ens, chains, range(6), pv.times, vo, V), what=(name, path, points, V))
            assert pv.outside.any() and pv.passes == 2 and np.array_equal(pv.variant_of, vo)
            assert variants is not None or (pv.values.any() and np.array_equal(pv.final, ident))
    ens.close()


def _ensemble(kind):
    """(ensemble after a simulate_tau call with the event log, the call's result, the call's arguments)"""
    from vgsim_amd.ensemble import Ensemble
    if kind == "fresh":
        ens, call = Ensemble(_fresh("tau_c"), 6, seeds=SEEDS), dict(iterations=60)
    elif kind == "warm":
        sim, nt = warm("tau_d")
        ens, call = Ensemble(sim, 6, seeds=SEEDS), dict(iterations=nt)
    else:
        ens, call = Ensemble(_near_critical_warm(), 16, seeds=500 + np.arange(16, dtype=np.int64)), dict(iterations=300, attempts=4)
    call.update(sample_size=BIG, record_events=True)
    res = ens.simulate_tau(**call)
    if kind == "restarted":
        assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    return ens, res, call


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["fresh", "warm", "restarted"])
def test_final_is_the_final_infectious_state(kind, path, monkeypatch):
    """Independent of the restatement: with every haplotype tracked the running sum over the whole chain ends in the state the
    engine holds."""
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, _, _ = _ensemble(kind)
    states = ens.replicate_states_tau()
    t_end = float(states[3].max())
    for times in ([0.5 * t_end], [-1.0], [t_end + 1.0], np.linspace(0.1 * t_end, 0.9 * t_end, 12)):
        pv = ens.tau_prevalence(times=times)
        assert np.array_equal(pv.final, states[0]), (kind, path, len(times))
    assert not np.array_equal(pv.values[:, 0], pv.values[:, -1])
    behind = ens.tau_prevalence(times=[t_end + 1.0])
    assert np.array_equal(behind.values[:, 0], states[0]) and not behind.outside[:, 1].any()
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["warm", "restarted"])
def test_classes_sum_to_the_trajectories(kind, path, monkeypatch):
    """Independent of the restatement: over a window that starts after the prefix's last time the sum over all classes is the
    infectious total the tau kernels binned themselves, at every point of every replicate, restarted ones included
    (tests/test_tau_prevalence_rule.py checks on the oracle's chains that the rule satisfies this identity)."""
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, res, call = _ensemble(kind)
    t_start, t_last = float(ens.model.currentTime), float(final_times(ens).max())
    assert ens.model.events.ptr > 0 and float(ens.model.events.times[ens.model.events.ptr - 1]) <= t_start < t_last
    window = (t_start + 0.05 * (t_last - t_start), t_last - 0.05 * (t_last - t_start))
    for T in (33, 1):
        again = ens.simulate_tau(traj_points=T, traj_window=window, **call)
        assert np.array_equal(again.events, res.events) and np.array_equal(again.restarts, res.restarts)
        traj = ens.trajectories()
        pv = ens.tau_prevalence(points=T, window=window)
        assert traj.shape == (ens.R, T, ens.model.popNum, 2) and pv.values.shape[:3] == traj.shape[:3]
        assert np.array_equal(pv.values.sum(axis=-1), traj[..., 0])
        assert T == 1 or any(not np.array_equal(traj[r, 0], traj[r, -1]) for r in range(ens.R))
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix(path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0 and not sim.simulation.first_simulation
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=BIG, record_events=True)
    chains = chains_of(ens)
    assert any(c[0].own_steps > 1 for c in chains.values()) and all(c[0].events.ptr == c[0].own_steps for c in chains.values())
    t_end = float(final_times(ens).max())
    H = ens.model.hapNum
    for points in (7, 1):
        pv = ens.tau_prevalence(points=points, window=(0.2 * t_end, 0.8 * t_end))
        assert_equals(pv, *want_block(ens, chains, range(6), pv.times, np.arange(H), H), what=("no prefix", points))
        assert pv.values.any() and pv.passes == 1
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_own_steps(path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 4, seeds=np.array([1, 2, 3, 4], dtype=np.int64))
    ens.simulate_tau(nt, sample_size=BIG, attempts=0, record_events=True)     # no step is recorded: every chain is the prefix alone
    chains = chains_of(ens)
    assert all(c[0].own_steps == 0 and c[0].events.ptr == ens.model.events.ptr > 0 for c in chains.values())
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    H = ens.model.hapNum
    pv = ens.tau_prevalence(points=7, window=(0.3 * t_pre, 0.8 * t_pre))
    assert_equals(pv, *want_block(ens, chains, range(4), pv.times, np.arange(H), H), what="prefix alone")
    assert pv.values[0].any() and pv.outside[0].all() and pv.passes == 1
    assert np.array_equal(pv.final[0], ens.model.infectious) and not np.array_equal(pv.values[0, 0], pv.values[0, -1])
    assert all(np.array_equal(pv.values[r], pv.values[0]) and np.array_equal(pv.final[r], pv.final[0]) and
               np.array_equal(pv.outside[r], pv.outside[0]) for r in range(4))
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_restarted_replicates_have_no_prefix(path, monkeypatch):
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, res, _ = _ensemble("restarted")
    chains = chains_of(ens)
    m = ens.model
    P, H, n_pre = m.popNum, m.hapNum, int(m.events.ptr)
    t_pre = float(m.events.times[n_pre - 1])
    # restarted chains start again at time 0: grid times inside the prefix, behind it and behind most chains
    grid = np.array([0.5 * t_pre, np.nextafter(t_pre, np.inf), 2.0 * t_pre + 1.0, 0.9 * float(final_times(ens).max()) + 2.0 * t_pre + 2.0])
    vo = np.arange(H)
    pv = ens.tau_prevalence(times=grid)
    assert_equals(pv, *want_block(ens, chains, range(16), grid, vo, H), what="restart")
    for r in range(16):
        host, mev, events, rows = chains[r]
        assert host.restarted == (res.restarts[r] > 0)
        k = len(events[0]) - host.own_steps                   # the replicate's own steps alone (their row ranges index `mev` as they are)
        own = restate_weighted_prevalence([c[k:] for c in events], mev, P, grid, vo, H, fold(host.initial_infectious, vo, H), rows[k:])
        if host.restarted:                                    # own steps only, from the initial state
            assert k == 0 and np.array_equal(pv.values[r], own[0]) and np.array_equal(pv.outside[r], own[2])
        else:                                                 # the prefix in front: its events, then the own steps
            assert k == n_pre
            whole = restate_weighted_prevalence(events, mev, P, grid, vo, H, fold(host.initial_infectious, vo, H), rows)
            assert np.array_equal(pv.values[r], whole[0]) and not np.array_equal(whole[0], own[0])
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
    yield ens, window, ens.tau_prevalence(points=100, window=window)
    ens.close()


def test_tiles_chunks_and_subsets_give_the_same_rows(tau_b_ensemble, monkeypatch):
    ens, window, whole = tau_b_ensemble
    H = ens.model.hapNum
    assert whole.passes == 2                                                   # the prefix, then all replicates
    assert_equals(whole, *want_block(ens, chains_of(ens), range(6), whole.times, np.arange(H), H), what="default tile")
    for tile in ("1", "64"):
        monkeypatch.setenv("VGX_PREVALENCE_TILE_EVENTS", tile)
        pv = ens.tau_prevalence(points=100, window=window)
        monkeypatch.delenv("VGX_PREVALENCE_TILE_EVENTS")
        assert_equals(pv, whole.values, whole.final, whole.outside, what=tile)
    order = [4, 0, 5, 2, 1]
    sub = ens.tau_prevalence(points=100, window=window, replicates=order)
    assert list(sub.replicates) == order and sub.passes == 2
    assert_equals(sub, whole.values[order], whole.final[order], whole.outside[order], what="subset")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "1000")                   # 102 bounds of 4 bytes + 64 per replicate: 2 per chunk
    split = ens.tau_prevalence(points=100, window=window, replicates=order)
    assert split.passes == 1 + 3
    assert_equals(split, whole.values[order], whole.final[order], whole.outside[order], what="chunks")


def test_summary_in_the_same_call(tau_b_ensemble):
    ens, window, _ = tau_b_ensemble
    variants = np.arange(ens.model.hapNum) % 3
    block = ens.tau_prevalence(points=9, window=window, variants=variants).values
    assert 0 <= block.min() and block.max() < 2 ** 31 and np.ptp(block, axis=0).max() > 0
    by = np.array([0, 1, 0, 1, 0, 1])
    for method in ("lower", "higher", "linear"):
        band = ens.tau_prevalence(points=9, window=window, variants=variants, summary=dict(quantiles=Q, by=by, method=method), values=False)
        assert band.values is None and band.summary.method == method and band.final.shape == block[:, 0].shape
        assert_summary(band.summary, block, by, 2, method)
    reps = np.array([5, 0, 2, 3])                                               # group_of follows the order of `replicates`
    band = ens.tau_prevalence(points=9, window=window, variants=variants, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.values, block[reps]) and np.array_equal(band.summary.count, [2, 2])
    left = np.full(6, -1)
    left[reps] = by[reps]
    assert_summary(band.summary, block, left, 2, 'lower')
    one = ens.tau_prevalence(points=9, window=window, variants=variants, summary=dict(quantiles=Q, method='higher'))   # by='auto': one group
    assert_summary(one.summary, block, np.zeros(6, dtype=np.int64), 1, 'higher')
    share = one.share()
    assert share.shape == block.shape and np.allclose(share.sum(axis=-1)[block.sum(axis=-1) > 0], 1.0)


def test_the_librarys_own_refusals():
    """Ensemble.tau_prevalence checks its arguments before the library is called; these calls go to vgx_get_tau_prevalence itself.
    After every refused call a good one still works."""
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 3, seeds=np.array([3, 4, 5]))
    eng = ens.engine
    P, H = ens.model.popNum, ens.model.hapNum

    def call(reps=(0, 1, 2), grid=(0.0, 1.0, 2.0), pre=None, null_prefix=False, V=None, vo=None):
        reps, grid = np.array(reps, dtype=np.int64), np.array(grid, dtype=np.float64)
        V = H if V is None else V
        vo = np.arange(H, dtype=np.int32) if vo is None else np.asarray(vo, dtype=np.int32)
        io = _capi.VgxTauPrevalenceIO()
        values = np.zeros((len(reps), len(grid), P, V), dtype=np.int64)
        final = np.zeros((len(reps), P, V), dtype=np.int64)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.grid = len(reps), _capi._p(reps), len(grid), _capi._p(grid)
        io.V, io.variant_of = V, vo.ctypes.data_as(C.POINTER(C.c_int32))
        io.values, io.final, io.outside = _capi._p(values), _capi._p(final), _capi._p(outside)
        eng._check(eng.lib.vgx_get_tau_prevalence(eng.handle, C.byref(io), None if null_prefix else C.byref(pre)))
        return values, final, outside

    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_prevalence: the last call was not vgx_simulate_tau"):
        call(null_prefix=True)
    with pytest.raises(ValueError, match=r"tau_prevalence\(\) counts tau chains only"):
        ens.tau_prevalence(times=[0.0])
    ens.simulate_tau(nt, sample_size=BIG, record_events=False)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_prevalence: the last call recorded no multievent rows"):
        call(null_prefix=True)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_prevalence(times=[0.0])
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    t_end = float(final_times(ens).max())
    good = ens.tau_prevalence(times=[0.0, 0.5 * t_end, t_end])
    assert good.values.any() and np.array_equal(good.final, ens.replicate_states_tau()[0])

    def still_works():
        values, final, outside = call(grid=(0.0, 0.5 * t_end, t_end), pre=ens._tau_prefix_struct())
        assert np.array_equal(values, good.values) and np.array_equal(final, good.final) and np.array_equal(outside, good.outside)

    still_works()
    pre = ens._tau_prefix_struct()
    n_pre = int(pre.ev_ptr)
    assert n_pre > 1
    wide = 65536 // (8 * P) + 1                                                # P * V * 8 just above the LDS budget
    for kw, msg in ((dict(reps=(1, 1)), "replicates must be distinct"), (dict(reps=(0, 3)), "replicate index out of range"),
                    (dict(grid=(0.0, 1.0, 1.0)), r"grid must increase strictly \(grid\[2\]\)"),
                    (dict(grid=(0.0, float("inf"))), r"grid\[1\] is not finite"), (dict(grid=()), "T = 0 grid points"),
                    (dict(V=0), "V = 0 classes"), (dict(vo=[H] + [0] * (H - 1)), r"variant_of\[0\] = %d is outside \[-1, %d\)" % (H, H)),
                    (dict(V=wide, vo=[wide - 1] * H), "%d populations x %d classes need %d bytes of cells, above the 65536 bytes of LDS" % (P, wide, 8 * P * wide))):
        with pytest.raises(_capi.VgxError, match="vgx_get_tau_prevalence: " + msg):
            call(pre=pre, **kw)
        still_works()
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_prevalence: replicate 0: its chain continues a log of %d events, the prefix holds 0" % n_pre):
        call(null_prefix=True)
    pre.ev_ptr, pre.ev_types = n_pre, None
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_prevalence: null prefix column"):
        call(pre=pre)
    still_works()
    for kw, msg in ((dict(times=[0.0], replicates=[1, 1]), "distinct"), (dict(times=[0.0, 0.0]), "increase strictly"),
                    (dict(times=[0.0], variants=np.full(H, wide - 1)), "bytes of cells")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_prevalence(**kw)
    with pytest.raises(ValueError, match=r"^prevalence\(\) counts direct chains only: the last call was simulate_tau"):
        ens.prevalence(times=[0.0])
    still_works()
    ens.close()
