"""Ensemble.milestones(): peaks, first passages and extinctions of every replicate on the device (vgx_get_milestones).  Expected
values come from the chain replicate_events() gives (the route there was before) through the literal restatement of the rule in
test_milestones_rule.py, from replicate_state() and from prevalence(), never from the code under test; every comparison is
array_equal (times: NaN at the same places, array_equal elsewhere).

The shapes are the smallest at which the walk can still go wrong: the scenario family of test_hip_param_sets.py as
test_hip_prevalence.py builds it (16 replicates, 4 scenarios, at most 2000 events, P = 3, H = 16) with tiles of 64 events, so
that chains span up to 30 tiles and one round is a whole tile.  The thresholds are chosen from the oracle's runs of the family
(peaks stay below 50 hosts here): 20 is reached by some replicates and not by others, 50 by none, and the small ones are crossed,
lost and crossed again within a round."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_ensemble_timelines import _ensemble
from test_hip_incidence import event_chain
from test_hip_param_sets import ATTEMPTS, BLOCK, N_EVENTS, SEEDS, base_sim, reference, scenarios_of
from test_hip_prevalence import H, IDENT, P, T, THREE, WINDOW, grid_of, start_of
from test_incidence_rule import chain_of
from test_milestones_rule import INT_FIELDS, NEVER, TIME_FIELDS, restate, same_times
from test_prevalence_rule import deltas, fold

pytestmark = pytest.mark.gpu

THRESHOLDS = (1, 2, 5, 10, 20, 50)


@pytest.fixture(scope="module")
def family():
    """The scenario ensemble, run once, and its results; shared and never changed."""
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    ens = Ensemble(base, 16, seeds=np.array(SEEDS * 4, dtype=np.int64), scenarios=scenarios_of(base), scenario_of=BLOCK)
    res = ens.simulate(N_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True, traj_points=T, traj_window=WINDOW)
    yield ens, res
    ens.close()


@pytest.fixture
def tile64(monkeypatch):
    monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", "64")


def want_rows(ens, reps, variant_of, V, thresholds=THRESHOLDS):
    got = [restate(*event_chain(ens, int(r)), P, variant_of, V, fold(start_of(ens, int(r)), variant_of, V), thresholds) for r in reps]
    return {k: np.stack([g[k] for g in got]) for k in got[0]}


def assert_equals(ms, want, what=""):
    got = dict(final=ms.final, peak=ms.peak, peak_event=ms.peak_event, last_positive_event=ms.last_positive_event, first_event=ms.first_event,
               peak_time=ms.peak_time, extinction_time=ms.extinction_time, first_time=ms.first_time)
    for k in INT_FIELDS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in TIME_FIELDS:
        assert got[k].dtype == np.float64 and same_times(got[k], want[k]), (what, k)
    for k in ("extinct", "reached", "never_present"):
        assert np.array_equal(getattr(ms, k), want[k]), (what, k)
    assert np.array_equal(ms.extinction_event[want["extinct"]], want["last_positive_event"][want["extinct"]] + 1), what


def values_of(m, variant_of, V):
    """x[-1 .. n_ev - 1] of one oracle run as an array [n_ev + 1, P + 1, V]: what the inputs are judged by, not the code under test."""
    t, cols = chain_of(m)
    x = np.zeros((len(t) + 1, P + 1, V), dtype=np.int64)
    x[0, :P] = fold(m.initial_infectious, variant_of, V)
    x[0, P] = x[0, :P].sum(axis=0)
    for i in range(len(t)):
        x[i + 1] = x[i]
        for p, c, d in deltas([col[i] for col in cols], P, variant_of):
            x[i + 1, p, c] += d
            x[i + 1, P, c] += d
    return x


def assert_the_inputs_reach_the_branches(runs, variant_of, V):
    xs = [values_of(m, variant_of, V) for m in runs]
    assert sum(m.good_attempt > 1 for m in runs) >= 2                                    # restarted replicates
    assert sum(m.events.ptr == 0 for m in runs) >= 2                                     # replicates with zero events
    assert sum(bool(((x[:, P] > 0).any(axis=0) & (x[-1, P] == 0)).any()) for x in xs) >= 2      # row P extinct ...
    assert sum(bool((x[-1, P] > 0).any()) for x in xs) >= 2                                     # ... and not extinct
    reached = np.array([[bool((x >= th).any()) for x in xs] for th in THRESHOLDS])
    assert (reached.sum(axis=1) >= 2).any() and ((reached.sum(axis=1) >= 2) & ((~reached).sum(axis=1) >= 2)).any()
    falls = twice = 0
    for x in xs:
        fell = False
        for th in THRESHOLDS:
            at = x >= th
            first = np.where(at.any(axis=0), at.argmax(axis=0), -1)                      # (row index = event + 1)
            for p, c in zip(*np.nonzero(first >= 0)):
                fell = fell or bool((x[first[p, c] + 1:first[p, c] + 65, p, c] < th).any())
        falls += fell
        top = x == x.max(axis=0)
        entered = top & ~np.concatenate([np.zeros((1,) + top.shape[1:], dtype=bool), top[:-1]])
        twice += bool((entered.sum(axis=0) > 1).any())
    assert falls >= 2 and twice >= 2


def test_every_replicate_equals_the_restatement(oracle_mod, family, tile64):
    ens, res = family
    ref = reference(oracle_mod)
    runs = [ref[g][k].simulation for g in range(4) for k in range(4)]                    # BLOCK: replicate 4 g + k
    assert [int(n) for n in res.events] == [m.events.ptr for m in runs] and max(res.events) > 20 * 64
    assert (res.restarts > 0).sum() >= 2
    for variant_of, V, variants in ((IDENT, H, None), (THREE, 3, THREE)):
        assert_the_inputs_reach_the_branches(runs, variant_of, V)
        ms = ens.milestones(variants=variants, thresholds=THRESHOLDS)
        assert np.array_equal(ms.variant_of, variant_of) and list(ms.replicates) == list(range(16)) and ms.thresholds.tolist() == list(THRESHOLDS)
        assert ms.peak.shape == (16, P + 1, V) and ms.first_event.shape == (16, len(THRESHOLDS), P + 1, V) and ms.passes == 1
        want = want_rows(ens, range(16), variant_of, V)
        assert_equals(ms, want, V)
        assert np.array_equal(ms.final[:, P], ms.final[:, :P].sum(axis=1)) and (ms.peak[:, P] <= ms.peak[:, :P].sum(axis=1)).all()
        assert ms.reached[:, 4].any() and not ms.reached[:, 5].any() and len(np.unique(ms.peak_event)) > 10
        prob = ms.extinction_probability()
        assert prob.shape == (4, P + 1, V)
        for g in range(4):
            assert np.array_equal(prob[g], want["extinct"][BLOCK == g].mean(axis=0))
    none = ens.milestones(variants=THREE)                                                # K = 0
    assert none.first_event.shape == (16, 0, P + 1, 3) and np.array_equal(none.peak, ms.peak) and np.array_equal(none.peak_event, ms.peak_event)
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0


def test_tiles_chunks_and_subsets_give_the_same_rows(family, monkeypatch):
    ens, _ = family

    def rows(ms, sel=slice(None)):
        return {k: getattr(ms, k)[sel] for k in INT_FIELDS + TIME_FIELDS + ("extinct", "reached", "never_present")}
    monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", "64")
    small = ens.milestones(variants=THREE, thresholds=THRESHOLDS)
    assert small.passes == 1 and len(np.unique(small.peak_event)) > 10
    for tile in ("1000", None):
        if tile is None:
            monkeypatch.delenv("VGX_MILESTONES_TILE_EVENTS")
        else:
            monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", tile)
        assert_equals(ens.milestones(variants=THREE, thresholds=THRESHOLDS), rows(small), tile)
    monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", "64")
    monkeypatch.setenv("VGX_MILESTONES_WAVES", "4")            # four wavefronts per tile taking rounds in turn: tiles of 64 and of 1000 events
    assert_equals(ens.milestones(variants=THREE, thresholds=THRESHOLDS), rows(small), "four waves")
    monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", "1000")
    assert_equals(ens.milestones(variants=None, thresholds=THRESHOLDS), want_rows(ens, range(16), IDENT, H), "four waves, tiles of 1000")
    monkeypatch.delenv("VGX_MILESTONES_WAVES")
    monkeypatch.setenv("VGX_MILESTONES_TILE_EVENTS", "64")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "20000")
    split = ens.milestones(variants=THREE, thresholds=THRESHOLDS)
    assert split.passes > 4
    assert_equals(split, rows(small), "chunks")
    monkeypatch.delenv("VGX_TIMELINES_CHUNK_BYTES")
    order = np.array([11, 2, 7, 14, 0])
    sub = ens.milestones(variants=THREE, thresholds=THRESHOLDS, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_equals(sub, rows(small, order), "subset")
    assert_equals(sub, want_rows(ens, order, THREE, 3), "subset against the restatement")
    assert np.array_equal(sub.extinction_probability()[0], sub.extinct[BLOCK[order] == 0].mean(axis=0))


def test_independent_routes(family, tile64):
    ens, _ = family
    grid = grid_of(T, WINDOW)
    for variant_of, V, variants in ((IDENT, H, None), (THREE, 3, THREE)):
        ms = ens.milestones(variants=variants, thresholds=THRESHOLDS)
        pv = ens.prevalence(times=grid, variants=variants)
        assert np.array_equal(ms.final[:, :P], pv.final)
        for r in range(16):
            assert np.array_equal(ms.final[r, :P], fold(ens.replicate_state(r).infectious, variant_of, V)), (V, r)
        assert (ms.peak[:, :P] >= pv.values.max(axis=1)).all() and pv.values.max() > 5
        assert (ms.peak[:, P] >= pv.values.sum(axis=2).max(axis=1)).all()


def test_refusals_leave_the_ensemble_usable(family, tile64):
    from vgsim_amd import _capi
    ens, _ = family
    eng = ens.engine
    i32 = C.POINTER(C.c_int32)

    def library(reps=(0, 1), vo=THREE, V=3, th=THRESHOLDS):
        """vgx_get_milestones itself, past the facade's checks"""
        io = _capi.VgxMilestonesIO()
        reps = np.asarray(reps, dtype=np.int64)
        vo = np.ascontiguousarray(vo, dtype=np.int32)
        th = np.ascontiguousarray(th, dtype=np.int32)
        peak = np.zeros((len(reps), P + 1, max(V, 1)), dtype=np.int32)
        io.n, io.replicates, io.V, io.variant_of, io.K, io.thresholds = len(reps), _capi._p(reps), V, vo.ctypes.data_as(i32), len(th), th.ctypes.data_as(i32)
        io.peak = peak.ctypes.data_as(i32)                       # (every other output is NULL: not written)
        eng._check(eng.lib.vgx_get_milestones(eng.handle, C.byref(io)))
        return peak

    good = ens.milestones(variants=THREE, thresholds=THRESHOLDS)
    assert np.array_equal(library(), good.peak[:2])
    wide = np.arange(H) * 100                                   # 4 x 1501 classes x 10 records: 240160 bytes
    for kw, text in ((dict(reps=(1, 1)), "vgx_get_milestones: replicates must be distinct"),
                     (dict(reps=(0, 16)), "vgx_get_milestones: replicate index out of range"),
                     (dict(V=0), "vgx_get_milestones: V = 0"),
                     (dict(vo=np.where(THREE == 2, 3, THREE)), r"vgx_get_milestones: variant_of\[2\] = 3 is outside \[-1, 3\)"),
                     (dict(vo=np.where(THREE == 2, -2, THREE)), r"vgx_get_milestones: variant_of\[2\] = -2 is outside"),
                     (dict(th=np.arange(17)), "vgx_get_milestones: K = 17 thresholds: at most 16"),
                     (dict(vo=wide, V=1501), r"vgx_get_milestones: 3 populations \(and their total\) x 1501 classes x 6 thresholds need 240160 bytes of records, "
                                             "above the 65536 bytes of LDS")):
        with pytest.raises(_capi.VgxError, match=text) as ei:
            library(**kw)
        assert ei.value.code == 1
        assert np.array_equal(ens.milestones(variants=THREE, thresholds=THRESHOLDS).peak, good.peak)
    with pytest.raises(ValueError, match="distinct"):
        ens.milestones(replicates=[1, 1])
    with pytest.raises(ValueError, match=r"3 populations \(and their total\) x 1501 classes x 0 thresholds need 96064 bytes"):
        ens.milestones(variants=wide)


def test_the_wrong_last_call_is_refused_by_the_library_too():
    from vgsim_amd import _capi
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)
    eng = ens.engine
    good = ens.milestones(thresholds=(3,))
    assert good.peak.max() > 3 and good.reached.any()

    def library():
        io = _capi.VgxMilestonesIO()
        reps, vo = np.arange(2, dtype=np.int64), np.zeros(ens.model.hapNum, dtype=np.int32)
        io.n, io.replicates, io.V, io.variant_of = 2, _capi._p(reps), 1, vo.ctypes.data_as(C.POINTER(C.c_int32))
        eng._check(eng.lib.vgx_get_milestones(eng.handle, C.byref(io)))

    library()
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match=r"milestones\(\).*record_events"):
        ens.milestones()
    with pytest.raises(_capi.VgxError, match="vgx_get_milestones: the last call did not record events"):
        library()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match=r"milestones\(\).*direct chains only"):
        ens.milestones()
    with pytest.raises(_capi.VgxError, match="vgx_get_milestones: the last call was vgx_simulate_tau"):
        library()
    ens.close()
