"""Ensemble.tau_milestones(): peaks, first passages and extinctions of every replicate of a tau ensemble on the device
(vgx_get_tau_milestones), on both tau paths.  The engine's tau chain is distributional, not oracle-identical, so the expected
results are the literal restatement of the rule (test_tau_milestones_rule.restate) over the chain the engine itself recorded,
assembled from read-outs that exist without this feature (test_hip_ensemble_tau_timelines.recorded_chain; no prefix for a
restarted replicate).  Two checks need no restatement: `final` against replicate_states_tau(), and peaks, first passages and
last positive events formed with numpy from tau_prevalence() evaluated at every event's time.  Integers are compared with
array_equal, times are equal with NaN at the same places.

Not covered here: values beyond 2^32 and steps of more than 256 touched cells are covered by the CPU hook test
(tests/test_tau_milestones_rule.py), which runs the same header."""
import ctypes as C

import numpy as np
import pytest

import helpers
from test_hip_tau_prevalence import BIG, PATHS, SEEDS, _ensemble, chains_of, start_of, three_classes, warm
from test_milestones_rule import same_times
from test_tau_milestones_rule import INT32_FIELDS, INT64_FIELDS, NEVER, TIME_FIELDS, restate

pytestmark = pytest.mark.gpu

FIELDS = INT64_FIELDS + INT32_FIELDS + TIME_FIELDS
THRESHOLDS = (1, 10, 100)


def assert_rows(ms, want, what=""):
    """Every row of `ms` against the list of restatements `want`."""
    assert ms.final.dtype == np.int64 and ms.peak.dtype == np.int64 and ms.thresholds.dtype == np.int64, what
    assert len(want) == len(ms.replicates)
    for i, w in enumerate(want):
        for k in INT64_FIELDS + INT32_FIELDS:
            got = getattr(ms, k)[i]
            assert got.dtype == (np.int64 if k in INT64_FIELDS else np.int32) and got.shape == w[k].shape, (what, i, k)
            assert np.array_equal(got, w[k]), (what, i, k)
        for k in TIME_FIELDS:
            assert same_times(getattr(ms, k)[i], w[k]), (what, i, k)
        assert np.array_equal(ms.extinct[i], w["extinct"]) and np.array_equal(ms.reached[i], w["reached"]), (what, i)


def without_thresholds(w):
    out = dict(w)
    for k in ("first_event", "first_time", "reached"):
        out[k] = w[k][:0]
    return out


def t_start_of(ens, host):
    """The time of event -1: 0.0 for a chain that starts at the beginning of the model's history, else where the call started."""
    return 0.0 if host.restarted or ens.model.events.ptr > 0 else float(ens.model.currentTime)


def want_rows(ens, chains, reps, vo, V, thresholds=THRESHOLDS):
    out = []
    for r in reps:
        host, mev, events, rows = chains[int(r)]
        out.append(restate(events, mev, ens.model.popNum, vo, V, start_of(ens, host, vo, V), thresholds, t_start_of(ens, host), rows))
    return out


def check_against_restatement(ens, monkeypatch, what):
    """Identity map and three classes, thresholds (1, 10, 100) and none, tiles of 64 rows and of one event."""
    chains = chains_of(ens)
    reps = range(ens.R)
    H = ens.model.hapNum
    seen = []
    for variants, V in ((None, H), three_classes(ens, chains)):
        vo = np.arange(H) if variants is None else variants
        want = want_rows(ens, chains, reps, vo, V)
        for tile in ("64", "1"):
            monkeypatch.setenv("VGX_TAU_MILESTONES_TILE_ROWS", tile)
            ms = ens.tau_milestones(variants=variants, thresholds=THRESHOLDS)
            assert_rows(ms, want, what + (V, tile))
            assert np.array_equal(ms.variant_of, vo) and ms.thresholds.tolist() == list(THRESHOLDS)
            bare = ens.tau_milestones(variants=variants)
            assert bare.first_event.shape == (ens.R, 0, ens.model.popNum + 1, V)
            assert_rows(bare, [without_thresholds(w) for w in want], what + (V, tile, "K = 0"))
            monkeypatch.delenv("VGX_TAU_MILESTONES_TILE_ROWS")
        seen.append(ms)
    return chains, seen


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_warm_up_cases_equal_the_restatement(name, path, monkeypatch):
    """A tau call that continues a direct warm-up: every chain is the prefix, walked once, then the replicate's own steps."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    assert ens.model.events.ptr > 0
    chains, (ident, _) = check_against_restatement(ens, monkeypatch, (name, path))
    assert all(c[0].own_steps > 1 and not c[0].restarted for c in chains.values())
    assert ident.passes == 2 and (ident.peak_event >= 0).any() and ident.reached.any()
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["fresh", "restarted"])
def test_fresh_and_restarted_chains_equal_the_restatement(kind, path, monkeypatch):
    """No prefix at all (the call's start state, the call's start time at index -1), and an ensemble in which some replicates
    restarted (own steps only, from the initial state at time 0) next to others that carry the prefix."""
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, res, _ = _ensemble(kind)
    chains, (ident, _) = check_against_restatement(ens, monkeypatch, (kind, path))
    if kind == "fresh":
        assert ident.passes == 1 and all(c[0].events.ptr == c[0].own_steps for c in chains.values())
    else:
        assert ident.passes == 2 and {c[0].restarted for c in chains.values()} == {True, False} and res.restarts.max() > 0
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["fresh", "warm", "restarted"])
def test_final_is_the_final_infectious_state(kind, path, monkeypatch):
    """Independent of the restatement: with every haplotype tracked the walk's final values are the state the engine holds."""
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, _, _ = _ensemble(kind)
    P = ens.model.popNum
    states = ens.replicate_states_tau()[0]
    ms = ens.tau_milestones(thresholds=(1,))
    assert np.array_equal(ms.final[:, :P], states) and np.array_equal(ms.final[:, P], states.sum(axis=1)), (kind, path)
    assert (ms.peak >= ms.final).all() and states.any()
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["fresh", "warm"])
def test_peaks_and_passages_from_the_prevalence_at_every_event(kind, path, monkeypatch):
    """Independent of the restatement, through merged code: a grid point at an event's time has the event applied, so on a chain
    whose event times increase strictly tau_prevalence(times=<the event times>) is x[0 .. n); plain numpy over that block and
    the start gives the peak, its first event, the first passages and the last positive event."""
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    ens, _, _ = _ensemble(kind)
    P, H = ens.model.popNum, ens.model.hapNum
    chains = chains_of(ens)
    rising = [r for r, c in chains.items() if (np.diff(np.asarray(c[2][0], dtype=np.float64)) > 0).all()]
    r = max(rising, key=lambda r: len(chains[r][2][0]))              # the longest of the chains whose event times increase strictly
    host, _, events, _ = chains[r]
    times = np.asarray(events[0], dtype=np.float64)
    n = len(times)
    assert n > 2 and (np.diff(times) > 0).all()
    pv = ens.tau_prevalence(times=times, replicates=[r])
    x = np.zeros((n + 1, P + 1, H), dtype=np.int64)
    x[0, :P] = start_of(ens, host, np.arange(H), H)
    x[1:, :P] = pv.values[0]
    x[:, P] = x[:, :P].sum(axis=1)
    ms = ens.tau_milestones(thresholds=THRESHOLDS, replicates=[r])
    assert np.array_equal(ms.final[0], x[-1]) and np.array_equal(ms.peak[0], x.max(axis=0))
    assert np.array_equal(ms.peak_event[0], x.argmax(axis=0) - 1)                      # (argmax: the first index that attains it)
    for k, th in enumerate(THRESHOLDS):
        met = x >= th
        assert np.array_equal(ms.first_event[0, k], np.where(met.any(axis=0), met.argmax(axis=0) - 1, NEVER)), (kind, path, th)
    pos = x > 0
    assert np.array_equal(ms.last_positive_event[0], np.where(pos.any(axis=0), n - 1 - pos[::-1].argmax(axis=0), -2))
    assert (x != x[0]).any() and ms.reached[0, 0].any()               # (the values move, a cell holds a host)
    ens.close()


@pytest.fixture(scope="module")
def tau_b_ensemble():
    """tau_b with chains of more than two tiles of 64 rows, and its milestones at the default tile."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    for mult in (1, 2, 4, 8, 16):
        ens.simulate_tau(nt * mult, sample_size=BIG, record_events=True)
        own_rows = [len(ens.engine.multievents(r)["num"]) for r in range(6)]
        if min(own_rows) > 2 * 64:
            break
    assert min(own_rows) > 2 * 64, own_rows
    yield ens, ens.tau_milestones(variants=np.arange(ens.model.hapNum) % 3, thresholds=THRESHOLDS)
    ens.close()


def test_nothing_depends_on_geometry(tau_b_ensemble, monkeypatch):
    ens, whole = tau_b_ensemble
    variants = np.arange(ens.model.hapNum) % 3
    assert whole.passes == 2                                                   # the prefix's walk, counted once, then all replicates
    assert_rows(whole, want_rows(ens, chains_of(ens), range(6), variants, 3), "default tile")

    def same(ms, rows, what):
        for k in FIELDS:
            x, y = getattr(ms, k), getattr(whole, k)[rows]
            assert x.dtype == y.dtype and (same_times(x, y) if k in TIME_FIELDS else np.array_equal(x, y)), (what, k)

    everyone = list(range(6))
    for tile in ("64", "4096", "1"):
        for waves in ("1", "4"):
            monkeypatch.setenv("VGX_TAU_MILESTONES_TILE_ROWS", tile)
            monkeypatch.setenv("VGX_TAU_MILESTONES_WAVES", waves)
            same(ens.tau_milestones(variants=variants, thresholds=THRESHOLDS), everyone, (tile, waves))
            monkeypatch.delenv("VGX_TAU_MILESTONES_TILE_ROWS")
            monkeypatch.delenv("VGX_TAU_MILESTONES_WAVES")
    order = [4, 0, 5, 2, 1]
    sub = ens.tau_milestones(variants=variants, thresholds=THRESHOLDS, replicates=order)
    assert list(sub.replicates) == order and sub.passes == 2
    same(sub, order, "subset")
    # chunks: budgets from too small for one replicate's tables, bases and slots (refused before any launch) upwards; the first
    # that fits the largest replicate holds less than two of its kind, so the five replicates go in several chunks
    from vgsim_amd import _capi
    for tile in ("64", "4096"):
        monkeypatch.setenv("VGX_TAU_MILESTONES_TILE_ROWS", tile)
        refused = 0
        for budget in (1500, 3000, 6000, 12000, 24000, 48000, 96000, 192000):
            monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", str(budget))
            try:
                split = ens.tau_milestones(variants=variants, thresholds=THRESHOLDS, replicates=order)
            except _capi.VgxError as err:
                assert "vgx_get_tau_milestones: replicate " in str(err) and "above the %d bytes of device memory the call may use" % budget in str(err)
                refused += 1
                continue
            break
        assert refused > 0 and 1 + 2 <= split.passes <= 1 + 5, (tile, budget, split.passes)   # the prefix once, then the chunks
        same(split, order, ("chunks", tile, budget))
    monkeypatch.delenv("VGX_TIMELINES_CHUNK_BYTES")
    monkeypatch.delenv("VGX_TAU_MILESTONES_TILE_ROWS")
    assert ens.tau_milestones(variants=variants, replicates=[]).final.shape == (0, ens.model.popNum + 1, 3)


def test_the_librarys_own_refusals():
    """Ensemble.tau_milestones checks its arguments before the library is called; these calls go to vgx_get_tau_milestones itself
    and return before any launch.  After every refused call a good one still works."""
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 3, seeds=np.array([3, 4, 5]))
    eng = ens.engine
    P, H = ens.model.popNum, ens.model.hapNum
    i32 = C.POINTER(C.c_int32)

    def call(reps=(0, 1, 2), pre=None, null_prefix=False, V=None, vo=None, thresholds=(1, 10)):
        reps, th = np.array(reps, dtype=np.int64), np.array(thresholds, dtype=np.int64)
        V = H if V is None else V
        vo = np.arange(H, dtype=np.int32) if vo is None else np.asarray(vo, dtype=np.int32)
        io = _capi.VgxTauMilestonesIO()
        final = np.zeros((len(reps), P + 1, max(V, 1)), dtype=np.int64)
        first = np.zeros((len(reps), max(len(th), 1), P + 1, max(V, 1)), dtype=np.int32)
        io.n, io.replicates, io.V, io.variant_of = len(reps), _capi._p(reps), V, vo.ctypes.data_as(i32)
        io.K, io.thresholds = len(th), _capi._p(th)
        io.final, io.first_event = _capi._p(final), first.ctypes.data_as(i32)      # (the other outputs stay NULL: not written)
        eng._check(eng.lib.vgx_get_tau_milestones(eng.handle, C.byref(io), None if null_prefix else C.byref(pre)))
        return final, first[:, :len(th)]

    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_milestones: the last call was not vgx_simulate_tau"):
        call(null_prefix=True)
    with pytest.raises(ValueError, match=r"tau_milestones\(\) walks tau chains only"):
        ens.tau_milestones()
    ens.simulate_tau(nt, sample_size=BIG, record_events=False)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_milestones: the last call recorded no multievent rows"):
        call(null_prefix=True)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    good = ens.tau_milestones(thresholds=(1, 10))
    assert good.reached.any() and np.array_equal(good.final[:, :P], ens.replicate_states_tau()[0])

    def still_works():
        final, first = call(pre=ens._tau_prefix_struct())
        assert np.array_equal(final, good.final) and np.array_equal(first, good.first_event)

    still_works()
    pre = ens._tau_prefix_struct()
    n_pre = int(pre.ev_ptr)
    assert n_pre > 1
    K = 2
    wide = (65536 - 16) // ((P + 1) * (40 + 4 * K)) + 1                        # the records just above the LDS budget
    need = (P + 1) * wide * (40 + 4 * K) + 16
    assert need > 65536 >= (P + 1) * (wide - 1) * (40 + 4 * K) + 16
    for kw, msg in ((dict(reps=(1, 1)), "replicates must be distinct"), (dict(reps=(0, 3)), "replicate index out of range"),
                    (dict(thresholds=range(17)), "K = 17 thresholds: at most 16"),
                    (dict(V=0), "V = 0 classes"), (dict(vo=[H] + [0] * (H - 1)), r"variant_of\[0\] = %d is outside \[-1, %d\)" % (H, H)),
                    (dict(V=wide, vo=[wide - 1] * H), r"%d populations \(and their total\) x %d classes x %d thresholds need %d bytes of records, above the 65536 "
                                                      "bytes of LDS" % (P, wide, K, need))):
        with pytest.raises(_capi.VgxError, match="vgx_get_tau_milestones: " + msg):
            call(pre=pre, **kw)
        still_works()
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_milestones: replicate 0: its chain continues a log of %d events, the prefix holds 0" % n_pre):
        call(null_prefix=True)
    pre.ev_ptr, pre.ev_types = n_pre, None
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_milestones: null prefix column"):
        call(pre=pre)
    still_works()
    with pytest.raises(ValueError, match=r"^milestones\(\) walks direct chains only: the last call was simulate_tau"):
        ens.milestones()
    still_works()
    ens.close()
