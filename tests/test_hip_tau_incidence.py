"""Ensemble.tau_incidence(): event counts per time bin, population and channel of every replicate of a tau ensemble on the device
(vgx_get_tau_incidence), on both tau paths.  The engine's tau chain is distributional, not oracle-identical, so the expected
blocks are the literal restatement of the rule (test_tau_incidence_rule.restate_weighted) over the chain the engine itself
recorded, assembled from read-outs that exist without this feature (test_hip_ensemble_tau_timelines.recorded_chain: the model's
events / multievents before the call, replicate_events(r), engine.multievents(r) with their row ranges shifted; no prefix for a
restarted replicate).  The conservation check needs no restatement at all.  Every comparison is array_equal on integers.

Not covered here: the summary's refusal of a count of 2^31 or more cannot be reached by a run of a few seconds; int64 sums beyond
2^32 in one cell are covered by the CPU hook test (tests/test_tau_incidence_rule.py)."""
import numpy as np
import pytest

import helpers
from test_hip_ensemble_tau_timelines import EV_COLUMNS, SEEDS, _fresh, _near_critical_warm, recorded_chain
from test_hip_incidence import Q, assert_summary
from test_hip_tau_trajectories import PATHS, warm
from test_tau_incidence_rule import restate_weighted

pytestmark = pytest.mark.gpu

BINS = (100, 7, 1)
BIG = 10 ** 12


def chains_of(ens, reps=None):
    states = ens.replicate_states_tau()
    return {int(r): recorded_chain(ens, int(r), states) for r in (range(ens.R) if reps is None else reps)}


def want_block(ens, chains, reps, edges, haplotypes=None):
    got = []
    for r in reps:
        host, mev = chains[int(r)]
        events = [host.events.times] + [getattr(host.events, c) for c in EV_COLUMNS]
        got.append(restate_weighted(events, mev, ens.model.popNum, edges, haplotypes))
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def assert_equals(inc, counts, outside, what=""):
    assert inc.counts.dtype == np.int64 and inc.counts.shape == counts.shape, what
    assert np.array_equal(inc.counts, counts), what
    assert inc.outside.dtype == np.int64 and np.array_equal(inc.outside, outside), what


def final_times(ens):
    return ens.replicate_states_tau()[3]


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_warm_up_cases_equal_the_restatement(name, path, monkeypatch):
    """A tau call that continues a direct warm-up: the window runs from half of the prefix's last time to 0.9 of the latest final
    time, so prefix rows and own rows lie both inside and outside it."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    m = ens.model
    assert m.events.ptr > 0
    t_pre = float(m.events.times[m.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    chains = chains_of(ens)
    assert all(host.own_steps > 1 and not host.restarted for host, _ in chains.values())
    for bins in BINS:
        inc = ens.tau_incidence(bins=bins, window=window)
        assert_equals(inc, *want_block(ens, chains, range(6), inc.edges), what=(name, path, bins))
        assert inc.counts.any() and inc.outside.any() and inc.passes == 2
        assert np.array_equal(inc.new_infections(), inc.counts[..., 0] + inc.counts[..., 5])
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
    assert any(host.own_steps > 1 for host, _ in chains.values()) and all(host.events.ptr == host.own_steps for host, _ in chains.values())
    t_end = float(final_times(ens).max())
    for bins in (7, 1):
        inc = ens.tau_incidence(bins=bins, window=(0.2 * t_end, 0.8 * t_end))
        assert_equals(inc, *want_block(ens, chains, range(6), inc.edges), what=("no prefix", bins))
        assert inc.counts.any() and inc.passes == 1
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_restarted_replicates_have_no_prefix(path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _near_critical_warm()
    ens = Ensemble(sim, 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=BIG, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    chains = chains_of(ens)
    m = ens.model
    t_pre = float(m.events.times[m.events.ptr - 1])
    # the first bin holds the whole prefix and nothing else can lie before it; restarted chains start again at time 0
    edges = np.array([0.0, np.nextafter(t_pre, np.inf), 2.0 * t_pre + 1.0, 0.9 * float(final_times(ens).max()) + 2.0 * t_pre + 2.0])
    inc = ens.tau_incidence(edges=edges)
    assert_equals(inc, *want_block(ens, chains, range(16), edges), what="restart")
    pre = restate_weighted([m.events.times[:m.events.ptr]] + [getattr(m.events, c)[:m.events.ptr] for c in EV_COLUMNS],
                           {c: getattr(m.multievents, c) for c in ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")},
                           m.popNum, edges)[0]
    assert pre[0].sum() == m.events.ptr                     # twelve direct events, every one in some cell of bin 0
    for r in range(16):
        host, _ = chains[r]
        assert host.restarted == (res.restarts[r] > 0)
        k = host.events.ptr - host.own_steps                # the replicate's own steps alone (their row ranges index `mev` as they are)
        own = restate_weighted([host.events.times[k:]] + [getattr(host.events, c)[k:] for c in EV_COLUMNS], chains[r][1], m.popNum, edges)[0]
        # restarted replicates carry no prefix counts, the others carry the prefix's on top of their own
        assert np.array_equal(inc.counts[r], own if host.restarted else own + pre), r
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_own_steps(path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 4, seeds=np.array([1, 2, 3, 4], dtype=np.int64))
    ens.simulate_tau(nt, sample_size=BIG, attempts=0, record_events=True)     # no step is recorded: every chain is the prefix alone
    chains = chains_of(ens)
    assert all(host.own_steps == 0 and host.events.ptr == ens.model.events.ptr > 0 for host, _ in chains.values())
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    inc = ens.tau_incidence(bins=7, window=(0.3 * t_pre, 0.8 * t_pre))
    assert_equals(inc, *want_block(ens, chains, range(4), inc.edges), what="prefix alone")
    assert inc.counts[0].any() and inc.outside[0].all() and inc.passes == 1
    assert all(np.array_equal(inc.counts[r], inc.counts[0]) and np.array_equal(inc.outside[r], inc.outside[0]) for r in range(4))
    ens.close()
    sim = _fresh("tau_b")                                                      # ... and on an empty log: nothing at all
    ens = Ensemble(sim, 3, seeds=np.array([1, 2, 3], dtype=np.int64))
    ens.simulate_tau(20, sample_size=BIG, attempts=0, record_events=True)
    inc = ens.tau_incidence(bins=5, window=(0.0, 1.0), summary=dict(quantiles=(0.5,), method='lower'))
    assert inc.counts.shape == (3, 5, ens.model.popNum, 7) and not inc.counts.any() and not inc.outside.any() and inc.passes == 0
    assert not inc.summary.quantiles.any() and np.array_equal(inc.summary.count, [3])
    ens.close()


def test_tile_borders(monkeypatch):
    """Tiles of 64 and 257 rows against the default: every chain spans more than two tiles of 257 rows."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    for mult in (1, 2, 4, 8, 16):
        ens.simulate_tau(nt * mult, sample_size=BIG, record_events=True)
        own_rows = [len(ens.engine.multievents(r)["num"]) for r in range(6)]
        if min(own_rows) > 2 * 257:
            break
    assert min(own_rows) > 2 * 257, own_rows
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    chains = chains_of(ens)
    for bins in (100, 7):
        whole = ens.tau_incidence(bins=bins, window=window)
        assert_equals(whole, *want_block(ens, chains, range(6), whole.edges), what=("default tile", bins))
        for tile in ("64", "257"):
            monkeypatch.setenv("VGX_INCIDENCE_TILE_EVENTS", tile)
            inc = ens.tau_incidence(bins=bins, window=window)
            monkeypatch.delenv("VGX_INCIDENCE_TILE_EVENTS")
            assert_equals(inc, whole.counts, whole.outside, what=(tile, bins))
    ens.close()


@pytest.fixture(scope="module")
def tau_b_ensemble():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    yield ens, window, ens.tau_incidence(bins=100, window=window)
    ens.close()


def test_chunks_and_subsets(tau_b_ensemble, monkeypatch):
    ens, window, whole = tau_b_ensemble
    assert whole.passes == 2                                                   # the prefix, then all replicates
    order = [4, 0, 5, 2, 1]
    sub = ens.tau_incidence(bins=100, window=window, replicates=order)
    assert list(sub.replicates) == order and sub.passes == 2
    assert_equals(sub, whole.counts[order], whole.outside[order], what="subset")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "1000")                   # 101 cuts of 4 bytes + 64 per replicate: 2 per chunk
    split = ens.tau_incidence(bins=100, window=window, replicates=order)
    assert split.passes == 1 + 3
    assert_equals(split, whole.counts[order], whole.outside[order], what="chunks")


def test_haplotype_filter(tau_b_ensemble):
    ens, window, whole = tau_b_ensemble
    H = ens.model.hapNum
    occupied = sorted({int(h) for h in np.argwhere(ens.replicate_states_tau()[0][0] > 0)[:, 1]})
    absent = [h for h in range(H) if h not in occupied][:1]
    assert occupied and absent
    chains = chains_of(ens)
    inc = ens.tau_incidence(bins=7, window=window, haplotypes=occupied + absent)
    counts, outside = want_block(ens, chains, range(6), inc.edges, haplotypes=occupied + absent)
    assert_equals(inc, counts, outside, what="filter")
    assert 0 < inc.counts.sum() < whole.counts.sum() and np.array_equal(inc.outside, whole.outside)   # `outside` is unfiltered
    assert not inc.counts[..., 4].any()                                        # immunity changes carry no haplotype


@pytest.mark.parametrize("path", sorted(PATHS))
def test_whole_chain_window_conserves_the_infectious_totals(path, monkeypatch):
    """Independent of the restatement: births and arrivals minus deaths and samplings over the whole chain give the final totals."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm("tau_d")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    states = ens.replicate_states_tau()
    inc = ens.tau_incidence(bins=10, window=(0.0, float(np.nextafter(states[3].max(), np.inf))))
    assert not inc.outside.any() and inc.counts.any()
    for r in range(6):
        net = inc.counts[r].sum(axis=0)
        start = np.asarray(ens.replicate_state(r).initial_infectious, dtype=np.int64).sum(axis=1)
        assert np.array_equal(net[:, 0] + net[:, 5] - net[:, 1] - net[:, 2], states[0][r].sum(axis=1) - start), (path, r)
    ens.close()


def test_summary_in_the_same_call(tau_b_ensemble):
    ens, window, _ = tau_b_ensemble
    block = ens.tau_incidence(bins=9, window=window).counts
    assert block.max() < 2 ** 31 and np.ptp(block, axis=0).max() > 0
    by = np.array([0, 1, 0, 1, 0, 1])
    for method in ("lower", "higher", "linear"):
        band = ens.tau_incidence(bins=9, window=window, summary=dict(quantiles=Q, by=by, method=method), counts=False)
        assert band.counts is None and band.summary.method == method
        assert_summary(band.summary, block, by, 2, method)
    reps = np.array([5, 0, 2, 3])                                               # group_of follows the order of `replicates`
    band = ens.tau_incidence(bins=9, window=window, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.counts, block[reps]) and np.array_equal(band.summary.count, [2, 2])
    left = np.full(6, -1)
    left[reps] = by[reps]
    assert_summary(band.summary, block, left, 2, 'lower')
    one = ens.tau_incidence(bins=9, window=window, summary=dict(quantiles=Q, method='higher'))   # by='auto': one group
    assert_summary(one.summary, block, np.zeros(6, dtype=np.int64), 1, 'higher')


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match="simulate_tau"):
        ens.tau_incidence(edges=[0.0, 1.0])
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_incidence(edges=[0.0, 1.0])
    ens.simulate_tau(nt, sample_size=BIG, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_incidence(edges=[0.0, 1.0])
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    for kw, msg in ((dict(edges=[0.0, 1.0], replicates=[1, 1]), "distinct"), (dict(edges=[0.0, 1.0, 1.0]), "increase strictly"),
                    (dict(edges=[0.0, 2.0, 1.0]), "increase strictly"), (dict(edges=[0.0, 1.0], replicates=[0, 2]), "out of range")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_incidence(**kw)
    with pytest.raises(ValueError, match="incidence\\(\\) counts direct chains only: the last call was simulate_tau"):
        ens.incidence(edges=[0.0, 1.0])
    assert ens.tau_incidence(edges=[0.0, 1.0]).counts.shape == (2, 1, ens.model.popNum, 7)   # the ensemble stays usable
    ens.close()


def test_the_librarys_own_refusals():
    """Ensemble.tau_incidence checks its arguments before the library is called; these calls go to vgx_get_tau_incidence itself."""
    import ctypes as C

    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 3, seeds=np.array([3, 4, 5]))
    eng = ens.engine
    P = ens.model.popNum

    def call(reps=(0, 1, 2), edges=(0.0, 1.0, 2.0), pre=None, null_prefix=False):
        reps, edges = np.array(reps, dtype=np.int64), np.array(edges, dtype=np.float64)
        io = _capi.VgxTauIncidenceIO()
        block = np.zeros((len(reps), len(edges) - 1, P, 7), dtype=np.int64)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.edges = len(reps), _capi._p(reps), len(edges) - 1, _capi._p(edges)
        io.counts, io.outside = _capi._p(block), _capi._p(outside)
        eng._check(eng.lib.vgx_get_tau_incidence(eng.handle, C.byref(io), None if null_prefix else C.byref(pre)))
        return block, outside

    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_incidence: the last call was not vgx_simulate_tau"):
        call(null_prefix=True)
    ens.simulate_tau(nt, sample_size=BIG, record_events=False)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_incidence: the last call recorded no multievent rows"):
        call(null_prefix=True)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    pre = ens._tau_prefix_struct()
    n_pre = int(pre.ev_ptr)
    assert n_pre > 1
    for kw, msg in ((dict(reps=(1, 1)), "replicates must be distinct"), (dict(reps=(0, 3)), "replicate index out of range"),
                    (dict(edges=(0.0, 1.0, 1.0)), r"edges must increase strictly \(edges\[2\]\)"),
                    (dict(edges=(0.0, float("inf"))), r"edges\[1\] is not finite"), (dict(edges=(0.0,)), "T = 0 bins")):
        with pytest.raises(_capi.VgxError, match="vgx_get_tau_incidence: " + msg):
            call(pre=pre, **kw)
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_incidence: replicate 0: its chain continues a log of %d events, the prefix holds 0" % n_pre):
        call(null_prefix=True)
    pre.ev_ptr = n_pre - 1                                                     # a prefix of another length than ev_first_new
    with pytest.raises(_capi.VgxError, match="continues a log of %d events, the prefix holds %d" % (n_pre, n_pre - 1)):
        call(pre=pre)
    pre.ev_ptr, pre.ev_types = n_pre, None
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_incidence: null prefix column"):
        call(pre=pre)
    t_end = float(final_times(ens).max())                                      # the engine stays usable, and the plain call equals the method's
    block, outside = call(edges=(0.0, 0.5 * t_end, t_end), pre=ens._tau_prefix_struct())
    inc = ens.tau_incidence(edges=[0.0, 0.5 * t_end, t_end])
    assert block.any() and np.array_equal(block, inc.counts) and np.array_equal(outside, inc.outside)
    ens.close()
