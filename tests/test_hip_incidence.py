"""Ensemble.incidence(): event counts per time bin, population and channel of every replicate on the device
(vgx_get_incidence).  Expected values come from the CPU oracle run on the same model and seed, or from the chain
replicate_events() gives (the route there was before), through the literal restatement of the rule in test_incidence_rule.py,
never from the code under test; every comparison is array_equal on integers."""
import ctypes as C

import numpy as np
import pytest

import helpers
import models
from test_hip_ensemble_timelines import TIME_STOP_LIMIT, _ensemble, _oracle_model, _seed_list
from test_hip_param_sets import base_sim, scenarios_of
from test_incidence_rule import chain_of, restate, restate_sorted

pytestmark = pytest.mark.gpu

BINS = (100, 7)


def edges_of(bins, window):
    t0, t1 = window
    return np.array([t0 + (k * (t1 - t0)) / bins for k in range(bins)] + [t1], dtype=np.float64)


def event_chain(ens, r):
    """(times, the five columns) of replicate r as replicate_events gives them."""
    a = ens.replicate_events(r)
    return a[0].copy(), [a[k].astype(np.int64) for k in range(1, 6)]


def want_block(ens, reps, edges, haplotypes=None):
    P = ens.model.popNum
    got = [restate_sorted(*event_chain(ens, int(r)), P, edges, haplotypes) for r in reps]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def assert_equals(inc, counts, outside, what=""):
    assert inc.counts.dtype == np.int32 and inc.counts.shape == counts.shape, what
    assert np.array_equal(inc.counts, counts), what
    assert np.array_equal(inc.outside, outside), what


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70", "extinct_restart", "time_stop"])
def test_batch_equals_restatement(oracle_mod, name):
    seeds = _seed_list(name)
    kw = dict(n_max=10 ** 9, epidemic_time=TIME_STOP_LIMIT) if name == "time_stop" else {}
    ens, run = _ensemble(name, seeds, **kw)
    want = [_oracle_model(oracle_mod, name, s, run) for s in seeds]
    t_end = max([float(m.currentTime) for m in want] + [1.0])
    window = (0.05 * t_end, 0.9 * t_end)
    events = 0
    for bins in BINS:
        inc = ens.incidence(bins=bins, window=window)
        assert list(inc.replicates) == list(range(len(seeds))) and inc.counts.shape == (len(seeds), bins, ens.model.popNum, 7)
        assert np.array_equal(inc.edges, edges_of(bins, window))
        for r, m in enumerate(want):
            t, cols = chain_of(m)
            counts, outside = restate(t, cols, m.popNum, inc.edges)
            assert np.array_equal(inc.counts[r], counts), (name, bins, r)
            assert np.array_equal(inc.outside[r], outside), (name, bins, r)
            events += len(t)
        assert np.array_equal(inc.new_infections(), inc.counts[..., 0] + inc.counts[..., 5])
    if name == "extinct_restart":
        assert events == 0 and not inc.counts.any() and not inc.outside.any()   # empty chains: all zero
    else:
        assert inc.counts.any() and inc.outside.any()
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0
    ens.close()


def test_tile_borders(monkeypatch):
    """Several tiles in a chain of 2000 events: a lost flush at a tile border or a double count would show here."""
    ens, _ = _ensemble("g5_short", 100 + np.arange(4, dtype=np.int64), n_max=2000)
    t_end = max(float(ens.replicate_state(r).currentTime) for r in range(4))
    window = (0.02 * t_end, 0.95 * t_end)
    whole = ens.incidence(bins=40, window=window)
    counts, outside = want_block(ens, range(4), whole.edges)
    assert_equals(whole, counts, outside, "default tile")
    assert whole.counts.sum() > 2000
    for tile in (64, 257):
        monkeypatch.setenv("VGX_INCIDENCE_TILE_EVENTS", str(tile))
        assert_equals(ens.incidence(bins=40, window=window), counts, outside, tile)
    ens.close()


def test_every_direct_kernels_log_is_read():
    from vgsim_amd import _capi
    seeds = 100 + np.arange(4, dtype=np.int64)
    ran = set()
    for kernel in ("wave", "lane", "quad", "quadg", "solo", "lone"):
        try:
            ens, run = _ensemble("g5_short", seeds, n_max=2000, kernel=kernel)
        except _capi.VgxError as e:   # a kernel that does not take the model refuses the call (bad argument); anything else is a failure
            assert e.code == 1, (kernel, str(e))
            continue
        ran.add(ens.engine.last_kernel)
        t_end = max(float(ens.replicate_state(r).currentTime) for r in range(4))
        inc = ens.incidence(bins=25, window=(0.0, 0.9 * t_end))
        assert_equals(inc, *want_block(ens, range(4), inc.edges), kernel)
        assert inc.counts.any()
        ens.close()
    assert {"wave", "quad", "quadg", "solo"} <= ran, ran


def test_subsets_permutations_and_chunks(monkeypatch):
    R = 130
    ens, _ = _ensemble("g9_short", 7000 + np.arange(R, dtype=np.int64), n_max=1500)
    t_end = max(float(ens.replicate_state(r).currentTime) for r in (0, 64, 129))
    edges = np.concatenate([[0.0], np.sort(np.random.default_rng(1).uniform(0.0, 0.8 * t_end, 30))])   # non-uniform
    full = ens.incidence(edges=edges)
    assert full.passes == 1 and np.array_equal(full.edges, edges)
    some = [0, 63, 64, 129]
    counts, outside = want_block(ens, some, edges)
    assert np.array_equal(full.counts[some], counts) and np.array_equal(full.outside[some], outside)
    order = np.random.default_rng(3).permutation(R)[:40]
    sub = ens.incidence(edges=edges, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_equals(sub, full.counts[order], full.outside[order], "subset")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "200000")
    split = ens.incidence(edges=edges)
    assert split.passes > 4
    assert_equals(split, full.counts, full.outside, "chunks")
    ens.close()


def test_haplotype_filter():
    ens, _ = _ensemble("stress_h64", _seed_list("stress_h64"))
    R, H = ens.R, ens.model.hapNum
    t_end = max(float(ens.replicate_state(r).currentTime) for r in range(R))
    edges = edges_of(12, (0.0, 0.95 * t_end))
    occupied = sorted({int(h) for h in np.argwhere(ens.replicate_state(0).infectious > 0)[:, 1]})   # ... at the end of replicate 0
    assert len(occupied) > 0
    inc = ens.incidence(edges=edges, haplotypes=occupied)
    assert_equals(inc, *want_block(ens, range(R), edges, occupied), "occupied")
    assert inc.counts.any()
    # a partition of all haplotypes into two masks: the sum is the unfiltered block but for the channel without a haplotype
    part = [h for h in range(H) if h % 3 == 1 or h == H - 1]
    rest = [h for h in range(H) if h not in part]
    a, b, whole = ens.incidence(edges=edges, haplotypes=part), ens.incidence(edges=edges, haplotypes=rest), ens.incidence(edges=edges)
    assert_equals(a, *want_block(ens, range(R), edges, part), "part")
    assert a.counts.any() and b.counts.any()
    keep = [0, 1, 2, 3, 5, 6]
    assert np.array_equal(a.counts[..., keep] + b.counts[..., keep], whole.counts[..., keep])
    assert not a.counts[..., 4].any() and not b.counts[..., 4].any()
    assert_equals(whole, *want_block(ens, range(R), edges), "unfiltered")
    ens.close()


Q = (0.0, 0.025, 0.3, 0.5, 0.975, 1.0)


def assert_summary(s, block, group_of, G, method):
    from vgsim_amd.ensemble import _summary_lerp, _summary_ranks
    assert s.quantiles.shape == (G, len(Q)) + block.shape[1:]
    for g in range(G):
        rows = block[np.asarray(group_of) == g].astype(np.int64)
        m = len(rows)
        assert s.count[g] == m and m > 0
        assert np.array_equal(s.sum[g], rows.sum(axis=0)) and np.array_equal(s.min[g], rows.min(axis=0)) and np.array_equal(s.max[g], rows.max(axis=0))
        assert np.array_equal(s.sumsq[g], (rows.astype(object) ** 2).sum(axis=0))
        if method == 'linear':
            srt = np.sort(rows, axis=0)
            rk = _summary_ranks(Q, m, 'linear')
            want = _summary_lerp(srt[rk[:len(Q)]], srt[rk[len(Q):]], np.asarray(Q).reshape(len(Q), 1, 1, 1), m)
        else:
            want = np.quantile(rows, Q, axis=0, method=method)
        assert np.array_equal(s.quantiles[g], want), (g, method)


def test_summary_per_scenario_without_the_block():
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    scenario_of = np.arange(8) % 2
    ens = Ensemble(base, 8, seeds=1000 + np.arange(8, dtype=np.int64), scenarios=scenarios_of(base)[:2], scenario_of=scenario_of)
    with helpers.quiet():
        ens.simulate(2000, sample_size=10 ** 9, attempts=20, record_events=True)
    t_end = max(float(ens.replicate_state(r).currentTime) for r in range(8))
    window = (0.0, 0.9 * t_end)
    block, _ = want_block(ens, range(8), edges_of(9, window))
    assert np.ptp(block[scenario_of == 0], axis=0).max() > 0
    for method in ("lower", "higher", "linear"):
        band = ens.incidence(bins=9, window=window, summary=dict(quantiles=Q, by='auto', method=method), counts=False)
        assert band.counts is None and band.summary.method == method
        assert_summary(band.summary, block, scenario_of, 2, method)
    # a subset in another order: the groups hold the selected replicates only
    reps = np.array([7, 0, 2, 5, 4])
    band = ens.incidence(bins=9, window=window, replicates=reps, summary=dict(quantiles=Q, method='lower'))
    assert np.array_equal(band.counts, block[reps]) and np.array_equal(band.summary.count, [3, 2])
    left = np.full(8, -1)
    left[reps] = scenario_of[reps]
    assert_summary(band.summary, block, left, 2, 'lower')
    ens.close()


def test_summary_of_a_group_of_65_takes_the_workgroup_form():
    """65 members is the smallest group the wavefront form (up to 64 keys) does not take: int32 input through the LDS sort."""
    R = 65
    ens, _ = _ensemble("g9_short", 500 + np.arange(R, dtype=np.int64), n_max=600)
    t_end = max(float(ens.replicate_state(r).currentTime) for r in (0, 1, 2))
    edges = edges_of(5, (0.0, 0.9 * t_end))
    inc = ens.incidence(edges=edges, summary=dict(quantiles=Q, method='higher'))
    block, outside = want_block(ens, range(R), edges)
    assert_equals(inc, block, outside)
    assert np.array_equal(inc.summary.count, [R])
    assert_summary(inc.summary, block, np.zeros(R, dtype=np.int64), 1, 'higher')
    ens.close()


@pytest.mark.parametrize("name", ["stress_h64", "p70"])
def test_whole_chain_window_conserves_the_infectious_totals(name):
    ens, _ = _ensemble(name, _seed_list(name))
    states = [ens.replicate_state(r) for r in range(ens.R)]
    t_end = max(float(st.currentTime) for st in states)
    inc = ens.incidence(bins=10, window=(0.0, np.nextafter(t_end, np.inf)))
    assert not inc.outside.any()
    for r, st in enumerate(states):
        net = inc.counts[r].sum(axis=0).astype(np.int64)
        start = np.asarray(st.initial_infectious, dtype=np.int64).sum(axis=1)
        assert np.array_equal(net[:, 0] + net[:, 5] - net[:, 1] - net[:, 2], np.asarray(st.totalInfectious, dtype=np.int64) - start), (name, r)
    ens.close()


def test_refusals_leave_the_ensemble_usable():
    from vgsim_amd import Simulator, _capi
    from vgsim_amd.ensemble import Ensemble
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)
    eng = ens.engine
    edges = np.array([0.0, 0.5, 1.0])

    def library(reps=(0, 1), e=edges):
        """vgx_get_incidence itself, past the facade's checks"""
        io = _capi.VgxIncidenceIO()
        reps = np.asarray(reps, dtype=np.int64)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        block = np.zeros((len(reps), len(e) - 1, ens.model.popNum, 7), dtype=np.int32)
        io.n, io.replicates, io.T, io.edges = len(reps), _capi._p(reps), len(e) - 1, _capi._p(np.ascontiguousarray(e, dtype=np.float64))
        io.counts, io.outside = block.ctypes.data_as(C.POINTER(C.c_int32)), _capi._p(outside)
        eng._check(eng.lib.vgx_get_incidence(eng.handle, C.byref(io)))
        return block

    good = ens.incidence(edges=edges)
    assert np.array_equal(library(), good.counts)
    for kw, text in ((dict(reps=(1, 1)), "vgx_get_incidence: replicates must be distinct"), (dict(reps=(0, 2)), "vgx_get_incidence: replicate index out of range"),
                     (dict(e=[0.0, 1.0, 1.0]), "vgx_get_incidence: edges must increase"), (dict(e=[0.0, float("nan")]), "vgx_get_incidence: edges.1. is not finite")):
        with pytest.raises(_capi.VgxError, match=text) as ei:
            library(**kw)
        assert ei.value.code == 1
        assert np.array_equal(ens.incidence(edges=edges).counts, good.counts)
    with pytest.raises(ValueError, match="distinct"):
        ens.incidence(edges=edges, replicates=[1, 1])
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.incidence(edges=edges)
    with pytest.raises(_capi.VgxError, match="vgx_get_incidence: the last call did not record events"):
        library()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match="direct chains only"):
        ens.incidence(edges=edges)
    with pytest.raises(_capi.VgxError, match="vgx_get_incidence: the last call was vgx_simulate_tau"):
        library()
    ens.close()
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)   # ... and a fresh direct call counts again
    assert np.array_equal(ens.incidence(edges=edges).counts, good.counts)
    ens.close()
    with helpers.quiet():   # a model that already holds events when the ensemble starts
        sim, phases = models.build(Simulator, "g9_short")
        phases[0][0](sim)
        sim.simulate(300)
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with helpers.quiet():
        ens.simulate(300, sample_size=10 ** 9, record_events=True)
    late = [r for r in range(2) if ens.engine.counters(r).ev_first_new != 0]   # (a replicate that restarted rewinds its log to 0)
    assert late
    with pytest.raises(ValueError, match="replicate %d: its chain does not start" % late[0]):
        ens.incidence(edges=edges, replicates=late)
    eng = ens.engine
    with pytest.raises(_capi.VgxError, match="vgx_get_incidence: replicate %d: its chain does not start" % late[0]):
        library(reps=late)
    ens.close()


def test_incidence_timelines_and_genealogies_do_not_disturb_each_other():
    ens, _ = _ensemble("g9_short", 100 + np.arange(6, dtype=np.int64))
    keys = ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_time", "mig_offsets", "mig_node", "mig_time", "rng_raw")
    tl_keys = ("time_points", "infectious", "samples", "susceptible", "last_point")
    chains = [ens.replicate_events(r) for r in range(6)]
    t_end = max(c[0, -1] for c in chains)
    call = dict(bins=20, window=(0.0, t_end), summary=dict(quantiles=(0.5,), method='lower'))
    inf, sus = [(0, 0), (1, 0)], [(0, 0)]
    g0 = ens.genealogies(seed=7)
    i0 = ens.incidence(**call)
    t0 = ens.timelines(infectious=inf, susceptible=sus, step_num=100)
    i1 = ens.incidence(**call)
    g1 = ens.genealogies(seed=7)
    i2 = ens.incidence(**call)
    t1 = ens.timelines(infectious=inf, susceptible=sus, step_num=100)
    for k in keys:
        assert np.array_equal(getattr(g0, k), getattr(g1, k)), k
    for k in tl_keys:
        assert np.array_equal(getattr(t0, k), getattr(t1, k)), k
    for other in (i1, i2):
        assert np.array_equal(i0.counts, other.counts) and np.array_equal(i0.outside, other.outside)
        assert np.array_equal(i0.summary.quantiles, other.summary.quantiles) and np.array_equal(i0.summary.sum, other.summary.sum)
    assert i0.counts.any()
    for r in range(6):
        assert np.array_equal(ens.replicate_events(r), chains[r])
    ens.close()
