"""Ensemble.flows(): new infections per time bin, source population, destination population and variant class of every replicate
on the device (vgx_get_flows).  Expected values come from the CPU oracle run on the same model and seed, or from the chain
replicate_events() gives (the route there was before), through the restatements of the rule in test_flows_rule.py, and for the
margins from Ensemble.incidence(); never from the code under test; every comparison is array_equal on integers."""
import ctypes as C

import numpy as np
import pytest

import helpers
import models
from test_flows_rule import MIGRATION, forms_that_fit, offdiagonal_pairs, restate, restate_sorted, variant_maps
from test_hip_ensemble_timelines import TIME_STOP_LIMIT, _ensemble, _oracle_model, _seed_list
from test_hip_incidence import edges_of, event_chain
from test_hip_param_sets import base_sim, scenarios_of
from test_incidence_rule import chain_of

pytestmark = pytest.mark.gpu

BINS = (100, 7)


def want_block(ens, reps, edges, vo, V, within=True):
    P = ens.model.popNum
    got = [restate_sorted(*event_chain(ens, int(r)), P, edges, vo, V, within) for r in reps]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def assert_equals(fl, counts, outside, what=""):
    assert fl.counts.dtype == np.int32 and fl.counts.shape == counts.shape, what
    assert np.array_equal(fl.counts, counts), what
    assert np.array_equal(fl.outside, outside), what


def no_mismatches(ens):
    return ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0


def case_map(ens):
    """every haplotype its own class where the dense table of that fits the LDS (small blocks), else the three classes with
    untracked haplotypes"""
    P, H = ens.model.popNum, ens.model.hapNum
    vo, V = variant_maps(H)["own" if 4 * P * P * H <= 65536 else "three"]
    return (None if V == H else vo), vo, V


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70", "extinct_restart", "time_stop"])
def test_batch_equals_restatement(oracle_mod, name):
    seeds = _seed_list(name)
    kw = dict(n_max=10 ** 9, epidemic_time=TIME_STOP_LIMIT) if name == "time_stop" else {}
    ens, run = _ensemble(name, seeds, **kw)
    P, H = ens.model.popNum, ens.model.hapNum
    want = [_oracle_model(oracle_mod, name, s, run) for s in seeds]
    chains = [chain_of(m) for m in want]
    t_end = max([float(m.currentTime) for m in want] + [1.0])
    window = (0.05 * t_end, 0.9 * t_end)
    variants, vo, V = case_map(ens)
    calls = [(variants, vo, V, bins, True) for bins in BINS] + [(np.zeros(H, dtype=np.int64), np.zeros(H, dtype=np.int32), 1, 7, False)]
    total = across = 0
    for variants, vo, V, bins, within in calls:
        fl = ens.flows(bins=bins, window=window, variants=variants, within=within)
        assert list(fl.replicates) == list(range(len(seeds))) and fl.counts.shape == (len(seeds), bins, P, P, V)
        assert np.array_equal(fl.edges, edges_of(bins, window)) and np.array_equal(fl.variant_of, vo)
        assert fl.form == forms_that_fit(P, V)[0]
        for r, (t, cols) in enumerate(chains):
            counts, outside = restate(t, cols, P, fl.edges, vo, V, within)
            assert np.array_equal(fl.counts[r], counts), (name, bins, V, r)
            assert np.array_equal(fl.outside[r], outside), (name, bins, V, r)
            total += int(counts.sum())
            across += int(counts.sum() - np.einsum('bppc->', counts))
    if name == "extinct_restart":
        assert total == 0 and sum(len(t) for t, _ in chains) == 0 and not fl.outside.any()   # empty chains: all zero
    else:
        assert total > 0 and fl.outside.any()
        assert (across > 0) == any((cols[0] == MIGRATION).any() for _, cols in chains)
    assert no_mismatches(ens)
    ens.close()


def test_p70_runs_dense_with_one_class_and_split_with_four(oracle_mod, monkeypatch):
    from vgsim_amd import _capi
    seeds = _seed_list("p70")[:3]
    ens, run = _ensemble("p70", seeds)
    P, H = ens.model.popNum, ens.model.hapNum
    assert (P, H) == (70, 4)
    chains = [chain_of(_oracle_model(oracle_mod, "p70", s, run)) for s in seeds]
    t_end = max(float(t[-1]) for t, _ in chains)
    edges = edges_of(20, (0.02 * t_end, 0.95 * t_end))
    maps = variant_maps(H)
    pairs = 0
    for key, form in (("one", "dense"), ("own", "split")):
        vo, V = maps[key]
        fl = ens.flows(edges=edges, variants=vo)
        assert fl.form == form and fl.passes == 1
        for r, (t, cols) in enumerate(chains):
            counts, outside = restate(t, cols, P, edges, vo, V)
            assert np.array_equal(fl.counts[r], counts) and np.array_equal(fl.outside[r], outside), (key, r)
            pairs = max(pairs, offdiagonal_pairs(counts))
        if key == "one":
            monkeypatch.setenv("VGX_FLOWS_FORM", "split")
            forced = ens.flows(edges=edges, variants=vo)
            assert forced.form == "split" and np.array_equal(forced.counts, fl.counts)
            monkeypatch.delenv("VGX_FLOWS_FORM")
    assert pairs >= 100                                           # scattered transmissions across: hundreds of distinct pairs
    monkeypatch.setenv("VGX_FLOWS_FORM", "dense")
    with pytest.raises(_capi.VgxError, match="vgx_get_flows: 70 populations x 4 classes need 78400 bytes of cells in the dense form"):
        ens.flows(edges=edges)
    monkeypatch.setenv("VGX_FLOWS_FORM", "sparse")
    with pytest.raises(_capi.VgxError, match="vgx_get_flows: VGX_FLOWS_FORM=sparse is neither dense nor split"):
        ens.flows(edges=edges)
    monkeypatch.delenv("VGX_FLOWS_FORM")
    assert np.array_equal(ens.flows(edges=edges).counts, fl.counts)   # ... and the ensemble counts again
    assert no_mismatches(ens)
    ens.close()


def test_tile_borders_in_both_forms(monkeypatch):
    """Several tiles in a chain of 2000 events: a lost flush at a tile border or a double count would show here."""
    ens, _ = _ensemble("g5_short", 100 + np.arange(4, dtype=np.int64), n_max=2000)
    H = ens.model.hapNum
    vo, V = variant_maps(H)["own"]
    t_end = max(float(ens.replicate_state(r).currentTime) for r in range(4))
    window = (0.02 * t_end, 0.95 * t_end)
    whole = ens.flows(bins=40, window=window)
    counts, outside = want_block(ens, range(4), whole.edges, vo, V)
    assert_equals(whole, counts, outside, "default tile")
    assert whole.form == "dense" and whole.counts.sum() > 1000
    for tile in (64, 257):
        monkeypatch.setenv("VGX_FLOWS_TILE_EVENTS", str(tile))
        for form in ("dense", "split"):
            monkeypatch.setenv("VGX_FLOWS_FORM", form)
            fl = ens.flows(bins=40, window=window)
            assert fl.form == form
            assert_equals(fl, counts, outside, (tile, form))
    assert no_mismatches(ens)
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
        vo, V = variant_maps(ens.model.hapNum)["three"]
        t_end = max(float(ens.replicate_state(r).currentTime) for r in range(4))
        fl = ens.flows(bins=25, window=(0.0, 0.9 * t_end), variants=vo)
        assert_equals(fl, *want_block(ens, range(4), fl.edges, vo, V), kernel)
        assert fl.counts.any() and no_mismatches(ens)
        ens.close()
    assert {"wave", "quad", "quadg", "solo"} <= ran, ran


def test_subsets_permutations_and_chunks(monkeypatch):
    R = 130
    ens, _ = _ensemble("g9_short", 7000 + np.arange(R, dtype=np.int64), n_max=1500)
    vo, V = variant_maps(ens.model.hapNum)["three"]
    t_end = max(float(ens.replicate_state(r).currentTime) for r in (0, 64, 129))
    edges = np.concatenate([[0.0], np.sort(np.random.default_rng(1).uniform(0.0, 0.8 * t_end, 30))])   # non-uniform
    full = ens.flows(edges=edges, variants=vo)
    assert full.passes == 1 and np.array_equal(full.edges, edges)
    some = [0, 63, 64, 129]
    counts, outside = want_block(ens, some, edges, vo, V)
    assert np.array_equal(full.counts[some], counts) and np.array_equal(full.outside[some], outside)
    assert counts.any()
    order = np.random.default_rng(3).permutation(R)[:40]
    sub = ens.flows(edges=edges, variants=vo, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_equals(sub, full.counts[order], full.outside[order], "subset")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "200000")
    for form in ("dense", "split"):
        monkeypatch.setenv("VGX_FLOWS_FORM", form)
        split = ens.flows(edges=edges, variants=vo)
        assert split.passes > 4 and split.form == form
        assert_equals(split, full.counts, full.outside, ("chunks", form))
    assert no_mismatches(ens)
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
            want = _summary_lerp(srt[rk[:len(Q)]], srt[rk[len(Q):]], np.asarray(Q).reshape((len(Q),) + (1,) * (block.ndim - 1)), m)
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
    vo, V = variant_maps(ens.model.hapNum)["three"]
    t_end = max(float(ens.replicate_state(r).currentTime) for r in range(8))
    window = (0.0, 0.9 * t_end)
    block, outside = want_block(ens, range(8), edges_of(9, window), vo, V)
    assert np.ptp(block[scenario_of == 0], axis=0).max() > 0 and block.sum() - np.einsum('rbppc->', block) > 0
    for method in ("lower", "linear"):
        call = dict(bins=9, window=window, variants=vo, summary=dict(quantiles=Q, by='auto', method=method))
        band = ens.flows(counts=False, **call)
        assert band.counts is None and band.summary.method == method and np.array_equal(band.outside, outside)
        assert_summary(band.summary, block, scenario_of, 2, method)
        both = ens.flows(**call)
        assert np.array_equal(both.counts, block)
        for k in ("quantiles", "count", "sum", "sumsq", "min", "max"):
            assert np.array_equal(getattr(both.summary, k), getattr(band.summary, k)), k
    # a subset in another order: the groups hold the selected replicates only
    reps = np.array([7, 0, 2, 5, 4])
    band = ens.flows(bins=9, window=window, variants=vo, replicates=reps, summary=dict(quantiles=Q, method='lower'))
    assert np.array_equal(band.counts, block[reps]) and np.array_equal(band.summary.count, [3, 2])
    left = np.full(8, -1)
    left[reps] = scenario_of[reps]
    assert_summary(band.summary, block, left, 2, 'lower')
    assert no_mismatches(ens)
    ens.close()


@pytest.mark.parametrize("name", ["stress_h64", "p70"])
def test_margins_are_the_channels_of_incidence_on_the_device(name):
    ens, _ = _ensemble(name, _seed_list(name))
    H = ens.model.hapNum
    t_end = max(float(ens.replicate_state(r).currentTime) for r in range(ens.R))
    edges = edges_of(12, (0.0, 0.95 * t_end))
    vo, V = variant_maps(H)["three"]
    fl = ens.flows(edges=edges, variants=vo)
    c = fl.counts.astype(np.int64)
    assert np.array_equal(fl.local(), np.einsum('rbppc->rbpc', c)) and np.array_equal(fl.new_infections(), c.sum(axis=2))
    assert np.array_equal(fl.imports(), c.sum(axis=2) - fl.local()) and np.array_equal(fl.exports(), c.sum(axis=3) - fl.local())
    arrivals = 0
    for k in range(V):
        inc = ens.incidence(edges=edges, haplotypes=np.flatnonzero(vo == k))
        assert np.array_equal(inc.outside, fl.outside)
        assert np.array_equal(fl.new_infections()[..., k], inc.new_infections()), (name, k)
        assert np.array_equal(fl.imports()[..., k], inc.counts[..., 5]), (name, k)
        assert np.array_equal(fl.exports()[..., k], inc.counts[..., 6]), (name, k)
        assert np.array_equal(fl.local()[..., k], inc.counts[..., 0]), (name, k)
        arrivals += int(inc.counts[..., 5].sum())
    assert arrivals > 0
    share = fl.imported_share()
    new = fl.new_infections()
    assert np.isnan(share).sum() == (new == 0).sum() and np.array_equal(share[new > 0], fl.imports()[new > 0] / new[new > 0])
    across = ens.flows(edges=edges, variants=vo, within=False)   # without the births: the same block with an empty diagonal
    off = c.copy()
    off[:, :, np.arange(c.shape[2]), np.arange(c.shape[2])] = 0
    assert np.array_equal(across.counts, off) and off.any()
    assert no_mismatches(ens)
    ens.close()


def test_refusals_leave_the_ensemble_usable():
    from vgsim_amd import Simulator, _capi
    from vgsim_amd.ensemble import Ensemble
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)
    eng = ens.engine
    P, H = ens.model.popNum, ens.model.hapNum
    edges = np.array([0.0, 0.5, 1.0])

    def library(reps=(0, 1), e=edges, vo=np.arange(H, dtype=np.int32), V=H):
        """vgx_get_flows itself, past the facade's checks"""
        io = _capi.VgxFlowsIO()
        reps = np.asarray(reps, dtype=np.int64)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        block = np.zeros((len(reps), len(e) - 1, P, P, V), dtype=np.int32)
        io.n, io.replicates, io.T, io.edges = len(reps), _capi._p(reps), len(e) - 1, _capi._p(np.ascontiguousarray(e, dtype=np.float64))
        io.V, io.variant_of, io.within = V, vo.ctypes.data_as(C.POINTER(C.c_int32)), 1
        io.counts, io.outside = block.ctypes.data_as(C.POINTER(C.c_int32)), _capi._p(outside)
        eng._check(eng.lib.vgx_get_flows(eng.handle, C.byref(io)))
        assert io.form == 1
        return block

    good = ens.flows(edges=edges)
    assert np.array_equal(library(), good.counts) and good.counts.any()
    for kw, text in ((dict(reps=(1, 1)), "vgx_get_flows: replicates must be distinct"), (dict(reps=(0, 2)), "vgx_get_flows: replicate index out of range"),
                     (dict(e=[0.0, 1.0, 1.0]), "vgx_get_flows: edges must increase"), (dict(e=[0.0, float("nan")]), "vgx_get_flows: edges.1. is not finite"),
                     (dict(V=0), "vgx_get_flows: V = 0 classes"), (dict(V=H - 1), r"vgx_get_flows: variant_of\[%d\] = %d is outside" % (H - 1, H - 1))):
        with pytest.raises(_capi.VgxError, match=text) as ei:
            library(**kw)
        assert ei.value.code == 1
        assert np.array_equal(ens.flows(edges=edges).counts, good.counts)
    with pytest.raises(ValueError, match="distinct"):
        ens.flows(edges=edges, replicates=[1, 1])
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.flows(edges=edges)
    with pytest.raises(_capi.VgxError, match="vgx_get_flows: the last call did not record events"):
        library()
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match="direct chains only"):
        ens.flows(edges=edges)
    with pytest.raises(_capi.VgxError, match="vgx_get_flows: the last call was vgx_simulate_tau"):
        library()
    ens.close()
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)   # ... and a fresh direct call counts again
    assert np.array_equal(ens.flows(edges=edges).counts, good.counts)
    assert no_mismatches(ens)
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
        ens.flows(edges=edges, replicates=late)
    eng = ens.engine
    with pytest.raises(_capi.VgxError, match="vgx_get_flows: replicate %d: its chain does not start" % late[0]):
        library(reps=late)
    ens.close()
