"""Ensemble.tau_flows(): new infections per time bin, source population, destination population and variant class of every
replicate of a tau ensemble on the device (vgx_get_tau_flows), on both tau paths and in both forms of the counting workgroup's
table.  The engine's tau chain is distributional, not oracle-identical, so the expected blocks are the literal restatement of the
rule (test_tau_flows_rule.restate_weighted_flows) over the chain the engine itself recorded, assembled from read-outs that exist
without this feature (test_hip_ensemble_tau_timelines.recorded_chain); the margins come from Ensemble.tau_incidence().  Every
comparison is array_equal on integers.

Not covered here: the summary's refusal of a count of 2^31 or more cannot be reached by a run of a few seconds; int64 sums beyond
2^32 in one cell are covered by the CPU hook test (tests/test_tau_flows_rule.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import helpers
import models
from test_flows_rule import offdiagonal_pairs, variant_maps
from test_hip_ensemble_tau_timelines import EV_COLUMNS, SEEDS, _fresh, _near_critical_warm, recorded_chain
from test_hip_incidence import Q, assert_summary
from test_hip_tau_trajectories import PATHS, warm
from test_tau_flows_rule import flat_records, forms_that_fit, migrations_of, restate_weighted_flows

pytestmark = pytest.mark.gpu

BINS = (100, 7, 1)
BIG = 10 ** 12


def chains_of(ens, reps=None):
    """replicate -> (event columns, multievent columns, the flattened records) of its recorded chain"""
    states = ens.replicate_states_tau()
    out = {}
    for r in (range(ens.R) if reps is None else reps):
        host, mev = recorded_chain(ens, int(r), states)
        events = [host.events.times] + [getattr(host.events, c) for c in EV_COLUMNS]
        out[int(r)] = (events, mev, flat_records(events, mev), host)
    return out


def want_block(ens, chains, reps, edges, vo, V, within=True):
    got = [restate_weighted_flows(chains[int(r)][0], chains[int(r)][1], ens.model.popNum, edges, vo, V, within, flat=chains[int(r)][2]) for r in reps]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def assert_equals(fl, counts, outside, what=""):
    assert fl.counts.dtype == np.int64 and fl.counts.shape == counts.shape, what
    assert np.array_equal(fl.counts, counts), what
    assert fl.outside.dtype == np.int64 and np.array_equal(fl.outside, outside), what


def final_times(ens):
    return ens.replicate_states_tau()[3]


def across(block):
    """the summed counts off the diagonal of a [..., P, P, V] block"""
    return int(block.sum() - np.diagonal(block, axis1=-3, axis2=-2).sum())


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_b", "tau_c", "tau_d"])
def test_warm_up_cases_equal_the_restatement(name, path, monkeypatch):
    """A tau call that continues a direct warm-up: the window runs from half of the prefix's last time to 0.9 of the latest final
    time, so prefix rows and own rows lie both inside and outside it."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    m = ens.model
    P, H = m.popNum, m.hapNum
    assert m.events.ptr > 0 and P > 1
    t_pre = float(m.events.times[m.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    chains = chains_of(ens)
    assert all(c[3].own_steps > 1 and not c[3].restarted for c in chains.values())
    maps = variant_maps(H)
    for bins, key in zip(BINS, ("three", "own", "one")):
        vo, V = maps[key]
        fl = ens.tau_flows(bins=bins, window=window, variants=vo)
        assert_equals(fl, *want_block(ens, chains, range(6), fl.edges, vo, V), what=(name, path, bins))
        assert fl.form == forms_that_fit(P, V)[0] and fl.passes == 2 and np.array_equal(fl.variant_of, vo)
        assert across(fl.counts) > 0 and fl.outside.any()
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
    assert any(c[3].own_steps > 1 for c in chains.values()) and all(c[3].events.ptr == c[3].own_steps for c in chains.values())
    t_end = float(final_times(ens).max())
    vo, V = variant_maps(ens.model.hapNum)["own"]
    for bins in (7, 1):
        fl = ens.tau_flows(bins=bins, window=(0.2 * t_end, 0.8 * t_end))
        assert_equals(fl, *want_block(ens, chains, range(6), fl.edges, vo, V), what=("no prefix", bins))
        assert fl.counts.any() and fl.passes == 1
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
    assert m.popNum == 1
    vo, V = variant_maps(m.hapNum)["own"]
    t_pre = float(m.events.times[m.events.ptr - 1])
    # the first bin holds the whole prefix and nothing else can lie before it; restarted chains start again at time 0
    edges = np.array([0.0, np.nextafter(t_pre, np.inf), 2.0 * t_pre + 1.0, 0.9 * float(final_times(ens).max()) + 2.0 * t_pre + 2.0])
    fl = ens.tau_flows(edges=edges)
    assert_equals(fl, *want_block(ens, chains, range(16), edges, vo, V), what="restart")
    assert fl.counts.shape == (16, 3, 1, 1, V) and fl.counts.any()            # one population: every count lies on the diagonal
    pre_events = [m.events.times[:m.events.ptr]] + [getattr(m.events, c)[:m.events.ptr] for c in EV_COLUMNS]
    pre = restate_weighted_flows(pre_events, {c: getattr(m.multievents, c) for c in ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")},
                                 1, edges, vo, V)[0]
    assert pre[0].sum() == (np.asarray(pre_events[1]) == 0).sum() > 0 and not pre[1:].any()   # the births of the twelve direct events, in bin 0
    for r in range(16):
        events, mev, _, host = chains[r]
        assert host.restarted == (res.restarts[r] > 0)
        k = host.events.ptr - host.own_steps                # the replicate's own steps alone (their row ranges index `mev` as they are)
        own = restate_weighted_flows([c[k:] for c in events], mev, 1, edges, vo, V)[0]
        # restarted replicates carry no prefix counts, the others carry the prefix's on top of their own
        assert np.array_equal(fl.counts[r], own if host.restarted else own + pre), r
    ens.close()


def test_the_wide_model_runs_split_by_necessity(monkeypatch):
    """130 populations x 64 haplotypes: no dense table fits, and with every haplotype its own class not the diagonal either."""
    from vgsim_amd import Simulator, _capi
    from vgsim_amd.ensemble import Ensemble
    ctor, phases = models.tau_case("tau_wide_table")
    with helpers.quiet():
        sim = Simulator(**ctor)
        phases[0][0](sim)
        sim.simulate(**phases[0][1])
    assert sim.simulation.events.ptr == 4000
    ens = Ensemble(sim, 4, seeds=SEEDS[:4])
    ens.simulate_tau(20, sample_size=BIG, record_events=True)
    m = ens.model
    P, H = m.popNum, m.hapNum
    assert (P, H) == (130, 64)
    vo, V = variant_maps(H)["three"]
    assert forms_that_fit(P, V) == ["split"]
    chains = chains_of(ens)
    t_pre = float(m.events.times[m.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    fl = ens.tau_flows(bins=7, window=window, variants=vo)
    assert fl.form == "split" and fl.passes == 2
    counts, outside = want_block(ens, chains, range(4), fl.edges, vo, V)
    assert_equals(fl, counts, outside, "wide")
    assert offdiagonal_pairs(counts.sum(axis=0)) > 10 and outside.any()
    with pytest.raises(ValueError, match="130 populations x 64 classes need 66560 bytes of 8-byte cells in the split form"):
        ens.tau_flows(bins=7, window=window)
    monkeypatch.setenv("VGX_FLOWS_FORM", "dense")                              # the dense form forced where it does not fit
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: 130 populations x 3 classes need 405600 bytes of 8-byte cells in the dense form") as ei:
        ens.tau_flows(bins=7, window=window, variants=vo)
    assert ei.value.code == 1
    monkeypatch.delenv("VGX_FLOWS_FORM")
    again = ens.tau_flows(bins=7, window=window, variants=vo)                  # a later call counts again
    assert_equals(again, counts, outside, "after the refusal")
    # the library itself, past the facade
    io = _capi.VgxTauFlowsIO()
    reps, edges, own = np.arange(4, dtype=np.int64), np.ascontiguousarray(fl.edges), np.arange(H, dtype=np.int32)
    outside2 = np.zeros((4, 2), dtype=np.int64)
    io.n, io.replicates, io.T, io.edges = 4, _capi._p(reps), 7, _capi._p(edges)
    io.V, io.variant_of, io.within, io.counts, io.outside = H, own.ctypes.data_as(C.POINTER(C.c_int32)), 1, None, _capi._p(outside2)
    pre = ens._tau_prefix_struct()
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: 130 populations x 64 classes need 66560 bytes of 8-byte cells in the split form") as ei:
        ens.engine._check(ens.engine.lib.vgx_get_tau_flows(ens.engine.handle, C.byref(io), C.byref(pre)))
    assert ei.value.code == 1
    assert_equals(ens.tau_flows(bins=7, window=window, variants=vo), counts, outside, "after the library's refusal")
    ens.close()


def test_tile_borders_in_both_forms(monkeypatch):
    """Tiles of 64 and 257 rows against the default, in both forms: every chain spans several tiles."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    for mult in (1, 2, 4, 8, 16):
        ens.simulate_tau(nt * mult, sample_size=BIG, record_events=True)
        own_rows = [len(ens.engine.multievents(r)["num"]) for r in range(6)]
        if min(own_rows) > 1000:
            break
    assert min(own_rows) > 1000, own_rows
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    chains = chains_of(ens)
    vo, V = variant_maps(ens.model.hapNum)["three"]
    assert forms_that_fit(ens.model.popNum, V) == ["dense", "split"]
    for bins in (100, 7):
        whole = ens.tau_flows(bins=bins, window=window, variants=vo)
        assert whole.form == "dense"
        assert_equals(whole, *want_block(ens, chains, range(6), whole.edges, vo, V), what=("default tile", bins))
        assert across(whole.counts) > 0
        for form in ("dense", "split"):
            monkeypatch.setenv("VGX_FLOWS_FORM", form)
            for tile in ("64", "257", None):
                if tile is not None:
                    monkeypatch.setenv("VGX_FLOWS_TILE_EVENTS", tile)
                fl = ens.tau_flows(bins=bins, window=window, variants=vo)
                monkeypatch.delenv("VGX_FLOWS_TILE_EVENTS", raising=False)
                assert fl.form == form
                assert_equals(fl, whole.counts, whole.outside, what=(form, tile, bins))
            monkeypatch.delenv("VGX_FLOWS_FORM")
    ens.close()


def test_subsets_permutations_and_chunks(monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    R = 130
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, R, seeds=7000 + np.arange(R, dtype=np.int64))
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    vo, V = variant_maps(ens.model.hapNum)["three"]
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    t_end = float(final_times(ens).max())
    # non-uniform; 1501 cuts of 4 bytes + 64 per replicate: 32 replicates per chunk of 200000 bytes
    edges = np.concatenate([[0.5 * t_pre], np.sort(np.random.default_rng(1).uniform(0.5 * t_pre, 0.9 * t_end, 1500))])
    assert np.all(np.diff(edges) > 0)
    full = ens.tau_flows(edges=edges, variants=vo)
    assert full.passes == 2 and np.array_equal(full.edges, edges)
    some = [0, 63, 64, 129]
    counts, outside = want_block(ens, chains_of(ens, some), some, edges, vo, V)
    assert np.array_equal(full.counts[some], counts) and np.array_equal(full.outside[some], outside)
    assert across(counts) > 0
    order = np.random.default_rng(3).permutation(R)[:40]
    sub = ens.tau_flows(edges=edges, variants=vo, replicates=order)
    assert list(sub.replicates) == list(order)
    assert_equals(sub, full.counts[order], full.outside[order], "subset")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "200000")
    for form in ("dense", "split"):
        monkeypatch.setenv("VGX_FLOWS_FORM", form)
        split = ens.tau_flows(edges=edges, variants=vo)
        assert split.passes > 4 and split.form == form
        assert_equals(split, full.counts, full.outside, ("chunks", form))
    ens.close()


@pytest.fixture(scope="module")
def tau_b_ensemble():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    t_pre = float(ens.model.events.times[ens.model.events.ptr - 1])
    window = (0.5 * t_pre, 0.9 * float(final_times(ens).max()))
    yield ens, window
    ens.close()


def merged(block, summary=None):
    """test_hip_incidence.assert_summary takes columns of three axes: the block, or a summary over it, with (dst, class) as one axis
    (the summary is per column: merging axes changes no value)"""
    if summary is None:
        return block.reshape(block.shape[:3] + (-1,))
    view = types.SimpleNamespace(count=summary.count)
    for k in ("quantiles", "sum", "sumsq", "min", "max"):
        v = getattr(summary, k)
        setattr(view, k, v.reshape(v.shape[:-2] + (-1,)))
    return view


def test_summary_in_the_same_call(tau_b_ensemble):
    ens, window = tau_b_ensemble
    vo, _ = variant_maps(ens.model.hapNum)["three"]
    block = ens.tau_flows(bins=9, window=window, variants=vo).counts
    assert block.max() < 2 ** 31 and np.ptp(block, axis=0).max() > 0 and across(block) > 0
    by = np.array([0, 1, 0, 1, 0, 1])
    for method in ("lower", "higher", "linear"):
        band = ens.tau_flows(bins=9, window=window, variants=vo, summary=dict(quantiles=Q, by=by, method=method), counts=False)
        assert band.counts is None and band.summary.method == method
        assert_summary(merged(block, band.summary), merged(block), by, 2, method)
    reps = np.array([5, 0, 2, 3])                                               # group_of follows the order of `replicates`
    band = ens.tau_flows(bins=9, window=window, variants=vo, replicates=reps, summary=dict(quantiles=Q, by=by, method='lower'))
    assert np.array_equal(band.counts, block[reps]) and np.array_equal(band.summary.count, [2, 2])
    left = np.full(6, -1)
    left[reps] = by[reps]
    assert_summary(merged(block, band.summary), merged(block), left, 2, 'lower')
    one = ens.tau_flows(bins=9, window=window, variants=vo, summary=dict(quantiles=Q, method='higher'))   # by='auto': one group
    assert_summary(merged(block, one.summary), merged(block), np.zeros(6, dtype=np.int64), 1, 'higher')


def test_margins_are_the_channels_of_tau_incidence_on_the_device(tau_b_ensemble):
    ens, window = tau_b_ensemble
    vo, V = variant_maps(ens.model.hapNum)["three"]
    fl = ens.tau_flows(bins=12, window=window, variants=vo)
    c = fl.counts
    assert np.array_equal(fl.local(), np.einsum('rbppc->rbpc', c)) and np.array_equal(fl.new_infections(), c.sum(axis=2))
    assert np.array_equal(fl.imports(), c.sum(axis=2) - fl.local()) and np.array_equal(fl.exports(), c.sum(axis=3) - fl.local())
    # no MIGRATION of the recorded chains has equal keys: the diagonal is the births alone
    assert all(migrations_of(ch[2])[2] == 0 and migrations_of(ch[2])[0] > 0 for ch in chains_of(ens).values())
    arrivals = 0
    for k in range(V):
        inc = ens.tau_incidence(edges=fl.edges, haplotypes=np.flatnonzero(vo == k))
        assert np.array_equal(inc.outside, fl.outside)
        assert np.array_equal(fl.new_infections()[..., k], inc.new_infections()), k
        assert np.array_equal(fl.imports()[..., k], inc.counts[..., 5]), k
        assert np.array_equal(fl.exports()[..., k], inc.counts[..., 6]), k
        assert np.array_equal(fl.local()[..., k], inc.counts[..., 0]), k
        arrivals += int(inc.counts[..., 5].sum())
    assert arrivals > 0
    share, new = fl.imported_share(), fl.new_infections()
    assert np.isnan(share).sum() == (new == 0).sum() and np.array_equal(share[new > 0], fl.imports()[new > 0] / new[new > 0])
    only = ens.tau_flows(edges=fl.edges, variants=vo, within=False)            # without the births: the same block with an empty diagonal
    off = c.copy()
    off[:, :, np.arange(c.shape[2]), np.arange(c.shape[2])] = 0
    assert np.array_equal(only.counts, off) and off.any() and np.array_equal(only.outside, fl.outside)


def test_refusals_leave_the_ensemble_usable(monkeypatch):
    """Argument errors returned before any launch: vgx_get_tau_flows itself past the facade, and the facade's own."""
    from vgsim_amd import _capi
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 3, seeds=np.array([3, 4, 5]))
    eng = ens.engine
    P, H = ens.model.popNum, ens.model.hapNum

    def library(reps=(0, 1, 2), e=(0.0, 1.0, 2.0), vo=np.arange(H, dtype=np.int32), V=H, pre=None, null_prefix=False):
        reps, e = np.array(reps, dtype=np.int64), np.array(e, dtype=np.float64)
        io = _capi.VgxTauFlowsIO()
        block = np.zeros((len(reps), max(len(e) - 1, 1), P, P, max(V, 1)), dtype=np.int64)
        outside = np.zeros((len(reps), 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.edges = len(reps), _capi._p(reps), len(e) - 1, _capi._p(e)
        io.V, io.variant_of, io.within = V, vo.ctypes.data_as(C.POINTER(C.c_int32)), 1
        io.counts, io.outside = _capi._p(block), _capi._p(outside)
        eng._check(eng.lib.vgx_get_tau_flows(eng.handle, C.byref(io), None if null_prefix else C.byref(pre if pre is not None else ens._tau_prefix_struct())))
        assert io.form == 1
        return block, outside

    with pytest.raises(ValueError, match="simulate_tau"):
        ens.tau_flows(edges=[0.0, 1.0])
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_flows(edges=[0.0, 1.0])
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: the last call was not vgx_simulate_tau") as ei:
        library(null_prefix=True)
    assert ei.value.code == 1
    ens.simulate_tau(nt, sample_size=BIG, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_flows(edges=[0.0, 1.0])
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: the last call recorded no multievent rows"):
        library(null_prefix=True)
    ens.simulate_tau(nt, sample_size=BIG, record_events=True)
    t_end = float(final_times(ens).max())
    edges = (0.0, 0.5 * t_end, t_end)
    good = ens.tau_flows(edges=edges)
    assert good.counts.any() and across(good.counts) > 0
    block, outside = library(e=edges)                                          # the plain call equals the method's
    assert np.array_equal(block, good.counts) and np.array_equal(outside, good.outside)
    n_pre = int(ens._tau_prefix_struct().ev_ptr)
    assert n_pre > 1
    for kw, text in ((dict(reps=(1, 1)), "replicates must be distinct"), (dict(reps=(0, 3)), "replicate index out of range"),
                     (dict(e=(0.0, 1.0, 1.0)), r"edges must increase strictly \(edges\[2\]\)"), (dict(e=(0.0, 2.0, 1.0)), "edges must increase strictly"),
                     (dict(e=(0.0, float("nan"))), r"edges\[1\] is not finite"), (dict(e=(0.0,)), "T = 0 bins"),
                     (dict(V=0), "V = 0 classes"), (dict(V=H - 1), r"variant_of\[%d\] = %d is outside \[-1, %d\)" % (H - 1, H - 1, H - 1)),
                     (dict(null_prefix=True), "replicate 0: its chain continues a log of %d events, the prefix holds 0" % n_pre)):
        with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: " + text) as ei:
            library(**kw)
        assert ei.value.code == 1
        assert np.array_equal(ens.tau_flows(edges=edges).counts, good.counts)  # after each refusal a good call returns the earlier block
    pre = ens._tau_prefix_struct()
    pre.ev_types = None
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: null prefix column"):
        library(pre=pre)
    monkeypatch.setenv("VGX_FLOWS_FORM", "sparse")
    with pytest.raises(_capi.VgxError, match="vgx_get_tau_flows: VGX_FLOWS_FORM=sparse is neither dense nor split"):
        ens.tau_flows(edges=edges)
    monkeypatch.delenv("VGX_FLOWS_FORM")
    for kw, text in ((dict(replicates=[1, 1]), "distinct"), (dict(replicates=[0, 3]), "out of range")):
        with pytest.raises(ValueError, match=text):
            ens.tau_flows(edges=edges, **kw)
    with pytest.raises(ValueError, match="flows\\(\\) counts direct chains only: the last call was simulate_tau"):
        ens.flows(edges=[0.0, 1.0])
    again = ens.tau_flows(edges=edges)
    assert np.array_equal(again.counts, good.counts) and np.array_equal(again.outside, good.outside)
    ens.close()
