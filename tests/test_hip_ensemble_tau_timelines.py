"""Ensemble.tau_timelines(): the log replays get_data_infectious / get_data_susceptible of every replicate of a tau ensemble on the
device (vgx_get_tau_timelines).  The engine's tau chain is distributional, not oracle-identical, so the expected series are the
LITERAL replay (oracle/timelines.py) of the chain the engine itself recorded, assembled from read-outs that exist without this
feature: the model's events / multievents before the call (the prefix), replicate_events(r) and engine.multievents(r) (the
replicate's own steps, their row ranges shifted by the prefix's row count), the replicate's currentTime.  The 'compartment'
semantics are checked against replicate_states_tau().  No tolerance anywhere."""
import types

import numpy as np
import pytest

import helpers
import models
from test_hip_tau_trajectories import PATHS, warm

pytestmark = pytest.mark.gpu

SEEDS = np.array([3, 17, 101, 4242, 9, 77], dtype=np.int64)
EV_COLUMNS = ("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")
MEV_COLUMNS = ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")
B, D, SA, MU, SC, MI, MULTI = range(7)
KEYS = ("time_points", "infectious", "samples", "susceptible", "last_point")


def recorded_chain(ens, r, states):
    """(model-shaped object, multievent columns) of the whole chain of replicate r as the reference would hold it: the prefix (none
    for a replicate that restarted), then the replicate's MULTITYPE records.  Plain lists: the literal replay indexes them."""
    eng, m = ens.engine, ens.model
    c = eng.counters(r)
    restarted = c.restarts > 0
    n_pre = 0 if restarted else int(m.events.ptr)
    assert c.ev_first_new == n_pre
    k_pre = 0 if restarted else int(m.multievents.ptr)
    own = ens.replicate_events(r)[:, n_pre:]
    rows = eng.multievents(r)
    assert (own[1] == MULTI).all()
    ev = types.SimpleNamespace(ptr=n_pre + own.shape[1], times=m.events.times[:n_pre].tolist() + own[0].tolist())
    for j, name in enumerate(EV_COLUMNS):
        col = own[j + 1].astype(np.int64)
        if name in ("haplotypes", "populations"):
            col = col + k_pre                        # the MULTITYPE records' row ranges, behind the prefix's rows
        setattr(ev, name, getattr(m.events, name)[:n_pre].tolist() + col.tolist())
    mev = {name: getattr(m.multievents, name)[:k_pre].tolist() + rows[name].tolist() for name in MEV_COLUMNS}
    st, pp, tt = eng.lockdowns(r)
    loc = types.SimpleNamespace(states=([] if restarted else list(m.loc.states)) + [bool(x) for x in st],
                                populationsId=([] if restarted else list(m.loc.populationsId)) + [int(x) for x in pp],
                                times=([] if restarted else list(m.loc.times)) + [float(x) for x in tt])
    init = ens.replicate_state(r)
    host = types.SimpleNamespace(events=ev, currentTime=float(states[3][r]), initial_infectious=init.initial_infectious,
                                 initial_susceptible=init.initial_susceptible, loc=loc, restarted=restarted, own_steps=own.shape[1])
    return host, mev


def queries(ens, states, n_inf=8, n_sus=4, seed=0):
    """Seeded compartments, the ones occupied at the end of replicate 0 first; the first of each list is given twice."""
    m = ens.model
    rng = np.random.default_rng(seed)
    occ = [tuple(int(x) for x in ph) for ph in np.argwhere(states[0][0] > 0)]
    rng.shuffle(occ)
    inf = occ[:(n_inf - 1) // 2]
    while len(inf) < n_inf - 1:
        inf.append((int(rng.integers(0, m.popNum)), int(rng.integers(0, m.hapNum))))
    sus = [(int(rng.integers(0, m.popNum)), int(rng.integers(0, m.susNum))) for _ in range(n_sus)]
    return inf + [inf[0]], sus


def assert_equals_literal(tl, r, host, mev, inf, sus, step_num, what):
    from oracle import timelines
    done = {}
    for k, (p, h) in enumerate(inf):
        if (p, h) not in done:
            done[(p, h)] = timelines.get_data_infectious(host, mev, p, h, step_num)
        data, sample, tp, ld = done[(p, h)]
        got = tl.data_infectious(r, k)
        assert got[0].dtype == data.dtype and np.array_equal(got[0], data), (what, r, "infectious", p, h, step_num)
        assert got[1].dtype == sample.dtype and np.array_equal(got[1], sample), (what, r, "sample", p, h, step_num)
        assert got[2] == tp, (what, r, "time_points", step_num)
        assert got[3] == ld, (what, r, "lockdowns", p)
    for k, (p, s) in enumerate(sus):
        data, tp, ld = timelines.get_data_susceptible(host, mev, p, s, step_num)
        got = tl.data_susceptible(r, k)
        assert got[0].dtype == data.dtype and np.array_equal(got[0], data), (what, r, "susceptible", p, s, step_num)
        assert got[1] == tp and got[2] == ld, (what, r, "susceptible time_points / lockdowns", p)


def literal_last_point(host, step_num):
    """The grid index the reference's loop (pyx:1978-1981) ends at."""
    tp = [i * host.currentTime / step_num for i in range(step_num + 1)]
    point = 0
    for t in host.events.times:
        while point != step_num and tp[point] < t:
            point += 1
    return point


def assert_ends_in_state(tl, states, inf, sus, what):
    """'compartment': Data[last_point] is the final state replicate_states_tau() read, and is repeated after it."""
    for i, r in enumerate(tl.replicates):
        last = int(tl.last_point[i])
        for k, (p, h) in enumerate(inf):
            assert tl.infectious[i, k, last] == states[0][r, p, h], (what, r, "infectious", p, h)
            assert (tl.infectious[i, k, last:] == tl.infectious[i, k, last]).all() and (tl.samples[i, k, last:] == tl.samples[i, k, last]).all()
        for k, (p, s) in enumerate(sus):
            assert tl.susceptible[i, k, last] == states[1][r, p, s], (what, r, "susceptible", p, s)
            assert (tl.susceptible[i, k, last:] == tl.susceptible[i, k, last]).all()


def check_both(ens, what, steps=(100, 7, 1), replicates=None):
    """The two checks of every case: 'reference' == the literal replay of the recorded chain; 'compartment' ends in the final state."""
    states = ens.replicate_states_tau()
    inf, sus = queries(ens, states)
    reps = list(range(ens.R)) if replicates is None else list(replicates)
    chains = {r: recorded_chain(ens, r, states) for r in reps}
    for step_num in steps:
        tl = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=step_num, replicates=replicates)
        assert list(tl.replicates) == reps and tl.infectious.shape == (len(reps), len(inf), step_num + 1)
        for r in reps:
            host, mev = chains[r]
            assert_equals_literal(tl, r, host, mev, inf, sus, step_num, what)
            assert tl.last_point[tl._index(r)] == literal_last_point(host, step_num)
        comp = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=step_num, replicates=replicates, semantics="compartment")
        assert np.array_equal(comp.time_points, tl.time_points) and np.array_equal(comp.last_point, tl.last_point)
        assert_ends_in_state(comp, states, inf, sus, what)
    return chains


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["tau_a", "tau_b", "tau_c", "tau_d"])
def test_warm_up_cases_equal_the_literal_replay(name, path, monkeypatch):
    """A tau call that continues a direct warm-up, on both tau paths: step_num = 100 and 7 (wavefronts straddle cuts) and 1 (never)."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm(name)
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    chains = check_both(ens, name)
    assert all(host.own_steps > 1 and not host.restarted for host, _ in chains.values())
    assert ens.model.events.ptr > 0 and all(host.events.ptr == ens.model.events.ptr + host.own_steps for host, _ in chains.values())
    if name == "tau_d":   # the long warm-up switched population 0's lockdown on: the prefix's records come first
        tl = ens.tau_timelines(infectious=[(0, 0)], step_num=7)
        pre = [[bool(s), float(t)] for s, p, t in zip(ens.model.loc.states, ens.model.loc.populationsId, ens.model.loc.times) if p == 0]
        assert pre
        for r in range(ens.R):
            st, pp, tt = ens.engine.lockdowns(r)
            assert tl.lockdowns(r, 0) == pre + [[bool(s), float(t)] for s, p, t in zip(st, pp, tt) if p == 0]
    ens.close()


def _fresh(name):
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim, phases = models.build(Simulator, name)
        phases[0][0](sim)
    return sim


@pytest.mark.parametrize("path", sorted(PATHS))
def test_no_prefix(path, monkeypatch):
    """simulate_tau as the first call of a model with an empty log (index case): the chain is the replicate's steps alone."""
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _fresh("tau_c")
    assert sim.simulation.events.ptr == 0 and not sim.simulation.first_simulation
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(60, sample_size=10 ** 12, record_events=True)
    chains = check_both(ens, "no prefix")
    assert any(host.own_steps > 1 for host, _ in chains.values())
    assert all(host.events.ptr == host.own_steps for host, _ in chains.values())
    ens.close()


def _near_critical_warm():
    """The near-critical model of test_hip_tau_trajectories.py::test_restarts_rebin_the_final_attempt after a short direct warm-up:
    the model holds a prefix, and attempts that die out restart the replicate without it."""
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim = Simulator(number_of_sites=1, populations_number=1, seed=9)    # (on this seed 12 events leave 3 infected hosts)
        sim.set_transmission_rate(1.1); sim.set_recovery_rate(0.9); sim.set_sampling_rate(0.1)
        sim.simulate(12, sample_size=10 ** 9)
    assert sim.simulation.events.ptr == 12 and 0 < sim.simulation.infectious.sum() < 10
    return sim


@pytest.mark.parametrize("path", sorted(PATHS))
def test_restarted_replicates_have_no_prefix(path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim = _near_critical_warm()
    assert sim.simulation.events.ptr > 0
    ens = Ensemble(sim, 16, seeds=500 + np.arange(16, dtype=np.int64))
    res = ens.simulate_tau(300, sample_size=10 ** 12, attempts=4, record_events=True)
    assert res.restarts.max() > 0 and res.restarts.min() == 0, res.restarts
    chains = check_both(ens, "restart", steps=(100, 7))
    for r, (host, _) in chains.items():
        assert host.restarted == (res.restarts[r] > 0)
        assert host.events.ptr == host.own_steps + (0 if host.restarted else ens.model.events.ptr)
    ens.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_time_limit_and_empty_chains(path, monkeypatch):
    from vgsim_amd.ensemble import Ensemble
    monkeypatch.setenv("VGX_TAU_STEP_KERNELS", PATHS[path])
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 4, seeds=np.array([1, 2, 3, 4], dtype=np.int64))
    t0 = float(ens.model.currentTime)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    times = ens.replicate_states_tau()[3]
    steps_full = [int(ens.engine.counters(r).ev_ptr) for r in range(ens.R)]
    limit = float(np.float32(t0 + 0.5 * (float(times.min()) - t0)))
    ens.simulate_tau(nt, sample_size=10 ** 12, epidemic_time=limit, record_events=True)
    chains = check_both(ens, "time limit", steps=(100, 7))
    for r, (host, _) in chains.items():
        assert host.currentTime >= limit and 0 < host.own_steps and int(ens.engine.counters(r).ev_ptr) < steps_full[r]   # stopped by the limit
    # attempts = 0 on the warmed model: no step is recorded, the chain is the prefix alone
    ens.simulate_tau(nt, sample_size=10 ** 12, attempts=0, record_events=True)
    chains = check_both(ens, "no steps after a warm-up", steps=(7,))
    assert all(host.own_steps == 0 and host.events.ptr == ens.model.events.ptr for host, _ in chains.values())
    ens.close()
    # ... and on a model with an empty log: an empty chain, Data == [start, 0, ...] and last_point == 0
    sim = _fresh("tau_b")
    ens = Ensemble(sim, 3, seeds=np.array([1, 2, 3], dtype=np.int64))
    ens.simulate_tau(20, sample_size=10 ** 12, attempts=0, record_events=True)
    inf, sus = [(0, 0), (1, 3), (2, 5)], [(0, 0), (2, 1)]
    for semantics in ("reference", "compartment"):
        tl = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=9, semantics=semantics)
        for r in range(ens.R):
            st = ens.replicate_state(r)
            assert int(ens.engine.counters(r).ev_ptr) == 0 and tl.last_point[r] == 0
            for k, (p, h) in enumerate(inf):
                start = float(st.initial_infectious[p, h])
                assert tl.infectious[r, k].tolist() == [start] + [0.0 if semantics == "reference" else start] * 9
                assert not tl.samples[r, k].any()
            for k, (p, s) in enumerate(sus):
                start = float(st.initial_susceptible[p, s])
                assert tl.susceptible[r, k].tolist() == [start] + [0.0 if semantics == "reference" else start] * 9
    ens.close()


def test_forced_splits_and_subsets(monkeypatch):
    """The queries over several launches (VGX_TIMELINES_LDS_BYTES), the replicates over several chunks (VGX_TIMELINES_CHUNK_BYTES), a
    subset of replicates in non-ascending order: the results of the unsplit call."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    inf, sus = queries(ens, ens.replicate_states_tau())
    whole = {s: ens.tau_timelines(infectious=inf, susceptible=sus, step_num=100, semantics=s) for s in ("reference", "compartment")}
    assert whole["reference"].passes == 1
    order = [4, 0, 5, 2, 1]
    sub = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=100, replicates=order)
    assert list(sub.replicates) == order and sub.passes == 1
    for k in KEYS:
        assert np.array_equal(getattr(sub, k), getattr(whole["reference"], k)[order]), k
    with pytest.raises(KeyError):
        sub.data_infectious(3, 0)
    # 7 distinct infectious + 4 susceptible queries at step_num = 100: 8 (2 + 2 ni + ns) 101 + 4 (100 + 3 table) bytes per launch; 6000
    # bytes hold two infectious series or four susceptible ones: 4 + 1 launches per chunk; 16 624 bytes per replicate and 40 000 per
    # chunk: 2 replicates per chunk, 3 chunks of the 5 selected
    monkeypatch.setenv("VGX_TIMELINES_LDS_BYTES", "6000")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "40000")
    for semantics, one in whole.items():
        split = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=100, replicates=order, semantics=semantics)
        assert split.passes >= 6 and split.passes % 3 == 0, split.passes     # (15 when no two seeded queries coincide)
        for k in KEYS:
            assert np.array_equal(getattr(split, k), getattr(one, k)[order]), (semantics, k)
        for r in order:
            assert split.lockdowns(r, 0) == one.lockdowns(r, 0)
    ens.close()


def test_wide_counters_on_the_device(monkeypatch):
    """The model's multievent log extended by hand with num = 2^31 + 5, 2^31 + 5 and 3 * 2^30 in ONE bin, on a keyed counter and on
    the query-independent rows: the one place where the width of the LDS counters is observable."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    m = sim.simulation
    big = 2 ** 31 + 5
    nums = [big, big, 3 * 2 ** 30, big, big, 3 * 2 ** 30]
    kinds = [B, B, B, SA, SA, D]
    haps = [1, 1, 1, 2, 2, 2]
    k0 = int(m.multievents.ptr)
    m.multievents.extend([m.currentTime] * 6, num=nums, types=kinds, haplotypes=haps, populations=[1] * 6, newHaplotypes=[0] * 6,
                         newPopulations=[0] * 6)
    ev = m.events
    ev.CreateEvents(1)
    ev.times[ev.ptr], ev.types[ev.ptr], ev.haplotypes[ev.ptr], ev.populations[ev.ptr] = m.currentTime, MULTI, k0, k0 + 6
    ev.newHaplotypes[ev.ptr] = ev.newPopulations[ev.ptr] = 0
    ev.ptr += 1
    ens = Ensemble(sim, 2, seeds=SEEDS[:2])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    states = ens.replicate_states_tau()
    inf, sus = [(1, 1), (1, 2), (0, 0), (1, 1)], [(1, 0), (0, 0)]
    for step_num in (100, 1):
        tl = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=step_num)
        for r in range(2):
            host, mev = recorded_chain(ens, r, states)
            assert mev["num"][k0:k0 + 6] == nums
            assert_equals_literal(tl, r, host, mev, inf, sus, step_num, "wide counters")
        assert np.abs(tl.infectious).max() > 2 ** 32 and tl.samples.max() >= 2 * big
    ens.close()


def test_refusals():
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_c")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match="simulate_tau"):
        ens.tau_timelines(infectious=[(0, 0)])
    with helpers.quiet():
        ens.simulate(200, sample_size=10 ** 9, record_events=True)
    with pytest.raises(ValueError, match="tau chains only"):
        ens.tau_timelines(infectious=[(0, 0)])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.tau_timelines(infectious=[(0, 0)])
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True)
    m = ens.model
    for kw, msg in ((dict(step_num=0), "step_num"), (dict(infectious=[(m.popNum, 0)]), "population index"),
                    (dict(infectious=[(0, m.hapNum)]), "haplotype index"), (dict(susceptible=[(0, m.susNum)]), "group index"),
                    (dict(susceptible=[(-1, 0)]), "population index"), (dict(replicates=[0, 2]), "out of range"),
                    (dict(replicates=[1, 1]), "distinct"), (dict(semantics="exact"), "semantics")):
        with pytest.raises(ValueError, match=msg):
            ens.tau_timelines(**kw)
    with pytest.raises(ValueError, match="direct chains only"):
        ens.timelines(infectious=[(0, 0)])
    assert ens.tau_timelines(infectious=[(0, 0)], step_num=3).infectious.shape == (2, 1, 4)
    ens.close()


def test_read_outs_are_not_disturbed():
    """A tau_timelines() call between two trajectories() / replicate_multievents() read-outs does not change them."""
    from vgsim_amd.ensemble import Ensemble
    sim, nt = warm("tau_b")
    ens = Ensemble(sim, 6, seeds=SEEDS)
    t0 = float(ens.model.currentTime)
    ens.simulate_tau(nt, sample_size=10 ** 12, record_events=True, traj_points=17, traj_window=(t0 - 0.1, t0 + 2.0))
    traj = ens.trajectories()
    off, rows = ens.replicate_multievents()
    states = ens.replicate_states_tau()
    inf, sus = queries(ens, states)
    first = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=100)
    assert np.array_equal(ens.trajectories(), traj)
    off2, rows2 = ens.replicate_multievents()
    assert np.array_equal(off, off2) and all(np.array_equal(rows[k], rows2[k]) for k in rows)
    second = ens.tau_timelines(infectious=inf, susceptible=sus, step_num=100)
    for k in KEYS:
        assert np.array_equal(getattr(first, k), getattr(second, k)), k
    for a, b in zip(states, ens.replicate_states_tau()):
        assert np.array_equal(a, b)
    ens.close()
