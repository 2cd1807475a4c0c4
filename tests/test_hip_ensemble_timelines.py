"""Ensemble.timelines(): the log replays get_data_infectious / get_data_susceptible of every replicate on the device
(vgx_get_timelines).  Expected values come from the CPU oracle run on the same model and seed and the literal restatement
oracle/timelines.py (never from the code under test); the 'compartment' semantics are checked against the engine's own final
state; plus every direct kernel's log, partly filled launches, subsets, query splits over several launches, refusals, and the
initial state read back after a first call."""
import numpy as np
import pytest

import helpers
import models

pytestmark = pytest.mark.gpu

STEPS = (100, 7)
# the case's own epidemic_time (7.3) gives 137 351 events on its seed; at 4.5 the ORACLE's chain on that seed (9) is stopped by the
# time limit after 1773 events (the other five seeds: 1222, 6737, 1208, 1460 and 1857)
TIME_STOP_LIMIT = 4.5


def _sim(name, seed=None):
    from vgsim_amd import Simulator
    ctor, phases = models.CASES[name]
    with helpers.quiet():
        sim = Simulator(**(ctor if seed is None else dict(ctor, seed=int(seed))))
        phases[0][0](sim)
    return sim, phases[0][1]


def _ensemble(name, seeds, n_max=3000, epidemic_time=-1, **kw):
    from vgsim_amd.ensemble import Ensemble
    sim, ph = _sim(name)
    ens = Ensemble(sim, len(seeds), seeds=np.asarray(seeds, dtype=np.int64))
    run = dict(iterations=min(ph["iterations"], n_max), epidemic_time=epidemic_time, attempts=ph.get("attempts", 200))
    with helpers.quiet():
        ens.simulate(run["iterations"], sample_size=10 ** 9, epidemic_time=epidemic_time, attempts=run["attempts"], record_events=True, **kw)
    return ens, run


def _oracle_model(oracle_mod, name, seed, run):
    sim, _ = _sim(name, seed)
    m = sim.simulation
    assert oracle_mod.run_direct(m, run["iterations"], 10 ** 9, run["epidemic_time"], run["attempts"]) == 0
    return m


def _seed_list(name):
    base = models.CASES[name][0]["seed"]
    return np.array([base, base + 1, base + 7, base + 100, 5, 123456789], dtype=np.int64)   # (test_hip_ensemble.py:26)


def _queries(m, n_inf, n_sus, seed=0):
    """Seeded compartments of model m's shape, the ones occupied at the end first."""
    rng = np.random.default_rng(seed)
    occ = [tuple(int(x) for x in ph) for ph in np.argwhere(m.infectious > 0)]
    rng.shuffle(occ)
    inf = occ[:n_inf // 2]
    while len(inf) < n_inf:
        inf.append((int(rng.integers(0, m.popNum)), int(rng.integers(0, m.hapNum))))
    sus = [(int(rng.integers(0, m.popNum)), int(rng.integers(0, m.susNum))) for _ in range(n_sus)]
    return inf, sus


def assert_rows_equal_oracle(tl, r, m, inf, sus, step_num, what):
    from oracle import timelines
    for k, (p, h) in enumerate(inf):
        data, sample, tp, ld = timelines.get_data_infectious(m, None, p, h, step_num)
        got = tl.data_infectious(r, k)
        assert got[0].dtype == data.dtype and np.array_equal(got[0], data), (what, r, "infectious", p, h, step_num)
        assert got[1].dtype == sample.dtype and np.array_equal(got[1], sample), (what, r, "sample", p, h, step_num)
        assert got[2] == tp, (what, r, "time_points", step_num)
        assert got[3] == ld, (what, r, "lockdowns", p)
    for k, (p, s) in enumerate(sus):
        data, tp, ld = timelines.get_data_susceptible(m, None, p, s, step_num)
        got = tl.data_susceptible(r, k)
        assert got[0].dtype == data.dtype and np.array_equal(got[0], data), (what, r, "susceptible", p, s, step_num)
        assert got[1] == tp and got[2] == ld, (what, r, "susceptible time_points / lockdowns", p)
    return sum(len(tl.lockdowns(r, p)) for p, _ in list(inf) + list(sus))   # lockdown records compared


@pytest.mark.parametrize("name", ["g9_short", "stress_h64", "c3_s5_p16", "p70", "extinct_restart", "time_stop"])
def test_batch_equals_oracle_replay(oracle_mod, name):
    seeds = _seed_list(name)
    kw = dict(n_max=10 ** 9, epidemic_time=TIME_STOP_LIMIT) if name == "time_stop" else {}
    ens, run = _ensemble(name, seeds, **kw)
    want = [_oracle_model(oracle_mod, name, s, run) for s in seeds]
    if name == "time_stop":
        assert 0 < want[0].events.ptr < 5000 and want[0].currentTime >= TIME_STOP_LIMIT   # stopped by the time limit (1773 events)
    inf, sus = _queries(want[0], 8, 4)
    locked = sorted({p for m in want for p in m.loc.populationsId})   # populations with lockdown records among the queried ones
    for i, p in enumerate(locked[:3]):
        inf[-1 - i] = (p, 0)
        sus[-1 - i] = (p, 0)
    lockdowns = 0
    for step_num in STEPS:
        tl = ens.timelines(infectious=inf, susceptible=sus, step_num=step_num)
        assert list(tl.replicates) == list(range(len(seeds))) and tl.infectious.shape == (len(seeds), 8, step_num + 1)
        for r, m in enumerate(want):
            lockdowns += assert_rows_equal_oracle(tl, r, m, inf, sus, step_num, name)
            assert tl.last_point[r] == (step_num if m.events.ptr else 0)
    if name == "p70":
        assert lockdowns > 0
    if name == "extinct_restart":
        assert all(m.events.ptr == 0 for m in want)   # empty chains: Data == [start, 0, ...]
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0
    ens.close()


def test_every_direct_kernels_log_is_read(oracle_mod):
    from vgsim_amd import _capi
    seeds = 100 + np.arange(4, dtype=np.int64)
    ran, want = set(), None
    for kernel in ("wave", "lane", "quad", "quadg", "solo", "lone"):
        try:
            ens, run = _ensemble("g5_short", seeds, n_max=2000, kernel=kernel)
        except _capi.VgxError as e:   # a kernel that does not take the model refuses the call (bad argument); anything else is a failure
            assert e.code == 1, (kernel, str(e))
            continue
        ran.add(ens.engine.last_kernel)
        if want is None:
            want = [_oracle_model(oracle_mod, "g5_short", s, run) for s in seeds]
            inf, sus = _queries(want[0], 8, 4)
        tl = ens.timelines(infectious=inf, susceptible=sus, step_num=50)
        for r, m in enumerate(want):
            assert_rows_equal_oracle(tl, r, m, inf, sus, 50, kernel)
        ens.close()
    assert {"wave", "quad", "quadg", "solo"} <= ran, ran


def _host_model(ens, r):
    """replicate_state(r) with the replicate's events and lockdowns attached (as Ensemble.genealogy builds its model)."""
    from vgsim_amd._model import Events, Lockdowns
    m = ens.replicate_state(r)
    chain = ens.replicate_events(r)
    ev = Events()
    ev.CreateEvents(max(chain.shape[1], 1))
    ev.times[:chain.shape[1]] = chain[0]
    for k, name in enumerate(ev.COLUMNS):
        getattr(ev, name)[:chain.shape[1]] = chain[k + 1].astype(np.int64)
    ev.ptr = chain.shape[1]
    m.events = ev
    m.loc = Lockdowns()
    for st, pp, tt in zip(*ens.engine.lockdowns(r)):
        m.loc.AddLockdown(st, pp, tt)
    return m


def test_philox_stream_clock():
    """mode='fast_philox': the clock must take the counter-based stream.  The oracle has no such stream, so the chain comes from
    replicate_events and the expected series from the oracle's replay of it."""
    seeds = 100 + np.arange(4, dtype=np.int64)
    ens, _ = _ensemble("g5_short", seeds, n_max=2000, mode="fast_philox")
    models_ = [_host_model(ens, r) for r in range(4)]
    inf, sus = _queries(models_[0], 8, 4)
    tl = ens.timelines(infectious=inf, susceptible=sus, step_num=50)
    for r, m in enumerate(models_):
        assert m.events.ptr > 0
        assert_rows_equal_oracle(tl, r, m, inf, sus, 50, "fast_philox")
    ens.close()


@pytest.mark.parametrize("name", ["stress_h64", "p70", "extinct_restart"])
def test_compartment_series_end_in_the_engines_final_state(name):
    ens, _ = _ensemble(name, _seed_list(name))
    states = [ens.replicate_state(r) for r in range(ens.R)]
    inf, sus = _queries(states[0], 8, 4)
    ref = ens.timelines(infectious=inf, susceptible=sus, step_num=20)
    tl = ens.timelines(infectious=inf, susceptible=sus, step_num=20, semantics="compartment")
    for r, st in enumerate(states):
        last = int(tl.last_point[r])
        for k, (p, h) in enumerate(inf):
            assert tl.infectious[r, k, last] == st.infectious[p, h], (name, r, p, h)
            assert (tl.infectious[r, k, last:] == tl.infectious[r, k, last]).all() and (tl.samples[r, k, last:] == tl.samples[r, k, last]).all()
        for k, (p, s) in enumerate(sus):
            assert tl.susceptible[r, k, last] == st.susceptible[p, s], (name, r, p, s)
            assert np.array_equal(tl.susceptible[r, k, :last + 1], ref.susceptible[r, k, :last + 1])
    ens.close()


def test_partial_launches_subsets_duplicates_and_splits(monkeypatch):
    R = 130
    ens, _ = _ensemble("g9_short", 7000 + np.arange(R, dtype=np.int64), n_max=1500)
    inf, sus = _queries(ens.replicate_state(0), 8, 4, seed=2)
    full = ens.timelines(infectious=inf, susceptible=sus, step_num=100)
    assert full.passes == 1
    for r in (0, 63, 64, 129):   # the batch against the product's host replay of the same replicate
        m = _host_model(ens, r)
        for k, (p, h) in enumerate(inf):
            data, sample, tp, ld = m.get_data_infectious(p, h, 100)
            got = full.data_infectious(r, k)
            assert np.array_equal(got[0], data) and np.array_equal(got[1], sample) and got[2] == tp and got[3] == ld
    order = np.random.default_rng(3).permutation(R)[:40]
    sub = ens.timelines(infectious=inf, susceptible=sus, step_num=100, replicates=order)
    assert list(sub.replicates) == list(order)
    for k in ("time_points", "infectious", "samples", "susceptible", "last_point"):
        assert np.array_equal(getattr(sub, k), getattr(full, k)[order]), k
    with pytest.raises(KeyError):
        sub.data_infectious(int(np.setdiff1d(np.arange(R), order)[0]), 0)
    # duplicate and empty query lists
    dup = ens.timelines(infectious=[inf[0], inf[1], inf[0]], susceptible=[sus[0], sus[0]], step_num=100)
    assert np.array_equal(dup.infectious[:, 0], full.infectious[:, 0]) and np.array_equal(dup.infectious[:, 2], full.infectious[:, 0])
    assert np.array_equal(dup.infectious[:, 1], full.infectious[:, 1]) and np.array_equal(dup.samples[:, 2], full.samples[:, 0])
    assert np.array_equal(dup.susceptible[:, 0], full.susceptible[:, 0]) and np.array_equal(dup.susceptible[:, 1], full.susceptible[:, 0])
    only_sus = ens.timelines(susceptible=sus, step_num=100)
    assert only_sus.infectious.shape == (R, 0, 101) and np.array_equal(only_sus.susceptible, full.susceptible)
    none = ens.timelines(step_num=100)
    assert none.susceptible.shape == (R, 0, 101) and none.passes == 0
    assert np.array_equal(none.time_points, full.time_points) and np.array_equal(none.last_point, full.last_point)
    # the queries split over several launches (the LDS budget knob), the replicates over several chunks
    whole = {"reference": full, "compartment": ens.timelines(infectious=inf, susceptible=sus, step_num=100, semantics="compartment")}
    monkeypatch.setenv("VGX_TIMELINES_LDS_BYTES", "4096")
    monkeypatch.setenv("VGX_TIMELINES_CHUNK_BYTES", "2000000")
    for semantics, one in whole.items():
        split = ens.timelines(infectious=inf, susceptible=sus, step_num=100, semantics=semantics)
        assert split.passes > 4 * one.passes
        for k in ("time_points", "infectious", "samples", "susceptible", "last_point"):
            assert np.array_equal(getattr(split, k), getattr(one, k)), (semantics, k)
    ens.close()


def test_thousand_steps_and_128_distinct_queries():
    """step_num = 1000 with 64 + 64 DISTINCT queries (p70: 70 x 4 infectious, 70 x 2 susceptible compartments): the counters exceed
    the LDS budget and the queries run as the 15 launches DESIGN.md §11 states (6 infectious + 1 susceptible series per launch of
    64 KiB, then 13 and 10 susceptible ones); equal to the per-replicate host replay."""
    ens, _ = _ensemble("p70", 40 + np.arange(4, dtype=np.int64))
    m0 = ens.replicate_state(0)
    rng = np.random.default_rng(4)
    occ = [tuple(int(x) for x in ph) for ph in np.argwhere(m0.infectious > 0)]
    rest = [(p, h) for p in range(m0.popNum) for h in range(m0.hapNum) if (p, h) not in set(occ)]
    inf = (occ + [rest[i] for i in rng.permutation(len(rest))])[:64]
    allsus = [(p, s) for p in range(m0.popNum) for s in range(m0.susNum)]
    sus = [allsus[i] for i in rng.permutation(len(allsus))[:64]]
    assert len(set(inf)) == 64 and len(set(sus)) == 64
    tl = ens.timelines(infectious=inf, susceptible=sus, step_num=1000)
    assert tl.passes == 15 and tl.infectious.shape == (4, 64, 1001) and tl.susceptible.shape == (4, 64, 1001)
    for r in range(4):
        m = _host_model(ens, r)
        for k, (p, h) in enumerate(inf):
            data, sample, tp, _ = m.get_data_infectious(p, h, 1000)
            assert np.array_equal(tl.infectious[r, k], data) and np.array_equal(tl.samples[r, k], sample), (r, p, h)
            assert tl.time_points[r].tolist() == tp
        for k, (p, s) in enumerate(sus):
            assert np.array_equal(tl.susceptible[r, k], m.get_data_susceptible(p, s, 1000)[0]), (r, p, s)
    ens.close()


def test_initial_state_is_read_back_after_a_first_call(oracle_mod):
    """The snapshot of the first call (pyx:435-448) reaches replicate_state(r) and, through the facade, the model."""
    from oracle import timelines
    name = "stress_h64"
    seeds = _seed_list(name)
    ens, run = _ensemble(name, seeds)
    inf, sus = None, None
    for r, s in enumerate(seeds):
        want = _oracle_model(oracle_mod, name, s, run)
        st = ens.replicate_state(r)
        assert want.initial_infectious.any() and want.initial_susceptible.any()
        assert np.array_equal(st.initial_infectious, want.initial_infectious) and np.array_equal(st.initial_susceptible, want.initial_susceptible)
        if inf is None:
            inf, sus = _queries(want, 8, 4)
            tl = ens.timelines(infectious=inf, susceptible=sus, step_num=100)
        m = _host_model(ens, r)   # the product's host path on the same replicate
        for k, (p, h) in enumerate(inf):
            data, sample, tp, ld = m.get_data_infectious(p, h, 100)
            got = tl.data_infectious(r, k)
            assert np.array_equal(got[0], data) and np.array_equal(got[1], sample) and got[2] == tp and got[3] == ld
        for k, (p, g) in enumerate(sus):
            data, tp, ld = m.get_data_susceptible(p, g, 100)
            got = tl.data_susceptible(r, k)
            assert np.array_equal(got[0], data) and got[1] == tp and got[2] == ld
    ens.close()
    # the facade: a first Simulator.simulate()
    sim, ph = _sim(name)
    with helpers.quiet():
        sim.simulate(3000, sample_size=10 ** 9)
    run = dict(iterations=3000, epidemic_time=-1, attempts=200)
    want = _oracle_model(oracle_mod, name, models.CASES[name][0]["seed"], run)
    m = sim.simulation
    assert np.array_equal(m.initial_infectious, want.initial_infectious) and np.array_equal(m.initial_susceptible, want.initial_susceptible)
    for p, g in sus:
        data, tp, ld = timelines.get_data_susceptible(want, None, p, g, 100)
        got = m.get_data_susceptible(p, g, 100)
        assert np.array_equal(got[0], data) and got[1] == tp and got[2] == ld


def test_refusals():
    from vgsim_amd import Simulator
    from vgsim_amd.ensemble import Ensemble
    sim, _ = _sim("g9_short")
    ens = Ensemble(sim, 2, seeds=np.array([3, 4]))
    with pytest.raises(ValueError, match="simulate"):
        ens.timelines(infectious=[(0, 0)])
    ens.close()
    ens, _ = _ensemble("g9_short", [3, 4], n_max=500)
    m = ens.model
    for kw, msg in ((dict(step_num=0), "step_num"), (dict(infectious=[(m.popNum, 0)]), "population index"),
                    (dict(infectious=[(0, m.hapNum)]), "haplotype index"), (dict(susceptible=[(0, m.susNum)]), "group index"),
                    (dict(susceptible=[(-1, 0)]), "population index"), (dict(replicates=[0, 2]), "out of range"),
                    (dict(replicates=[1, 1]), "distinct"), (dict(semantics="exact"), "semantics")):
        with pytest.raises(ValueError, match=msg):
            ens.timelines(**kw)
    with helpers.quiet():
        ens.simulate(500, sample_size=10 ** 9, record_events=False)
    with pytest.raises(ValueError, match="record_events"):
        ens.timelines(infectious=[(0, 0)])
    with helpers.quiet():
        ens.simulate_tau(20, sample_size=10 ** 12, record_events=True)
    with pytest.raises(ValueError, match="direct chains only"):
        ens.timelines(infectious=[(0, 0)])
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
        ens.timelines(infectious=[(0, 0)], replicates=late)
    ens.close()


def test_timelines_and_genealogies_do_not_disturb_each_other():
    ens, _ = _ensemble("g9_short", 100 + np.arange(6, dtype=np.int64))
    inf, sus = _queries(ens.replicate_state(0), 8, 4)
    keys = ("status", "node_offsets", "tree", "tree_pop", "times", "mut_offsets", "mut_node", "mut_time", "mig_offsets", "mig_node", "mig_time", "rng_raw")
    chains = [ens.replicate_events(r) for r in range(6)]
    before = ens.genealogies(seed=7)
    first = ens.timelines(infectious=inf, susceptible=sus, step_num=100)
    after = ens.genealogies(seed=7)
    second = ens.timelines(infectious=inf, susceptible=sus, step_num=100)
    for k in keys:
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    for k in ("time_points", "infectious", "samples", "susceptible", "last_point"):
        assert np.array_equal(getattr(first, k), getattr(second, k)), k
    for r in range(6):
        assert np.array_equal(ens.replicate_events(r), chains[r])
    ens.close()
