"""Scenario ensembles on the GPU (vgx_set_param_sets, the scenario entry points of vgx_direct.hip): G parameter sets over one start
state in one launch.  Every replicate must be, bit for bit, the run of the CPU oracle on its own scenario's model with its own seed.

The model family is small (2 sites, 3 populations, 2 susceptibility groups, 400 hosts per population) and still reaches what can
go wrong per set: lockdown switches, failed attempts and Restart (list classes restored from the set's own table), extinction,
attempts used up, mutation, immunity loss and migration, different class counts and class numbers per haplotype between sets."""
import copy
import functools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SEEDS = [1000, 1001, 1002, 1003]
N_EVENTS, ATTEMPTS = 2000, 20
STATE = ("infectious", "susceptible", "lockdownON", "contactDensity")


def base_sim():
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim = Simulator(number_of_sites=2, populations_number=3, number_of_susceptible_groups=2, seed=1)
    sim.set_transmission_rate(1.8); sim.set_recovery_rate(1.0); sim.set_sampling_rate(0.1)
    sim.set_population_size(400); sim.set_migration_probability(0.05); sim.set_mutation_rate(0.05)
    sim.set_susceptibility_type(1); sim.set_susceptibility(0.3, susceptibility_type=1)
    sim.set_immunity_transition(0.05, source=1, target=0); sim.set_npi([0.2, 0.02, 0.004])
    return sim


def scenarios_of(base):
    """Deep copies of ``base`` (parameters and state) as scenarios A to D."""
    a, b, c, d = (copy.deepcopy(base) for _ in range(4))
    b.set_transmission_rate(2.6, haplotype=0)
    b.set_recovery_rate(0.8, haplotype=5)
    b.set_susceptibility(0.5, susceptibility_type=1, haplotype=2)
    c.set_npi([0.5, 0.05, 0.01], population=0)
    c.set_npi([0.1, 0.01, 0.002], population=2)
    c.set_migration_probability(0.1, source=1, target=2)
    c.set_sampling_multiplier(3.0, population=0)
    c.set_mutation_rate(0.2)
    d.set_transmission_rate(0.9)
    return [a, b, c, d]


def oracle_run(oracle_mod, sim, seed, iterations):
    """The oracle's run of a deep copy of ``sim`` under ``seed``; returns the copy (a Simulator)."""
    one = copy.deepcopy(sim)
    one.simulation.user_seed = int(seed)
    assert oracle_mod.run_direct(one.simulation, iterations, 10 ** 9, -1, ATTEMPTS) == 0
    return one


@functools.lru_cache(maxsize=None)
def reference(oracle_mod):
    """want[g][k]: scenario g under SEEDS[k], run once by the oracle and shared (never changed) by the tests below."""
    scen = scenarios_of(base_sim())
    return [[oracle_run(oracle_mod, s, seed, N_EVENTS) for seed in SEEDS] for s in scen]


def assert_replicate_equals(ens, r, want, what, first=0):
    m = want.simulation
    n = m.events.ptr
    assert ens.engine.counters(r).ev_ptr == n, (what, "events.ptr")
    chain = ens.replicate_events(r)
    assert chain.shape == (6, n)
    assert np.array_equal(chain[:, first:], m.events.as_array()[:, first:n]), \
        (what, helpers.describe_first_diff(chain[:, first:], m.events.as_array()[:, first:n], n - first))
    st = ens.replicate_state(r)
    for k in m.COUNTERS + ("good_attempt",):
        assert getattr(st, k) == getattr(m, k), (what, k, getattr(st, k), getattr(m, k))
    for k in STATE:
        assert np.array_equal(getattr(st, k), getattr(m, k)), (what, k)
    assert st.currentTime == m.currentTime, (what, "currentTime")
    return st


def run_ensemble(scenario_of):
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    ens = Ensemble(base, 16, seeds=np.array(SEEDS * 4, dtype=np.int64), scenarios=scenarios_of(base), scenario_of=scenario_of)
    res = ens.simulate(N_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
    return ens, res


BLOCK, CYCLE = np.repeat(np.arange(4), 4), np.arange(16) % 4


@pytest.mark.parametrize("scenario_of", [BLOCK, CYCLE], ids=["block", "cycle"])
def test_replicates_equal_the_oracle_of_their_own_scenario(oracle_mod, scenario_of):
    want = reference(oracle_mod)
    if scenario_of is BLOCK:
        # what the family is there to reach, on the oracle's own results (an edit of the models must not lose it silently)
        for g in range(4):
            ms = [w.simulation for w in want[g]]
            assert any(m.swapLockdown > 0 for m in ms), g
            assert any(m.good_attempt > 1 for m in ms), g
            assert any(m.events.ptr < N_EVENTS for m in ms), g
            assert any(m.mCounter > 0 for m in ms) and any(m.iCounter > 0 for m in ms) and any(m.migPlus > 0 for m in ms), g
        for k in (1, 2):   # D, seeds 1001 and 1002: every attempt fails
            assert want[3][k].simulation.events.ptr == 0 and want[3][k].simulation.good_attempt == 0
        rows = [len(np.unique(np.column_stack([w[0].simulation.bRate, w[0].simulation.dRate, w[0].simulation.susceptibility]), axis=0))
                for w in want]
        assert rows[0] == 1 and rows[1] == 4    # B has other rate classes, and other class numbers per haplotype, than A
    ens, res = run_ensemble(scenario_of)
    assert ens.engine.last_kernel == "wave"
    assert np.array_equal(ens.scenario_of, scenario_of)
    for r in range(16):
        g, k = int(scenario_of[r]), r % 4
        st = assert_replicate_equals(ens, r, want[g][k], "replicate %d (scenario %d, seed %d)" % (r, g, SEEDS[k]))
        assert res.events[r] == want[g][k].simulation.events.ptr
        assert np.array_equal(st.bRate, want[g][k].simulation.bRate) and st is not ens.scenarios[g]   # a copy of its scenario's model
    ens.close()


def test_start_state_with_set_dependent_list_classes(oracle_mod):
    """A start state in which a haplotype whose class number differs between the sets (3: class 0 in A, 1 in B) occupies every
    population, a lockdown is on and the contact densities differ: the lists' classes must come from every replicate's own set."""
    from vgsim_amd.ensemble import Ensemble
    base = base_sim()
    m = base.simulation
    m.user_seed = 1001
    assert oracle_mod.run_direct(m, 600, 10 ** 9, -1, ATTEMPTS) == 0
    assert m.events.ptr == 600 and (m.infectious[:, 3] > 0).all()
    assert list(m.lockdownON) == [0, 1, 0] and list(m.contactDensity) == [1.0, 0.2, 1.0]
    scen = scenarios_of(base)
    seeds = [7, 8, 9] * 4
    ens = Ensemble(base, 12, seeds=np.array(seeds, dtype=np.int64), scenarios=scen, scenario_of=np.repeat(np.arange(4), 3))
    ens.simulate(800, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
    survived = 0
    for r in range(12):
        g = r // 3
        want = oracle_run(oracle_mod, scen[g], seeds[r], 800)
        assert 600 <= want.simulation.events.ptr <= 1400
        survived += want.simulation.events.ptr == 1400
        assert_replicate_equals(ens, r, want, "replicate %d (scenario %d, seed %d)" % (r, g, seeds[r]), first=600)
    assert survived > 0
    ens.close()


def test_one_set_equals_no_sets():
    from vgsim_amd.ensemble import Ensemble
    R = 6
    runs = []
    for kw in (dict(), dict(scenarios=[base_sim()])):
        ens = Ensemble(base_sim(), R, seeds=np.arange(1000, 1000 + R), **kw)
        res = ens.simulate(N_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True, kernel='wave')
        runs.append((res.events.copy(), [ens.replicate_events(r) for r in range(R)]))
        ens.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][0].max() > 0
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)


def test_log_consumers(oracle_mod):
    want = reference(oracle_mod)
    ens, _ = run_ensemble(BLOCK)
    batch = ens.genealogies(seed=None)
    for g in range(4):
        ok = [r for r in range(4 * g, 4 * g + 4) if batch.status[r] == 0]
        assert ok, "no replicate of scenario %d coalesces" % g
        got, one = batch.replicate(ok[0]), ens.genealogy(ok[0], None)
        assert set(got) == set(one)
        for k in got:
            assert np.array_equal(got[k], one[k]), (g, ok[0], k)
    inf, sus, steps = [(0, 0), (1, 3)], [(0, 0)], 20
    tl = ens.timelines(infectious=inf, susceptible=sus, step_num=steps)
    for r in range(16):
        sim = want[r // 4][r % 4]
        for k, (p, h) in enumerate(inf):
            data, sample, tp, ld = sim.get_data_infectious(p, h, steps)
            got = tl.data_infectious(r, k)
            assert np.array_equal(got[0], data) and np.array_equal(got[1], sample) and got[2] == list(tp) and got[3] == ld, (r, p, h)
        for k, (p, s) in enumerate(sus):
            data, tp, ld = sim.get_data_susceptible(p, s, steps)
            got = tl.data_susceptible(r, k)
            assert np.array_equal(got[0], data) and got[1] == list(tp) and got[2] == ld, (r, p, s)
    ens.close()


def test_refusals_leave_the_ensemble_usable(oracle_mod):
    from vgsim_amd import _capi
    want = reference(oracle_mod)
    ens, _ = run_ensemble(BLOCK)
    for call in (lambda: ens.simulate(N_EVENTS, mode='fast'), lambda: ens.simulate(N_EVENTS, kernel='quad'), lambda: ens.simulate_tau(N_EVENTS)):
        with pytest.raises(ValueError, match="scenario ensemble"):
            call()
    # the library's own refusals, below the Python checks
    eng = ens.engine
    o = _capi.VgxRunOpts()
    o.record_events = 1
    for mode, kernel, text in ((1, 0, "mode 0"), (0, 3, "kernel 0 or 1")):
        o.mode, o.kernel = mode, kernel
        with pytest.raises(_capi.VgxError, match=text) as err:
            eng._check(eng.lib.vgx_simulate_direct(eng.handle, N_EVENTS, 10 ** 9, -1.0, ATTEMPTS, o))
        assert err.value.code == 1
    for fn, args in ((eng.lib.vgx_simulate_tau, (N_EVENTS, 10 ** 9, -1.0, ATTEMPTS, o)), (eng.lib.vgx_stage_tau, ())):
        with pytest.raises(_capi.VgxError, match="tau-leaping runs one set only") as err:
            eng._check(fn(eng.handle, *args))
        assert err.value.code == 1
    ens.simulate(N_EVENTS, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
    for r in (1, 6, 11, 12):
        assert_replicate_equals(ens, r, want[r // 4][r % 4], "replicate %d after the refusals" % r)
    ens.close()
