"""Scenario ensembles on the tau path (vgx_simulate_tau after vgx_set_param_sets, the scenario entry points of vgx_taus.hip): G parameter
sets over one start state in one launch of the on-device step loop.  Replicate r must be, bit for bit, replicate k of a plain one-set
``Ensemble`` built on ``scenarios[scenario_of[r]]`` (which holds the base's start state) with seed ``seeds[r]``.

The family is tests/test_hip_param_sets.py's made tau-sized (2 sites, 3 populations, 2 susceptibility groups, 10^6 hosts per
population): A; B with other rate classes and class numbers per haplotype (its C and CB differ); C with other NPI thresholds,
migration, sampling multiplier and mutation rate; D subcritical; E with a per-haplotype mutation rate (mut_uniform differs)."""
import copy
import functools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

# Seeds on which the one-set loop runs every scenario of the family from both start states.  (Among seeds 1000 .. 1015 it ends D's
# runs from the warmed state, and a few of A's, C's and E's from the index case, with its own "tau underflow in the halving loop"
# error once few hosts are infected; a scenario ensemble with such a replicate ends with the same message.  Such a seed has no
# yardstick to compare with.  The error is the dead end bench.py's tau_small leg describes: a compartment left below zero because
# the bounds check books migrants on their source.)
SEEDS = [1004, 1007, 1008, 1009]
G, R = 5, 20
STEPS, TRAJ = 200, 21
BLOCK, CYCLE = np.repeat(np.arange(G), 4), np.arange(R) % G
STATE = ("infectious", "susceptible", "lockdownON", "contactDensity")


def seed_index(scenario_of):
    """k[r]: replicate r is the k-th replicate of its scenario (every scenario gets SEEDS[0..3])."""
    seen, k = {}, []
    for g in scenario_of:
        k.append(seen.get(int(g), 0))
        seen[int(g)] = k[-1] + 1
    return k


def base_sim():
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim = Simulator(number_of_sites=2, populations_number=3, number_of_susceptible_groups=2, seed=1)
    sim.set_transmission_rate(1.8); sim.set_recovery_rate(1.0); sim.set_sampling_rate(0.1)
    sim.set_population_size(10 ** 6); sim.set_migration_probability(0.05); sim.set_mutation_rate(0.05)
    sim.set_susceptibility_type(1); sim.set_susceptibility(0.3, susceptibility_type=1)
    sim.set_immunity_transition(0.05, source=1, target=0); sim.set_npi([0.2, 0.02, 0.004])
    return sim


def scenarios_of(base):
    """Deep copies of ``base`` (parameters and state) as scenarios A to E."""
    a, b, c, d, e = (copy.deepcopy(base) for _ in range(G))
    b.set_transmission_rate(2.6, haplotype=0)
    b.set_recovery_rate(0.8, haplotype=5)
    b.set_susceptibility(0.5, susceptibility_type=1, haplotype=2)
    c.set_npi([0.5, 0.05, 0.01], population=0)
    c.set_npi([0.1, 0.01, 0.002], population=2)
    c.set_migration_probability(0.1, source=1, target=2)
    c.set_sampling_multiplier(3.0, population=0)
    c.set_mutation_rate(0.2)
    d.set_transmission_rate(0.9)
    e.set_mutation_rate(0.3, haplotype=3)
    e.set_mutation_rate(0.01, haplotype=7, mutation=1)
    return [a, b, c, d, e]


def warmed_base():
    """The common start state: a direct warm-up of 2000 events from the index case (on the CPU oracle: the model then holds no
    engine, and copies of it are scenarios)."""
    from oracle import oracle
    oracle.build()
    base = base_sim()
    assert oracle.run_direct(base.simulation, 2000, 10 ** 9, -1, 200) == 0
    assert base.simulation.events.ptr == 2000
    return base


def index_case_base():
    return base_sim()


def flip_base():
    """A start state in which the preparation's lockdown check switches population 2 on under C's thresholds (1 % of its hosts) and
    not under A's (2 %): 15 000 hosts infected there before the first simulation, no lockdown on."""
    base = base_sim()
    m = base.simulation
    m.infectious[2, 3] += 9000; m.infectious[2, 0] += 6000
    m.susceptible[2, 0] -= 15000
    m.infectious[0, 0] += 40; m.susceptible[0, 0] -= 40
    m.totalInfectious[2] += 15000; m.totalSusceptible[2] -= 15000
    m.totalInfectious[0] += 40; m.totalSusceptible[0] -= 40
    m.globalInfectious += 15040
    return base


def record_all(ens, res):
    """Everything the contract lists, per replicate."""
    off, rows = ens.replicate_multievents()
    traj = ens.trajectories()
    out = []
    for r in range(ens.R):
        st = ens.replicate_state(r)
        rec = {k: np.array(getattr(st, k)) for k in STATE}
        for k in st.COUNTERS + ("good_attempt", "currentTime"):
            rec[k] = getattr(st, k)
        rec["restarts"], rec["events"], rec["events_drawn"] = int(res.restarts[r]), int(res.events[r]), int(res.events_drawn[r])
        rec["chain"] = ens.replicate_events(r)
        rec["lockdowns"] = np.column_stack([np.asarray(x, dtype=np.float64) for x in ens.engine.lockdowns(r)])
        # (the rows of a step stand in the order its lanes took their slots: compared as a set per step, sorted here)
        mine = np.column_stack([rows[k][off[r]:off[r + 1]] for k in ("steps", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations", "num")])
        rec["rows"] = mine[np.lexsort(mine.T[::-1])]
        rec["traj"] = traj[r].copy()
        out.append(rec)
    return out


def assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


def tau_call(ens, iterations, attempts, t0):
    return ens.simulate_tau(iterations, sample_size=10 ** 12, attempts=attempts, record_events=True, traj_points=TRAJ,
                            traj_window=(t0, t0 + 4.0), per_scenario=ens.scenarios is not None)


def run_scenarios(make_base, scenario_of, iterations=STEPS, attempts=200, keep=False):
    from vgsim_amd.ensemble import Ensemble
    base = make_base()
    k = seed_index(scenario_of)
    seeds = np.array([SEEDS[i] for i in k], dtype=np.int64)
    ens = Ensemble(base, R, seeds=seeds, scenarios=scenarios_of(base), scenario_of=scenario_of)
    res = tau_call(ens, iterations, attempts, base.simulation.currentTime)
    recs = record_all(ens, res)
    if keep:
        return ens, recs
    ens.close()
    return recs


@functools.lru_cache(maxsize=None)
def yardstick(make_base, iterations=STEPS, attempts=200):
    """want[g][k]: replicate k (seed SEEDS[k]) of a plain one-set ensemble on scenario g, run once and shared (never changed)."""
    from vgsim_amd.ensemble import Ensemble
    base = make_base()
    want = []
    for s in scenarios_of(base):
        ens = Ensemble(s, 4, seeds=np.array(SEEDS, dtype=np.int64))
        res = tau_call(ens, iterations, attempts, base.simulation.currentTime)
        want.append(record_all(ens, res))
        ens.close()
    return want


def assert_equals_yardstick(recs, want, scenario_of, what=""):
    k = seed_index(scenario_of)
    for r in range(R):
        g = int(scenario_of[r])
        assert_same(recs[r], want[g][k[r]], "%sreplicate %d (scenario %d, seed %d)" % (what, r, g, SEEDS[k[r]]))


@pytest.mark.parametrize("scenario_of", [BLOCK, CYCLE], ids=["block", "cycle"])
def test_replicates_equal_the_one_set_ensemble_of_their_own_scenario(scenario_of):
    want = yardstick(warmed_base)
    assert_equals_yardstick(run_scenarios(warmed_base, scenario_of), want, scenario_of)


def test_the_family_reaches_what_it_is_there_for():
    """On the yardstick runs alone: a later edit of the models must not hollow the tests out."""
    want = yardstick(warmed_base)
    finals = [np.concatenate([want[g][0]["infectious"].ravel(), want[g][0]["susceptible"].ravel()]) for g in range(G)]
    for g in range(G):
        assert all(w["events"] > 2000 for w in want[g]), g
        for g2 in range(g):
            assert not np.array_equal(finals[g], finals[g2]), (g, g2)     # pairwise different final states under one seed
    # a lockdown switch during the tau steps (a record later than the start; a Restart's re-check carries the time 0) in some set,
    # none in another: the 200 steps from the warmed state reach no threshold, the 300 from the index case do
    index = yardstick(index_case_base, 300, 5)
    switches = [sum(int((w["lockdowns"][:, 2] > 0.0).sum()) for w in index[g]) for g in range(G)]
    print("lockdown switches during the tau steps per scenario, from the index case:", switches)
    assert max(switches) > 0 and min(switches) == 0
    scen = scenarios_of(base_sim())
    rows = [len(np.unique(np.column_stack([s.simulation.bRate, s.simulation.dRate, s.simulation.susceptibility]), axis=0)) for s in scen]
    assert rows[0] == 1 and rows[1] == 4     # B's C (and CB) differ from A's
    uniform = [bool((s.simulation.mRate == s.simulation.mRate[0]).all()) for s in scen]
    assert uniform == [True, True, True, True, False]     # E alone has a non-uniform mutation model


def test_restarts_run_under_the_replicates_own_set():
    """From the index case: D's replicates die out within 100 steps and restart, so Restart re-checks the lockdowns with the set's own
    thresholds and the guard of the restored state is the set's own."""
    want = yardstick(index_case_base, 300, 5)
    print("restarts per scenario and seed:", [[w["restarts"] for w in ws] for ws in want])
    assert any(w["restarts"] > 0 for w in want[3])
    assert any(w["restarts"] == 0 for w in want[0])
    for scenario_of in (BLOCK, CYCLE):
        assert_equals_yardstick(run_scenarios(index_case_base, scenario_of, 300, 5), want, scenario_of)


def test_preparation_lockdown_check_is_per_set():
    """swapLockdown, the first lockdown record and the starting contact density come from the replicate's own set's preparation."""
    want = yardstick(flip_base, 120, 5)
    a, c = want[0][0], want[2][0]
    assert len(a["lockdowns"]) == 0 or a["lockdowns"][0, 2] > 0.0          # A: nothing switches at the start
    assert list(c["lockdowns"][0]) == [1.0, 2.0, 0.0]                        # C: population 2 on, at time 0
    assert c["swapLockdown"] >= 1
    recs = run_scenarios(flip_base, BLOCK, 120, 5)
    assert_equals_yardstick(recs, want, BLOCK)
    assert recs[8]["swapLockdown"] == c["swapLockdown"] and recs[0]["swapLockdown"] == a["swapLockdown"]


@pytest.mark.parametrize("threads", ["64", "256", "512"])
def test_scenario_run_does_not_depend_on_the_workgroup_size(monkeypatch, threads):
    monkeypatch.setenv("VGX_TAUS_THREADS", threads)
    assert_equals_yardstick(run_scenarios(warmed_base, CYCLE), yardstick(warmed_base), CYCLE, "%s threads: " % threads)


def direct_record(ens, res, r):
    st = ens.replicate_state(r)
    rec = {k: np.array(getattr(st, k)) for k in STATE}
    for k in st.COUNTERS + ("good_attempt", "currentTime"):
        rec[k] = getattr(st, k)
    rec["events"], rec["chain"] = int(res.events[r]), ens.replicate_events(r)
    return rec


def test_direct_then_tau_then_direct_on_one_ensemble():
    from vgsim_amd.ensemble import Ensemble
    base = warmed_base()
    scen = scenarios_of(base)
    k = seed_index(CYCLE)
    ens = Ensemble(base, R, seeds=np.array([SEEDS[i] for i in k], dtype=np.int64), scenarios=scen, scenario_of=CYCLE)
    direct = []
    for s in scen:
        one = Ensemble(s, 4, seeds=np.array(SEEDS, dtype=np.int64))
        res = one.simulate(1500, sample_size=10 ** 9, attempts=20, record_events=True, kernel='wave')
        direct.append([direct_record(one, res, r) for r in range(4)])
        one.close()
    for call in ("direct", "tau", "direct"):
        if call == "tau":
            res = tau_call(ens, STEPS, 200, base.simulation.currentTime)
            assert_equals_yardstick(record_all(ens, res), yardstick(warmed_base), CYCLE, "tau call: ")
        else:
            res = ens.simulate(1500, sample_size=10 ** 9, attempts=20, record_events=True)
            for r in range(R):
                assert_same(direct_record(ens, res, r), direct[int(CYCLE[r])][k[r]], "direct call, replicate %d" % r)
    ens.close()


def test_analytics_group_by_scenario():
    from vgsim_amd.ensemble import Ensemble
    ens, recs = run_scenarios(warmed_base, CYCLE, keep=True)
    base = warmed_base()
    t0 = base.simulation.currentTime
    k = seed_index(CYCLE)
    yard = []
    for s in scenarios_of(base):
        one = Ensemble(s, 4, seeds=np.array(SEEDS, dtype=np.int64))
        tau_call(one, STEPS, 200, t0)
        yard.append(one)
    members = [np.nonzero(CYCLE == g)[0] for g in range(G)]

    def check_summary(s, block):
        assert list(s.groups) == list(range(G)) and list(s.count) == [4] * G
        for g in range(G):
            assert np.array_equal(s.sum[g], block[members[g]].sum(axis=0)), g
            assert np.array_equal(s.min[g], block[members[g]].min(axis=0)) and np.array_equal(s.max[g], block[members[g]].max(axis=0)), g
            # ('lower': a member's value, exact; the interpolated form differs from numpy's in the last bits, as on any ensemble)
            assert np.array_equal(s.quantiles[g], np.quantile(block[members[g]].astype(np.float64), s.q, axis=0, method='lower')), g

    def same_summary(a, b):
        for name in ("count", "sum", "min", "max", "quantiles"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name

    ts = ens.trajectory_summary(method='lower')
    check_summary(ts, ens.trajectories().astype(np.int64))
    same_summary(ts, ens.trajectory_summary(by=CYCLE, method='lower'))
    grid = dict(bins=8, window=(t0, t0 + 4.0))
    points = dict(points=9, window=(t0, t0 + 4.0))
    calls = (("tau_incidence", grid, "counts"), ("tau_flows", grid, "counts"), ("tau_prevalence", points, "values"),
             ("tau_susceptibles", points, "values"))
    for name, kw, field in calls:
        got = getattr(ens, name)(summary=dict(method='lower'), **kw)
        block = getattr(got, field)
        check_summary(got.summary, block)
        same_summary(got.summary, getattr(ens, name)(summary=dict(by=CYCLE, method='lower'), **kw).summary)
        for g in range(G):
            want = getattr(getattr(yard[g], name)(**kw), field)
            for r in members[g]:
                assert np.array_equal(block[r], want[k[r]]), (name, r)
    ext = ens.tau_milestones().extinction_probability()
    assert ext.shape[0] == G
    for g in range(G):
        assert np.array_equal(ext[g], yard[g].tau_milestones().extinction_probability()[0]), g
    two = [2, 11]      # scenarios C and B
    gen = ens.tau_genealogies(replicates=two)
    tl = ens.tau_timelines(infectious=[(0, 0), (1, 3)], susceptible=[(2, 0)], step_num=20, replicates=two)
    for i, r in enumerate(two):
        g = int(CYCLE[r])
        wg = yard[g].tau_genealogies(replicates=[k[r]])
        assert gen.status[i] == wg.status[0] == 0, (r, gen.message(i))
        a, b = gen.replicate(r), wg.replicate(k[r])
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), (r, key)
        wt = yard[g].tau_timelines(infectious=[(0, 0), (1, 3)], susceptible=[(2, 0)], step_num=20, replicates=[k[r]])
        for q in range(2):
            x, y = tl.data_infectious(r, q), wt.data_infectious(k[r], q)
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3], (r, q)
        x, y = tl.data_susceptible(r, 0), wt.data_susceptible(k[r], 0)
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], r
    for one in yard:
        one.close()
    ens.close()


def test_refusals_leave_the_ensemble_usable(monkeypatch):
    from vgsim_amd import Simulator, _capi
    from vgsim_amd.ensemble import Ensemble
    with helpers.quiet():
        big = Simulator(number_of_sites=7, populations_number=3, seed=1)
    big.set_population_size(10 ** 6)
    other = copy.deepcopy(big)
    other.set_transmission_rate(2.5)
    ens = Ensemble(big, 4, scenarios=[big, other])
    with pytest.raises(_capi.VgxError, match=r"vgx_simulate_tau: .*49152.*8192") as err:
        ens.simulate_tau(50, per_scenario=True)
    assert err.value.code == 1
    ens.close()

    base = warmed_base()
    scen = scenarios_of(base)
    k = seed_index(CYCLE)
    ens = Ensemble(base, R, seeds=np.array([SEEDS[i] for i in k], dtype=np.int64), scenarios=scen, scenario_of=CYCLE)
    for name in ("VGX_TAU_STEP_KERNELS", "VGX_TAU_LARGE_MODEL_THRESHOLDS"):
        monkeypatch.setenv(name, "1")
        with pytest.raises(_capi.VgxError, match="vgx_simulate_tau: 5 parameter sets.*%s=1" % name) as err:
            ens.simulate_tau(STEPS, per_scenario=True)
        assert err.value.code == 1
        monkeypatch.delenv(name)
    with pytest.raises(_capi.VgxError, match="tau-leaping runs one set only"):
        ens.engine.stage_tau()
    with pytest.raises(ValueError, match="scenario ensemble.*per_scenario=True"):     # a call that does not ask for the scenarios
        ens.simulate_tau(STEPS)
    res = ens.simulate(1500, sample_size=10 ** 9, attempts=20, record_events=True)
    one = Ensemble(scen[2], 4, seeds=np.array(SEEDS, dtype=np.int64))
    want = one.simulate(1500, sample_size=10 ** 9, attempts=20, record_events=True, kernel='wave')
    assert_same(direct_record(ens, res, 7), direct_record(one, want, k[7]), "replicate 7 after the refusals")
    one.close()
    res = tau_call(ens, STEPS, 200, base.simulation.currentTime)
    assert_equals_yardstick(record_all(ens, res), yardstick(warmed_base), CYCLE, "after the refusals: ")
    ens.close()
