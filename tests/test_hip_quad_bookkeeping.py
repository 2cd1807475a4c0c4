"""The bookkeeping of the one-class row kernel (vgx_quad.hip) outside its list passes, against the CPU oracle bit for bit with the
kernel forced: the population choice from the lanes' register copy of infectPopRate and of the slot sums (no LDS round trip; the
copy is patched wherever a rate is rewritten), and the countdown that stands in for the integer loop conditions.  Shapes: one slot
of populations, the slot border (16 / 17) and four slots; 1, 4 and 64 haplotypes; 1, 5 and 8 replicates (idle rows, a wavefront
with one live row, rows that diverge).  Every stop of the loop at its boundary: log capacity, sample count, time limit, extinction
with and without Restart (also one row of a wavefront restarting beside rows that go on), the attempt limit, a continued call.
Ensembles are compared with single seeded oracle runs of the same seeds: event chains, counters, final compartments, times."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SEEDS = np.array([11, 12, 13, 2020, 5, 777, 100003, 9], dtype=np.int64)


def _sim(sites, P, seed, beta=2.5, mut=0.01, mig=0.01, size=10 ** 5, samp=0.1):
    from vgsim_amd import Simulator
    with helpers.quiet():
        s = Simulator(number_of_sites=sites, populations_number=P, number_of_susceptible_groups=1, seed=int(seed))
    s.set_transmission_rate(beta); s.set_recovery_rate(0.9); s.set_sampling_rate(samp)
    if sites > 0:
        s.set_mutation_rate(mut)
    if P > 1:
        s.set_total_migration_probability(mig)
        s.set_migration_probability(min(2.0 * mig, 0.5), source=0, target=1)     # uneven routes: migration attempts are also rejected
    s.set_population_size(size)
    return s


def _oracle_run(oracle_mod, make, seed, n, ss, tm, at):
    m = make(seed).simulation
    assert oracle_mod.run_direct(m, n, ss, tm, at) == 0
    return m


def _check_ensemble(oracle_mod, make, R, n, ss=10 ** 9, tm=-1, at=200):
    """R replicates on the forced kernel against R single oracle runs; returns (result, oracle models)."""
    from vgsim_amd.ensemble import Ensemble
    seeds = SEEDS[:R]
    ens = Ensemble(make(seeds[0]), R, seeds=seeds)
    res = ens.simulate(n, sample_size=ss, epidemic_time=tm, attempts=at, record_events=True, kernel="quad")
    assert ens.engine.last_kernel == "quad"
    refs = []
    for r in range(R):
        m = _oracle_run(oracle_mod, make, seeds[r], n, ss, tm, at)
        refs.append(m)
        assert res.events[r] == m.events.ptr, "replicate %d: %d events, oracle %d" % (r, res.events[r], m.events.ptr)
        chain = ens.replicate_events(r)
        assert np.array_equal(chain, m.events.as_array()[:, :m.events.ptr]), "replicate %d: %s" % (
            r, helpers.describe_first_diff(chain, m.events.as_array(), m.events.ptr))
        st = ens.replicate_state(r)
        assert np.array_equal(st.infectious, m.infectious) and np.array_equal(st.susceptible, m.susceptible), "replicate %d" % r
        assert st.currentTime == m.currentTime and st.good_attempt == m.good_attempt, "replicate %d" % r
        for k in st.COUNTERS:
            assert getattr(st, k) == getattr(m, k), "replicate %d %s" % (r, k)
    ens.close()
    return res, refs


def _check_single(oracle_mod, make, seed, n, ss=10 ** 9, tm=-1, at=200):
    hip = make(seed)
    with helpers.quiet():
        hip.simulate(n, sample_size=ss, epidemic_time=tm, attempts=at, kernel="quad")
    assert hip.simulation._engine.last_kernel == "quad"
    ref = _oracle_run(oracle_mod, make, seed, n, ss, tm, at)
    helpers.assert_models_equal(hip.simulation, ref, "seed %d" % seed)
    return ref


# (populations, sites, replicates, events): one slot, the slot border, four slots; 1 / 4 / 64 haplotypes; idle rows, one live row in
# the second wavefront, two full wavefronts
SHAPES = [(1, 0, 1, 300), (1, 1, 5, 600), (16, 1, 8, 1500), (17, 3, 5, 2000), (17, 0, 1, 800), (64, 3, 8, 2000), (64, 1, 5, 1200),
          (16, 3, 1, 1000)]


@pytest.mark.parametrize("P,sites,R,n", SHAPES)
def test_shapes_stop_at_log_capacity(oracle_mod, P, sites, R, n):
    """Every replicate runs until its log is full: exactly n events, the last one the oracle's."""
    res, _ = _check_ensemble(oracle_mod, lambda seed: _sim(sites, P, seed, mig=0.05), R, n)
    assert (np.asarray(res.events) == n).all()


@pytest.mark.parametrize("P,sites,R", [(17, 3, 8), (64, 1, 5), (3, 3, 5)])
def test_slow_paths_rewrite_every_rate(oracle_mod, P, sites, R):
    """Mutations and migrations at rates of the order of the births: every slow path (list insertions and removals, accepted and
    rejected migrations) rewrites infectPopRate, birthC and the totals many times, so a stale lane copy or a stale slot sum
    changes the chain.  The chains hold a choice in the population of the event before and a choice elsewhere."""
    res, refs = _check_ensemble(oracle_mod, lambda seed: _sim(sites, P, seed, mut=0.6, mig=0.3, size=20000), R, 2000)
    m = refs[0]
    n = m.events.ptr
    ty, pop = np.asarray(m.events.types[:n]), np.asarray(m.events.populations[:n])
    assert (ty == 3).sum() > 50 and (ty == 5).sum() > 20, "mutations %d, migrations %d" % ((ty == 3).sum(), (ty == 5).sum())
    assert m.migNonPlus > 0
    same = pop[1:] == pop[:-1]
    assert same.any() and (~same).any()


def test_single_runs_through_the_simulator(oracle_mod):
    """The one-replicate path of the same kernel (three idle rows), with the model's own log."""
    _check_single(oracle_mod, lambda seed: _sim(3, 17, seed, mut=0.3, mig=0.2, size=50000), 31, 1500)
    _check_single(oracle_mod, lambda seed: _sim(0, 64, seed, mig=0.1), 32, 1000)


def test_continued_call_logs_behind_the_first(oracle_mod):
    """A second call on the same object: the log of the call starts behind the events of the first (a slot base above zero), the
    counters and the time go on."""
    def make(seed):
        return _sim(3, 17, seed, mut=0.3, mig=0.2, size=50000)
    hip = make(41)
    with helpers.quiet():
        hip.simulate(900, sample_size=10 ** 9, kernel="quad")
        hip.simulate(700, sample_size=10 ** 9, kernel="quad")
    assert hip.simulation._engine.last_kernel == "quad"
    ref = make(41).simulation
    assert oracle_mod.run_direct(ref, 900, 10 ** 9, -1, 200) == 0 and oracle_mod.run_direct(ref, 700, 10 ** 9, -1, 200) == 0
    assert ref.events.ptr == 1600
    helpers.assert_models_equal(hip.simulation, ref, "continued")


@pytest.mark.parametrize("P,sites,R,ss", [(2, 1, 5, 40), (17, 3, 8, 25), (1, 0, 1, 30)])
def test_stop_at_sample_size(oracle_mod, P, sites, R, ss):
    """The loop ends with the first iteration after sCounter passes sample_size, row by row."""
    res, refs = _check_ensemble(oracle_mod, lambda seed: _sim(sites, P, seed, samp=0.3, mig=0.05), R, 50000, ss=ss)
    for m in refs:
        assert m.sCounter == ss + 1 and m.events.ptr < 50000


def test_sample_stop_inside_the_first_hundred_events_restarts(oracle_mod):
    """An attempt that ends by its sample count within a hundred events is restarted like one that died out (pyx:414-418): every
    attempt ends so here, the countdown is formed again after each Restart, and the run ends at the attempt limit."""
    res, refs = _check_ensemble(oracle_mod, lambda seed: _sim(0, 1, seed, samp=0.3), 5, 50000, ss=1, at=40)
    assert (np.asarray(res.restarts) == 40).all() and all(m.good_attempt == 0 and m.events.ptr == 0 for m in refs)


@pytest.mark.parametrize("P,sites,R,tm", [(2, 1, 5, 3.5), (64, 3, 8, 2.25), (16, 0, 1, 4.0)])
def test_stop_at_time_limit(oracle_mod, P, sites, R, tm):
    """The first event past the time limit is the last (the countdown leaves the time compare in place)."""
    res, refs = _check_ensemble(oracle_mod, lambda seed: _sim(sites, P, seed, mig=0.05), R, 200000, tm=tm)
    for m in refs:
        n = m.events.ptr
        assert 1 < n < 200000 and m.events.times[n - 1] >= tm > m.events.times[n - 2]


def _near_critical(seed):
    return _sim(1, 2, seed, beta=1.25, mig=0.05, size=10 ** 6)


def test_one_row_restarts_beside_rows_that_go_on(oracle_mod):
    """A near-critical epidemic from one case: most attempts die out within a hundred events and Restart, the others run on.  The
    rows of a wavefront restart at different iterations and a different number of times, so they draw from their random batches out
    of step, and a restarted row forms its countdown again and starts a new random batch."""
    res, refs = _check_ensemble(oracle_mod, _near_critical, 8, 700, at=200)
    restarts = np.asarray(res.restarts)
    assert (restarts == 0).any() and (restarts > 0).any() and len(set(restarts.tolist())) >= 3, restarts
    for r, m in enumerate(refs):
        assert m.good_attempt == restarts[r] + 1


def test_extinction_without_restart(oracle_mod):
    """Fewer than 101 iterations asked for: an attempt that dies out is the run's result (pyx:414-418)."""
    res, refs = _check_ensemble(oracle_mod, _near_critical, 8, 80, at=3)
    assert (np.asarray(res.restarts) == 0).all()
    assert any(1 < m.events.ptr < 80 and m.globalInfectious == 0 for m in refs) and any(m.events.ptr == 80 for m in refs)
    _check_single(oracle_mod, lambda seed: _sim(0, 1, seed, beta=0.95), 3, 50, at=3)


@pytest.mark.parametrize("at", [1, 3])
def test_stop_at_attempt_limit(oracle_mod, at):
    """A subcritical epidemic dies out in every attempt: the run ends when the attempts are used up, after exactly `at` of them."""
    res, refs = _check_ensemble(oracle_mod, lambda seed: _sim(1, 2, seed, beta=0.8, mig=0.05), 8, 1000, at=at)
    assert sum(m.good_attempt == 0 and m.events.ptr == 0 for m in refs) >= 5
    for r, m in enumerate(refs):
        assert res.restarts[r] == (at if m.good_attempt == 0 else m.good_attempt - 1), "replicate %d" % r
    _check_single(oracle_mod, lambda seed: _sim(1, 17, seed, beta=0.8, mig=0.05), 3, 1000, at=at)
