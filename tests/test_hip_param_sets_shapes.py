"""Scenario ensembles on the GPU at the shapes test_hip_param_sets.py leaves out (the families of scenario_families.py): more than 64
populations (vgx_direct_sets_kernel, the runtime population stride; 64 populations stay on vgx_direct_sets_kernel_p64), occupancy
lists of several 64-entry tiles at the start (vgx_init_reps_sets_kernel) and after a Restart, a set 0 that cannot switch a lockdown
beside sets that can, recombinant births, one and three susceptibility groups, one set per replicate in any order, a largest set that
nobody runs, stops by sample size and by time.

Every replicate must be, bit for bit, the CPU oracle's run of its own scenario with its own seed (test_scenario_families.py asserts on
those runs that they reach what they are here for): chain with times, counters, compartments, clock, and the lockdown log of the call.
No test runs more than 40 wavefronts of at most 3000 events."""

import copy

import numpy as np
import pytest

import scenario_families as fam
from test_hip_ensemble_genealogy import assert_batch_equals_host
from test_hip_param_sets import ATTEMPTS, N_EVENTS, SEEDS, assert_replicate_equals, oracle_run, reference
from test_incidence_rule import restate_sorted

pytestmark = pytest.mark.gpu


def no_clock_mismatch(ens):
    assert ens.engine.lib.vgx_clock_mismatches(ens.engine.handle) == 0


def run(base, scen, scenario_of, seeds, events, **stop):
    from vgsim_amd.ensemble import Ensemble
    stop.setdefault("sample_size", 10 ** 9)
    ens = Ensemble(base, len(seeds), seeds=np.asarray(seeds, dtype=np.int64), scenarios=scen, scenario_of=np.asarray(scenario_of))
    res = ens.simulate(events, attempts=ATTEMPTS, record_events=True, **stop)
    no_clock_mismatch(ens)
    assert ens.engine.last_kernel == "wave"
    assert np.array_equal(ens.scenario_of, scenario_of)
    return ens, res


def assert_equals_oracle(ens, r, want, what, first=0, loc_first=0):
    """``assert_replicate_equals`` and the lockdown log of the call: the oracle's records from ``loc_first`` on."""
    st = assert_replicate_equals(ens, r, want, what, first=first)
    loc = want.simulation.loc
    states, pops, times = ens.engine.lockdowns(r)
    assert np.array_equal(states, np.asarray(loc.states[loc_first:], dtype=np.int64)), (what, "lockdown states")
    assert np.array_equal(pops, np.asarray(loc.populationsId[loc_first:], dtype=np.int64)), (what, "lockdown populations")
    assert np.array_equal(times, np.asarray(loc.times[loc_first:], dtype=np.float64)), (what, "lockdown times")
    no_clock_mismatch(ens)
    return st


@pytest.mark.parametrize("P", fam.WIDE_P)
def test_wide(oracle_mod, P):
    want = fam.reference_wide(oracle_mod, P)
    base, scen = fam.wide(P)
    of = np.arange(12) % 3
    ens, res = run(base, scen, of, SEEDS * 3, fam.WIDE_EVENTS)
    switched = 0
    for r in range(12):
        g, k = r % 3, r % 4      # 12 replicates: every set meets every seed once
        assert_equals_oracle(ens, r, want[g][k], "P = %d, replicate %d (scenario %d, seed %d)" % (P, r, g, SEEDS[k]))
        assert res.events[r] == fam.WIDE_EVENTS
        switched += len(ens.engine.lockdowns(r)[0]) > 0
    assert switched == 8         # the replicates of B and C, whose log set 0 alone would not have sized
    ens.close()


def test_long_lists(oracle_mod):
    want = fam.reference_long_lists(oracle_mod)
    base, scen = fam.long_lists(oracle_mod)
    loc0 = len(base.simulation.loc.states)
    seeds = list(fam.LONG_SEEDS) * 3
    ens, _ = run(base, scen, np.repeat(np.arange(3), 3), seeds, fam.LONG_EVENTS)
    for r in range(9):
        g, k = r // 3, r % 3
        assert_equals_oracle(ens, r, want[g][k], "replicate %d (scenario %d, seed %d)" % (r, g, seeds[r]), first=fam.LONG_WARM, loc_first=loc0)
    ens.close()


def test_recombinant(oracle_mod):
    from vgsim_amd._model import Recombination
    want = fam.reference_recombinant(oracle_mod)
    base, scen = fam.recombinant()
    seeds = list(fam.RECOMB_SEEDS) * 3
    ens, _ = run(base, scen, np.repeat(np.arange(3), 3), seeds, fam.RECOMB_EVENTS)
    for r in range(9):
        g, k = r // 3, r % 3
        what = "replicate %d (scenario %d, seed %d)" % (r, g, seeds[r])
        assert_equals_oracle(ens, r, want[g][k], what)
        rec = want[g][k].simulation.rec
        cols = ens.engine.recombinations(r)
        assert len(cols) == 5 and len(cols[0]) > 0
        got = Recombination()     # the engine's rows as a host model takes them (HipEngine._absorb), as the oracle's adapter does
        for row in zip(*cols):
            got.AddRecombination_forward(*row)
        for name in ("idevents", "his", "hi2s", "nhis", "posRecombs"):
            assert getattr(got, name) == getattr(rec, name), (what, "rec." + name)
    ens.close()


def test_one_group(oracle_mod):
    want = fam.reference_one_group(oracle_mod)
    base, scen = fam.one_group()
    seeds = list(fam.ONE_GROUP_SEEDS) * 3
    of = np.arange(9) // 3
    ens, _ = run(base, scen, of, seeds, fam.ONE_GROUP_EVENTS)
    for r in range(9):
        g, k = r // 3, r % 3
        assert_equals_oracle(ens, r, want[g][k], "replicate %d (scenario %d, seed %d)" % (r, g, seeds[r]))
    ens.close()


def test_many_sets(oracle_mod):
    want = fam.reference_many_sets(oracle_mod)
    base, scen = fam.many_sets()
    ens, res = run(base, scen, fam.MANY_OF, fam.MANY_SEEDS, fam.MANY_EVENTS)
    for r in range(fam.MANY_G):
        assert_equals_oracle(ens, r, want[r], "replicate %d (scenario %d, seed %d)" % (r, fam.MANY_OF[r], fam.MANY_SEEDS[r]))
        assert res.events[r] == want[r].simulation.events.ptr
    ens.close()


def test_unused_largest(oracle_mod):
    want = reference(oracle_mod)
    base, scen = fam.unused_largest()
    ens, _ = run(base, scen, fam.UNUSED_OF, fam.UNUSED_SEEDS, N_EVENTS)
    chains = []
    for r in range(8):
        g = int(fam.UNUSED_OF[r])
        assert_equals_oracle(ens, r, want[fam.UNUSED_SOURCE[g]][r % 4], "replicate %d (set %d, seed %d)" % (r, g, fam.UNUSED_SEEDS[r]))
        chains.append(ens.replicate_events(r))
    ens.close()
    # the same replicates without the set nobody runs: tables sized by the used sets alone
    used = [0, 2, 3, 4]
    ens, _ = run(base, [scen[g] for g in used], np.array([used.index(int(g)) for g in fam.UNUSED_OF]), fam.UNUSED_SEEDS, N_EVENTS)
    for r in range(8):
        assert np.array_equal(ens.replicate_events(r), chains[r]), r
        assert_equals_oracle(ens, r, want[fam.UNUSED_SOURCE[int(fam.UNUSED_OF[r])]][r % 4], "replicate %d without the unused set" % r)
    ens.close()


@pytest.mark.parametrize("stop", sorted(fam.STOPS))
def test_stops(oracle_mod, stop):
    want = fam.reference_stop(oracle_mod, stop)
    base, scen = fam.small()
    of = np.arange(16) % 4
    seeds = [SEEDS[(r // 4 + r) % 4] for r in range(16)]   # shifted by one per block of four: every set meets every seed once
    ens, res = run(base, scen, of, seeds, fam.STOP_EVENTS, **fam.STOPS[stop])
    for r in range(16):
        g, k = r % 4, (r // 4 + r) % 4
        w, rc = want[g][k]
        assert rc == 0
        assert_equals_oracle(ens, r, w, "%s stop, replicate %d (scenario %d, seed %d)" % (stop, r, g, SEEDS[k]))
        assert res.events[r] == w.simulation.events.ptr
    ens.close()


def test_log_consumers_on_long_lists(oracle_mod):
    """incidence() and genealogies() read a replicate's log from index 0 and refuse a chain that continues a model's own events, as
    the long_lists ensemble's does (Limits).  They are therefore run on the same start state taken as a new
    beginning: the base model's log emptied and its event counters zeroed, everything else (lists, lockdown, clock, sets) as it
    is.  The chains are then the oracle's columns 6000.. of the same scenario and seed.  The oracle's walks over these 3000 events
    do not coalesce (a few hundred samples among thousands of infectious hosts): the batch is compared with the host pass of
    every replicate, by status and text where that one raises."""
    want = fam.reference_long_lists(oracle_mod)
    base, scen = fam.long_lists(oracle_mod)
    seeds = list(fam.LONG_SEEDS) * 3
    of = np.repeat(np.arange(3), 3)
    ens, _ = run(base, scen, of, seeds, fam.LONG_EVENTS)
    for call in (lambda: ens.incidence(bins=7, window=(4.0, 5.0)), lambda: ens.genealogies(seed=None)):
        with pytest.raises(ValueError, match="does not start in the last call's device log"):
            call()
    ens.close()
    from vgsim_amd._model import Events
    for s in [base] + scen:
        m = s.simulation
        m.events = Events()
        for c in m.COUNTERS:
            setattr(m, c, 0)
    ens, res = run(base, scen, of, seeds, fam.LONG_EVENTS)
    t_end = 0.0
    for r in range(9):
        w = want[r // 3][r % 3].simulation
        chain = ens.replicate_events(r)
        assert res.events[r] == fam.LONG_EVENTS
        assert np.array_equal(chain, w.events.as_array()[:, fam.LONG_WARM:fam.LONG_WARM + fam.LONG_EVENTS]), r
        st = ens.replicate_state(r)
        assert np.array_equal(st.infectious, w.infectious) and np.array_equal(st.susceptible, w.susceptible), r
        assert st.currentTime == w.currentTime
        t_end = max(t_end, w.currentTime)
    t0 = base.simulation.currentTime
    inc = ens.incidence(bins=7, window=(t0 + 0.05 * (t_end - t0), t0 + 0.9 * (t_end - t0)))
    assert inc.counts.shape == (9, 7, base.simulation.popNum, 7) and inc.counts.any() and inc.outside.any()
    for r in range(9):
        a = ens.replicate_events(r)
        counts, outside = restate_sorted(a[0].copy(), [a[k].astype(np.int64) for k in range(1, 6)], base.simulation.popNum, inc.edges)
        assert np.array_equal(inc.counts[r], counts) and np.array_equal(inc.outside[r], outside), r
    batch = ens.genealogies(seed=None)
    assert_batch_equals_host(ens, batch, None)   # (a walk that does coalesce is compared key by key)
    no_clock_mismatch(ens)
    ens.close()


def test_contact_density_a_scenario_cannot_start_from_is_refused(oracle_mod):
    """Every replicate starts with its own set's contact densities for the lockdown state of the start state (wide's B, whose
    set_contact_density the shared start state does not hold, is the run).  A scenario whose model holds another value, here a
    new NPI for a population that is locked down already, which the reference applies at the next switch only, is refused
    before anything is uploaded, and the ensemble runs on."""
    from vgsim_amd.ensemble import Ensemble
    base = fam.small()[0]
    m = base.simulation
    m.user_seed = 1001
    assert oracle_mod.run_direct(m, 600, 10 ** 9, -1, ATTEMPTS) == 0 and list(m.lockdownON) == [0, 1, 0]
    scen = [copy.deepcopy(base) for _ in range(2)]
    scen[1].set_npi([0.6, 0.02, 0.004], population=1)
    assert scen[1].simulation.contactDensity[1] == 0.2 and scen[1].simulation.contactDensityAfterLockdown[1] == 0.6
    ens = Ensemble(base, 2, seeds=np.array([7, 8], dtype=np.int64), scenarios=scen)
    with pytest.raises(ValueError, match="scenario 1: the contact density of population 1 is 0.2, its own settings give 0.6"):
        ens.simulate(800, sample_size=10 ** 9, attempts=ATTEMPTS, record_events=True)
    ens.close()
    ens, _ = run(base, scen[:1] * 2, np.array([0, 1]), [7, 8], 800)
    for r in range(2):
        assert_equals_oracle(ens, r, oracle_run(oracle_mod, scen[0], 7 + r, 800), "replicate %d" % r, first=600,
                             loc_first=len(m.loc.states))
    ens.close()
