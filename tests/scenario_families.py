"""Model families for scenario ensembles beyond the small one of test_hip_param_sets.py: every family is a base model (the
start state) and the list of its scenarios, deep copies of the base with other parameters, as ``base_sim`` / ``scenarios_of``
are there.  test_scenario_families.py asserts, on the CPU oracle alone, what each family exists to reach;
test_hip_param_sets_shapes.py runs them on the GPU against the same oracle runs (made once, shared and never changed).

wide(P)         more than 64 populations (the scenario kernel with a runtime population stride), set 0 without any NPI
long_lists      occupancy lists of more than one and more than two 64-entry tiles, 3 susceptibility groups, a lockdown that is on
                at the start, row counts of 6, 33 and 2 classes
recombinant     recombinant births under every set
one_group       one susceptibility group, 1024 haplotypes, 16 populations
many_sets       40 sets, one replicate each, the map from replicate to set not in order
unused_largest  the set with the most classes is installed and run by nobody
small           the family of test_hip_param_sets.py, for stops by sample size and by time"""
import copy
import functools

import numpy as np

import helpers
import models
from test_hip_param_sets import ATTEMPTS, SEEDS, base_sim, oracle_run, scenarios_of

WIDE_P = (64, 65, 70)
WIDE_EVENTS = 3000
LONG_WARM, LONG_EVENTS, LONG_SEEDS = 6000, 3000, (7, 8, 9)
RECOMB_EVENTS, RECOMB_SEEDS = 2500, (11, 12, 13)
ONE_GROUP_EVENTS, ONE_GROUP_SEEDS = 3000, (21, 22, 23)
MANY_G, MANY_EVENTS = 40, 2000
MANY_SEEDS = 1000 + np.arange(MANY_G, dtype=np.int64)
MANY_OF = np.arange(MANY_G)[::-1].copy()
UNUSED_OF = np.array([0, 2, 3, 4, 2, 3, 4, 0])             # index 1 (B, the most classes) is run by nobody
UNUSED_SEEDS = np.array(SEEDS * 2, dtype=np.int64)
UNUSED_SOURCE = (0, 1, 2, 3, 0)                            # the scenario of scenarios_of() behind every index of the five-set list
STOPS = {"sample": dict(sample_size=25, epidemic_time=-1), "time": dict(sample_size=10 ** 9, epidemic_time=12.0)}
STOP_EVENTS = 2000


def _case(name):
    from vgsim_amd import Simulator
    with helpers.quiet():
        sim, phases = models.build(Simulator, name)
        phases[0][0](sim)
    return sim


def wide(P):
    from vgsim_amd import Simulator
    with helpers.quiet():
        base = Simulator(number_of_sites=1, populations_number=P, number_of_susceptible_groups=2, seed=99)
    base.set_transmission_rate(2.2); base.set_recovery_rate(0.8); base.set_sampling_rate(0.05); base.set_mutation_rate(0.2)
    base.set_susceptibility_type(1); base.set_susceptibility(0.5, susceptibility_type=1)
    base.set_immunity_transition(0.05, source=1, target=0)
    base.set_population_size(300); base.set_total_migration_probability(0.3)
    a, b, c = (copy.deepcopy(base) for _ in range(3))
    b.set_transmission_rate(3.0, haplotype=2)
    b.set_recovery_rate(0.6, haplotype=1)
    for pn in (0, 3, P - 6, P - 1):
        b.set_npi([0.3, 0.02, 0.005], population=pn)
    b.set_contact_density(1.5, population=P - 5)
    b.set_sampling_multiplier(3.0, population=P - 4)
    c.set_npi([0.1, 0.01, 0.002])
    c.set_migration_probability(0.01, source=0, target=P - 1)
    c.set_mutation_rate(0.4)
    return base, [a, b, c]


@functools.lru_cache(maxsize=None)
def _long_lists_base(oracle_mod):
    base = _case("stress_h256")
    m = base.simulation
    m.user_seed = 4242
    assert oracle_mod.run_direct(m, LONG_WARM, 10 ** 9, -1, ATTEMPTS) == 0
    assert m.events.ptr == LONG_WARM
    return base


def long_lists(oracle_mod):
    """The base is warmed up by the oracle once; every call returns copies of that one start state."""
    base = copy.deepcopy(_long_lists_base(oracle_mod))
    a, b, c = (copy.deepcopy(base) for _ in range(3))
    b.set_transmission_rate(4.0, haplotype='A***')
    b.set_recovery_rate(0.5, haplotype='**C*')
    b.set_susceptibility_type(0, haplotype='*G**')
    b.set_sampling_rate(0.3, haplotype='***T')
    c.set_transmission_rate(2.5, haplotype='G***')
    c.set_transmission_rate(2.5, haplotype='*T*C')
    c.set_recovery_rate(0.9, haplotype='C***')
    c.set_mutation_rate(1.5)
    c.set_npi([0.5, 0.001, 0.0002], population=2)
    return base, [a, b, c]


def recombinant():
    base = _case("recomb_a")
    a, b, c = (copy.deepcopy(base) for _ in range(3))
    b.set_transmission_rate(2.0, haplotype='*G*')
    b.set_recovery_rate(0.7, haplotype='A**')
    b.set_mutation_rate(0.6)
    c.set_npi([0.3, 0.01, 0.002])
    c.set_migration_probability(0.1)
    return base, [a, b, c]


def one_group():
    """10^7 hosts per population: the NPI thresholds are a few hundred infectious hosts, which 3000 events reach."""
    base = _case("c3_s5_p16")
    a, b, c = (copy.deepcopy(base) for _ in range(3))
    b.set_transmission_rate(3.2, haplotype='*G***')
    b.set_recovery_rate(0.7, haplotype='**C**')
    b.set_mutation_rate(0.3)
    b.set_npi([0.4, 2e-5, 5e-6], population=0)
    c.set_transmission_rate(2.0, haplotype='T****')
    c.set_mutation_rate(0.5)
    c.set_total_migration_probability(0.2)
    c.set_npi([0.3, 5e-6, 1e-6])
    return base, [a, b, c]


def many_sets():
    base = base_sim()
    scen = []
    for g in range(MANY_G):
        s = copy.deepcopy(base)
        s.set_transmission_rate(1.5 + 0.03 * g)
        s.set_recovery_rate(0.7 + 0.01 * g, haplotype=g % 16)
        scen.append(s)
    return base, scen


def unused_largest():
    base = base_sim()
    four = scenarios_of(base)
    return base, four + [copy.deepcopy(four[0])]


def small():
    base = base_sim()
    return base, scenarios_of(base)


def class_rows(sim):
    """The distinct (transmission, recovery, sampling, susceptibility row) classes of a model's haplotypes."""
    m = sim.simulation
    cols = [m.bRate, m.dRate, m.sRate, m.suscType, np.asarray(m.susceptibility).reshape(m.hapNum, -1)]
    return len(np.unique(np.column_stack(cols), axis=0))


def list_lengths(m):
    """Occupied haplotypes per population: the lengths of the kernel's occupancy lists."""
    return (np.asarray(m.infectious) > 0).sum(axis=1)


def can_switch(m):
    """The engine's own rule (a population can switch on only if its threshold lies below its size, off only if it is on)."""
    sizes = np.asarray(m.sizes, dtype=np.float64)
    return bool((np.asarray(m.startLD) * sizes < sizes).any() or np.asarray(m.lockdownON).any())


def run_stop(oracle_mod, sim, seed, stop):
    """``oracle_run`` with one of ``STOPS``: (the copy that ran, the oracle's return code)."""
    one = copy.deepcopy(sim)
    one.simulation.user_seed = int(seed)
    kw = STOPS[stop]
    rc = oracle_mod.run_direct(one.simulation, STOP_EVENTS, kw["sample_size"], kw["epidemic_time"], ATTEMPTS)
    return one, rc


# ---------------------------------------------------------------- the oracle's runs, made once (never changed by a test)
@functools.lru_cache(maxsize=None)
def reference_wide(oracle_mod, P):
    """want[g][k]: scenario g of wide(P) under SEEDS[k]."""
    _, scen = wide(P)
    return [[oracle_run(oracle_mod, s, seed, WIDE_EVENTS) for seed in SEEDS] for s in scen]


@functools.lru_cache(maxsize=None)
def reference_long_lists(oracle_mod):
    _, scen = long_lists(oracle_mod)
    return [[oracle_run(oracle_mod, s, seed, LONG_EVENTS) for seed in LONG_SEEDS] for s in scen]


@functools.lru_cache(maxsize=None)
def reference_recombinant(oracle_mod):
    _, scen = recombinant()
    return [[oracle_run(oracle_mod, s, seed, RECOMB_EVENTS) for seed in RECOMB_SEEDS] for s in scen]


@functools.lru_cache(maxsize=None)
def reference_one_group(oracle_mod):
    _, scen = one_group()
    return [[oracle_run(oracle_mod, s, seed, ONE_GROUP_EVENTS) for seed in ONE_GROUP_SEEDS] for s in scen]


@functools.lru_cache(maxsize=None)
def reference_many_sets(oracle_mod):
    """want[r]: replicate r, which runs set MANY_OF[r] under MANY_SEEDS[r]."""
    _, scen = many_sets()
    return [oracle_run(oracle_mod, scen[int(MANY_OF[r])], MANY_SEEDS[r], MANY_EVENTS) for r in range(MANY_G)]


@functools.lru_cache(maxsize=None)
def reference_stop(oracle_mod, stop):
    """want[g][k] = (model, return code): scenario g of small() under SEEDS[k], stopped as STOPS[stop] says."""
    _, scen = small()
    return [[run_stop(oracle_mod, s, seed, stop) for seed in SEEDS] for s in scen]
